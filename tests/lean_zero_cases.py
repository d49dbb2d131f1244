"""Shared by tests/test_lean_zero_mark_rules.py (CPU) and tests/test_gpu_lean_zero_mark.py (GPU): pairs on which the local walk of a
lean build (csrc/dp_affine_tag.hip LEAN) has to read "this cell scores 0" from a pointer word, and the rule itself in numpy.

The rule (aln_device.h::lean_score).  A lean word says "score 0" when it is
  0xFFFF                  a border, masked or untouched cell;
  P_MATCH | 1             an interior cell (row >= 2 and column >= 2) the clip key won: match, tag bit 0.  No candidate carries this
                          word (match candidates have tag 0, gap candidates another priority), and decode_ptr ignores a match word's tag;
  anything with bit 15    a cell of row 1 or column 1: these are not clipped against a key and keep their origin pointer.
Every other word says "score > 0".  Bits 0 .. 12 of every lean word decode like the full build's word.

What a paid gap can and cannot do.  A gap candidate replaces the diagonal one only when it is strictly greater, and the diagonal
candidate of a local build is >= 0: the cell a deletion or insertion jump lands on always scores > 0.  The only jumps that land on
a zero cell are those of row 1 and column 1 to the origin.  So "the walk stops after a gap jump" is built here as: the jump lands
on the path's first cell, in column 1, in row 1 (whose own pointer then leads to the origin) or in column 1024 (whose diagonal
neighbour in column 1023 scores 0), and the walk stops at the very next look.

Sizes: queries of 3 .. 40 residues, templates of 1026 .. 2046 columns (T counts the two sentinels, as in lean_cases), because the
lean instantiation is the one the dispatch takes beyond 1024 columns.  No GPU; of the project's modules only range_cases and
lean_cases are imported."""
import functools

import numpy as np

import lean_cases as lc
import range_cases as rc

ALPHA, BLOSUM = rc.load_blosum62()
ALL_NEGATIVE = rc.table_families(ALPHA, BLOSUM)["all_negative"]
TABLES = {"blosum62": BLOSUM, "all_negative": ALL_NEGATIVE}

NULLW, TAGMAX = 0xFFFF, 2047
P_MATCH, ORIGIN_DEL, ORIGIN_INS = 3 << 11, (2 << 11) | TAGMAX, (1 << 11) | TAGMAX
ZERO_MATCH, ZERO_BIT = P_MATCH | 1, 0x8000

# W scores below 0 against every residue but W, Y and F; C scores above 0 against C alone (BLOSUM62).  Over the other sixteen
# residues a row of W's is a row of zeros, and a lone C is the only positive cell of its row.
QUIET = "".join(ch for ch in ALPHA[:20] if ch not in "WYFC")


def _check_alphabet():
    tab = np.asarray(BLOSUM).astype(np.int64)
    w, c = ALPHA.index("W"), ALPHA.index("C")
    for ch in QUIET:
        assert tab[w, ALPHA.index(ch)] < 0 and tab[c, ALPHA.index(ch)] <= 0, ch
    assert tab[w, c] < 0 and tab[c, c] == 9


_check_alphabet()


def quiet_seq(seed, n):
    rng = np.random.RandomState(seed)
    return "".join(QUIET[k] for k in rng.randint(0, len(QUIET), n))


# ---- the word rule ---------------------------------------------------------------------------------------------------------

def encode_words(PQ, PT):
    """aln_device.h::encode_ptr, dialect 1, on whole planes -> uint16 (0xFFFF where the pointer is null)"""
    PQ, PT = np.asarray(PQ, np.int64), np.asarray(PT, np.int64)
    Q, T = PQ.shape
    i, j = np.meshgrid(np.arange(Q), np.arange(T), indexing="ij")
    W = np.where(PQ == i - 1, np.where(PT == j - 1, P_MATCH, (2 << 11) | (TAGMAX - PT)), (1 << 11) | (TAGMAX - PQ))
    return np.where((PQ < 0) | (PT < 0), NULLW, W).astype(np.uint16)


def lean_words(D, PQ, PT, forget_mark=False):
    """The words a lean build leaves, from the full build's planes.  forget_mark: interior zero cells keep the plain match word, as
    a kernel whose clip key lacks the mark would store them."""
    D = np.asarray(D)
    Q, T = D.shape
    full = encode_words(PQ, PT)
    W = full.copy()
    written = full != NULLW
    assert (D[~written] == 0).all()                                   # an untouched cell scores 0 and keeps 0xFFFF
    assert (full[written] < (1 << 13)).all()
    zero = written & (D == 0)
    zero[Q - 1, T - 1] = False                                        # the final cell is dp_corner_kernel's: never read by the walk
    edge = np.zeros((Q, T), bool)
    edge[1, :] = True
    edge[:, 1] = True
    assert (full[zero & ~edge] == P_MATCH).all()                      # the full build stores a match pointer where the clip won
    assert not (full[written & (D > 0)] == ZERO_MATCH).any()
    if not forget_mark:
        W[zero & ~edge] = ZERO_MATCH
    W[zero & edge] |= ZERO_BIT
    return W


def lean_score(w):
    w = int(w)
    return 0.0 if (w == NULLW or w == ZERO_MATCH or (w & ZERO_BIT)) else 1.0


def decode_word(w, i, j):
    """decode_ptr, dialect 1: bits 13 .. 15 are not looked at, nor is the tag of a match word"""
    prio, k = (w >> 11) & 3, TAGMAX - (w & TAGMAX)
    if prio == 3:
        return i - 1, j - 1
    if prio == 2:
        return i - 1, k
    return k, j - 1


def walk(W, best):
    """the local loop of optimal.h:79-105 on the words alone -> the list in list order, how the walk ended, where it stopped"""
    Q, T = W.shape
    lst = [(Q - 1, T - 1), best]
    q, t = best
    end = "loop"
    while q > 0:
        w = int(W[q, t])
        if w == NULLW:
            q, t = -1, -1
            end = "null"
            break
        pq, pt = decode_word(w, q, t)
        diag = (pq, pt) == (q - 1, t - 1)
        q, t = pq, pt
        if lean_score(W[q, t]) <= 0:
            end = "border" if (q == 0 or t == 0) else ("diag0" if diag else "gap0")
            break
        lst.append((q, t))
    if q != 0 and t != 0:
        lst.append((0, 0))
    return np.array(lst[::-1], dtype=np.int32).reshape(-1, 2), end, (q, t)


# ---- the pairs -------------------------------------------------------------------------------------------------------------

class Case:
    """kind: 'diag' (the walk stops on the diagonal at the zero cell `cell`), 'del' / 'ins' (a deletion / insertion jump lands on
    the path's first cell `cell`, and the walk stops at the next look), 'negative' (nothing scores: the lone seed)"""

    def __init__(self, name, kind, q, t, gi, ge, cell=None, table="blosum62"):
        self.name, self.kind, self.q, self.t, self.gi, self.ge, self.cell, self.table = name, kind, q, t, gi, ge, cell, table

    @property
    def T(self):
        return len(self.t) + 2

    @property
    def Q(self):
        return len(self.q) + 2


_HEAD_SRC = rc.random_seq(ALPHA, 8101, 44)
_HEAD_Q = lc.headed_copy(ALPHA, _HEAD_SRC, 40, 8102)
_HEAD_BASE = rc.random_seq(ALPHA, 8103, 2100) + _HEAD_SRC + rc.random_seq(ALPHA, 8104, 2200)
_HEAD_ROW, _HEAD_OFF = 4, 6          # under 11/1 the walk of _HEAD_Q stops at row 4, six columns into _HEAD_SRC (asserted by both tests)


def headed_case(col, T):
    """one headed copy (lean_cases.headed_copy), the template's window shifted so that the zero cell lies in column `col`"""
    s = 2100 + _HEAD_OFF - col
    return Case("col%d" % col, "diag", _HEAD_Q, _HEAD_BASE[s:s + T - 2], 11, 1, cell=(_HEAD_ROW, col))


def w_headed_case(name, k, col, n, T, seed):
    """k rows of W (all zero over QUIET), then a copy of the template's residues col .. col+n-1: the zero cell is (k, col)"""
    t = quiet_seq(seed, T - 2)
    return Case(name, "diag", "W" * k + t[col:col + n], t, 11, 1, cell=(k, col))


def last_column_case(T):
    """zero cell in column T-3: the path is the single cell (3, T-2), the seed, the only C against the only C"""
    t = quiet_seq(8110, T - 3) + "C"
    return Case("colT-3", "diag", "WWC", t, 11, 1, cell=(2, T - 3))


def jump_case(kind, k, col, T, seed, n=16):
    """k rows of W, a lone C that meets the template's only C in column `col` (score 9), then a piece of n residues reached by a
    deletion over 3 columns (kind 'del') or an insertion over 3 rows of W (kind 'ins'); gaps 3/1, so the jump pays (9 - 5 > 0)"""
    t = list(quiet_seq(seed, T - 2))
    t[col - 1] = "C"
    t = "".join(t)
    if kind == "del":
        q = "W" * k + "C" + t[col + 3:col + 3 + n]
    else:
        q = "W" * k + "C" + "WWW" + t[col:col + n]
    where = "row1" if k == 0 else "col%d" % col
    return Case("%s_%s" % (kind, where), kind, q, t, 3, 1, cell=(k + 1, col))


def negative_case(Q, T=1026):
    return Case("negative_Q%d" % Q, "negative", rc.random_seq(ALPHA, 8130 + Q, Q - 2), rc.random_seq(ALPHA, 8131 + Q, T - 2), 11, 1, table="all_negative")


@functools.lru_cache(maxsize=None)
def cases():
    out = [headed_case(c, T) for c, T in ((1, 1026), (7, 1026), (8, 1027), (511, 1026), (512, 1031), (1023, 1100), (1024, 1100),
                                          (1025, 1101), (1535, 1600), (1536, 2046))]
    out.append(last_column_case(2046))
    out.append(w_headed_case("row1", 1, 700, 20, 1026, 8111))
    out += [jump_case("del", 2, 1, 1026, 8120), jump_case("del", 0, 600, 1026, 8121), jump_case("del", 2, 1024, 1100, 8122),
            jump_case("ins", 2, 1, 1026, 8123), jump_case("ins", 0, 600, 1026, 8124), jump_case("ins", 2, 1024, 1100, 8125)]
    out += [negative_case(3), negative_case(4), negative_case(40)]
    assert len({c.name for c in out}) == len(out)
    return out


def case(name):
    return next(c for c in cases() if c.name == name)


RAGGED_T = (10, 515, 1026, 1031, 1537, 2046)


@functools.lru_cache(maxsize=None)
def ragged_pairs():
    """T in RAGGED_T beside one 2046-column pair: the owner of column T-2 falls in each group of each wave and at both ends of a
    16-byte chunk ((T-2) mod 8 = 0, 1, 0, 5, 7, 4).  The walks run through column T-2 (lean_cases.make_pair, from the end)."""
    out = []
    for k, T in enumerate(RAGGED_T):
        out.append(lc.make_pair(ALPHA, 8140 + 3 * k, 5 if T == 10 else (24, 33, 40, 17, 64)[k - 1], T - 2, at_end=True))
    out.append(lc.make_pair(ALPHA, 8170, 40, 2044, at_end=False))
    return out


# ---- the int64 reference ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference(q, t, table, gi, ge):
    """-> S, H, Optimal's list, on the int64 planes of range_cases (computed once per pair and gaps; nobody writes to them)"""
    S = rc.sim_int(q, t, ALPHA, TABLES[table])
    H, corner, _ = rc.affine_reference(S, rc.LOCAL, gi, ge)
    L = lc.reference_list(H, gi, ge)
    for a in (S, H, L):
        a.setflags(write=False)
    return S, H, L


def check_purpose(c, H, L):
    """The case holds what it is for, on a score plane H (any integer-valued array) and Optimal's list L of it."""
    H = np.asarray(H)
    L = [tuple(int(v) for v in p) for p in np.asarray(L).reshape(-1, 2)]
    Q, T = H.shape
    assert (Q, T) == (c.Q, c.T)
    if c.kind == "negative":
        assert H[:Q - 1, :T - 1].max() == 0 and L[-2] == (Q - 2, T - 2), c.name
        return
    first = L[1] if L[0] == (0, 0) else L[0]
    assert H[first] > 0
    if c.kind == "diag":
        assert L[0] == (0, 0) and (first[0] - 1, first[1] - 1) == c.cell, (c.name, first, c.cell)
        assert H[c.cell] == 0, c.name
        return
    assert first == c.cell, (c.name, first, c.cell)
    nxt = L[2] if L[0] == (0, 0) else L[1]
    if c.kind == "del":
        assert nxt[0] == first[0] + 1 and nxt[1] == first[1] + 4, (c.name, first, nxt)
    else:
        assert nxt[0] == first[0] + 4 and nxt[1] == first[1] + 1, (c.name, first, nxt)
    i, j = c.cell
    if i == 1 or j == 1:
        assert L[0] != (0, 0), c.name                                 # the landing cell's own pointer leads to the origin
    else:
        assert L[0] == (0, 0) and H[i - 1, j - 1] == 0, c.name        # its diagonal neighbour scores 0
