"""Shared by tests/test_lean_path_checker.py (CPU) and tests/test_gpu_lean_rebuild_ranges.py (GPU): what Optimal must report for
a local build, restated on the int64 planes of range_cases.affine_reference alone, the sequences of the lean-rebuild cases and
the gap settings of their rounds.  No GPU; of the project's modules only range_cases is imported.

A local list in list order: (0,0) if the walk ended inside the matrix, the aligned cells rising, the end cell (find_max), and the
final cell (Q-1, T-1).  Q and T count the sentinels.  A pair with an empty sequence has the list [seed, final cell], after
(0,0) when only the template is empty.
"""
import numpy as np

import range_cases as rc

VARIANT = dict(dp_variant_nw=2, dp_variant_r=2, dp_variant_x=8)      # the one instantiation that has a lean form
ROUNDS = [(11, 1), (3, 0), (40, 3), (11, 1)]                         # (gi, ge) of a refinement loop's rebuilds
ORACLE_MAX = (300, 700)                                              # residues: larger pairs go through the int64 reference
CHUNK = 8                                                            # cells of the 16-byte score chunk a lean build writes around column T-2

# (residues of the query, T = template residues + 2): column T-2 is 296 / 303 (inside group 0 of wave 0, first / last cell of a
# lane's chunk), 511 | 512 (groups 0 | 1 of wave 0), 1023 | 1024 (wave 0 | wave 1, whose first column the exchange delivers),
# 1535 | 1536 (groups of wave 1), 2046 (the last lane of all)
SHAPES = [(0, 5), (1, 298), (2, 305), (40, 298), (7, 513), (33, 514), (17, 1025), (40, 1026), (25, 1537), (3, 1538), (40, 2048), (0, 2048)]


def fits_oracle(q, t):
    return len(q) <= ORACLE_MAX[0] and len(t) <= ORACLE_MAX[1]


# ---- assertions on a batch (anything with kernel_name() and plane_bytes_per_cell()) and on Optimal's results ----------------------

def assert_lean(b):
    assert ",lean" in b.kernel_name(), b.kernel_name()
    assert b.plane_bytes_per_cell() == 2


def assert_full(b, bytes_per_cell=4):
    assert "lean" not in b.kernel_name(), b.kernel_name()
    assert b.plane_bytes_per_cell() == bytes_per_cell


def same_optimal(got, want):
    """scores bit for bit, status and every list exactly"""
    assert np.array_equal(np.ascontiguousarray(got[0], np.float32).view(np.uint32), np.ascontiguousarray(want[0], np.float32).view(np.uint32))
    assert np.array_equal(got[2], want[2])
    assert len(got[1]) == len(want[1])
    for p, (a, c) in enumerate(zip(got[1], want[1])):
        assert np.array_equal(a, c), p


# ---- Optimal on the reference planes ----------------------------------------------------------------------------------------

def find_max_cell(H):
    """Optimal's end cell (csrc/search_topk.hip, optimal.h:108-124): the seed (Q-2, T-2), replaced by the first strictly greater
    cell in row-major order; so the seed wins when it holds the maximum and when nothing is positive."""
    H = np.asarray(H)
    Q, T = H.shape
    seed = (Q - 2, T - 2)
    if Q <= 2 or T <= 2:
        return seed
    sub = H[1:Q - 1, 1:T - 1]
    k = int(np.argmax(sub))                                          # the first maximal cell, row-major
    best = sub.flat[k]
    if best <= 0 or H[seed] == best:
        return seed
    i, j = divmod(k, T - 2)
    return (i + 1, j + 1)


def predecessor(H, i, j, gi, ge):
    """The cell the recurrence took (i, j)'s value from (local build, interior cell): the diagonal cell first, then the deletions
    (row i-1, column k ascending), then the insertions (column j-1, row k ascending); only a strictly larger candidate replaces
    an earlier one.  Row 1 and column 1 start at the origin."""
    if i == 1 or j == 1:
        return 0, 0
    Q, T = H.shape
    best, at = int(H[i - 1, j - 1]), (i - 1, j - 1)
    if j >= 3:
        ks = np.arange(1, j - 1, dtype=np.int64)
        cand = H[i - 1, 1:j - 1] - rc.gap_cost(ks, j, T - 1, True, gi, ge)
        k = int(np.argmax(cand))
        if cand[k] > best:
            best, at = int(cand[k]), (i - 1, k + 1)
    if i >= 3:
        ks = np.arange(1, i - 1, dtype=np.int64)
        cand = H[1:i - 1, j - 1] - rc.gap_cost(ks, i, Q - 1, True, gi, ge)
        k = int(np.argmax(cand))
        if cand[k] > best:
            best, at = int(cand[k]), (k + 1, j - 1)
    return at


def reference_list(H, gi, ge):
    """The local loop of optimal.h:79-105 on the reference plane -> int32 [n, 2] in list order."""
    H = np.asarray(H, np.int64)
    Q, T = H.shape
    q, t = find_max_cell(H)
    lst = [(Q - 1, T - 1), (q, t)]
    while q > 0:
        if t <= 0:                                                   # an empty template: the seed's column holds no cell
            q, t = -1, -1
            break
        q, t = predecessor(H, q, t, gi, ge)
        if H[q, t] <= 0:
            break
        lst.append((q, t))
    if q != 0 and t != 0:
        lst.append((0, 0))
    return np.array(lst[::-1], np.int32).reshape(-1, 2)


def check_local_list(S, H, pairs, gi, ge):
    """Raises AssertionError unless `pairs` is what Optimal reports for the local build with planes S, H (int64, of
    range_cases.sim_int / affine_reference)."""
    S, H = np.asarray(S, np.int64), np.asarray(H, np.int64)
    Q, T = H.shape
    L = [(int(a), int(b)) for a, b in np.asarray(pairs).reshape(-1, 2)]
    end = find_max_cell(H)
    assert len(L) >= 2 and L[-1] == (Q - 1, T - 1), ("final cell", L[-2:])
    assert L[-2] == end, ("end cell", L[-2], end)
    if Q == 2 or T == 2:                                             # an empty sequence: nothing to walk; the seed of an empty
        head = [(0, 0)] if (T == 2 and Q > 2) else []                # template lies in column 0, which holds no cell at all
        assert L == head + [end, (Q - 1, T - 1)], ("empty pair", L)
        return
    inner = L[:-1]
    origin = inner[0] == (0, 0)
    if origin:
        inner = inner[1:]
    assert len(inner) >= 1, L
    for (i, j) in inner:
        assert 1 <= i <= Q - 2 and 1 <= j <= T - 2, ("outside the interior", (i, j))
    i0, j0 = inner[0]
    assert origin == (i0 > 1 and j0 > 1), ("(0,0) goes with a start inside the matrix", inner[0], origin)
    if H[end] <= 0:                                                  # nothing scores: the lone seed
        assert inner == [end], ("all-zero case", inner)
        return
    total = 0
    for n, (i, j) in enumerate(inner):
        assert H[i, j] > 0, ("a listed cell scores <= 0", (i, j), int(H[i, j]))
        total += int(S[i, j])
        if n == 0:
            continue
        pi, pj = inner[n - 1]
        assert pi < i and pj < j, ("not strictly rising", (pi, pj), (i, j))
        assert pi == i - 1 or pj == j - 1, ("neither diagonal, deletion nor insertion", (pi, pj), (i, j))
        total -= int(rc.gap_cost(pj, j, T - 1, True, gi, ge)) + int(rc.gap_cost(pi, i, Q - 1, True, gi, ge))
        assert predecessor(H, i, j, gi, ge) == (pi, pj), ("not the recurrence's predecessor", (i, j), (pi, pj))
    # the walk really stopped at the first cell: what it came from scores nothing (row 1 and column 1 come from the origin)
    pi, pj = predecessor(H, i0, j0, gi, ge)
    assert i0 == 1 or j0 == 1 or H[pi, pj] <= 0, ("stopped early", inner[0], (pi, pj), int(H[pi, pj]))
    assert total == H[end], ("path sum", total, int(H[end]))


def stale_sign_cells(Ha, Hb):
    """Interior cells a lean build does not write (outside row Q-2 and outside the chunk of column T-2) whose sign (> 0) differs
    between two builds: where a reader of the stale score plane would go wrong."""
    Q, T = Ha.shape
    if Q < 4 or T < 4:
        return 0
    diff = (Ha > 0) != (Hb > 0)
    mask = np.zeros((Q, T), bool)
    mask[1:Q - 2, 1:T - 1] = True
    c0 = (T - 2) // CHUNK * CHUNK
    mask[:, c0:c0 + CHUNK] = False
    return int(np.count_nonzero(diff & mask))


def longest_jumps(pairs):
    """-> (largest column jump of a deletion, largest row jump of an insertion) between consecutive aligned cells"""
    p = np.asarray(pairs).reshape(-1, 2)
    if len(p) < 4:
        return 0, 0
    inner = p[1:-1] if (p[0] == 0).all() else p[:-1]
    d = np.diff(inner, axis=0)
    if len(d) == 0:
        return 0, 0
    return int(d[:, 1].max()) - 1, int(d[:, 0].max()) - 1


# ---- sequences --------------------------------------------------------------------------------------------------------------

def mutated(alphabet, s, seed, every=6, first=3):
    """s with every `every`-th residue replaced by a random one"""
    noise = rc.random_seq(alphabet, seed, max(len(s), 1))
    out = list(s)
    for k in range(first, len(s), every):
        out[k] = noise[k]
    return "".join(out)


_BLOSUM = {}


def _self_and_worst(alphabet):
    if not _BLOSUM:
        a, tab = rc.load_blosum62()
        assert a == alphabet
        _BLOSUM["tab"] = np.asarray(tab).astype(np.int64)
    tab = _BLOSUM["tab"]

    def worst(ch, avoid=""):
        """the residue that scores lowest against ch and does not score against any residue of `avoid`"""
        cost = tab[alphabet.index(ch), :20].copy()
        for a in avoid:
            cost += 4 * np.maximum(tab[alphabet.index(a), :20] + 1, 0)
        return alphabet[int(np.argmin(cost))]
    return (lambda ch: int(tab[alphabet.index(ch), alphabet.index(ch)])), worst


def headed_copy(alphabet, src, n, seed, every=6):
    """A noisy copy of src (n + 4 residues) that is n residues long and whose alignment with src begins with a weak head, so that
    Optimal's walk ends INSIDE the matrix at a cell whose sign depends on the gaps (BLOSUM62 scores):
      2 residues that score badly | a small piece (self-score 8 .. 14) | 2 residues of src skipped | a mismatch |
      a larger piece (24 .. 45) | 2 skipped | a mismatch | the body, every `every`-th residue replaced.
    With gaps 3/0 everything chains; with 11/1 the small piece does not pay for its gap (8 .. 14 < 12 + 3); with 40/3 neither
    piece does.  The cells next to the two gaps are positive under one setting and zero under another: a walk that reads them
    from a plane left by another setting stops too early or too late.  Copies of fewer than 20 residues get the small piece only."""
    assert len(src) == n + 4
    score, worst = _self_and_worst(alphabet)
    out, k = [], 0

    def piece(lo):
        nonlocal k
        got = 0
        while got < lo:
            out.append(src[k])
            got += score(src[k])
            k += 1

    def gap():
        nonlocal k
        k += 2
        out.append(worst(src[k], src[k - 3:k] + src[k + 1:k + 2]))  # (it must not fit a skipped residue or a neighbour instead)
        k += 1

    for _ in range(2 if n >= 12 else 1):
        out.append(worst(src[k]))
        k += 1
    piece(8)
    gap()
    if n >= 20:
        piece(24)
        gap()
    else:
        k += 2                                                       # (short copies: the second gap closes the body instead)
        out.append(src[k])
        k += 1
    body = mutated(alphabet, src[k:], seed, every=every)
    q = "".join(out) + body
    assert len(q) == n, (len(q), n)
    return q


def make_pair(alphabet, seed, qlen, tlen, at_end):
    """template random; query = a headed noisy copy (headed_copy) of a piece from its end or its middle, so the walk is long, ends
    inside the matrix and, from the template's end, runs through column T-2"""
    t = rc.random_seq(alphabet, seed, tlen)
    if qlen == 0:
        return "", t
    if qlen < 7:
        start = tlen - qlen if at_end else (tlen - qlen) // 2
        return mutated(alphabet, t[start:start + qlen], seed + 1), t
    start = tlen - qlen - 4 if at_end else (tlen - qlen - 4) // 2
    return headed_copy(alphabet, t[start:start + qlen + 4], qlen, seed + 1), t


def shape_pairs(alphabet):
    """One pair per entry of SHAPES -> list of (q, t)"""
    out = []
    for k, (ql, T) in enumerate(SHAPES):
        out.append(("", "ACD") if (ql, T) == (0, 5) else make_pair(alphabet, 9100 + 3 * k, ql, T - 2, at_end=(k % 2 == 0)))
    return out


def long_pairs(alphabet, homolog_pair):
    """The long-query shapes, name -> (q, t); homolog_pair is aln_amd.synth's.
      ins60: the template lacks a 60-residue block of the query (an insertion jump over 60 rows once gaps are cheap)
      del70: the query lacks the template's residues 991 .. 1060 (a deletion jump across column 1024, the wave boundary)
      end700: the query is a mutated copy of the template's last 700 residues (the best cell is the seed)
      q14 / q15 / q16: row Q-2 is the last row of the first 16-row ring cycle, the first and the second row of the next"""
    out = {}
    out["hom2046"] = homolog_pair(4243, 2046)
    t = rc.random_seq(alphabet, 7098, 2046)                          # (a homolog starts in row 1: this one starts inside)
    out["head2046"] = (headed_copy(alphabet, t + rc.random_seq(alphabet, 7099, 4), 2046, 7100), t)
    q = rc.random_seq(alphabet, 7101, 2046)
    out["2046x300"] = (q, headed_copy(alphabet, q[900:1204], 300, 7102))
    t = rc.random_seq(alphabet, 7103, 1030)
    out["1030x1030"] = (headed_copy(alphabet, t[:400] + t[404:] + rc.random_seq(alphabet, 7104, 8), 1030, 7105), t)
    t = rc.random_seq(alphabet, 7106, 1500)
    out["end700"] = (headed_copy(alphabet, t[796:], 700, 7107, every=9), t)
    a, b, c = rc.random_seq(alphabet, 7108, 570), rc.random_seq(alphabet, 7109, 60), rc.random_seq(alphabet, 7110, 570)
    out["ins60"] = (a + b + c, headed_copy(alphabet, a[16:] + c[:-20], 1100, 7111, every=9))
    t = rc.random_seq(alphabet, 7112, 1400)
    out["del70"] = (headed_copy(alphabet, t[426:990] + t[1060:], 900, 7113, every=9), t)
    for n in (14, 15, 16):
        out["q%d" % n] = make_pair(alphabet, 7120 + 3 * n, n, 1024, at_end=(n != 15))
    want = {"hom2046": (2046, 2046), "2046x300": (2046, 300), "1030x1030": (1030, 1030), "end700": (700, 1500), "ins60": (1200, 1100),
            "del70": (900, 1400), "q14": (14, 1024), "q15": (15, 1024), "q16": (16, 1024), "head2046": (2046, 2046)}
    for name, (q, t) in out.items():
        assert (len(q), len(t)) == want[name], (name, len(q), len(t))
    return out


# at most four batches for the rounds: the ragged short shapes, then the long ones by size
LONG_BATCHES = [("q14", "q15", "q16", "2046x300", "end700"), ("1030x1030", "ins60", "del70"), ("hom2046", "head2046")]


def stale_settings(has_short):
    """round r of ROUNDS (1 ..) -> the setting of the last FULL build before it, whose scores a lean build of round r leaves in the
    plane; None where the round's build is full.  A batch with pairs the oracle reaches reads its cells after round 1, so its
    round 2 is full; every other round follows an Optimal and is lean."""
    return {1: ROUNDS[0], 2: None, 3: ROUNDS[2]} if has_short else {1: ROUNDS[0], 2: ROUNDS[0], 3: ROUNDS[0]}


# ---- what a reader of the stale score plane would report -----------------------------------------------------------------------

def stale_list(H, H_stale, gi, ge):
    """reference_list with the pointers of the right plane H but the stop test `score <= 0` read from the plane a lean build
    leaves behind: H_stale everywhere except row Q-2 and the chunk of column T-2, which a lean build writes.  Where this differs
    from reference_list(H), a traceback that looked at the score plane after a lean build is caught."""
    H, seen = np.asarray(H, np.int64), np.array(H_stale, np.int64)
    Q, T = H.shape
    if Q > 2 and T > 2:
        seen[Q - 2, :] = H[Q - 2, :]
        c0 = (T - 2) // CHUNK * CHUNK
        seen[1:Q - 1, c0:c0 + CHUNK] = H[1:Q - 1, c0:c0 + CHUNK]
    q, t = find_max_cell(H)
    lst = [(Q - 1, T - 1), (q, t)]
    while q > 0:
        if t <= 0:
            q, t = -1, -1
            break
        q, t = predecessor(H, q, t, gi, ge)
        if seen[q, t] <= 0:
            break
        lst.append((q, t))
    if q != 0 and t != 0:
        lst.append((0, 0))
    return np.array(lst[::-1], np.int32).reshape(-1, 2)
