"""Shared by tests/test_value_range_reference.py (CPU) and tests/test_gpu_value_ranges.py (GPU): a plain int64 restatement
of the constant-affine recurrence, and the generators of scoring systems and sequences that sit near the value-range limits
of the kernels.  Nothing here imports aln_amd: the reference cannot share an integer width, a "minus infinity" or a wrap-around
with any kernel.

The recurrence (oracle/aln_oracle.cpp build_forward, Q and T counted WITH the sentinels '^' and '$'):
  H[0,0] = 0; row 0, column 0, the last row and the last column stay 0 except the corner (Q-1, T-1)
  H[1,1] = S[1,1];  H[1,j] = S[1,j] - del(0, j);  H[i,1] = S[i,1] - ins(0, i)
  H[i,j] = S[i,j] + max(H[i-1,j-1],  max_{1<=k<=j-2} H[i-1,k] - del(k, j),  max_{1<=k<=i-2} H[k,j-1] - ins(k, i))
  corner = S + max(H[Q-2,T-2],  max_{1<=k<=T-2} H[Q-2,k] - del(k, T-1),  max_{1<=k<=Q-2} H[k,T-2] - ins(k, Q-1))
  del(t1, t2): 0 when t2 - t1 < 2, 0 when deletions at the ends are free and t1 == 0 or t2 == T-1, else gi + ge (t2 - t1 - 2)
  ins(q1, q2): the same along the query.  Local builds clip every interior and corner value at 0.
A pair with an empty sequence (Q == 2 or T == 2) has one cell: the corner, reached from (0,0) by one gap, never clipped.
"""
import os

import numpy as np

GLOBAL_LOCAL, GLOBAL, LOCAL_GLOBAL, LOCAL, SEMI_LOCAL = 0, 1, 2, 3, 4
ALIGN_TYPES = (GLOBAL_LOCAL, GLOBAL, LOCAL_GLOBAL, LOCAL, SEMI_LOCAL)
EXACT_LIMIT = 1 << 24          # fp32 holds every integer of smaller magnitude exactly
BLOSUM_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "BLOSUM62")


def free_ends(align_type):
    """-> (deletions at the template's ends are free, insertions at the query's ends are free): orc.deletion / orc.insertion"""
    return align_type in (LOCAL, SEMI_LOCAL, LOCAL_GLOBAL), align_type in (LOCAL, SEMI_LOCAL, GLOBAL_LOCAL)


def gap_cost(a, b, last, free, gi, ge):
    """Cost of a gap between positions a < b of a sequence whose last index is `last` (arrays or scalars, int64)."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    ln = b - a - 1
    cost = gi + ge * (ln - 1)
    zero = ln < 1
    if free:
        zero = zero | (a == 0) | (b == last)
    return np.where(zero, 0, cost)


def sim_int(q, t, alphabet, table):
    """Similarity plane of '^'+q+'$' against '^'+t+'$' in int64 (sentinel rows and columns 0).  The table must be integral."""
    tab = np.asarray(table)
    ti = tab.astype(np.int64)
    assert np.array_equal(ti.astype(tab.dtype), tab), "integral tables only"
    idx = {ch: k for k, ch in enumerate(alphabet)}
    qi = np.array([idx[c] for c in q], np.int64)
    tj = np.array([idx[c] for c in t], np.int64)
    S = np.zeros((len(q) + 2, len(t) + 2), np.int64)
    if len(q) and len(t):
        S[1:-1, 1:-1] = ti[qi[:, None], tj[None, :]]
    return S


def affine_reference(S, align_type, gi, ge):
    """-> H (int64, every cell), corner score, local maximum (find_max: the largest value of H[:Q-1, :T-1]).
    Row by row: the deletion term of row i is a running maximum over H[i-1,k] + ge k, the insertion term a running maximum
    per column over H[k,j-1] + ge k.  Asserts |value| < 2^24 for every cell and every candidate it forms."""
    S = np.asarray(S, np.int64)
    gi, ge = int(gi), int(ge)
    assert gi == gi and ge == ge
    Q, T = S.shape
    local = align_type == LOCAL
    fdel, fins = free_ends(align_type)
    H = np.zeros((Q, T), np.int64)
    big = 0
    if Q == 2:
        H[1, T - 1] = S[1, T - 1] - int(gap_cost(0, T - 1, T - 1, fdel, gi, ge))
    elif T == 2:
        H[Q - 1, 1] = S[Q - 1, 1] - int(gap_cost(0, Q - 1, Q - 1, fins, gi, ge))
    else:
        clip = (lambda x: np.maximum(x, 0)) if local else (lambda x: x)
        NEG = -(1 << 40)
        js = np.arange(2, T - 1, dtype=np.int64)                 # interior columns 2 .. T-2
        H[1, 1] = clip(S[1, 1])
        H[1, 2:T - 1] = clip(S[1, 2:T - 1] - gap_cost(0, js, T - 1, fdel, gi, ge))
        ii = np.arange(2, Q - 1, dtype=np.int64)
        H[2:Q - 1, 1] = clip(S[2:Q - 1, 1] - gap_cost(0, ii, Q - 1, fins, gi, ge))
        ks = np.arange(1, T - 1, dtype=np.int64)                 # source columns 1 .. T-2
        colmax = np.full(T, NEG, np.int64)                       # max over rows k <= i-2 of H[k, c] + ge k
        for i in range(2, Q - 1):
            if i >= 3:
                colmax[1:T - 1] = np.maximum(colmax[1:T - 1], H[i - 2, 1:T - 1] + ge * (i - 2))
            prev = H[i - 1]
            if T > 3:
                cand = prev[1:T - 2].copy()                                          # diagonal: H[i-1, j-1], j = 2 .. T-2
                if T > 4:
                    run = np.maximum.accumulate(prev[1:T - 3] + ge * ks[:T - 4])      # k = 1 .. j-2 for j = 3 .. T-2
                    dele = run - gi - ge * (js[1:] - 2)
                    cand[1:] = np.maximum(cand[1:], dele)
                    big = max(big, int(np.abs(dele).max()))
                if i >= 3:
                    inse = colmax[1:T - 2] - gi - ge * (i - 2)
                    cand = np.maximum(cand, inse)
                    big = max(big, int(np.abs(inse).max()))
                raw = cand + S[i, 2:T - 1]
                big = max(big, int(np.abs(raw).max()))
                H[i, 2:T - 1] = clip(raw)
        # the corner: every cell of row Q-2 by a deletion to T-1, every cell of column T-2 by an insertion to Q-1
        best = H[Q - 2, T - 2]
        d = H[Q - 2, 1:T - 1] - gap_cost(ks, T - 1, T - 1, fdel, gi, ge)
        qs = np.arange(1, Q - 1, dtype=np.int64)
        n = H[1:Q - 1, T - 2] - gap_cost(qs, Q - 1, Q - 1, fins, gi, ge)
        best = max(int(best), int(d.max()), int(n.max()))
        big = max(big, int(np.abs(d).max()), int(np.abs(n).max()))
        H[Q - 1, T - 1] = clip(best + S[Q - 1, T - 1])
    big = max(big, int(np.abs(H).max()))
    assert big < EXACT_LIMIT, "case leaves fp32's exact integer range: |value| reaches %d" % big
    return H, int(H[Q - 1, T - 1]), int(H[:Q - 1, :T - 1].max())


def reference_score(H, align_type):
    """What Optimal reports: find_max for local alignments, the corner for the four other align types."""
    Q, T = H.shape
    return int(H[:Q - 1, :T - 1].max()) if align_type == LOCAL else int(H[Q - 1, T - 1])


def pointers_consistent(H, PQ, PT, S, align_type, gi, ge):
    """Every written cell's score follows from the cell its pointer names: H[i,j] == H[PQ,PT] + S[i,j] - gap(PQ,PT -> i,j),
    clipped at 0 in local builds (a clipped cell is a local start and points at the diagonal cell, or at the origin from row 1
    and column 1); untouched cells carry (-1,-1) and 0.
    -> number of cells that violate this (0 for a consistent build)."""
    H = np.asarray(H).astype(np.int64)
    S = np.asarray(S).astype(np.int64)
    PQ, PT = np.asarray(PQ).astype(np.int64), np.asarray(PT).astype(np.int64)
    Q, T = H.shape
    gi, ge = int(gi), int(ge)
    local = align_type == LOCAL
    fdel, fins = free_ends(align_type)
    bad = 0
    for r0 in range(0, Q, 512):                                  # in blocks of rows: the index arrays of a 8192 x 8192 plane are large
        r1 = min(r0 + 512, Q)
        written = np.zeros((r1 - r0, T), bool)
        if Q == 2 or T == 2:
            if r1 == Q:
                written[Q - 1 - r0, T - 1] = True
        else:
            written[max(r0, 1) - r0:min(r1, Q - 1) - r0, 1:T - 1] = True
            if r1 == Q:
                written[Q - 1 - r0, T - 1] = True
        h, pq_, pt_ = H[r0:r1], PQ[r0:r1], PT[r0:r1]
        bad += int(np.count_nonzero((~written) & ((pq_ != -1) | (pt_ != -1) | (h != 0))))
        i, j = np.nonzero(written)
        pq, pt = pq_[i, j], pt_[i, j]
        i = i + r0
        inb = (pq >= 0) & (pq < i) & (pt >= 0) & (pt < j)
        bad += int(np.count_nonzero(~inb))
        i, j, pq, pt = i[inb], j[inb], pq[inb], pt[inb]
        # a predecessor is the diagonal cell, a cell of the previous row (deletion) or of the previous column (insertion);
        # the single cell of an empty pair takes its gap from (0,0) along the non-empty sequence
        dele = gap_cost(pt, j, T - 1, fdel, gi, ge)
        inse = gap_cost(pq, i, Q - 1, fins, gi, ge)
        shape_ok = (pq == i - 1) | (pt == j - 1)
        bad += int(np.count_nonzero(~shape_ok))
        gap = np.where(pq == i - 1, dele, inse)
        want = H[pq, pt] + S[i, j] - gap
        if local and Q > 2 and T > 2:
            want = np.maximum(want, 0)
            # a local start (score clipped to 0) keeps the pointer the scan began with, since only a strictly larger candidate
            # replaces it: the origin in row 1 and column 1, the diagonal cell elsewhere
            start = H[i, j] == 0
            first = (i == 1) | (j == 1)
            ok = np.where(first, (pq == 0) & (pt == 0), (pq == i - 1) & (pt == j - 1))
            bad += int(np.count_nonzero(start & ~ok))
        bad += int(np.count_nonzero(shape_ok & (want != H[i, j])))
    return bad


# ---- scoring systems -----------------------------------------------------------------------------------------------------

def load_blosum62():
    """-> alphabet (24 letters), float32 table; the parser of orc.load_blosum restated so that this file stands alone"""
    lines = open(BLOSUM_PATH).read().split("\n")
    k = 0
    while lines[k].startswith("#"):
        k += 1
    alphabet = "".join(ch for ch in lines[k] if ch not in " \n")
    n = len(alphabet)
    toks = " ".join(lines[k + 1:]).split()
    rows = [[float(toks[i * (n + 1) + 1 + j]) for j in range(n)] for i in range(n)]
    return alphabet, np.array(rows, np.float32)


def scaled(table, k):
    return (np.asarray(table, np.float32) * np.float32(k)).astype(np.float32)


def with_outlier(alphabet, table, a, b, value):
    t = np.array(table, np.float32)
    t[alphabet.index(a), alphabet.index(b)] = value
    return t


def table_families(alphabet, table):
    """name -> table over BLOSUM62's alphabet.  maxs (the largest |entry|) of each: see maxs()."""
    n = len(alphabet)
    eye = np.eye(n, dtype=np.float32)
    return {
        "blosum62": np.array(table, np.float32),
        "blosum62x9": scaled(table, 9),
        "blosum62x-1": scaled(table, -1),
        "all_negative": (np.asarray(table, np.float32) - 12).astype(np.float32),
        "all_zero": np.zeros((n, n), np.float32),
        "constant+3": np.full((n, n), 3, np.float32),
        "identity5": (5 * eye - 5 * (1 - eye)).astype(np.float32),
        "outlier_WW_2047": with_outlier(alphabet, table, "W", "W", 2047),
        "outlier_WW_2048": with_outlier(alphabet, table, "W", "W", 2048),
    }


GAP_FAMILIES = [(0, 0), (0, 1), (40, 0), (1, 5), (11, 1)]          # (gi, ge): zero, gi = 0, large gi with ge = 0, ge > gi, usual


def maxs(table):
    return int(np.abs(np.asarray(table)).max())


# ---- sequences ------------------------------------------------------------------------------------------------------------

def best_residue(alphabet, table):
    """The residue whose self-score is the table's largest entry, if there is one on the diagonal (W for BLOSUM62)."""
    d = np.diag(np.asarray(table))
    return alphabet[int(np.argmax(d))]


def worst_partner(alphabet, table, a):
    """The residue that scores lowest against residue a (first such)."""
    return alphabet[int(np.argmin(np.asarray(table)[alphabet.index(a)]))]


def random_seq(alphabet, seed, n):
    rng = np.random.RandomState(seed)
    letters = alphabet[:20]                                   # the 20 amino acids; B, Z, X, * stay out of random data
    return "".join(letters[k] for k in rng.randint(0, len(letters), n))


def run(ch, n):
    return ch * n


def shaped_pairs(alphabet, table, n, m, seed=1):
    """The sequence shapes of the value-range tests at lengths n (query) and m (template) -> list of (name, q, t)."""
    a = best_residue(alphabet, table)
    w = worst_partner(alphabet, table, a)
    r = random_seq(alphabet, seed, max(n, m))
    return [
        ("run_vs_run", run(a, n), run(a, m)),
        ("run_vs_worst", run(a, n), run(w, m)),
        ("identical", r[:min(n, m)], r[:min(n, m)]),
        ("random", random_seq(alphabet, seed + 1, n), random_seq(alphabet, seed + 2, m)),
        ("run_vs_1", run(a, n), a),
        ("2_vs_run", a + w, run(a, m)),
        ("empty_q", "", run(a, m)),
        ("empty_t", run(a, n), ""),
        ("empty_both", "", ""),
    ]


def ragged_batch(alphabet, table, seed, maxlen=200):
    """About 16 ragged pairs of at most `maxlen` residues: empty, 1-residue, run-vs-run, run-vs-worst, identical, random."""
    a = best_residue(alphabet, table)
    w = worst_partner(alphabet, table, a)
    rng = np.random.RandomState(seed)
    ident = random_seq(alphabet, seed + 100, maxlen // 2)
    pairs = [("", ""), ("", run(a, 7)), (run(a, 9), ""), (a, a), (a, w), (a, run(a, 33)), (run(w, 40), a + w),
             (run(a, 70), run(a, 64)), (run(a, 31), run(w, 45)), (ident, ident), (ident[:50], ident[3:60]),
             (run(a, maxlen), run(a, maxlen))]
    for k in range(4):
        n, m = int(rng.randint(2, maxlen)), int(rng.randint(2, maxlen))
        pairs.append((random_seq(alphabet, seed + 10 + k, n), random_seq(alphabet, seed + 20 + k, m)))
    return pairs


# ---- the predicates, restated as arithmetic (Q, T with sentinels; the batch's maxQ / maxT) --------------------------------

def lhs_tag11(ms, gi, ge, Q, T):
    return (ms + ge) * (Q + T) + gi + ms                     # < 65536, Q, T <= 2048


def lhs_tag12(ms, gi, ge, Q, T):
    return ms * min(Q, T) + 2 * gi + 3 * ge * max(Q, T) + ms, gi + ge * max(Q, T)      # < 100000 and < 16000, Q, T <= 4096


def lhs_h16(ms, Q, T):
    return ms * min(Q, T)                                     # < 65536


def lhs_key16(ms, gi, ge, Q, T):
    L = max(Q, T)
    return ms * min(Q, T) + ge * L + ms, gi + ge * L + ms     # < 32767 and < 8000


def lhs_int(ms, gi, ge, Q, T):
    return (ms + ge) * (Q + T) + gi + ms                     # < 2^23 with gi <= 65536, ge <= 4096, row <= 8192


def lhs_packed(ms, gi, ge, Q, T):
    T = min(T, 2048)
    L = max(Q, T)
    return ms * min(Q, T) + ge * L + ms, ge * L + gi + ms, ms   # < 30000, < 8000, < 2048


def lhs_score32(ms, gi, ge, Q, T):
    return (ms + ge) * (Q + min(T, 2048)) + gi + ms           # < 2^23
