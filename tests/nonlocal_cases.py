"""Shared by tests/test_nonlocal_strip_rules.py (CPU) and tests/test_gpu_hits_align_nonlocal.py: the tie inputs, a numpy
restatement of what hit_global_kernel (csrc/search_align.h) does — the strip byte of every cell, the final cell's
pointer, the walk — computed from the oracle's D plane, and the census of the cases a set of lists went through."""
import numpy as np

import orc

NONLOCAL = [orc.GLOBAL_LOCAL, orc.GLOBAL, orc.LOCAL_GLOBAL, orc.SEMI_LOCAL]
TIE_GAPS = [(0, 0), (0, 1), (1, 5), (11, 1)]
TIE_SEEDS = range(6)
NEG = -(1 << 40)


def free_ends(mode):
    """(free_del, free_ins): which end gaps cost nothing (aasubalib.h:34-49,60-75)"""
    return mode in (orc.SEMI_LOCAL, orc.LOCAL_GLOBAL), mode in (orc.SEMI_LOCAL, orc.GLOBAL_LOCAL)


def low_complexity(seed, n, alpha):
    rs = np.random.RandomState(seed)
    if rs.randint(3) == 0:                                     # a repeat such as ACACAC... with a few point changes
        unit = "".join(alpha[x] for x in rs.randint(len(alpha), size=rs.randint(1, 4)))
        s = list((unit * (n // len(unit) + 1))[:n])
        for _ in range(rs.randint(0, 4)):
            s[rs.randint(n)] = alpha[rs.randint(len(alpha))]
        return "".join(s)
    return "".join(alpha[x] for x in rs.randint(len(alpha), size=n))


def tie_table(alpha):
    table = np.full((len(alpha), len(alpha)), -1, dtype=np.float32)
    np.fill_diagonal(table, 2)
    return table


def tie_sequences(alpha):
    qs, ts = [], []
    for seed in TIE_SEEDS:
        rs = np.random.RandomState(1000 + seed)
        qs.append(low_complexity(5000 + seed, rs.randint(20, 121), alpha))
        ts.append(low_complexity(7000 + seed, rs.randint(20, 121), alpha))
    return qs, ts


_ORACLE = {}


def oracle_pair(q, t, alpha, table, mode, gi, ge):
    """-> (D, score, list) of orc.dp_build + orc.optimal(..., False); computed once per input and left unchanged"""
    key = (q, t, alpha, table.tobytes(), mode, gi, ge)
    if key not in _ORACLE:
        S = orc.sim_submatrix(q, t, alpha, table)
        rc, D, PQ, PT = orc.dp_build(S, orc.Gap(mode, gi, ge))
        rc2, sc, pl = orc.optimal(D, PQ, PT, False)
        assert rc == 0 and rc2 == 0
        _ORACLE[key] = (D, sc, pl)
    return _ORACLE[key]


# ---- the kernel's rules, restated ---------------------------------------------------------------------------------------------
def strip_bytes(D, gi, ge):
    """strip[i][c], i = 2 .. Q-2, c = 1 .. T-2: bits 0-1 the move into (i, c+1) (0 match, 1 deletion, 2 insertion), bit 2 cell
    (i-1, c) as a deletion source (an earlier column of its row holds at least its key), bit 3 as an insertion source (an
    earlier row of its column does)."""
    Q, T = D.shape
    Di = D.astype(np.int64)
    cols = np.arange(T, dtype=np.int64)
    strip = np.zeros((Q, T), dtype=np.uint8)
    gmx = np.full(T, NEG, dtype=np.int64)                      # max over rows k <= i-2 of D[k][c] + ge k
    for i in range(2, Q - 1):
        m = Di[i - 1].copy()
        m[0] = m[T - 1] = NEG                                  # columns outside the interior are never sources
        A = m + ge * cols
        pv = np.concatenate(([NEG], np.maximum.accumulate(A)[:-1]))   # max of the keys left of the column
        e = pv - (ge * cols + gi - ge)
        f = gmx - (gi + ge * (i - 2))
        key = m + ge * (i - 1)
        b = np.where(m >= np.maximum(e, f), 0, np.where(e >= f, 1, 2)).astype(np.uint8)
        b |= np.where(pv >= A, 4, 0).astype(np.uint8)
        b |= np.where(gmx >= key, 8, 0).astype(np.uint8)
        strip[i] = b
        gmx = np.maximum(gmx, key)
    return strip


def final_pointer(D, gi, ge, free_del, free_ins):
    """the final cell's predecessor (dpmatrix.h:505-534): match, deletions k ascending, insertions k ascending, a later
    candidate wins only when strictly greater"""
    Q, T = D.shape
    Di = D.astype(np.int64)
    match = Di[Q - 2, T - 2]
    dl = [(Di[Q - 2, k] - (0 if free_del or k == T - 2 else gi + ge * (T - 3 - k)), -k) for k in range(1, T - 1)]
    dlv, dlc = max(dl)
    dlc = -dlc                                                 # value max, column min
    il = [(Di[k, T - 2] - (0 if free_ins else gi + ge * (Q - 3 - k)), -k) for k in range(1, Q - 2)]   # rows <= Q-3
    ilv, ilr = max(il) if il else (NEG, 0)
    ilr = -ilr
    score = max(match, dlv, ilv)
    if ilv > max(match, dlv):
        return ilr, T - 2, score
    if dlv > match:
        return Q - 2, dlc, score
    return Q - 2, T - 2, score


def walk(D, gi, ge, free_del, free_ins):
    """-> (score, list in list order) by the kernel's rules alone"""
    Q, T = D.shape
    strip = strip_bytes(D, gi, ge)
    i, j, score = final_pointer(D, gi, ge, free_del, free_ins)
    trav = [(Q - 1, T - 1), (i, j)]
    while i >= 2 and j >= 2:
        mv = strip[i, j - 1] & 3
        if mv == 0:
            i, j = i - 1, j - 1
        elif mv == 1:                                          # walk row i-1 leftwards from column j-2 to the first clear bit 2
            k = j - 2
            while strip[i, k] & 4:
                k -= 1
            assert k >= 1
            i, j = i - 1, k
        else:                                                  # walk column j-1 upwards from row i-2 to the first clear bit 3
            k = i - 2
            while strip[k + 1, j - 1] & 8:
                k -= 1
            assert k >= 1
            i, j = k, j - 1
        trav.append((i, j))
    trav.append((0, 0))
    return np.float32(score), np.array(trav[::-1], dtype=np.int32)


# ---- census -------------------------------------------------------------------------------------------------------------------
CENSUS_MIN = dict(final_del=40, final_ins=15, row1=50, col1=50, del_jumps=500, ins_jumps=400, ties=1000)


def top_two_equal(Di, i, j, gi, ge):
    """cell (i, j), i, j >= 2: do the two best of (match, best deletion, best insertion) tie?  (dpmatrix.h:447-486 restated)"""
    m = Di[i - 1, j - 1]
    k = np.arange(1, j - 1)
    e = (Di[i - 1, 1:j - 1] - gi - ge * (j - k - 2)).max() if j > 2 else NEG
    k = np.arange(1, i - 1)
    f = (Di[1:i - 1, j - 1] - gi - ge * (i - k - 2)).max() if i > 2 else NEG
    a = sorted([m, e, f], reverse=True)
    return a[0] == a[1]


def census(D, pl, gi, ge, into):
    """adds what the list pl = (0,0) .. (Q-1,T-1) went through to the counters of `into`"""
    Q, T = D.shape
    Di = D.astype(np.int64)
    assert (pl[0] == 0).all() and tuple(pl[-1]) == (Q - 1, T - 1) and len(pl) >= 3
    last = pl[-2]
    into["final_del"] += int(last[0] == Q - 2 and last[1] < T - 2)
    into["final_ins"] += int(last[1] == T - 2 and last[0] < Q - 2)
    first = pl[1]
    into["row1"] += int(first[0] == 1 and first[1] != 1)
    into["col1"] += int(first[1] == 1 and first[0] != 1)
    path = pl[1:-1]
    for a, b in zip(path[:-1], path[1:]):
        into["del_jumps"] += int(b[0] - a[0] == 1 and b[1] - a[1] > 1)
        into["ins_jumps"] += int(b[1] - a[1] == 1 and b[0] - a[0] > 1)
    for c in path:
        if c[0] >= 2 and c[1] >= 2:
            into["ties"] += int(top_two_equal(Di, int(c[0]), int(c[1]), gi, ge))


def new_census():
    return dict.fromkeys(CENSUS_MIN, 0)


def census_ok(c):
    return all(c[k] >= v for k, v in CENSUS_MIN.items())
