"""The reference of tests/test_gpu_search_ranges.py (tests/search_cases.py), pinned to the oracle on small pairs, and the
construction of its cases, asserted here so that no GPU test passes vacuously: the cases do lie on the stated sides of the
kernels' bounds, their rows do tie, their top K do hold negative scores, their planes do hold a maximum of 0 and maxima in
several cells, and their shuffle scores do have squares beyond 32 bits.  No GPU."""
import math

import numpy as np
import pytest

import aln_amd
import orc
import range_cases as rc
import search_cases as sc

SMALL_SYSTEMS = [("blosum62", 11, 1), ("blosum62x-1", 1, 5), ("constant+3", 0, 0)]
NEGATIVE_FREE = ("constant+3", "all_zero")                           # tables without a negative entry under free gaps: no score < 0
Z_SEED = 2024


def small_set():
    """the shapes of a case's set at 40 x 57, without the two long templates: every pair is at most 40 x 60"""
    qs, ts = sc.sequences(sc.Case("small", None, 0, 0, 40, 57))
    return qs, ts[:8]


def oracle(q, t, table, mode, gi, ge):
    S = orc.sim_submatrix(q, t, sc.ALPHA, sc.TABLES[table])
    err, D, PQ, PT = orc.dp_build(S, orc.Gap(mode, gi, ge))
    err2, score, pl = orc.optimal(D, PQ, PT, mode == rc.LOCAL)
    assert err == 0 and err2 == 0
    return D, float(score), pl


def find_max_of(D):
    """optimal.h:108-124 over the oracle's plane: the seed (Q-2, T-2), replaced by the first strictly greater cell of rows
    0 .. Q-2 and columns 0 .. T-2 in row-major order"""
    Q, T = D.shape
    sub = D[:Q - 1, :T - 1]
    first = np.unravel_index(np.argmax(sub), sub.shape)
    return (int(first[0]), int(first[1])) if D[Q - 2, T - 2] < sub.max() else (Q - 2, T - 2)


_DENSE = {}


def dense(name, mode):
    if (name, mode) not in _DENSE:
        c = sc.CASES[name]
        qs, ts = sc.sequences(c)
        _DENSE[(name, mode)] = sc.dense_reference(qs, ts, c.table, mode, c.gi, c.ge)
    return _DENSE[(name, mode)]


# ---- 1. the reference equals the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
@pytest.mark.parametrize("system", SMALL_SYSTEMS, ids=lambda s: s[0])
def test_dense_reference_equals_the_oracle(system, mode):
    table, gi, ge = system
    qs, ts = small_set()
    scores, ends = sc.dense_reference(qs, ts, table, mode, gi, ge)
    assert scores.dtype == np.int64 and scores.shape == (len(qs), len(ts)) and ends.shape == (len(qs), len(ts), 2)
    for i, q in enumerate(qs):
        for j, t in enumerate(ts):
            D, score, pl = oracle(q, t, table, mode, gi, ge)
            assert float(scores[i, j]) == score, (i, j)
            if mode == rc.LOCAL:
                assert tuple(ends[i, j]) == find_max_of(D) == (int(pl[-2][0]), int(pl[-2][1])), (i, j)
            else:
                assert tuple(ends[i, j]) == (len(q) + 1, len(t) + 1) == tuple(pl[-1]), (i, j)
                sc2, pl2 = sc.nonlocal_reference(q, t, table, mode, gi, ge)
                assert float(sc2) == score and np.array_equal(pl2, pl)


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
@pytest.mark.parametrize("system", SMALL_SYSTEMS, ids=lambda s: s[0])
def test_zstats_reference_equals_the_oracle(system, mode):
    table, gi, ge = system
    qs, ts = small_set()
    n = 5
    spread = 0
    for r in (2, 3, 5):                                              # two random queries and the one-residue query
        for t in (ts[0], ts[3], ts[5]):
            s, ss, col = sc.zstats_reference(Z_SEED, r, qs[r], t, table, mode, gi, ge, n)
            direct = [int(oracle(aln_amd.shuffle_query(Z_SEED, r, k, qs[r]), t, table, mode, gi, ge)[1]) for k in range(n)]
            assert col == direct and s == sum(direct) and ss == sum(v * v for v in direct)
            assert isinstance(s, int) and isinstance(ss, int)
            spread += n * ss != s * s
    assert spread or table == "constant+3"                            # the samples are not all constant


def test_z_restated():
    assert sc.z_restated(1, 7, 7, 49).view(np.uint32) == 0           # n < 2
    assert sc.z_restated(4, 9, 20, 100).view(np.uint32) == 0         # D == 0
    s, ss = 1 + 2 + 3 + 6, 1 + 4 + 9 + 36                            # mean 3, sample variance 14 / 3
    z = sc.z_restated(4, 10, s, ss)
    assert z.dtype == np.float32 and abs(float(z) - 7 / math.sqrt(14 / 3)) < 1e-6
    assert sc.z_restated(4, -4, s, ss).view(np.uint32) == (-z).view(np.uint32)


def test_topk_reference_orders_as_the_header_says():
    inf = math.inf
    row = [-0.0, 5.0, 0.0, -3.0, -inf, 5.0, -3.0, 0.0]
    assert sc.topk_reference(row, 8) == [1, 5, 0, 2, 7, 3, 6, 4]     # one zero: -0.0 at index 0 precedes +0.0 at index 2
    assert sc.topk_reference(row, 4) == [1, 5, 0, 2]
    assert sc.topk_reference(row, 1024) == [1, 5, 0, 2, 7, 3, 6, 4]
    assert sc.topk_reference(row, 8, 0.0) == [1, 5, 0, 2, 7]         # -0.0 >= 0.0
    assert sc.topk_reference(row, 8, -3.0) == [1, 5, 0, 2, 7, 3, 6]  # -inf only passes "no threshold"
    assert sc.topk_reference(row, 8, 5.5) == []
    assert sc.topk_reference([3, 3, 3, 3], 2) == [0, 1]
    assert sc.topk_reference(np.array([-7, 0, -7, 2], np.int64), 4) == [3, 1, 0, 2]


# ---- 2. the construction of the cases -----------------------------------------------------------------------------------------
def test_the_case_table():
    assert list(sc.CASES) == ["score32_in", "score32_out", "packed_in", "constant+3", "all_zero", "all_negative", "blosum62x-1",
                              "identity5", "blosum62"]
    assert (sc.W, sc.WORST) == ("W", "N")
    for name, c in sc.CASES.items():
        qs, ts = sc.sequences(c)
        assert [len(q) for q in qs] == [c.n, c.n, min(c.n, c.m), c.n, 0, 1]
        assert [len(t) for t in ts] == [c.m, c.m, min(c.n, c.m), c.m, 0, 2, min(c.n, c.m), c.m, 254, 255]
        assert ts[6] == ts[2] == qs[2] and ts[7] == ts[0] and len(set(ts)) == 8
        assert (c.n, c.m) == ((300, 300) if name in sc.BIG else (130, 257))
        assert ((254 + 2 + 255) // 256, (255 + 2 + 255) // 256) == (1, 2)
    assert np.signbit(sc.TABLES["blosum62x-1"][sc.BLOSUM == 0]).all() and (sc.BLOSUM == 0).any()      # the -0.0 entries
    assert (sc.TABLES["all_negative"] < 0).all()


def test_the_bounds_are_straddled():
    def sides(name):
        c = sc.CASES[name]
        qs, ts = sc.sequences(c)
        Q, T = max(map(len, qs)) + 2, max(map(len, ts)) + 2
        ms = rc.maxs(sc.TABLES[c.table])
        return rc.lhs_score32(ms, c.gi, c.ge, Q, T), rc.lhs_packed(ms, c.gi, c.ge, Q, T)
    inside, _ = sides("score32_in")
    outside, _ = sides("score32_out")
    assert inside == 8387624 and 0.99 * (1 << 23) < inside < 1 << 23
    assert outside == 8388624 and outside >= 1 << 23
    s32, packed = sides("packed_in")
    assert packed == (29997, 110, 99) and packed[0] < 30000 and packed[1] < 8000 and packed[2] < 2048 and s32 < 1 << 23
    for name in sc.CASES:
        if name not in ("score32_out",):
            assert sides(name)[0] < 1 << 23, name
    # the 16-bit lanes of packed_in and the int32 lanes of score32_in do hold values near their limits
    assert dense("packed_in", rc.LOCAL)[0].max() == 29700
    lo = min(int(dense("score32_in", m)[0].min()) for m in rc.ALIGN_TYPES)
    hi = max(int(dense("score32_in", m)[0].max()) for m in rc.ALIGN_TYPES)
    assert (lo, hi) == (-1228704, 2930400)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_rows_tie_and_hold_negative_scores(name):
    """every row ties inside its top 10 (the duplicated templates) and at least two rows of six inside their top 4; apart from
    the tables without a negative entry, some row's top 4 holds a negative score under a non-local align type"""
    negative = False
    for mode in rc.ALIGN_TYPES:
        scores, _ = dense(name, mode)
        for K, least in ((sc.N_TEMPLATES, 6), (4, 2)):
            tied = [sc.has_tie(scores[r], sc.topk_reference(scores[r], K)) for r in range(scores.shape[0])]
            assert sum(tied) >= least, (name, mode, K, tied)
        if mode != rc.LOCAL:
            negative |= any(scores[r][t] < 0 for r in range(scores.shape[0]) for t in sc.topk_reference(scores[r], 4))
        else:
            assert (scores >= 0).all()
    assert negative == (name not in NEGATIVE_FREE), name


def _maxima(name):
    """-> per pair with an interior: (cells that hold the plane's maximum, the maximum, is the seed one of them)"""
    c = sc.CASES[name]
    qs, ts = sc.sequences(c)
    out = []
    for q in qs:
        for t in ts:
            if q and t:
                H = sc.plane(q, t, c.table, rc.LOCAL, c.gi, c.ge)[1]
                sub = H[1:-1, 1:-1]
                out.append((int((sub == sub.max()).sum()), int(sub.max()), bool(sub[-1, -1] == sub.max())))
    return out


def test_seed_rule_cases():
    """find_max's seed rule decides in these planes.  all_negative, all_zero: every plane's maximum is 0, every end cell is the
    seed.  constant+3 with free gaps: H[i][j] = 3 min(i, j), so the maximum sits in several cells and the seed is always one
    of them, never the first in row-major order (an observer that takes >= or forgets the seed reports another cell); a plane
    whose maximum sits in several cells WITHOUT the seed (first cell in row-major order wins) comes from identity5 and the
    BLOSUM62 family."""
    for name in ("all_negative", "all_zero"):
        c = sc.CASES[name]
        qs, ts = sc.sequences(c)
        scores, ends = dense(name, rc.LOCAL)
        assert (scores == 0).all()
        for i, q in enumerate(qs):
            for j, t in enumerate(ts):
                assert tuple(ends[i, j]) == (len(q), len(t))
    m = _maxima("constant+3")
    several = [x for x in m if x[0] > 1]
    assert len(several) >= 30 and all(x[2] and x[1] > 0 for x in several)
    qs, ts = sc.sequences(sc.CASES["constant+3"])
    scores, ends = dense("constant+3", rc.LOCAL)
    assert tuple(ends[0, 0]) == (130, 257) and scores[0, 0] == 390   # the first maximal cell is (130, 130)
    for name in ("identity5", "blosum62", "blosum62x-1", "packed_in", "score32_in", "score32_out"):
        m = _maxima(name)
        assert sum(x[0] > 1 and x[2] for x in m) >= 5 and sum(x[0] > 1 and not x[2] for x in m) >= 5, name


def test_shuffle_scores_square_beyond_32_bits_and_constant_samples():
    c = sc.CASES["score32_in"]
    qs, ts = sc.sequences(c)
    s, ss, col = sc.zstats_reference(Z_SEED, 0, qs[0], ts[0], c.table, rc.LOCAL, c.gi, c.ge, 9)
    assert col == [2930400] * 9 and 2930400 ** 2 > 1 << 32 and ss == 9 * 2930400 ** 2 > 1 << 46
    assert 9 * ss - s * s == 0                                       # a run has one permutation: D == 0 with n >= 2
    for name, c in sc.CASES.items():
        qs, ts = sc.sequences(c)
        for mode in (rc.LOCAL, rc.GLOBAL):
            s, ss, col = sc.zstats_reference(Z_SEED, 0, qs[0], ts[7], c.table, mode, c.gi, c.ge, 9)
            assert 9 * ss == s * s and len(set(col)) == 1, name
        if name not in ("all_zero", "constant+3", "all_negative"):   # and a sample with spread, so that z is a real number
            s, ss, col = sc.zstats_reference(Z_SEED, 3, qs[3], ts[2], c.table, rc.LOCAL, c.gi, c.ge, 9)
            assert 9 * ss > s * s, name


def test_the_wide_set():
    qs, ts = sc.wide_sequences()
    assert [len(q) for q in qs] == [40, 40] and [len(t) for t in ts] == [1400, 1535, 1536, 2045, 2046]
    for table, gi, ge in sc.WIDE_SYSTEMS:
        scores, ends = sc.dense_reference(qs, ts, table, rc.LOCAL, gi, ge)
        assert (ends[0, :, 1] > 256).all()                           # the planted copies end beyond the first column group
        if table == "identity5":                                     # equal scores: the template index decides every row
            assert all(sc.has_tie(scores[r], range(5)) for r in range(2))
    assert (sc.dense_reference(qs, ts, "blosum62x-1", rc.GLOBAL, 1, 5)[0] < -6000).all()
