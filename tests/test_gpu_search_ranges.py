"""-m gpu: aln_search_topk, aln_hits_zscores and aln_hits_align under scoring systems beyond BLOSUM62 11/1, against a reference
that shares nothing with the device: the int64 planes of tests/range_cases.py (scores, find_max's end cells, local walks), Python
integers (sums, squares), the oracle's build and traceback (non-local lists) — tests/search_cases.py, pinned to the oracle and
with its construction asserted by tests/test_search_reference.py.  Scores and z are compared as uint32 patterns, everything else
for equality.

The cases (search_cases.CASES; 6 queries x 10 templates each, two templates duplicated, two straddling 256 columns):
  score32_in / score32_out   BLOSUM62 x 888, ge 4096, gi 4000 | 5000, 300 x 300: inside ScoreRun::prepare's 2^23 bound by under
                             1 % | outside it, where the search goes through full builds, the alignment through batches and
                             the z-scores answer ALN_E_NOT_INTEGRAL; shuffle scores of 2 930 400, squares beyond 2^32
  packed_in                  BLOSUM62 x 9, 11/0, 300 x 300: the packed 16-bit kernel at its limit (29 997 < 30 000)
  constant+3, all_zero 0/0   rows in which every score is equal, planes whose maximum sits in many cells or is 0
  all_negative 0/1           every local score 0: find_max's seed everywhere; negative keys in every non-local top K
  blosum62x-1 1/5            -0.0 table entries, ge > gi;  identity5 40/0: large gi, ge 0;  blosum62 11/1: the control
and a wide set (2 queries of 40 residues, templates of 1400 .. 2046 residues: length classes 6, 7 and 8) under identity5 40/0 and
blosum62x-1 1/5, which reaches the instantiations <6>, <7> and <8> of the score, shuffle and align kernels."""
import ctypes as C

import numpy as np
import pytest

import aln_amd
import gpu_util
import lean_cases as lc
import range_cases as rc
import search_cases as sc

pytestmark = pytest.mark.gpu

U32 = np.uint32
ALPHA = sc.ALPHA
SEED = 2024
K_ALL = sc.N_TEMPLATES
LOCAL_FUSED_CLASSES = range(1, 8)            # ResidueQuery::kFusedLocal / kFusedGlobal (csrc/score_common.h)
NONLOCAL_FUSED_CLASSES = range(1, 9)
Z_MODES_BIG = (rc.LOCAL, rc.GLOBAL)
Z_33 = ("score32_in", "identity5")           # one case per size also runs 33 shuffles
Z_PARAMS = [(n, m) for n in sc.CASES for m in (Z_MODES_BIG if n in sc.BIG else rc.ALIGN_TYPES)]


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(U32)


def setup(name):
    c = sc.CASES[name]
    qs, ts = sc.sequences(c)
    return c, qs, ts, sc.TABLES[c.table]


_DENSE = {}


def dense(key, qs, ts, table, mode, gi, ge):
    """the reference's scores and end cells of a set: computed once, read-only"""
    k = (key, table, mode, gi, ge)
    if k not in _DENSE:
        _DENSE[k] = sc.dense_reference(qs, ts, table, mode, gi, ge)
    return _DENSE[k]


def case_dense(name, mode):
    c, qs, ts, _ = setup(name)
    return dense(name, qs, ts, c.table, mode, c.gi, c.ge)


def check_hits(hits, n_hits, scores, ends, K, min_score=-np.inf, what=None):
    """hits of the rows `scores` / `ends` describe: the header's selection, the score's bits, the end cell, the padding"""
    rows = scores.shape[0]
    assert hits.shape == (rows, K) and n_hits.shape == (rows,), what
    for r in range(rows):
        order = sc.topk_reference(scores[r], K, min_score)
        n = len(order)
        w = (what, r, K, hits[r].tolist(), order)
        assert n_hits[r] == n, w
        assert hits["t"][r, :n].tolist() == order, w
        assert np.array_equal(u32(hits["score"][r, :n]), u32(scores[r, order])), w
        assert np.array_equal(hits["q_end"][r, :n], ends[r, order, 0]) and np.array_equal(hits["t_end"][r, :n], ends[r, order, 1]), w
        pad = hits[r, n:]
        assert (pad["t"] == -1).all() and (u32(pad["score"]) == 0).all() and (pad["q_end"] == -1).all() and (pad["t_end"] == -1).all(), w


_HITS = {}


def searched(key, qs, ts, table, tname, mode, gi, ge, K):
    """the plain search of a set, checked against the reference once and left unchanged"""
    k = (key, tname, mode, gi, ge, K)
    if k not in _HITS:
        hits, n_hits = aln_amd.search_topk(gpu_util.ctx(), qs, ts, ALPHA, table, gi, ge, K, align_type=mode)
        scores, ends = dense(key, qs, ts, tname, mode, gi, ge)
        check_hits(hits, n_hits, scores, ends, K, what=k)
        hits.setflags(write=False)
        n_hits.setflags(write=False)
        _HITS[k] = (hits, n_hits)
    return _HITS[k]


def case_hits(name, mode, K):
    c, qs, ts, table = setup(name)
    return searched(name, qs, ts, table, c.table, mode, c.gi, c.ge, K)


def every_template(scores):
    """hand-made hits: every template for every row, in template order, with the reference's score"""
    rows, n_t = scores.shape
    hits = np.zeros((rows, n_t), dtype=aln_amd.HIT_DTYPE)
    hits["t"] = np.arange(n_t, dtype=np.int32)[None, :]
    hits["score"] = scores.astype(np.float32)
    hits["q_end"] = hits["t_end"] = -1
    return hits, np.full(rows, n_t, dtype=np.int32)


def used_slots(n_hits, K):
    return [(r, k) for r in range(len(n_hits)) for k in range(K) if k < n_hits[r]]


# ---- a. selection -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
@pytest.mark.parametrize("name", list(sc.CASES))
def test_selection(name, mode):
    """t, score, n_hits, the end cell and the padding of every row: plain, with the packed kernel forbidden, for a row block,
    and with a threshold at 0.0 and at the row's median (rows of equal scores, negative keys, -0.0 table entries, the 16-bit
    kernel at its limit, the int32 kernel at its limit and the full-build route beyond it)"""
    c, qs, ts, table = setup(name)
    ctx = gpu_util.ctx()
    scores, ends = case_dense(name, mode)
    args = (ALPHA, table, c.gi, c.ge)
    for K in sc.KS:
        case_hits(name, mode, K)                                     # plain
        with ctx.hints(score_packed=0):
            hits, n_hits = aln_amd.search_topk(ctx, qs, ts, *args, K, align_type=mode)
        check_hits(hits, n_hits, scores, ends, K, what=(name, mode, "unpacked"))
        hits, n_hits = aln_amd.search_topk(ctx, qs, ts, *args, K, q_begin=1, q_end=4, align_type=mode)
        check_hits(hits, n_hits, scores[1:4], ends[1:4], K, what=(name, mode, "row block"))
        hits, n_hits = aln_amd.search_topk(ctx, qs, ts, *args, K, min_score=0.0, align_type=mode)
        check_hits(hits, n_hits, scores, ends, K, 0.0, what=(name, mode, "min_score 0"))
        for r in range(len(qs)):
            med = float(np.median(scores[r]))
            assert float(np.float32(med)) == med
            hits, n_hits = aln_amd.search_topk(ctx, qs, ts, *args, K, min_score=med, q_begin=r, q_end=r + 1, align_type=mode)
            check_hits(hits, n_hits, scores[r:r + 1], ends[r:r + 1], K, med, what=(name, mode, "median", r))
            assert 1 <= n_hits[0] == min(K, int((scores[r] >= med).sum()))
    if mode != rc.LOCAL:                                             # the cell Optimal starts from
        hits, n_hits = case_hits(name, mode, K_ALL)
        assert (hits["q_end"] == np.array([len(q) + 1 for q in qs])[:, None]).all()
        assert (hits["t_end"] == np.array([len(ts[t]) + 1 for t in range(K_ALL)])[hits["t"]]).all()


def test_empty_rows_keep_the_padding_pattern():
    """a threshold above every score of the all-zero table: n_hits 0 and -1, 0, -1, -1 in every slot"""
    c, qs, ts, table = setup("all_zero")
    for mode in (rc.LOCAL, rc.GLOBAL):
        hits, n_hits = aln_amd.search_topk(gpu_util.ctx(), qs, ts, ALPHA, table, c.gi, c.ge, 4, min_score=0.5, align_type=mode)
        scores, ends = case_dense("all_zero", mode)
        check_hits(hits, n_hits, scores, ends, 4, 0.5)
        assert (n_hits == 0).all() and (hits["t"] == -1).all() and (u32(hits["score"]) == 0).all()
        assert (hits["q_end"] == -1).all() and (hits["t_end"] == -1).all()


# ---- b. local end cells -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.CASES))
def test_local_end_cells(name):
    """every pair of the set (K = the number of templates): q_end / t_end equal find_max over the int64 plane — seed (Q-2, T-2),
    replaced by the first strictly greater cell in row-major order — also where every cell is 0 and where many cells hold the
    maximum; score32_out takes its end cells from resident batches"""
    c, qs, ts, table = setup(name)
    ctx = gpu_util.ctx()
    scores, ends = case_dense(name, rc.LOCAL)
    hits, n_hits = case_hits(name, rc.LOCAL, K_ALL)
    assert (n_hits == K_ALL).all()
    for r in range(len(qs)):                                         # (ends: lean_cases.find_max_cell of every pair's plane)
        assert np.array_equal(hits["q_end"][r], ends[r, hits["t"][r], 0]) and np.array_equal(hits["t_end"][r], ends[r, hits["t"][r], 1]), (name, r)
        assert np.array_equal(u32(hits["score"][r]), u32(scores[r, hits["t"][r]])), (name, r)
    with ctx.hints(search_slab_rows=2, score_packed=0):
        again, n_again = aln_amd.search_topk(ctx, qs, ts, ALPHA, table, c.gi, c.ge, K_ALL)
    assert again.tobytes() == hits.tobytes() and np.array_equal(n_again, n_hits)
    if name in ("all_zero", "all_negative"):
        assert (hits["q_end"] == np.array([len(q) for q in qs])[:, None]).all() and (u32(hits["score"]) == 0).all()


# ---- c. z-scores --------------------------------------------------------------------------------------------------------------
def check_stats(stats, hits, n_hits, qs, ts, tname, mode, gi, ge, n, q_begin=0, what=None):
    rows, K = hits.shape
    assert stats.shape == (rows, K) and stats.dtype == aln_amd.HIT_STATS_DTYPE
    seen = dict(big_square=0, no_spread=0, spread=0)
    for r in range(rows):
        for k in range(K):
            st = stats[r, k]
            if k >= n_hits[r]:
                assert st.tobytes() == bytes(24), (what, r, k)
                continue
            t = int(hits["t"][r, k])
            s, ss, col = sc.zstats_reference(SEED, q_begin + r, qs[q_begin + r], ts[t], tname, mode, gi, ge, n)
            w = (what, r, k, t, st, s, ss)
            assert (int(st["sum"]), int(st["sumsq"]), int(st["n"])) == (s, ss, n), w
            want = sc.z_restated(n, hits["score"][r, k], s, ss)
            assert st["z"].view(U32) == want.view(U32), w + (want,)
            seen["big_square"] += max(v * v for v in col) > 1 << 32
            seen["no_spread"] += n * ss == s * s
            seen["spread"] += n * ss != s * s
    return seen


def raw_zscores(qs, ts, table, mode, gi, ge, K, hits, n_hits, n_shuffles):
    """the C entry itself with a stats buffer holding a pattern -> (status, buffer untouched?)"""
    qp, tp = aln_amd.SeqPool(qs), aln_amd.SeqPool(ts)
    tab = np.ascontiguousarray(table, dtype=np.float32)
    ab = ALPHA.encode()
    sub = aln_amd.AlnSubmatrix(len(ALPHA), ab, tab.ctypes.data_as(C.POINTER(C.c_float)))
    g = aln_amd.AlnGap()
    g.model, g.align_type, g.gap_init, g.gap_extn = aln_amd.GAP_AFFINE_CONST, int(mode), float(gi), float(ge)
    hits = np.ascontiguousarray(hits, dtype=aln_amd.HIT_DTYPE)
    n_hits = np.ascontiguousarray(n_hits, dtype=np.int32)
    stats = np.full(hits.size * 24, 0x5A, dtype=np.uint8)
    before = stats.tobytes()
    rc_ = aln_amd.lib().aln_hits_zscores(gpu_util.ctx().h, C.byref(qp.c), C.byref(tp.c), C.byref(sub), C.byref(g), 0, len(qs), K,
                                         hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits.ctypes.data_as(C.POINTER(C.c_int32)),
                                         n_shuffles, SEED, stats.ctypes.data_as(C.POINTER(aln_amd.AlnHitStats)))
    return rc_, stats.tobytes() == before


@pytest.mark.parametrize("name,mode", Z_PARAMS)
def test_zscores(name, mode):
    """sum, sumsq, n equal Python-integer sums over the reference's scores of aln_amd.shuffle_query's strings, z bit for bit: for
    the search's own hits and for hand-made hits of every template (the runs, whose samples have no spread, and the duplicated
    templates are always among them).  Beyond the 2^23 bound the call answers ALN_E_NOT_INTEGRAL and writes nothing."""
    c, qs, ts, table = setup(name)
    ctx = gpu_util.ctx()
    scores, ends = case_dense(name, mode)
    hits4, n4 = case_hits(name, mode, 4)
    every, n_every = every_template(scores)
    args = (ALPHA, table, c.gi, c.ge)
    if name == "score32_out":
        for h, nh in ((hits4, n4), (every, n_every)):
            assert raw_zscores(qs, ts, table, mode, c.gi, c.ge, h.shape[1], h, nh, 9) == (aln_amd.E_NOT_INTEGRAL, True)
        with pytest.raises(aln_amd.AlnError) as ei:
            aln_amd.hits_zscores(ctx, qs, ts, hits4, n4, *args, 9, seed=SEED, align_type=mode)
        assert ei.value.code == aln_amd.E_NOT_INTEGRAL
        return
    assert raw_zscores(qs, ts, table, mode, c.gi, c.ge, 4, hits4, n4, 9) == (0, False)     # the same call inside the bound writes
    ref = (qs, ts, c.table, mode, c.gi, c.ge)
    stats = aln_amd.hits_zscores(ctx, qs, ts, hits4, n4, *args, 9, seed=SEED, align_type=mode)
    check_stats(stats, hits4, n4, *ref, 9, what=(name, mode, "top 4"))
    full = aln_amd.hits_zscores(ctx, qs, ts, every, n_every, *args, 9, seed=SEED, align_type=mode)
    seen = check_stats(full, every, n_every, *ref, 9, what=(name, mode, "every template"))
    assert seen["no_spread"] >= 2 * K_ALL                            # the two runs at least
    assert seen["spread"] > 0 or name in ("all_zero", "constant+3", "all_negative")
    if name == "score32_in":
        assert seen["big_square"] >= 2 and int(full["sumsq"].max()) == 9 * 2930400 ** 2 > 1 << 46
    assert full[0, 0].tobytes() == full[0, 7].tobytes() and full[3, 2].tobytes() == full[3, 6].tobytes()   # the duplicates
    blk = aln_amd.hits_zscores(ctx, qs, ts, every[2:4], n_every[2:4], *args, 9, seed=SEED, q_begin=2, align_type=mode)
    assert blk.tobytes() == full[2:4].tobytes()
    if name in Z_33:
        stats = aln_amd.hits_zscores(ctx, qs, ts, hits4, n4, *args, 33, seed=SEED, align_type=mode)
        check_stats(stats, hits4, n4, *ref, 33, what=(name, mode, "33 shuffles"))


# ---- d. hit alignment ---------------------------------------------------------------------------------------------------------
def fused_expected(q, t, mode):
    Q, T = len(q) + 2, len(t) + 2
    classes = LOCAL_FUSED_CLASSES if mode == rc.LOCAL else NONLOCAL_FUSED_CLASSES
    return Q >= 3 and T >= 3 and T <= 2048 and (T + 255) // 256 in classes


def check_alignments(res, hits, n_hits, qs, ts, tname, mode, gi, ge, what=None):
    rec, lists, tl, ql, lengths, status = res
    K = hits.shape[1]
    assert status == 0, what
    for r in range(len(n_hits)):
        for k in range(K):
            e = rec[r, k]
            w = (what, r, k, e)
            if k >= n_hits[r]:
                assert e.tobytes() == bytes(16) and len(lists[r][k]) == 0 and tl[r][k] == "" and ql[r][k] == "" and lengths[r, k] == 0, w
                continue
            q, t = qs[r], ts[hits["t"][r, k]]
            if mode == rc.LOCAL:
                S, H = sc.plane(q, t, tname, mode, gi, ge)
                want = lc.reference_list(H, gi, ge)
                lc.check_local_list(S, H, lists[r][k], gi, ge)
                score = np.float32(rc.reference_score(H, mode))
            else:
                score, want = sc.nonlocal_reference(q, t, tname, mode, gi, ge)
            assert e["status"] == 0 and e["n_pairs"] == len(want), w
            assert np.array_equal(lists[r][k], want), w + (lists[r][k].tolist(), want.tolist())
            assert e["score"].view(U32) == np.float32(score).view(U32) == hits["score"][r, k].view(U32), w
            assert e["identity"].view(U32) == gpu_util.identity_for(q, t, want).view(U32), w
            t_line, q_lines, _ = gpu_util.strings_for(q, t, [want])
            assert (tl[r][k], ql[r][k], int(lengths[r, k])) == (t_line, q_lines[0], len(t_line)), w


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
@pytest.mark.parametrize("name", list(sc.CASES))
def test_hit_alignment(name, mode):
    """aln_hits_align on the search's own four best hits of every row.  Local: the list is the walk of optimal.h:79-105 over the
    int64 plane (lean_cases.reference_list) and passes check_local_list; the four other types: the oracle's list.  Scores equal
    the slot's, identities and lines the host helpers' on that list.  Inside the 2^23 bound every pair with an interior runs in
    the fused kernel, beyond it every pair goes through resident batches."""
    c, qs, ts, table = setup(name)
    ctx = gpu_util.ctx()
    hits, n_hits = case_hits(name, mode, 4)
    assert (n_hits == 4).all()
    res = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, ALPHA, table, c.gi, c.ge, align_type=mode)
    routes = aln_amd.hits_align_routes(ctx)
    n_used = int(n_hits.sum())
    if name == "score32_out":
        assert routes == (0, n_used)
    else:
        n_fused = sum(fused_expected(qs[r], ts[hits["t"][r, k]], mode) for r, k in used_slots(n_hits, 4))
        assert routes == (n_fused, n_used - n_fused) and n_fused >= 12, routes
    check_alignments(res, hits, n_hits, qs, ts, c.table, mode, c.gi, c.ge, what=(name, mode))


# ---- e. the wide set: length classes 6, 7 and 8 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sc.WIDE_MODES)
@pytest.mark.parametrize("system", sc.WIDE_SYSTEMS, ids=lambda s: s[0])
def test_the_wide_set(system, mode):
    """selection, end cells, z-scores (9 shuffles) and alignments of templates of 1400 .. 2046 residues: the instantiations
    <6>, <7>, <8> of the score, shuffle and non-local align kernels and <6>, <7> of the local one; class 8 local hits go the
    batch route"""
    tname, gi, ge = system
    table = sc.TABLES[tname]
    qs, ts = sc.wide_sequences()
    ctx = gpu_util.ctx()
    K = len(ts)
    scores, ends = dense("wide", qs, ts, tname, mode, gi, ge)
    hits, n_hits = searched("wide", qs, ts, table, tname, mode, gi, ge, K)
    hits2, n2 = aln_amd.search_topk(ctx, qs, ts, ALPHA, table, gi, ge, 2, align_type=mode)
    check_hits(hits2, n2, scores, ends, 2, what=("wide", tname, mode))
    assert (n_hits == K).all()
    stats = aln_amd.hits_zscores(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, 9, seed=SEED, align_type=mode)
    seen = check_stats(stats, hits, n_hits, qs, ts, tname, mode, gi, ge, 9, what=("wide", tname, mode))
    # the run has one permutation; the random query's sample has spread (not under blosum62x-1 1/5 global, where the end gaps
    # of some -7000 leave every permutation the same best path: a second kind of constant sample)
    assert seen["no_spread"] >= K and (seen["spread"] >= K or (tname, mode) == ("blosum62x-1", rc.GLOBAL))
    res = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, align_type=mode)
    routes = aln_amd.hits_align_routes(ctx)
    n_fused = sum(fused_expected(q, t, mode) for q in qs for t in ts)
    assert n_fused == (6 if mode == rc.LOCAL else 10) and routes == (n_fused, 2 * K - n_fused), routes
    check_alignments(res, hits, n_hits, qs, ts, tname, mode, gi, ge, what=("wide", tname, mode))
