"""-m gpu: aln_search_topk — for every query row the K best templates, selected on the device, with the cell the optimal
alignment ends in.  The selection is compared with a numpy restatement over aln_score_all_vs_all's dense matrix (score
descending, ties by template index, threshold, padding), the end cells of local hits with Optimal::find_max restated over the
oracle's matrix (seed (Q-2, T-2), strict <, row-major) and with the oracle's own traceback, and the hits with what aligning
them through a resident batch gives."""
import numpy as np
import pytest

import aln_amd
import gpu_util
import orc
from aln_amd.synth import AA20, MT19937, homolog_pair, residues

pytestmark = pytest.mark.gpu

KS = (1, 5, 40, 41, 64)
U32 = np.uint32


def mutate(g, s, rate=0.15):
    r = g.draw(2 * len(s))
    return "".join(AA20[int(r[2 * i + 1]) % 20] if r[2 * i] % 100 < int(rate * 100) else ch for i, ch in enumerate(s))


_SET = {}


def ragged_set():
    """9 queries of 1..400 residues, 41 templates of 0..1500 residues around the 256-column class boundaries: a planted homolog
    of query 3, three mosaics of mutated pieces of every longer query (so that the best hits of those rows are short, cheap for
    the CPU oracle) and four verbatim copies of the first mosaic at scattered indices (score ties in the top of every row)."""
    if _SET:
        return _SET["qs"], _SET["ts"]
    qlens = [1, 7, 64, 200, 333, 400, 25, 90, 150]
    qs = [residues(MT19937(91000 + n), ln) for n, ln in enumerate(qlens)]
    h1, h2 = homolog_pair(91500, 200)
    qs[3] = h1
    tlens = [0, 1, 5, 40, 120, 253, 254, 255, 256, 257, 300, 509, 510, 511, 512, 513, 600, 765, 766, 767, 1021, 1022, 1023, 1024,
             1025, 1100, 1279, 1500] + [int(x) for x in np.random.RandomState(7).randint(2, 400, 5)]
    ts = [residues(MT19937(92000 + n), ln) for n, ln in enumerate(tlens)]
    ts.append(h2)
    g = MT19937(93000)
    mosaics = []
    for m in range(3):
        parts = []
        for q in qs:
            if len(q) >= 25:
                off = 3 * m if len(q) >= 40 else 0
                parts.append(mutate(g, q[off:off + 24]) + residues(g, 3))
        mosaics.append("".join(parts))
    ts += mosaics
    assert len(ts) == 37
    for at in (3, 12, 17, 38):                              # the four copies, before and after the original
        ts.insert(at, mosaics[0])
    assert len(ts) == 41 and ts.count(mosaics[0]) == 5
    _SET["qs"], _SET["ts"] = qs, ts
    return qs, ts


_DENSE = {}


def dense_scores(qs, ts, blosum62, gi=11, ge=1, mode=aln_amd.LOCAL, key=None):
    """aln_score_all_vs_all's matrix, computed once per (set, gaps, align type) and never modified"""
    k = (key, gi, ge, mode)
    if key is None or k not in _DENSE:
        d = aln_amd.score_all_vs_all(gpu_util.ctx(), qs, ts, blosum62[0], blosum62[1], gi, ge, align_type=mode)
        d.setflags(write=False)
        if key is None:
            return d
        _DENSE[k] = d
    return _DENSE[k]


def check_selection(hits, n_hits, dense, K, min_score=-np.inf):
    """the semantics restated: candidates score >= min_score; score descending, ties by template index ascending"""
    rows = dense.shape[0]
    assert hits.shape == (rows, K) and n_hits.shape == (rows,)
    for r in range(rows):
        s = dense[r]
        cand = np.nonzero(s >= min_score)[0]
        order = cand[np.lexsort((cand, -s[cand]))][:K]
        n = len(order)
        assert n_hits[r] == n == min(K, len(cand)), (r, K)
        assert np.array_equal(hits["t"][r, :n], order), (r, K, hits["t"][r, :n], order)
        assert np.array_equal(hits["score"][r, :n].view(U32), s[order].view(U32)), (r, K)
        pad = hits[r, n:]
        assert (pad["t"] == -1).all() and (pad["score"].view(U32) == 0).all() and (pad["q_end"] == -1).all() and (pad["t_end"] == -1).all(), (r, K)


_ORACLE = {}


def oracle_end(q, t, blosum62, gi=11, ge=1):
    """-> (find_max's cell restated over the oracle's D, the oracle's own cell = the pair before the closing one, its score)"""
    k = (q, t, gi, ge)
    if k not in _ORACLE:
        S = orc.sim_submatrix(q, t, blosum62[0], blosum62[1])
        rc, D, PQ, PT = orc.dp_build(S, orc.Gap(orc.LOCAL, gi, ge))
        assert rc == 0
        Q, T = D.shape
        sub = D[:Q - 1, :T - 1]                              # optimal.h:115-116: rows 0..Q-2, columns 0..T-2
        first = np.unravel_index(np.argmax(sub), sub.shape)  # the first maximal cell in row-major order
        cell = (int(first[0]), int(first[1])) if D[Q - 2, T - 2] < sub.max() else (Q - 2, T - 2)   # seed, strict <
        rc2, sc, pl = orc.optimal(D, PQ, PT, True)
        assert rc2 == 0
        _ORACLE[k] = (cell, (int(pl[-2][0]), int(pl[-2][1])), sc)
    return _ORACLE[k]


def check_ends(hits, n_hits, qs, ts, blosum62, gi=11, ge=1, rows=None):
    n = 0
    for r in (range(len(qs)) if rows is None else rows):
        for k in range(n_hits[r]):
            h = hits[r, k]
            cell, cell2, sc = oracle_end(qs[r], ts[h["t"]], blosum62, gi, ge)
            assert cell == cell2, (r, k)
            assert (int(h["q_end"]), int(h["t_end"])) == cell, (r, k, int(h["t"]), h, cell)
            assert np.float32(h["score"]).view(U32) == np.float32(sc).view(U32), (r, k)
            n += 1
    return n


# ---- 1. selection equals the dense path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "median", "row_block", "unpacked"])
def test_selection_equals_dense_path(variant, blosum62):
    alpha, table = blosum62
    qs, ts = ragged_set()
    ctx = gpu_util.ctx()
    dense = dense_scores(qs, ts, blosum62, key="ragged")
    assert len(np.unique(dense[5])) < len(ts) - 3          # the copies do tie
    for K in KS:
        if variant == "plain":
            hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, K)
            check_selection(hits, n_hits, dense, K)
        elif variant == "median":
            for r in range(len(qs)):
                med = float(np.median(dense[r]))
                hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, K, min_score=med, q_begin=r, q_end=r + 1)
                check_selection(hits, n_hits, dense[r:r + 1], K, med)
                assert n_hits[0] == min(K, int((dense[r] >= med).sum())) and n_hits[0] >= 1
        elif variant == "row_block":
            hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, K, q_begin=2, q_end=7)
            check_selection(hits, n_hits, dense[2:7], K)
        else:
            with ctx.hints(score_packed=0):
                hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, K)
            check_selection(hits, n_hits, dense, K)


@pytest.mark.parametrize("mode", [aln_amd.GLOBAL, aln_amd.SEMI_LOCAL])
def test_selection_non_local(mode, blosum62):
    """negative scores exercise the key mapping; the end cell is (Q-1, T-1), where Optimal starts"""
    alpha, table = blosum62
    qs, ts = ragged_set()
    ctx = gpu_util.ctx()
    dense = dense_scores(qs, ts, blosum62, mode=mode, key="ragged")
    assert (dense < 0).any() and (dense > 0).any()
    for K in KS:
        hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, K, align_type=mode)
        check_selection(hits, n_hits, dense, K)
        for r in range(len(qs)):
            n = n_hits[r]
            assert (hits["q_end"][r, :n] == len(qs[r]) + 1).all()
            assert np.array_equal(hits["t_end"][r, :n], [len(ts[t]) + 1 for t in hits["t"][r, :n]])
    med = float(np.median(dense[4]))
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, 41, min_score=med, q_begin=4, q_end=5, align_type=mode)
    check_selection(hits, n_hits, dense[4:5], 41, med)


# ---- 2. selection edge shapes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_t", [1, 63, 64, 65, 257, 1025])
def test_selection_edge_shapes(n_t, blosum62):
    alpha, table = blosum62
    ctx = gpu_util.ctx()
    g = MT19937(94000 + n_t)
    lens = (g.draw(n_t) % 31).astype(int)                   # 0 .. 30 residues
    ts = [residues(g, int(ln)) for ln in lens]
    qs = [residues(g, 40), "", residues(g, 9)]
    same = [ts[0] if len(ts[0]) else "ACDEFGHIKL"] * n_t    # every score of a row equal: index order
    for tset in (ts, same):
        dense = dense_scores(qs, tset, blosum62)
        for K in (1, 64, 1024):
            hits, n_hits = aln_amd.search_topk(ctx, qs, tset, alpha, table, 11, 1, K)
            check_selection(hits, n_hits, dense, K)
            thr = float(dense[0].max())
            hits, n_hits = aln_amd.search_topk(ctx, qs, tset, alpha, table, 11, 1, K, min_score=thr)
            check_selection(hits, n_hits, dense, K, thr)
    n = min(n_t, 64)
    hits, n_hits = aln_amd.search_topk(ctx, qs, same, alpha, table, 11, 1, 64)
    assert (n_hits == n).all() and (hits["t"][:, :n] == np.arange(n)[None, :]).all()


# ---- 3. end cells equal find_max ----------------------------------------------------------------------------------------
def test_end_cells_equal_find_max_on_the_ragged_set(blosum62):
    alpha, table = blosum62
    qs, ts = ragged_set()
    hits, n_hits = aln_amd.search_topk(gpu_util.ctx(), qs, ts, alpha, table, 11, 1, 5)
    assert check_ends(hits, n_hits, qs, ts, blosum62) == 45


HAND = [("WPPPPW", "WCCCCW"), ("AAAA", "AAAAAAAA"), ("AAAA", "AAAAAAAAW"), ("WGGW", "WW"), ("W", "CW"), ("", "ACD")]


def test_end_cells_hand_cases(blosum62):
    """ties between maximal cells: the seed (Q-2, T-2) wins those it takes part in, otherwise the first cell in row-major order.
    The expected cells come from the oracle; the literals below only pin what the cases are meant to exercise."""
    alpha, table = blosum62
    ctx = gpu_util.ctx()
    qs, ts = [p[0] for p in HAND], [p[1] for p in HAND]
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, len(ts))
    assert (n_hits == len(ts)).all()
    dense = dense_scores(qs, ts, blosum62)
    check_selection(hits, n_hits, dense, len(ts))
    assert check_ends(hits, n_hits, qs, ts, blosum62) == len(qs) * len(ts)
    by_t = {(r, int(h["t"])): (int(h["q_end"]), int(h["t_end"]), float(h["score"])) for r in range(len(qs)) for h in hits[r]}
    assert by_t[(0, 0)] == (6, 6, 11.0)
    assert by_t[(1, 1)] == (4, 8, 16.0)
    assert by_t[(2, 2)][2] == 16.0 and by_t[(2, 2)][:2] != (4, 9)
    assert by_t[(3, 3)][:2] == (4, 2)
    assert by_t[(4, 4)][:2] == (1, 2)
    assert by_t[(5, 5)] == (0, 3, 0.0)


def test_end_cells_beyond_the_first_256_columns(blosum62):
    """a homolog planted near the end of templates of 300 .. 2040 residues: R = 2, 3, 5, 7, 8 column groups per lane"""
    alpha, table = blosum62
    ctx = gpu_util.ctx()
    g = MT19937(95000)
    q, h = homolog_pair(95001, 60)
    qs = [q, residues(g, 33)]
    ts = [residues(g, ln - 70) + h + residues(g, 10) for ln in (300, 600, 1100, 1700, 2040)] + [residues(g, 50)]
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, 5)
    check_selection(hits, n_hits, dense_scores(qs, ts, blosum62), 5)
    assert sorted(hits["t"][0].tolist()) == [0, 1, 2, 3, 4]
    assert (hits["t_end"][0] > np.array([len(ts[t]) for t in hits["t"][0]]) - 20).all()      # the planted ends
    assert check_ends(hits, n_hits, qs, ts, blosum62) == 10


# ---- 4. several slabs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [aln_amd.LOCAL, aln_amd.GLOBAL])
def test_several_slabs(mode, blosum62):
    alpha, table = blosum62
    qs, ts = ragged_set()
    ctx = gpu_util.ctx()
    for K in (5, 41):
        one, n_one = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, K, align_type=mode)
        with ctx.hints(search_slab_rows=3):
            assert ctx.get_hint("search_slab_rows") == 3
            many, n_many = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, K, align_type=mode)
            blk, n_blk = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, K, q_begin=1, q_end=8, align_type=mode)
        assert ctx.get_hint("search_slab_rows") == 0
        assert one.tobytes() == many.tobytes() and np.array_equal(n_one, n_many)
        assert one[1:8].tobytes() == blk.tobytes() and np.array_equal(n_one[1:8], n_blk)
        if mode == aln_amd.LOCAL:
            assert (one["q_end"][one["t"] >= 0] >= 0).all()


# ---- 5. full-build route ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gaps", [(11, 1), (4.73, 0.34)])
def test_full_build_route(gaps, blosum62):
    """templates beyond 2048 columns (and, with fractional gaps, every pair) are scored through full builds inside the call;
    the end cells of such hits come from a resident batch over just those hits"""
    alpha, table = blosum62
    gi, ge = gaps
    qlens = [5, 60, 40, 90]
    tlens = [300, 2047, 2048, 2600, 40]
    qs = [residues(MT19937(96000 + n), ln) for n, ln in enumerate(qlens)]
    ts = [residues(MT19937(97000 + n), ln) for n, ln in enumerate(tlens)]
    qs[2] = ts[3][2300:2340]                                  # a homolog inside the longest template
    ctx = gpu_util.ctx()
    dense = dense_scores(qs, ts, blosum62, gi, ge)
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, gi, ge, 3)
    check_selection(hits, n_hits, dense, 3)
    assert hits["t"][2, 0] == 3
    assert check_ends(hits, n_hits, qs, ts, blosum62, gi, ge, rows=[2]) == 3
    assert (hits["q_end"] >= 0).all() and (hits["t_end"] >= 0).all()
    with ctx.hints(search_slab_rows=3):
        many, n_many = aln_amd.search_topk(ctx, qs, ts, alpha, table, gi, ge, 3)
    assert many.tobytes() == hits.tobytes() and np.array_equal(n_many, n_hits)
    for mode in (aln_amd.GLOBAL, aln_amd.SEMI_LOCAL):
        hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, gi, ge, 3, align_type=mode)
        check_selection(hits, n_hits, dense_scores(qs, ts, blosum62, gi, ge, mode), 3)
        assert (hits["q_end"] == np.array([len(q) + 1 for q in qs])[:, None]).all()


# ---- 6. hits align to themselves ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 41])
def test_hits_align_to_themselves(K, blosum62):
    """K = 41 aligns every pair of the set, so end cells of every template length class are checked against the traceback"""
    alpha, table = blosum62
    qs, ts = ragged_set()
    ctx = gpu_util.ctx()
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, K)
    scores, lists = aln_amd.align_hits(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1)
    assert len(scores) == len(lists) == int(n_hits.sum()) == len(qs) * K
    flat = hits.reshape(-1)
    assert np.array_equal(scores.view(U32), flat["score"].view(U32))
    for k, pl in enumerate(lists):
        r = k // K
        assert tuple(pl[-1]) == (len(qs[r]) + 1, len(ts[flat["t"][k]]) + 1)
        assert tuple(pl[-2]) == (flat["q_end"][k], flat["t_end"][k]), (k, flat[k], pl[-2:])
    blk, n_blk = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, K, q_begin=2, q_end=7)
    s2, l2 = aln_amd.align_hits(ctx, qs, ts, blk, n_blk, alpha, table, 11, 1, q_begin=2)
    assert np.array_equal(s2.view(U32), blk.reshape(-1)["score"].view(U32))


# ---- 7. the debug path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [aln_amd.LOCAL, aln_amd.SEMI_LOCAL])
def test_search_debug_changes_no_result(mode, blosum62):
    """search_debug = 1 (four events per slab, a line on stderr) over slabs of 2 rows: hits and n_hits byte-equal to the default's,
    for residue queries and for their profiles; the template of 300 residues puts a second length class into every slab"""
    alpha, table = blosum62
    ctx = gpu_util.ctx()
    qs = [residues(MT19937(98000 + n), ln) for n, ln in enumerate((3, 11, 24, 33, 40))]
    ts = [residues(MT19937(98100 + n), ln) for n, ln in enumerate((3, 9, 17, 26, 35, 40, 300))]
    ts[6] = ts[6][:200] + qs[4] + ts[6][240:]                # a hit in class 2
    prof = aln_amd.profiles_from_sequences(qs, alpha, table)
    searches = [lambda: aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, 3, align_type=mode),
                lambda: aln_amd.search_topk_profiles(ctx, prof, ts, 11, 1, 3, align_type=mode)]
    for search in searches:
        hits, n_hits = search()
        assert (n_hits == 3).all() and 6 in hits["t"][4]
        with ctx.hints(search_debug=1, search_slab_rows=2):
            dbg, n_dbg = search()
        assert ctx.get_hint("search_debug") == 0
        assert dbg.tobytes() == hits.tobytes() and n_dbg.tobytes() == n_hits.tobytes()


# ---- 8. argument checks -------------------------------------------------------------------------------------------------
def test_argument_checks(blosum62):
    alpha, table = blosum62
    ctx = gpu_util.ctx()
    for K in (0, 1025, -3):
        with pytest.raises(aln_amd.AlnError) as ei:
            aln_amd.search_topk(ctx, ["ACD"], ["ACD"], alpha, table, 11, 1, K)
        assert ei.value.code == aln_amd.E_ARG
    with pytest.raises(aln_amd.AlnError) as ei:
        aln_amd.search_topk(ctx, ["ACJ"], ["ACD"], alpha, table, 11, 1, 3)
    assert ei.value.code == aln_amd.E_RESIDUE
    with pytest.raises(aln_amd.AlnError) as ei:
        aln_amd.search_topk(ctx, ["ACD"], ["ACD"], alpha, table, 11, 1, 3, q_begin=1, q_end=0)
    assert ei.value.code == aln_amd.E_ARG
    with pytest.raises(aln_amd.AlnError) as ei:
        ctx.set_hint("search_slab_cols", 1)
    assert ei.value.code == aln_amd.E_ARG
    # q_begin == q_end: ALN_OK and nothing is written
    L = aln_amd.lib()
    import ctypes as C
    qp, tp = aln_amd.SeqPool(["ACD", "WW"]), aln_amd.SeqPool(["ACD"])
    tab = np.ascontiguousarray(table, dtype=np.float32)
    ab = alpha.encode()
    sub = aln_amd.AlnSubmatrix(len(alpha), ab, tab.ctypes.data_as(C.POINTER(C.c_float)))
    g = aln_amd.AlnGap()
    g.model, g.align_type, g.gap_init, g.gap_extn = aln_amd.GAP_AFFINE_CONST, aln_amd.LOCAL, 11.0, 1.0
    hits = np.full(4, 0x5A, dtype=np.uint8).repeat(16).view(aln_amd.HIT_DTYPE)
    n_hits = np.full(1, 77, dtype=np.int32)
    before = hits.tobytes()
    rc = L.aln_search_topk(ctx.h, C.byref(qp.c), C.byref(tp.c), C.byref(sub), C.byref(g), 1, 1, 4, C.c_float(-np.inf),
                           hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0 and hits.tobytes() == before and n_hits[0] == 77
    # no template at all: every slot unused
    hits, n_hits = aln_amd.search_topk(ctx, ["ACD", "WW"], [], alpha, table, 11, 1, 2)
    assert (n_hits == 0).all() and (hits["t"] == -1).all() and (hits["q_end"] == -1).all()
