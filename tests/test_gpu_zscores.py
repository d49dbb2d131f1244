"""-m gpu: aln_hits_zscores — shuffle z-scores of search hits, scored and reduced on the device.

The reference of every sum is the dense path: the shuffled strings come from aln_amd.shuffle_query (pure Python), their scores
from aln_amd.score_all_vs_all against the templates, the sums are taken over Python integers; `sum`, `sumsq` and `n` are
compared for equality and `z` bit for bit with a Python restatement of the header's formula."""
import ctypes as C

import numpy as np
import pytest

import aln_amd
import gpu_util
from aln_amd.synth import MT19937, homolog_pair, residues
from search_cases import z_restated

pytestmark = pytest.mark.gpu

U32 = np.uint32
SEED = 2024
S_MAX = 65
MODES = (aln_amd.LOCAL, aln_amd.GLOBAL, aln_amd.GLOBAL_LOCAL, aln_amd.LOCAL_GLOBAL, aln_amd.SEMI_LOCAL)
HOMOLOG_ROW = 5

_SET = {}


def ragged_set():
    """8 queries of 0..400 residues (row 5 and the last template are a homolog pair), 26 templates around every boundary
    of the length classes R = ceil(columns / 256), up to the 2048 columns the register-resident kernels take"""
    if not _SET:
        qlens = [0, 1, 2, 7, 64, 200, 333, 400]
        qs = [residues(MT19937(81000 + n), ln) for n, ln in enumerate(qlens)]
        h1, h2 = homolog_pair(81500, 200)
        qs[HOMOLOG_ROW] = h1
        tlens = [0, 1, 5, 253, 254, 255, 256, 257, 509, 510, 511, 512, 513, 765, 766, 767, 1021, 1022, 1023, 1024, 1025, 1279, 1500,
                 2045, 2046]
        ts = [residues(MT19937(82000 + n), ln) for n, ln in enumerate(tlens)]
        ts.append(h2)
        _SET["qs"], _SET["ts"] = qs, ts
    return _SET["qs"], _SET["ts"]


_REF = {}


def background(key, q_index, q, ts, blosum62, n, seed=SEED, mode=aln_amd.LOCAL, gi=11, ge=1):
    """[n, len(ts)] int64: the dense path's scores of shuffles 0..n-1 of query q (pool index q_index) against every template
    of ts; computed once per (set, row, seed, align type) for the largest n asked so far and never modified"""
    k = (key, q_index, seed, mode, gi, ge)
    if k not in _REF or _REF[k].shape[0] < n:
        strings = [aln_amd.shuffle_query(seed, q_index, s, q) for s in range(max(n, 9))]
        d = aln_amd.score_all_vs_all(gpu_util.ctx(), strings, ts, blosum62[0], blosum62[1], gi, ge, align_type=mode)
        assert (d == np.rint(d)).all()
        d = d.astype(np.int64)
        d.setflags(write=False)
        _REF[k] = d
    return _REF[k][:n]


def check_stats(stats, hits, n_hits, ref_of_row, n):
    """ref_of_row(r) -> [>= n, n_templates] background of row r"""
    rows, K = hits.shape
    assert stats.shape == (rows, K) and stats.dtype == aln_amd.HIT_STATS_DTYPE
    checked = 0
    for r in range(rows):
        for k in range(K):
            st = stats[r, k]
            if k >= n_hits[r]:
                assert (int(st["sum"]), int(st["sumsq"]), int(st["n"])) == (0, 0, 0) and st["z"].view(U32) == 0, (r, k)
                continue
            ref = ref_of_row(r)
            assert ref.shape[0] >= n
            col = [int(v) for v in ref[:n, hits["t"][r, k]]]           # shuffle s does not depend on n: the first n rows
            s, ss = sum(col), sum(v * v for v in col)
            assert (int(st["sum"]), int(st["sumsq"]), int(st["n"])) == (s, ss, n), (r, k, int(hits["t"][r, k]), st, s, ss)
            want = z_restated(n, hits["score"][r, k], s, ss)
            assert st["z"].view(U32) == want.view(U32), (r, k, st["z"], want)
            checked += 1
    return checked


_HITS = {}


def searched(blosum62, mode=aln_amd.LOCAL, K=5):
    if (mode, K) not in _HITS:
        qs, ts = ragged_set()
        hits, n_hits = aln_amd.search_topk(gpu_util.ctx(), qs, ts, blosum62[0], blosum62[1], 11, 1, K, align_type=mode)
        hits.setflags(write=False)
        n_hits.setflags(write=False)
        _HITS[(mode, K)] = (hits, n_hits)
    return _HITS[(mode, K)]


def ragged_ref(blosum62, n, mode=aln_amd.LOCAL, seed=SEED, first=0):
    qs, ts = ragged_set()
    return lambda r: background("ragged", first + r, qs[first + r], ts, blosum62, n, seed, mode)


# ---- 1. the ragged set ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 33, 64, 65])
def test_ragged_set(n, blosum62):
    """n = 1: no spread (z = 0); 33 / 64 / 65: both sides of the boundary between two waves' groups of shuffles"""
    alpha, table = blosum62
    qs, ts = ragged_set()
    hits, n_hits = searched(blosum62)
    assert (n_hits == 5).all()
    classes = {(len(ts[t]) + 2 + 255) // 256 for t in hits["t"].ravel()}
    assert len(classes) >= 3                                 # the hits do spread over the length classes
    stats = aln_amd.hits_zscores(gpu_util.ctx(), qs, ts, hits, n_hits, alpha, table, 11, 1, n, seed=SEED)
    assert check_stats(stats, hits, n_hits, ragged_ref(blosum62, S_MAX), n) == 40
    if n == 1:
        assert (stats["z"].view(U32) == 0).all()
    else:
        assert (stats["z"][HOMOLOG_ROW:] != 0).any()


def test_every_template_of_the_set(blosum62):
    """K = number of templates: every length class 1..8 of the set, both kernels' degenerate shapes (0 and 1 residues)"""
    alpha, table = blosum62
    qs, ts = ragged_set()
    hits, n_hits = searched(blosum62, K=len(ts))
    stats = aln_amd.hits_zscores(gpu_util.ctx(), qs, ts, hits, n_hits, alpha, table, 11, 1, 9, seed=SEED)
    assert check_stats(stats, hits, n_hits, ragged_ref(blosum62, S_MAX), 9) == len(qs) * len(ts)


@pytest.mark.parametrize("mode", MODES)
def test_all_align_types(mode, blosum62):
    alpha, table = blosum62
    qs, ts = ragged_set()
    for K in (5, len(ts)):
        hits, n_hits = searched(blosum62, mode, K)
        stats = aln_amd.hits_zscores(gpu_util.ctx(), qs, ts, hits, n_hits, alpha, table, 11, 1, 9, seed=SEED, align_type=mode)
        assert check_stats(stats, hits, n_hits, ragged_ref(blosum62, 9, mode), 9) == len(qs) * K
    if mode == aln_amd.GLOBAL:
        assert (stats["sum"] < 0).any()


def test_length_class_seven(blosum62):
    """1537 .. 1792 columns: the one class the ragged set has no template of"""
    alpha, table = blosum62
    ctx = gpu_util.ctx()
    qs = [residues(MT19937(83000), 50), residues(MT19937(83001), 21)]
    ts = [residues(MT19937(83100 + n), ln) for n, ln in enumerate((1536, 1700, 1790))]
    for mode in (aln_amd.LOCAL, aln_amd.GLOBAL):
        hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, 3, align_type=mode)
        stats = aln_amd.hits_zscores(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, 5, seed=3, align_type=mode)
        ref = lambda r: background("class7", r, qs[r], ts, blosum62, 5, 3, mode)   # noqa: E731
        assert check_stats(stats, hits, n_hits, ref, 5) == 6


# ---- 2. independence -----------------------------------------------------------------------------------------------------
def test_independence_of_block_chunking_and_repetition(blosum62):
    alpha, table = blosum62
    qs, ts = ragged_set()
    ctx = gpu_util.ctx()
    hits, n_hits = searched(blosum62)
    args = (alpha, table, 11, 1, 33)
    full = aln_amd.hits_zscores(ctx, qs, ts, hits, n_hits, *args, seed=SEED)
    again = aln_amd.hits_zscores(ctx, qs, ts, hits, n_hits, *args, seed=SEED)
    assert full.tobytes() == again.tobytes()
    blk = aln_amd.hits_zscores(ctx, qs, ts, hits[4:6], n_hits[4:6], *args, seed=SEED, q_begin=4)
    assert blk.tobytes() == full[4:6].tobytes()
    assert check_stats(blk, hits[4:6], n_hits[4:6], ragged_ref(blosum62, S_MAX, first=4), 33) == 10
    for chunk in (1, 3):
        with ctx.hints(zscore_chunk_rows=chunk):
            assert ctx.get_hint("zscore_chunk_rows") == chunk
            cut = aln_amd.hits_zscores(ctx, qs, ts, hits, n_hits, *args, seed=SEED)
        assert ctx.get_hint("zscore_chunk_rows") == 0
        assert cut.tobytes() == full.tobytes(), chunk
    other = aln_amd.hits_zscores(ctx, qs, ts, hits, n_hits, *args, seed=SEED + 1)
    assert (other["sum"] != full["sum"]).any()
    assert check_stats(other, hits, n_hits, ragged_ref(blosum62, 33, seed=SEED + 1), 33) == 40


# ---- 3. hand-made lists --------------------------------------------------------------------------------------------------
def hand_hits(lists, K, dense):
    """lists[r] = template indices of row r -> hits[rows, K], n_hits (scores from the dense matrix of the real queries)"""
    hits = np.zeros((len(lists), K), dtype=aln_amd.HIT_DTYPE)
    hits["t"] = -1
    hits["q_end"] = hits["t_end"] = -1
    n_hits = np.array([len(x) for x in lists], dtype=np.int32)
    for r, x in enumerate(lists):
        for k, t in enumerate(x):
            hits[r, k] = (t, dense[r, t], -1, -1)
    return hits, n_hits


def test_hand_made_lists(blosum62):
    alpha, table = blosum62
    qs, ts = ragged_set()
    ctx = gpu_util.ctx()
    dense = aln_amd.score_all_vs_all(ctx, qs, ts, alpha, table, 11, 1)
    last = len(ts) - 1
    lists = [[3, last], [10], [], [8, 8, 2], [], [last, 0, last, 24], [], [1]]
    hits, n_hits = hand_hits(lists, 4, dense)
    hits["t"][2, :] = 99999                                  # slots beyond n_hits are not read
    n = 12
    stats = aln_amd.hits_zscores(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, n, seed=SEED)
    assert check_stats(stats, hits, n_hits, ragged_ref(blosum62, S_MAX), n) == sum(len(x) for x in lists)
    assert stats[3, 0].tobytes() == stats[3, 1].tobytes()    # the same template twice in a row
    assert stats[5, 0].tobytes() == stats[5, 2].tobytes() and stats[5, 0]["z"] > 0
    zero = np.zeros(1, dtype=aln_amd.HIT_STATS_DTYPE).tobytes()
    for r in (2, 4, 6):                                      # n_hits = 0: all padding
        assert stats[r].tobytes() == zero * 4
    assert stats[1, 1:].tobytes() == zero * 3
    # an empty and a one-residue query have one "permutation": no spread, z = 0, n as asked
    for r in (0, 1):
        for k in range(n_hits[r]):
            st = stats[r, k]
            assert st["n"] == n and n * int(st["sumsq"]) == int(st["sum"]) ** 2 and st["z"].view(U32) == 0, (r, k)


# ---- 4. templates beyond 2048 columns ------------------------------------------------------------------------------------
def test_full_build_route(blosum62):
    alpha, table = blosum62
    ctx = gpu_util.ctx()
    qs = [residues(MT19937(84000), 30), residues(MT19937(84001), 12)]
    ts = [residues(MT19937(84100), 2100), residues(MT19937(84101), 40), residues(MT19937(84102), 2047)]
    qs[0] = ts[0][1800:1830]                                 # found in the long template
    dense = aln_amd.score_all_vs_all(ctx, qs, ts, alpha, table, 11, 1)
    n = 8
    ref = lambda r: background("long", r, qs[r], ts, blosum62, n, 5)   # noqa: E731
    hits, n_hits = hand_hits([[0], []], 1, dense)
    stats = aln_amd.hits_zscores(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, n, seed=5)
    assert check_stats(stats, hits, n_hits, ref, n) == 1 and stats[0, 0]["z"] > 3
    hits, n_hits = hand_hits([[1, 0], [0, 2, 1]], 3, dense)  # short and long hits in one row
    stats = aln_amd.hits_zscores(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, n, seed=5)
    assert check_stats(stats, hits, n_hits, ref, n) == 5
    refg = lambda r: background("long", r, qs[r], ts, blosum62, n, 5, aln_amd.GLOBAL)   # noqa: E731
    dg = aln_amd.score_all_vs_all(ctx, qs, ts, alpha, table, 11, 1, align_type=aln_amd.GLOBAL)
    hits, n_hits = hand_hits([[0, 1], [2, 0, 0]], 3, dg)
    stats = aln_amd.hits_zscores(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, n, seed=5, align_type=aln_amd.GLOBAL)
    assert check_stats(stats, hits, n_hits, refg, n) == 5


# ---- 5. meaning ----------------------------------------------------------------------------------------------------------
def test_the_homolog_stands_out(blosum62):
    alpha, table = blosum62
    qs, ts = ragged_set()
    hits, n_hits = searched(blosum62, K=len(ts))
    r = HOMOLOG_ROW
    stats = aln_amd.hits_zscores(gpu_util.ctx(), qs, ts, hits[r:r + 1], n_hits[r:r + 1], alpha, table, 11, 1, 64, seed=SEED, q_begin=r)
    assert check_stats(stats, hits[r:r + 1], n_hits[r:r + 1], ragged_ref(blosum62, S_MAX, first=r), 64) == len(ts)
    z = stats["z"][0]
    k = int(np.nonzero(hits["t"][r] == len(ts) - 1)[0][0])
    assert z[k] > 0 and z[k] == z.max() and (z[np.arange(len(ts)) != k] < z[k]).all()


# ---- 6. arguments --------------------------------------------------------------------------------------------------------
def raw_call(qs, ts, blosum62, K, hits, n_hits, n_shuffles, gi=11.0, ge=1.0, table=None, q_begin=0, q_end=None):
    """the C entry itself with a stats buffer holding a pattern -> (status, buffer untouched?)"""
    alpha = blosum62[0]
    qp, tp = aln_amd.SeqPool(qs), aln_amd.SeqPool(ts)
    tab = np.ascontiguousarray(blosum62[1] if table is None else table, dtype=np.float32)
    ab = alpha.encode()
    sub = aln_amd.AlnSubmatrix(len(alpha), ab, tab.ctypes.data_as(C.POINTER(C.c_float)))
    g = aln_amd.AlnGap()
    g.model, g.align_type, g.gap_init, g.gap_extn = aln_amd.GAP_AFFINE_CONST, aln_amd.LOCAL, gi, ge
    hits = np.ascontiguousarray(hits, dtype=aln_amd.HIT_DTYPE)
    n_hits = np.ascontiguousarray(n_hits, dtype=np.int32)
    stats = np.full(max(hits.size, 1) * 24, 0x5A, dtype=np.uint8)
    before = stats.tobytes()
    rc = aln_amd.lib().aln_hits_zscores(gpu_util.ctx().h, C.byref(qp.c), C.byref(tp.c), C.byref(sub), C.byref(g), q_begin,
                                        len(qs) if q_end is None else q_end, K, hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)),
                                        n_hits.ctypes.data_as(C.POINTER(C.c_int32)), n_shuffles, 7,
                                        stats.ctypes.data_as(C.POINTER(aln_amd.AlnHitStats)))
    return rc, stats.tobytes() == before


def test_argument_checks(blosum62):
    qs, ts = ["ACDEFGHIKL", "WWPGA"], ["ACDEFGHIKL", "LKIHGFEDCA", "WW"]

    def hits_of(K, t=0, n=1):
        h = np.zeros((2, max(K, 1)), dtype=aln_amd.HIT_DTYPE)
        h["t"] = t
        h["score"] = 10.0
        return h, np.full(2, n, dtype=np.int32)

    h, nh = hits_of(2)
    assert raw_call(qs, ts, blosum62, 2, h, nh, 4) == (0, False)               # the valid call the others deviate from
    for K in (0, 1025):
        h, nh = hits_of(K)
        assert raw_call(qs, ts, blosum62, K, h, nh, 4) == (aln_amd.E_ARG, True), K
    h, nh = hits_of(2)
    for S in (0, 4097):
        assert raw_call(qs, ts, blosum62, 2, h, nh, S) == (aln_amd.E_ARG, True), S
    assert raw_call(qs, ts, blosum62, 2, h, np.array([1, 3], np.int32), 4) == (aln_amd.E_ARG, True)
    assert raw_call(qs, ts, blosum62, 2, h, np.array([-1, 1], np.int32), 4) == (aln_amd.E_ARG, True)
    for t in (-1, len(ts)):
        bad = h.copy()
        bad["t"][1, 0] = t
        assert raw_call(qs, ts, blosum62, 2, bad, nh, 4) == (aln_amd.E_ARG, True), t
        bad["t"][1, 0] = 0
        bad["t"][1, 1] = t                                                     # an unused slot may hold anything
        assert raw_call(qs, ts, blosum62, 2, bad, nh, 4) == (0, False), t
    frac = np.array(blosum62[1], dtype=np.float32).copy()
    frac[3, 5] = 0.5
    assert raw_call(qs, ts, blosum62, 2, h, nh, 4, table=frac) == (aln_amd.E_NOT_INTEGRAL, True)
    assert raw_call(qs, ts, blosum62, 2, h, nh, 4, ge=0.5) == (aln_amd.E_NOT_INTEGRAL, True)
    assert raw_call(["ACJ", "WW"], ts, blosum62, 2, h, nh, 4) == (aln_amd.E_RESIDUE, True)
    assert raw_call(qs, ts, blosum62, 2, h, nh, 4, q_begin=1, q_end=0) == (aln_amd.E_ARG, True)
    assert raw_call(qs, ts, blosum62, 2, h, nh, 4, q_begin=1, q_end=1) == (0, True)   # nothing to do, nothing written
    # through the wrapper: the status arrives as an exception
    with pytest.raises(aln_amd.AlnError) as ei:
        aln_amd.hits_zscores(gpu_util.ctx(), qs, ts, h, nh, blosum62[0], blosum62[1], 11, 1, 0)
    assert ei.value.code == aln_amd.E_ARG
    with pytest.raises(aln_amd.AlnError) as ei:
        gpu_util.ctx().set_hint("zscore_chunk_cols", 1)
    assert ei.value.code == aln_amd.E_ARG
    # no template at all: a list without used slots is all padding
    stats = aln_amd.hits_zscores(gpu_util.ctx(), qs, [], h, np.zeros(2, np.int32), blosum62[0], blosum62[1], 11, 1, 4)
    assert stats.tobytes() == bytes(stats.nbytes)
