"""-m gpu: aln_hits_zscores_profiles — shuffle z-scores for the hits of a profile search; the device reads ONE resident copy of
a profile's rows in permuted order (csrc/search_zscore.hip).

  1  profiles derived from residue queries equal aln_hits_zscores byte for byte: every length class, the degenerate shapes, both
     sides of the shuffle-group boundary, all five align types
  2  rows no table holds against the int64 reference (profile_zscore_cases), every fill and ring boundary of the staging
  3  wide templates (classes 6, 7, 8) and a 300-row profile against the dense path on the device
  4  independence of repetition, row block, chunking, per-chunk row upload; the seed; n = 33 / 65 share their first shuffles
  5  a 2100-residue template: the full-build route
  6  hand-made lists
  7  the argument checks, in the header's order, nothing written"""
import ctypes as C

import numpy as np
import pytest

import aln_amd
import gpu_util
import profile_cases as pc
import profile_zscore_cases as pz
import search_cases as sc
from aln_amd.synth import MT19937, homolog_pair, residues

pytestmark = pytest.mark.gpu

U32 = np.uint32
SEED = 2024
ALPHA = sc.ALPHA
MODES = (aln_amd.LOCAL, aln_amd.GLOBAL, aln_amd.GLOBAL_LOCAL, aln_amd.LOCAL_GLOBAL, aln_amd.SEMI_LOCAL)
ZERO = np.zeros(1, dtype=aln_amd.HIT_STATS_DTYPE).tobytes()


def pool(profiles):
    return aln_amd.QueryProfiles([np.asarray(p, np.float32) for p in profiles], ALPHA)


def every_template(dense):
    """hits[rows, n_t]: slot k of every row is template k with the dense score"""
    rows, n_t = dense.shape
    hits = np.zeros((rows, n_t), dtype=aln_amd.HIT_DTYPE)
    hits["t"] = np.arange(n_t)[None, :]
    hits["score"] = dense
    hits["q_end"] = hits["t_end"] = -1
    return hits, np.full(rows, n_t, np.int32)


def hand_hits(lists, K, dense):
    hits = np.zeros((len(lists), K), dtype=aln_amd.HIT_DTYPE)
    hits["t"] = -1
    hits["q_end"] = hits["t_end"] = -1
    n_hits = np.array([len(x) for x in lists], dtype=np.int32)
    for r, x in enumerate(lists):
        for k, t in enumerate(x):
            hits[r, k] = (t, dense[r, t], -1, -1)
    return hits, n_hits


_BG = {}


def background(key, q_index, profile, ts, n, seed, mode, gi=11, ge=1):
    """[n, len(ts)] int64, the dense path on the device: the n permuted copies of the profile (profile_zscore_cases.shuffled)
    as a pool of their own through aln_score_profiles_vs_all; computed once per key and read-only"""
    k = (key, q_index, seed, mode, gi, ge)
    if k not in _BG or _BG[k].shape[0] < n:
        copies = pool([pz.shuffled(seed, q_index, s, profile) for s in range(n)])
        d = aln_amd.score_profiles_vs_all(gpu_util.ctx(), copies, ts, gi, ge, align_type=mode)
        assert (d == np.rint(d)).all()
        d = d.astype(np.int64)
        d.setflags(write=False)
        _BG[k] = d
    return _BG[k][:n]


def check_stats(stats, hits, n_hits, ref_of_row, n):
    """ref_of_row(r) -> [>= n, n_templates] background of row r; -> the number of used slots"""
    rows, K = hits.shape
    assert stats.shape == (rows, K) and stats.dtype == aln_amd.HIT_STATS_DTYPE
    checked = 0
    for r in range(rows):
        for k in range(K):
            st = stats[r, k]
            if k >= n_hits[r]:
                assert st.tobytes() == ZERO, (r, k)
                continue
            col = [int(v) for v in ref_of_row(r)[:n, hits["t"][r, k]]]
            s, ss = sum(col), sum(v * v for v in col)
            assert (int(st["sum"]), int(st["sumsq"]), int(st["n"])) == (s, ss, n), (r, k, int(hits["t"][r, k]), st, s, ss)
            want = sc.z_restated(n, hits["score"][r, k], s, ss)
            assert st["z"].view(U32) == want.view(U32), (r, k, st["z"], want)
            checked += 1
    return checked


# ---- 1. equal to the residue entry -----------------------------------------------------------------------------------------
_SET = {}


def ragged_set(blosum62):
    """the set of tests/test_gpu_zscores.py, rebuilt from the same seeds: 8 queries of 0..400 residues, 26 templates on every
    boundary of the length classes up to 2046 residues; + the queries as derived profiles"""
    if not _SET:
        qlens = [0, 1, 2, 7, 64, 200, 333, 400]
        qs = [residues(MT19937(81000 + n), ln) for n, ln in enumerate(qlens)]
        h1, h2 = homolog_pair(81500, 200)
        qs[5] = h1
        tlens = [0, 1, 5, 253, 254, 255, 256, 257, 509, 510, 511, 512, 513, 765, 766, 767, 1021, 1022, 1023, 1024, 1025, 1279, 1500,
                 2045, 2046]
        ts = [residues(MT19937(82000 + n), ln) for n, ln in enumerate(tlens)]
        ts.append(h2)
        _SET["qs"], _SET["ts"] = qs, ts
        _SET["qp"] = aln_amd.profiles_from_sequences(qs, blosum62[0], blosum62[1])
    return _SET["qs"], _SET["ts"], _SET["qp"]


_HITS = {}


def searched(blosum62, mode=aln_amd.LOCAL, K=5):
    if (mode, K) not in _HITS:
        qs, ts, _ = ragged_set(blosum62)
        hits, n_hits = aln_amd.search_topk(gpu_util.ctx(), qs, ts, blosum62[0], blosum62[1], 11, 1, K, align_type=mode)
        hits.setflags(write=False)
        n_hits.setflags(write=False)
        _HITS[(mode, K)] = (hits, n_hits)
    return _HITS[(mode, K)]


def both_entries(blosum62, hits, n_hits, n, mode=aln_amd.LOCAL, seed=SEED, q_begin=0):
    alpha, table = blosum62
    qs, ts, qp = ragged_set(blosum62)
    ctx = gpu_util.ctx()
    got = aln_amd.hits_zscores_profiles(ctx, qp, ts, hits, n_hits, 11, 1, n, seed=seed, q_begin=q_begin, align_type=mode)
    want = aln_amd.hits_zscores(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, n, seed=seed, q_begin=q_begin, align_type=mode)
    return got, want


@pytest.mark.parametrize("n", [1, 2, 33, 64, 65])
def test_derived_profiles_equal_the_residue_entry(n, blosum62):
    """33 / 64 / 65: both sides of the boundary between two waves' groups of shuffles"""
    hits, n_hits = searched(blosum62)
    assert (n_hits == 5).all()
    got, want = both_entries(blosum62, hits, n_hits, n)
    assert got.tobytes() == want.tobytes()
    assert (got["n"] == n).all()
    if n > 1:
        assert (got["z"] != 0).any()


@pytest.mark.parametrize("mode", MODES)
def test_derived_profiles_in_all_align_types(mode, blosum62):
    """K = 26: every template of the set, so every length class 1..8 and the degenerate shapes (0 and 1 residues)"""
    _, ts, _ = ragged_set(blosum62)
    for K in (5, len(ts)):
        hits, n_hits = searched(blosum62, mode, K)
        got, want = both_entries(blosum62, hits, n_hits, 9, mode)
        assert got.tobytes() == want.tobytes(), K
        assert (got["n"] == 9).all()
    assert (np.int64(9) * got["sumsq"] != got["sum"] * got["sum"]).any()


# ---- 2. rows no table holds, against the int64 reference ---------------------------------------------------------------------
_LEN = {}


def length_reference(mode):
    """(profile, template) -> (sum, sumsq) of 5 shuffles under seed 2024, system 11/1; computed once per align type"""
    if mode not in _LEN:
        profiles, ts = pc.length_set()
        _, gi, ge = pc.LENGTH_SYSTEM
        _LEN[mode] = {(q, t): pz.zstats_reference(SEED, q, p, tt, mode, gi, ge, 5)[:2]
                      for q, p in enumerate(profiles) for t, tt in enumerate(ts)}
    return _LEN[mode]


@pytest.mark.parametrize("mode", MODES)
def test_position_specific_rows(mode):
    """18 profiles of 0 .. 130 interior rows (every boundary of the 8-row copies and of the ring of 32) + the peaked and the
    all-zero one, every one of the 10 templates a hit.

    The reference must show spread in at least half of the slots, so that a kernel that ignores the order cannot pass (measured:
    110 .. 125 of 180 per align type).  Where the reference has none — against template 0, 257 times the same letter, the
    profiles of 0, 1 and 2 rows and the all-zero one in every align type, the peaked one wherever the peak's position cannot
    matter (not GLOBAL and LOCAL_GLOBAL, whose end gaps price it) — z must be exactly 0 with n as asked."""
    profiles, ts = pc.length_set()
    _, gi, ge = pc.LENGTH_SYSTEM
    n = 5
    ref = length_reference(mode)
    spread = sum(1 for s, ss in ref.values() if n * ss - s * s != 0)
    assert 2 * spread >= len(ref), spread
    flat = [q for q in (0, 1, 2, 16, 17) if not (q == 16 and mode in (aln_amd.GLOBAL, aln_amd.LOCAL_GLOBAL))]
    assert len(ts[0]) == 257 and len(set(ts[0])) == 1
    for q in flat:
        s, ss = ref[(q, 0)]
        assert n * ss - s * s == 0, q
    ctx = gpu_util.ctx()
    qp = pool(profiles)
    dense = aln_amd.score_profiles_vs_all(ctx, qp, ts, gi, ge, align_type=mode)
    hits, n_hits = every_template(dense)
    stats = aln_amd.hits_zscores_profiles(ctx, qp, ts, hits, n_hits, gi, ge, n, seed=SEED, align_type=mode)
    for q in range(len(profiles)):
        for t in range(len(ts)):
            st = stats[q, t]
            s, ss = ref[(q, t)]
            assert (int(st["sum"]), int(st["sumsq"]), int(st["n"])) == (s, ss, n), (q, t, st, s, ss)
            want = sc.z_restated(n, dense[q, t], s, ss)
            assert st["z"].view(U32) == want.view(U32), (q, t, st["z"], want)
    for q in flat:
        assert stats[q, 0]["z"].view(U32) == 0 and stats[q, 0]["n"] == n, q


# ---- 3. wide templates and many ring revolutions -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [aln_amd.LOCAL, aln_amd.GLOBAL, aln_amd.SEMI_LOCAL])
def test_wide_templates(mode):
    profiles, ts = pc.wide_set(sc.TABLES["blosum62"])
    assert len(profiles[2]) == 300
    ctx = gpu_util.ctx()
    qp = pool(profiles)
    hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, ts, 11, 1, 5, align_type=mode)
    assert (n_hits == 5).all()
    stats = aln_amd.hits_zscores_profiles(ctx, qp, ts, hits, n_hits, 11, 1, 3, seed=SEED, align_type=mode)
    ref = lambda r: background("wide", r, profiles[r], ts, 3, SEED, mode)   # noqa: E731
    assert check_stats(stats, hits, n_hits, ref, 3) == 15
    assert (np.int64(3) * stats["sumsq"] != stats["sum"] * stats["sum"]).any()


# ---- 4. independence -----------------------------------------------------------------------------------------------------------
def test_independence_of_block_chunking_and_repetition(blosum62):
    qs, ts, qp = ragged_set(blosum62)
    ctx = gpu_util.ctx()
    hits, n_hits = searched(blosum62)
    call = lambda h=hits, nh=n_hits, n=33, **kw: aln_amd.hits_zscores_profiles(ctx, qp, ts, h, nh, 11, 1, n, **kw)   # noqa: E731
    full = call(seed=SEED)
    assert call(seed=SEED).tobytes() == full.tobytes()
    blk = call(hits[4:6], n_hits[4:6], seed=SEED, q_begin=4)
    assert blk.tobytes() == full[4:6].tobytes()
    for hint, values in (("zscore_chunk_rows", (1, 3)), ("zscore_rows_per_chunk", (1,))):
        for v in values:
            with ctx.hints(**{hint: v}):
                assert ctx.get_hint(hint) == v
                cut = call(seed=SEED)
            assert ctx.get_hint(hint) == 0
            assert cut.tobytes() == full.tobytes(), (hint, v)
    with ctx.hints(zscore_chunk_rows=3, zscore_rows_per_chunk=1):
        assert call(seed=SEED).tobytes() == full.tobytes()
        assert call(hits[4:6], n_hits[4:6], seed=SEED, q_begin=4).tobytes() == full[4:6].tobytes()
    other = call(seed=SEED + 1)
    assert (other["sum"] != full["sum"]).any()
    # shuffle s does not depend on n: row 4 (64 rows) against the dense path of its 65 permuted copies
    assert blosum62[0] == ALPHA and len(qp.profiles[4]) == 64
    prof = qp.profiles[4].astype(np.int64)
    ref = lambda r: background("ragged4", 4, prof, ts, 65, SEED, aln_amd.LOCAL)   # noqa: E731
    for n in (33, 65):
        st = call(hits[4:5], n_hits[4:5], n, seed=SEED, q_begin=4)
        assert check_stats(st, hits[4:5], n_hits[4:5], ref, n) == 5
    assert full[4:5].tobytes() == call(hits[4:5], n_hits[4:5], 33, seed=SEED, q_begin=4).tobytes()


# ---- 5. templates beyond 2048 columns ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [aln_amd.LOCAL, aln_amd.GLOBAL])
def test_full_build_route(mode):
    profiles, ts = pc.mixed_set()
    assert len(ts[1]) == 2100
    ctx = gpu_util.ctx()
    qp = pool(profiles)
    dense = aln_amd.score_profiles_vs_all(ctx, qp, ts, 11, 1, align_type=mode)
    n = 4
    ref = lambda r: background("mixed", r, profiles[r], ts, n, 5, mode)   # noqa: E731
    for lists, K in (([[1], []], 1), ([[0, 1], [1, 2, 4]], 3), ([[1, 1], [1, 0, 1]], 3)):
        hits, n_hits = hand_hits(lists, K, dense)
        stats = aln_amd.hits_zscores_profiles(ctx, qp, ts, hits, n_hits, 11, 1, n, seed=5, align_type=mode)
        assert check_stats(stats, hits, n_hits, ref, n) == sum(len(x) for x in lists), lists
    assert stats[0, 0].tobytes() == stats[0, 1].tobytes() and stats[1, 0].tobytes() == stats[1, 2].tobytes()
    if mode == aln_amd.LOCAL:
        assert stats[0, 0]["z"] > 3                          # the long template ends in a noisy copy of profile 0's query


# ---- 6. hand-made lists --------------------------------------------------------------------------------------------------------
def test_hand_made_lists(blosum62):
    alpha, table = blosum62
    qs, ts, qp = ragged_set(blosum62)
    ctx = gpu_util.ctx()
    dense = aln_amd.score_all_vs_all(ctx, qs, ts, alpha, table, 11, 1)
    last = len(ts) - 1
    lists = [[3, last], [10], [], [8, 8, 2], [], [last, 0, last, 24], [], [1]]
    hits, n_hits = hand_hits(lists, 4, dense)
    hits["t"][2, :] = 99999                                  # slots beyond n_hits are not read
    hits["t"][1, 1:] = 99999
    n = 12
    stats = aln_amd.hits_zscores_profiles(ctx, qp, ts, hits, n_hits, 11, 1, n, seed=SEED)
    want = aln_amd.hits_zscores(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, n, seed=SEED)
    assert stats.tobytes() == want.tobytes()
    assert stats[3, 0].tobytes() == stats[3, 1].tobytes() and stats[3, 0]["n"] == n
    assert stats[5, 0].tobytes() == stats[5, 2].tobytes() and stats[5, 0]["z"] > 0
    for r in (2, 4, 6):                                      # n_hits = 0: all padding
        assert stats[r].tobytes() == ZERO * 4
    assert stats[1, 1:].tobytes() == ZERO * 3


# ---- 7. arguments ----------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    L = aln_amd.lib()
    ctx = gpu_util.ctx()
    E = aln_amd
    good = [np.ones((3, pc.N)), np.full((5, pc.N), 2.0)]
    qp = pool(good)
    tp = aln_amd.SeqPool(["WWW", "AC", "ACDEFGHIKL"])
    n_t = 3

    def gap(ge=1.0, align_type=aln_amd.LOCAL):
        g = aln_amd.AlnGap()
        g.model, g.align_type, g.gap_init, g.gap_extn = aln_amd.GAP_AFFINE_CONST, align_type, 11.0, ge
        return g

    def qprof(**kw):
        d = dict(n_seqs=qp.c.n_seqs, offsets=qp.c.offsets, rows=qp.c.rows, n=qp.c.n, alphabet=qp.c.alphabet)
        d.update(kw)
        return aln_amd.AlnQProfiles(d["n_seqs"], d["offsets"], d["rows"], d["n"], d["alphabet"])

    def hits_of(K, t=0, n=1):
        h = np.zeros((2, max(K, 1)), dtype=aln_amd.HIT_DTYPE)
        h["t"] = t
        h["score"] = 10.0
        return h, np.full(2, n, dtype=np.int32)

    def call(K=2, hits=None, n_hits=None, S=4, prof=None, templ=None, g=None, qb=0, qe=2, null=None):
        """-> (status, stats buffer untouched?)"""
        h, nh = hits_of(K)
        h = h if hits is None else np.ascontiguousarray(hits, dtype=aln_amd.HIT_DTYPE)
        nh = nh if n_hits is None else np.ascontiguousarray(n_hits, dtype=np.int32)
        stats = np.full(max(h.size, 1) * 24, 0x5A, dtype=np.uint8)
        before = stats.tobytes()
        hp = None if null == "hits" else h.ctypes.data_as(C.POINTER(aln_amd.AlnHit))
        np_ = None if null == "n_hits" else nh.ctypes.data_as(C.POINTER(C.c_int32))
        sp = None if null == "stats" else stats.ctypes.data_as(C.POINTER(aln_amd.AlnHitStats))
        status = L.aln_hits_zscores_profiles(ctx.h, C.byref(qp.c if prof is None else prof), C.byref(tp.c if templ is None else templ),
                                             C.byref(gap() if g is None else g), qb, qe, K, hp, np_, S, 7, sp)
        return status, stats.tobytes() == before

    bad_t = aln_amd.SeqPool(["WWW", "A?", "AC"])
    frac = pool([np.ones((3, pc.N)), np.full((5, pc.N), 2.0)])
    frac.rows[7, 4] = 0.5                                    # an interior row of profile 1 (pool rows 5 .. 11)
    frac_c = frac.c

    assert call() == (0, False)                              # the valid call the others deviate from
    # 1. NULL hits / n_hits / stats, K, n_shuffles — before anything else
    for null in ("hits", "n_hits", "stats"):
        assert call(null=null) == (E.E_ARG, True), null
    for K in (0, 1025):
        assert call(K=K) == (E.E_ARG, True), K
        assert call(K=K, templ=bad_t.c) == (E.E_ARG, True), K
    for S in (0, 4097):
        assert call(S=S) == (E.E_ARG, True), S
        assert call(S=S, templ=bad_t.c) == (E.E_ARG, True), S
    # 2. aln_score_profiles_vs_all's checks, in its order
    assert call(qb=1, qe=0) == (E.E_ARG, True)
    assert call(qb=-1) == (E.E_ARG, True) and call(qe=3) == (E.E_ARG, True)
    assert call(g=gap(align_type=5)) == (E.E_ARG, True)
    for what, p in (("n 0", qprof(n=0)), ("n 31", qprof(n=31)), ("alphabet", qprof(alphabet=None))):
        assert call(prof=p) == (E.E_ARG, True), what
        assert call(prof=p, templ=bad_t.c) == (E.E_ARG, True), what          # the descriptor comes before the residues
    short = np.array([0, 5, 6], np.int64)
    assert call(prof=qprof(offsets=short.ctypes.data_as(C.POINTER(C.c_int64)))) == (E.E_ARG, True)
    assert call(templ=bad_t.c) == (E.E_RESIDUE, True)
    assert call(templ=bad_t.c, n_hits=[-1, 1]) == (E.E_RESIDUE, True)        # ... and the residues before the hit lists
    assert call(templ=bad_t.c, prof=frac_c) == (E.E_RESIDUE, True)
    # 3. n_hits and the used slots' t
    assert call(n_hits=[1, 3]) == (E.E_ARG, True)
    assert call(n_hits=[-1, 1]) == (E.E_ARG, True)
    assert call(n_hits=[-1, 1], prof=frac_c) == (E.E_ARG, True)              # ... before ALN_E_NOT_INTEGRAL
    h, nh = hits_of(2)
    for t in (-1, n_t):
        bad = h.copy()
        bad["t"][1, 0] = t
        assert call(hits=bad) == (E.E_ARG, True), t
        assert call(hits=bad, g=gap(ge=0.5)) == (E.E_ARG, True), t
        bad["t"][1, 0] = 0
        bad["t"][1, 1] = t                                   # an unused slot may hold anything
        assert call(hits=bad) == (0, False), t
    # 4. ALN_E_NOT_INTEGRAL last
    assert call(prof=frac_c) == (E.E_NOT_INTEGRAL, True)
    assert call(g=gap(ge=0.5)) == (E.E_NOT_INTEGRAL, True)
    # q_begin == q_end: ALN_OK, nothing written — also with lists that would be refused
    assert call(qb=1, qe=1) == (0, True)
    assert call(qb=1, qe=1, n_hits=[-1, 1]) == (0, True)
    # through the wrapper: the status arrives as an exception
    with pytest.raises(aln_amd.AlnError) as ei:
        aln_amd.hits_zscores_profiles(ctx, qp, tp, h, nh, 11, 1, 0)
    assert ei.value.code == E.E_ARG
    # no template at all: a list without used slots is all padding
    stats = aln_amd.hits_zscores_profiles(ctx, qp, [], h, np.zeros(2, np.int32), 11, 1, 4)
    assert stats.tobytes() == bytes(stats.nbytes)
