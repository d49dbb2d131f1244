"""-m gpu: aln_score_profiles_vs_all and aln_search_topk_profiles — all-vs-all scoring and search for queries given as
position-specific rows (aln_qprofiles) — through ctypes, scores compared as uint32 patterns.

  1  profiles derived from residue strings give the plain entries' scores and hits, byte for byte (search_cases.CASES)
  2  position-specific rows against the int64 reference (profile_cases), all five align types, every fill and ring boundary
     of the kernels' staging (rows reach LDS 8 at a time, into a ring of 32)
  3  wide templates: length classes 6, 7, 8, a 300-row profile
  4  mixed routes: a 2100-residue template among short ones; fractional rows against the oracle
  5  slabs and row blocks
  6  the hits against resident batches over the same planes
  7  the argument checks"""
import ctypes as C

import numpy as np
import pytest

import aln_amd
import gpu_util
import orc
import profile_cases as pc
import range_cases as rc
import search_cases as sc

pytestmark = pytest.mark.gpu

U32 = np.uint32
ALPHA = sc.ALPHA


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(U32)


def pool(profiles):
    return aln_amd.QueryProfiles([np.asarray(p, np.float32) for p in profiles], ALPHA)


def check_hits(hits, n_hits, scores, ends, K, min_score=-np.inf, what=None):
    """hits of the rows `scores` / `ends` describe: the header's selection (score >= min_score, score descending, ties by
    template index, at most K), the score's bits, the end cell, the padding {-1, 0, -1, -1}"""
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


def check_set(key, profiles, ts, mode, gi, ge, Ks, min_scores=(-np.inf,)):
    """scores and searches of a whole set against the int64 reference -> (scores, ends, the last hits, n_hits)"""
    ctx = gpu_util.ctx()
    scores, ends = pc.dense_reference(key, profiles, ts, mode, gi, ge)
    qp = pool(profiles)
    got = aln_amd.score_profiles_vs_all(ctx, qp, ts, gi, ge, align_type=mode)
    print(key, mode, gi, ge, "scores differ in", int((u32(got) != u32(scores)).sum()), "of", got.size)
    assert np.array_equal(u32(got), u32(scores)), (key, mode, np.argwhere(u32(got) != u32(scores))[:8].tolist())
    for K in Ks:
        for ms in min_scores:
            hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, ts, gi, ge, K, min_score=ms, align_type=mode)
            check_hits(hits, n_hits, scores, ends, K, ms, what=(key, mode, K, ms))
    return scores, ends, hits, n_hits


# ---- 1. derived profiles equal the plain entries --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.CASES))
def test_derived_profiles_equal_the_plain_entries(name):
    """score32_out takes the fallback on both sides; packed_in compares the packed table kernel with the 32-bit profile kernel;
    constant+3 and all_zero tie everywhere"""
    c = sc.CASES[name]
    qs, ts = sc.sequences(c)
    table = sc.TABLES[c.table]
    ctx = gpu_util.ctx()
    qp = aln_amd.profiles_from_sequences(qs, ALPHA, table)
    for mode in ((rc.LOCAL, rc.GLOBAL) if name in sc.BIG else rc.ALIGN_TYPES):
        want = aln_amd.score_all_vs_all(ctx, qs, ts, ALPHA, table, c.gi, c.ge, align_type=mode)
        got = aln_amd.score_profiles_vs_all(ctx, qp, ts, c.gi, c.ge, align_type=mode)
        assert got.tobytes() == want.tobytes(), (name, mode, np.argwhere(u32(got) != u32(want))[:8].tolist())
        for K in sc.KS:
            hw, nw = aln_amd.search_topk(ctx, qs, ts, ALPHA, table, c.gi, c.ge, K, align_type=mode)
            hg, ng = aln_amd.search_topk_profiles(ctx, qp, ts, c.gi, c.ge, K, align_type=mode)
            assert hg.tobytes() == hw.tobytes() and np.array_equal(ng, nw), (name, mode, K)


# ---- 2. position-specific rows against the int64 reference ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_position_specific_rows(mode):
    profiles, ts = pc.length_set()
    _, gi, ge = pc.LENGTH_SYSTEM
    scores, ends, hits, n_hits = check_set("length", profiles, ts, mode, gi, ge, sc.KS, (-np.inf, 0.0))
    if mode == rc.LOCAL:
        assert (scores[-1] == 0).all() and scores[-2].max() == 11          # the all-zero profile; the single positive row
        assert (ends[-1, :, 0] == 33).all()                                # ... whose every pair reports find_max's seed


# ---- 3. wide templates --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sc.WIDE_MODES)
@pytest.mark.parametrize("system", sc.WIDE_SYSTEMS, ids=lambda s: s[0])
def test_wide_templates(system, mode):
    tname, gi, ge = system
    profiles, ts = pc.wide_set(sc.TABLES[tname])
    assert [len(p) for p in profiles] == [40, 40, 300]
    check_set("wide-" + tname, profiles, ts, mode, gi, ge, (3, len(ts)))


# ---- 4. mixed routes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (rc.LOCAL, rc.GLOBAL))
def test_long_template_among_short_ones(mode):
    """the 2100-residue template's column comes from the plane fallback and lands in its slot, end cells included"""
    profiles, ts = pc.mixed_set()
    scores, ends, hits, n_hits = check_set("mixed", profiles, ts, mode, 11, 1, (2, len(ts)))
    if mode == rc.LOCAL:
        assert scores[0, 1] > 50                                              # the long column is no filler: it holds a real alignment


@pytest.mark.parametrize("mode", (rc.LOCAL, rc.GLOBAL))
def test_fractional_rows_against_the_oracle(mode):
    """rows scaled by 0.5: every pair takes the fallback; the oracle builds the same float plane"""
    profiles, ts = pc.mixed_set()
    ts = [ts[0], ts[2], ts[4]]
    half = [np.asarray(p, np.float32) * np.float32(0.5) for p in profiles]
    assert any((h != np.round(h)).any() for h in half)
    ctx = gpu_util.ctx()
    qp = aln_amd.QueryProfiles(half, ALPHA)
    got = aln_amd.score_profiles_vs_all(ctx, qp, ts, 11, 1, align_type=mode)
    hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, ts, 11, 1, len(ts), align_type=mode)
    want = np.zeros_like(got)
    ends = np.zeros(got.shape + (2,), np.int64)
    for i, h in enumerate(half):
        for j, t in enumerate(ts):
            S = aln_amd.profile_planes(h, t, ALPHA)
            err, D, PQ, PT = orc.dp_build(S, orc.Gap(mode, 11, 1))
            err2, score, pl = orc.optimal(D, PQ, PT, mode == rc.LOCAL)
            assert err == 0 and err2 == 0
            want[i, j] = score
            ends[i, j] = pl[-2] if mode == rc.LOCAL else (S.shape[0] - 1, S.shape[1] - 1)
    assert np.array_equal(u32(got), u32(want)), (mode, got.tolist(), want.tolist())
    check_hits(hits, n_hits, want, ends, len(ts), what=("half", mode))


# ---- 5. blocks and slabs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (rc.LOCAL, rc.SEMI_LOCAL))
def test_slabs_and_row_blocks(mode):
    profiles, ts = pc.length_set()
    _, gi, ge = pc.LENGTH_SYSTEM
    ctx = gpu_util.ctx()
    qp = pool(profiles)
    whole, n_whole = aln_amd.search_topk_profiles(ctx, qp, ts, gi, ge, 4, align_type=mode)
    dense = aln_amd.score_profiles_vs_all(ctx, qp, ts, gi, ge, align_type=mode)
    for slab in (1, 3):
        with ctx.hints(search_slab_rows=slab):
            hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, ts, gi, ge, 4, align_type=mode)
        assert hits.tobytes() == whole.tobytes() and np.array_equal(n_hits, n_whole), (mode, slab)
    for a, b in ((3, 11), (17, 18), (0, 1)):
        hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, ts, gi, ge, 4, q_begin=a, q_end=b, align_type=mode)
        assert hits.tobytes() == whole[a:b].tobytes() and np.array_equal(n_hits, n_whole[a:b]), (mode, a, b)
        part = aln_amd.score_profiles_vs_all(ctx, qp, ts, gi, ge, q_begin=a, q_end=b, align_type=mode)
        assert part.tobytes() == dense[a:b].tobytes(), (mode, a, b)
    hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, ts, gi, ge, 4, q_begin=5, q_end=5, align_type=mode)
    assert hits.shape == (0, 4) and n_hits.shape == (0,)
    hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, [], gi, ge, 4, align_type=mode)
    assert (n_hits == 0).all() and (hits["t"] == -1).all() and (u32(hits["score"]) == 0).all() and (hits["q_end"] == -1).all()


# ---- 6. against resident batches --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (rc.LOCAL, rc.SEMI_LOCAL))
def test_hits_against_resident_batches(mode):
    """Batch.dp_simmatrix(profile_planes) + optimal() over the hits: the score's bits, and, local, the pair before the closing one"""
    profiles, ts = pc.length_set()
    _, gi, ge = pc.LENGTH_SYSTEM
    ctx = gpu_util.ctx()
    hits, n_hits = aln_amd.search_topk_profiles(ctx, pool(profiles), ts, gi, ge, 4, align_type=mode)
    rows, slots = np.nonzero(np.arange(4)[None, :] < n_hits[:, None])
    assert len(rows) == 4 * len(profiles)
    placeholders = [ALPHA[0] * len(p) for p in profiles]
    b = aln_amd.Batch(ctx, placeholders, ts, rows, hits["t"][rows, slots])
    try:
        b.dp_simmatrix([aln_amd.profile_planes(profiles[r], ts[hits["t"][r, k]], ALPHA) for r, k in zip(rows, slots)], mode, gi, ge)
        scores, lists, status = b.optimal()
    finally:
        b.close()
    assert not status.any()
    assert np.array_equal(u32(scores), u32(hits["score"][rows, slots]))
    if mode == rc.LOCAL:
        for p, (r, k) in enumerate(zip(rows, slots)):
            assert tuple(lists[p][-2]) == (hits["q_end"][r, k], hits["t_end"][r, k]), (r, k)


# ---- 7. statuses --------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_leave_the_outputs_untouched():
    L = aln_amd.lib()
    ctx = gpu_util.ctx()
    qp = pool([np.ones((3, pc.N)), np.ones((5, pc.N))])
    tp = aln_amd.SeqPool(["WWW", "AC"])
    K = 2
    FILL = 0x5A

    def gap(model=aln_amd.GAP_AFFINE_CONST, align_type=aln_amd.LOCAL):
        g = aln_amd.AlnGap()
        g.model, g.align_type, g.gap_init, g.gap_extn = model, align_type, 11.0, 1.0
        return g

    def qprof(**kw):
        d = dict(n_seqs=qp.c.n_seqs, offsets=qp.c.offsets, rows=qp.c.rows, n=qp.c.n, alphabet=qp.c.alphabet)
        d.update(kw)
        return aln_amd.AlnQProfiles(d["n_seqs"], d["offsets"], d["rows"], d["n"], d["alphabet"])

    def both(want, prof="ok", templ="ok", g=None, qb=0, qe=2, K=K, outs=True, what=None):
        prof = qp.c if isinstance(prof, str) else prof
        templ = tp.c if isinstance(templ, str) else templ
        g = gap() if g is None else g
        scores = np.full((2, 2), np.float32(-7.5))
        hits = np.frombuffer(bytearray([FILL]) * (2 * 4 * 16), dtype=aln_amd.HIT_DTYPE).reshape(2, 4).copy()
        n_hits = np.full(2, 0x5A5A5A5A, np.int32)
        ref = lambda x: None if x is None else C.byref(x)
        rc1 = L.aln_score_profiles_vs_all(ctx.h, ref(prof), ref(templ), ref(g), qb, qe, scores.ctypes.data_as(C.POINTER(C.c_float)) if outs else None)
        rc2 = L.aln_search_topk_profiles(ctx.h, ref(prof), ref(templ), ref(g), qb, qe, K, -np.inf,
                                         hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)) if outs else None, n_hits.ctypes.data_as(C.POINTER(C.c_int32)))
        assert rc2 == want and (rc1 == want or what == "K"), (what, rc1, rc2, want)
        assert (scores == np.float32(-7.5)).all() or what == "K", what
        assert hits.tobytes() == bytes([FILL]) * (2 * 4 * 16) and (n_hits == 0x5A5A5A5A).all(), what

    E = aln_amd
    # 1. NULL arguments, K
    both(E.E_ARG, prof=None, what="no profiles")
    both(E.E_ARG, templ=None, what="no templates")
    both(E.E_ARG, outs=False, what="no outputs")
    both(E.E_ARG, K=0, what="K")
    both(E.E_ARG, K=1025, what="K")
    assert L.aln_score_profiles_vs_all(ctx.h, C.byref(qp.c), C.byref(tp.c), None, 0, 2, np.zeros(4, np.float32).ctypes.data_as(C.POINTER(C.c_float))) == E.E_ARG
    assert L.aln_score_profiles_vs_all(None, C.byref(qp.c), C.byref(tp.c), C.byref(gap()), 0, 2, np.zeros(4, np.float32).ctypes.data_as(C.POINTER(C.c_float))) == E.E_ARG
    # 2. the row range
    both(E.E_ARG, qb=-1, what="q_begin < 0")
    both(E.E_ARG, qe=3, what="q_end > n")
    both(E.E_ARG, qb=2, qe=1, what="q_begin > q_end")
    # 3. gap model and align type
    both(E.E_ARG, g=gap(model=aln_amd.GAP_AFFINE_TPOS_MIN), what="gap model")
    both(E.E_ARG, g=gap(align_type=5), what="align type 5")
    both(E.E_ARG, g=gap(align_type=-1), what="align type -1")
    # 4. the descriptor
    both(E.E_ARG, prof=qprof(n=0), what="n 0")
    both(E.E_ARG, prof=qprof(n=31), what="n 31")
    both(E.E_ARG, prof=qprof(alphabet=None), what="alphabet")
    both(E.E_ARG, prof=qprof(rows=None), what="rows")
    both(E.E_ARG, prof=qprof(offsets=None), what="offsets")
    short = np.array([0, 5, 6], np.int64)
    both(E.E_ARG, prof=qprof(offsets=short.ctypes.data_as(C.POINTER(C.c_int64))), what="a profile of one row")
    # 5. a template letter outside the alphabet — also when a later check would fail too
    bad = aln_amd.SeqPool(["WWW", "A?"])
    both(E.E_RESIDUE, templ=bad.c, what="residue")
    both(E.E_ARG, prof=qprof(n=31), templ=bad.c, what="the descriptor comes before the residues")
    # 6. too long
    long_rows = np.zeros((65535 + 7, pc.N), np.float32)
    long_off = np.array([0, 65535, 65535 + 7], np.int64)
    too_long = aln_amd.AlnQProfiles(2, long_off.ctypes.data_as(C.POINTER(C.c_int64)), long_rows.ctypes.data_as(C.POINTER(C.c_float)), pc.N, qp.c.alphabet)
    both(E.E_TOO_LONG, prof=too_long, what="65535 rows")
    both(E.E_RESIDUE, prof=too_long, templ=bad.c, what="the residues come before the lengths")
    both(E.E_TOO_LONG, templ=aln_amd.SeqPool(["W" * 65533, "AC"]).c, what="65535 residues")
    # q_begin == q_end: ALN_OK, nothing written
    both(0, qb=1, qe=1, what="empty block")
