"""-m gpu: aln_hits_align_profiles — the hits of a profile search aligned on the device (hit_local_kernel<R, ProfileQuery>,
hit_global_kernel<R, ProfileQuery>, csrc/search_align.h).  Every comparison is exact: pair lists and lengths as integers,
scores and identities as uint32, lines byte for byte.

  1  profiles derived from residue strings, consensus = those strings: aln_hits_align's outputs (search_cases.CASES)
  2  position-specific rows at every fill and ring boundary of the staging, with a random consensus and with none: one resident
     batch over the same planes and query letters, and the int64 references
  3  the tie profiles against the oracle, with the census of what the device's lists went through
  4  wide templates (classes 6, 7, 8, a 300-row profile), a 2100-residue template and an empty one, fractional rows: the routes
  5  chunks, rows per chunk, row blocks, output groups, strides that are too small, a slot whose score was altered
  6  the argument checks, in their order"""
import ctypes as C

import numpy as np
import pytest

import aln_amd
import gpu_util
import nonlocal_cases as nc
import profile_align_cases as pac
import profile_cases as pc
import range_cases as rc
import search_cases as sc

pytestmark = pytest.mark.gpu

U32 = np.uint32
ALPHA = sc.ALPHA


def pool(profiles, alpha=ALPHA):
    return aln_amd.QueryProfiles([np.asarray(p, np.float32) for p in profiles], alpha)


def used_slots(n_hits, K):
    return [(r, k) for r in range(len(n_hits)) for k in range(K) if k < n_hits[r]]


def random_consensus(profiles, alpha, seed):
    return [rc.random_seq(alpha, seed + n, len(p)) for n, p in enumerate(profiles)]


def placeholder(profiles, alpha):
    return [alpha[0] * len(p) for p in profiles]


def batch_comparator(ctx, profiles, letters, ts, hits, n_hits, mode, gi, ge, alpha=ALPHA, q_begin=0):
    """what callers did before the entry existed, and what it is defined by: one resident Batch over the used slots (row-major),
    query letters `letters`, Batch.dp_simmatrix(profile_planes) + optimal + optimal_strings
    -> per used slot (score, list, identity, tline, qline)"""
    slots = used_slots(n_hits, hits.shape[1])
    if not slots:
        return []
    b = aln_amd.Batch(ctx, letters, ts, [q_begin + r for r, k in slots], [int(hits["t"][r, k]) for r, k in slots])
    try:
        b.dp_simmatrix([aln_amd.profile_planes(np.asarray(profiles[q_begin + r], np.float32), ts[hits["t"][r, k]], alpha)
                        for r, k in slots], mode, gi, ge)
        scores, lists, status = b.optimal()
        s2, ident, st2, tl, ql = b.optimal_strings()
    finally:
        b.close()
    assert (status == 0).all() and (st2 == 0).all()
    assert np.array_equal(scores.view(U32), s2.view(U32))
    return [(scores[p], lists[p], ident[p], tl[p], ql[p]) for p in range(len(slots))]


def check_equal(res, hits, n_hits, ref):
    rec, lists, tl, ql, lengths, rcode = res
    K = hits.shape[1]
    slots = used_slots(n_hits, K)
    assert len(slots) == len(ref)
    for p, (r, k) in enumerate(slots):
        score, pl, idn, t_line, q_line = ref[p]
        e = rec[r, k]
        assert e["status"] == 0, (r, k, e)
        assert e["n_pairs"] == len(pl), (r, k, e, len(pl))
        assert np.float32(e["score"]).view(U32) == np.float32(score).view(U32), (r, k, e, score)
        assert np.float32(e["identity"]).view(U32) == np.float32(idn).view(U32), (r, k, e, idn)
        assert np.array_equal(lists[r][k], pl), (r, k, lists[r][k].tolist(), pl.tolist())
        assert tl[r][k] == t_line and ql[r][k] == q_line, (r, k)
        assert lengths[r, k] == len(t_line), (r, k)
    for r in range(len(n_hits)):
        for k in range(n_hits[r], K):
            assert rec[r, k].tobytes() == bytes(16), (r, k)
            assert lengths[r, k] == 0 and tl[r][k] == "" and ql[r][k] == "" and len(lists[r][k]) == 0
    assert rcode == 0


def same_results(a, b):
    assert a[0].tobytes() == b[0].tobytes()
    assert (a[1] is None) == (b[1] is None) and (a[2] is None) == (b[2] is None)
    if a[1] is not None:
        assert all(np.array_equal(x, y) for ra, rb in zip(a[1], b[1]) for x, y in zip(ra, rb))
    if a[2] is not None:
        assert a[2] == b[2] and a[3] == b[3] and np.array_equal(a[4], b[4])
    assert a[5] == b[5]


def check_int64(res, profiles, ts, hits, n_hits, mode, gi, ge, alpha=ALPHA, q_begin=0):
    """lists and scores against the restated rules on the int64 reference plane"""
    rec, lists = res[0], res[1]
    for r, k in used_slots(n_hits, hits.shape[1]):
        score, pl = pac.restated(profiles[q_begin + r], ts[hits["t"][r, k]], alpha, mode, gi, ge)
        if pl is not None:                                           # (a non-local pair without an interior: the score only)
            assert np.array_equal(lists[r][k], pl), (mode, r, k, lists[r][k].tolist(), pl.tolist())
        assert np.float32(rec["score"][r, k]).view(U32) == np.float32(score).view(U32), (mode, r, k)


def interior(p, t):
    return len(p) >= 1 and len(t) >= 1


# ---- 1. derived profiles equal the residue entry ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.CASES))
def test_derived_profiles_equal_the_residue_entry(name):
    c = sc.CASES[name]
    qs, ts = sc.sequences(c)
    table = sc.TABLES[c.table]
    ctx = gpu_util.ctx()
    qp = aln_amd.profiles_from_sequences(qs, ALPHA, table)
    K = sc.KS[0]
    for mode in ((rc.LOCAL, rc.GLOBAL) if name in sc.BIG else rc.ALIGN_TYPES):
        hits, n_hits = aln_amd.search_topk(ctx, qs, ts, ALPHA, table, c.gi, c.ge, K, align_type=mode)
        assert (n_hits == K).all()
        want = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, ALPHA, table, c.gi, c.ge, align_type=mode)
        routes_want = aln_amd.hits_align_routes(ctx)
        got = aln_amd.hits_align_profiles(ctx, qp, ts, hits, n_hits, c.gi, c.ge, consensus=qs, align_type=mode)
        routes_got = aln_amd.hits_align_routes(ctx)
        same_results(got, want)
        assert sum(routes_got) == sum(routes_want) == int(n_hits.sum()), (name, mode, routes_got, routes_want)
        assert (got[0]["status"] == 0).all() and got[5] == 0


# ---- 2. position-specific rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_position_specific_rows(mode):
    profiles, ts = pc.length_set()
    assert tuple(len(p) for p in profiles[:len(pc.INTERIOR_ROWS)]) == pc.INTERIOR_ROWS
    _, gi, ge = pc.LENGTH_SYSTEM
    ctx = gpu_util.ctx()
    qp = pool(profiles)
    K = 4
    hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, ts, gi, ge, K, align_type=mode)
    assert (n_hits == K).all()
    n_interior = sum(interior(profiles[r], ts[hits["t"][r, k]]) for r, k in used_slots(n_hits, K))
    for letters, consensus in ((random_consensus(profiles, ALPHA, 900), True), (placeholder(profiles, ALPHA), False)):
        res = aln_amd.hits_align_profiles(ctx, qp, ts, hits, n_hits, gi, ge, consensus=letters if consensus else None, align_type=mode)
        assert aln_amd.hits_align_routes(ctx) == (n_interior, K * len(profiles) - n_interior)
        check_equal(res, hits, n_hits, batch_comparator(ctx, profiles, letters, ts, hits, n_hits, mode, gi, ge))
        check_int64(res, profiles, ts, hits, n_hits, mode, gi, ge)
        if mode == rc.LOCAL:                                                   # the search's own end cell and score
            for r, k in used_slots(n_hits, K):
                assert tuple(res[1][r][k][-2]) == (hits["q_end"][r, k], hits["t_end"][r, k])
            assert np.array_equal(res[0]["score"].view(U32), hits["score"].view(U32))


# ---- 3. ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_tie_profiles_equal_the_oracle(mode):
    ctx = gpu_util.ctx()
    local = mode == rc.LOCAL
    cen = pac.new_local_census() if local else nc.new_census()
    for alpha in pac.TIE_ALPHAS:
        profiles, qs, ts = pac.tie_profiles(alpha)
        qp = pool(profiles, alpha)
        for gi, ge in pac.TIE_GAPS:
            hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, ts, gi, ge, 6, align_type=mode)
            assert (n_hits == 6).all()
            res = aln_amd.hits_align_profiles(ctx, qp, ts, hits, n_hits, gi, ge, consensus=qs, align_type=mode)
            assert aln_amd.hits_align_routes(ctx) == (36, 0)
            assert (res[0]["status"] == 0).all() and res[5] == 0
            for r, k in used_slots(n_hits, 6):
                t = ts[hits["t"][r, k]]
                D, score, pl = pac.oracle_pair(profiles[r], t, alpha, mode, gi, ge)
                got = res[1][r][k]
                assert np.array_equal(got, pl), (mode, alpha, gi, ge, r, k, got.tolist(), pl.tolist())
                assert np.float32(res[0]["score"][r, k]).view(U32) == np.float32(score).view(U32), (mode, alpha, gi, ge, r, k)
                assert res[0]["identity"][r, k].view(U32) == gpu_util.identity_for(qs[r], t, got).view(U32)
                if local:
                    pac.local_census(D, got, gi, ge, cen)
                else:
                    nc.census(D, got, gi, ge, cen)
    print("census", mode, cen)
    assert pac.meets(cen, pac.LOCAL_FLOORS if local else pac.NONLOCAL_FLOORS), cen


# ---- 4. wide and long ------------------------------------------------------------------------------------------------------------------
def check_routes(ctx, profiles, ts, hits, n_hits, expect_zero=False):
    """fused + batched = the used slots; fused is at least the used slots with an interior and T <= 1792 (classes 1 .. 7)"""
    fused, batched = aln_amd.hits_align_routes(ctx)
    slots = used_slots(n_hits, hits.shape[1])
    assert fused + batched == len(slots)
    if expect_zero:
        assert fused == 0
        return fused
    must = sum(interior(profiles[r], ts[hits["t"][r, k]]) and len(ts[hits["t"][r, k]]) + 2 <= 1792 for r, k in slots)
    can = sum(interior(profiles[r], ts[hits["t"][r, k]]) and len(ts[hits["t"][r, k]]) + 2 <= 2048 for r, k in slots)
    assert must <= fused <= can, (fused, must, can)
    return fused


@pytest.mark.parametrize("mode", sc.WIDE_MODES)
@pytest.mark.parametrize("system", sc.WIDE_SYSTEMS, ids=lambda s: s[0])
def test_wide_templates(system, mode):
    tname, gi, ge = system
    profiles, ts = pc.wide_set(sc.TABLES[tname])
    assert [len(p) for p in profiles] == [40, 40, 300]
    ctx = gpu_util.ctx()
    qp = pool(profiles)
    K = len(ts)
    hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, ts, gi, ge, K, align_type=mode)
    letters = random_consensus(profiles, ALPHA, 910)
    res = aln_amd.hits_align_profiles(ctx, qp, ts, hits, n_hits, gi, ge, consensus=letters, align_type=mode)
    fused = check_routes(ctx, profiles, ts, hits, n_hits)
    assert fused >= 9                                              # classes 6, 7, 7 for three profiles
    check_equal(res, hits, n_hits, batch_comparator(ctx, profiles, letters, ts, hits, n_hits, mode, gi, ge))
    if mode != rc.LOCAL:
        with ctx.hints(align_fused_nonlocal=0):
            again = aln_amd.hits_align_profiles(ctx, qp, ts, hits, n_hits, gi, ge, consensus=letters, align_type=mode)
            check_routes(ctx, profiles, ts, hits, n_hits, expect_zero=True)
        same_results(again, res)


@pytest.mark.parametrize("mode", sc.WIDE_MODES)
def test_long_and_empty_templates_and_fractional_rows(mode):
    profiles, ts = pc.mixed_set()
    assert len(ts[1]) == 2100 and ts[3] == ""
    ctx = gpu_util.ctx()
    K = len(ts)
    letters = random_consensus(profiles, ALPHA, 920)
    qp = pool(profiles)
    hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, ts, 11, 1, K, align_type=mode)
    assert (n_hits == K).all()
    res = aln_amd.hits_align_profiles(ctx, qp, ts, hits, n_hits, 11, 1, consensus=letters, align_type=mode)
    assert check_routes(ctx, profiles, ts, hits, n_hits) == 2 * 3       # all but the long and the empty template
    check_equal(res, hits, n_hits, batch_comparator(ctx, profiles, letters, ts, hits, n_hits, mode, 11, 1))
    check_int64(res, profiles, ts, hits, n_hits, mode, 11, 1)
    if mode != rc.LOCAL:
        with ctx.hints(align_fused_nonlocal=0):
            again = aln_amd.hits_align_profiles(ctx, qp, ts, hits, n_hits, 11, 1, consensus=letters, align_type=mode)
            check_routes(ctx, profiles, ts, hits, n_hits, expect_zero=True)
        same_results(again, res)
    # rows x 0.5: every slot goes through batches
    half = [np.asarray(p, np.float32) * np.float32(0.5) for p in profiles]
    assert any((h != np.round(h)).any() for h in half)
    hp = aln_amd.QueryProfiles(half, ALPHA)
    hh, hn = aln_amd.search_topk_profiles(ctx, hp, ts, 11, 1, K, align_type=mode)
    hres = aln_amd.hits_align_profiles(ctx, hp, ts, hh, hn, 11, 1, consensus=letters, align_type=mode)
    check_routes(ctx, half, ts, hh, hn, expect_zero=True)
    check_equal(hres, hh, hn, batch_comparator(ctx, half, letters, ts, hh, hn, mode, 11, 1))


# ---- 5. chunks, blocks, outputs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (rc.LOCAL, rc.SEMI_LOCAL))
def test_chunks_blocks_and_outputs(mode):
    profiles, ts = pc.length_set()
    _, gi, ge = pc.LENGTH_SYSTEM
    ctx = gpu_util.ctx()
    qp = pool(profiles)
    K = 4
    letters = random_consensus(profiles, ALPHA, 930)
    hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, ts, gi, ge, K, align_type=mode)
    call = lambda h=hits, n=n_hits, **kw: aln_amd.hits_align_profiles(ctx, qp, ts, h, n, gi, ge, consensus=letters, align_type=mode, **kw)
    whole = call()
    routes = aln_amd.hits_align_routes(ctx)
    assert routes[0] > 0 and (whole[0]["status"] == 0).all()
    assert ctx.get_hint("align_rows_per_chunk") == 0
    for chunk in (1, 3):
        for per_chunk in (0, 1):
            with ctx.hints(align_chunk_hits=chunk, align_rows_per_chunk=per_chunk):
                again = call()
            assert aln_amd.hits_align_routes(ctx) == routes
            same_results(again, whole)
    assert ctx.get_hint("align_rows_per_chunk") == 0 and ctx.get_hint("align_chunk_hits") == 0
    for a, b in ((3, 11), (17, 18), (0, 1)):
        for per_chunk in (0, 1):
            with ctx.hints(align_rows_per_chunk=per_chunk):
                part = call(hits[a:b], n_hits[a:b], q_begin=a)
            assert part[0].tobytes() == whole[0][a:b].tobytes(), (mode, a, b)
            assert all(np.array_equal(x, y) for ra, rb in zip(part[1], whole[1][a:b]) for x, y in zip(ra, rb))
            assert part[2] == whole[2][a:b] and part[3] == whole[3][a:b] and np.array_equal(part[4], whole[4][a:b])
    empty = call(hits[5:5], n_hits[5:5], q_begin=5)
    assert empty[0].shape == (0, K) and empty[5] == 0
    # a row without hits, unused slots that still hold a hit, duplicates
    h2, n2 = hits.copy(), n_hits.copy()
    n2[4] = 0
    n2[6] = 2
    h2[9, 1] = h2[9, 0]
    res2 = call(h2, n2)
    check_equal(res2, h2, n2, batch_comparator(ctx, profiles, letters, ts, h2, n2, mode, gi, ge))
    assert np.array_equal(res2[1][9][1], res2[1][9][0]) and res2[2][9][1] == res2[2][9][0]
    # pairs only, lines only, neither
    lines_only = call(want_pairs=False)
    assert lines_only[1] is None and lines_only[0].tobytes() == whole[0].tobytes()
    assert lines_only[2] == whole[2] and lines_only[3] == whole[3] and np.array_equal(lines_only[4], whole[4])
    pairs_only = call(want_lines=False)
    assert pairs_only[2] is None and pairs_only[4] is None and pairs_only[0].tobytes() == whole[0].tobytes()
    assert all(np.array_equal(x, y) for ra, rb in zip(pairs_only[1], whole[1]) for x, y in zip(ra, rb))
    neither = call(want_pairs=False, want_lines=False)
    assert neither[0].tobytes() == whole[0].tobytes()
    # a pair_stride / line_stride that is too small: per-slot ALN_E_OVERFLOW, the first pair_stride entries are written
    small = call(pair_stride=6)
    long_ = whole[0]["n_pairs"] > 6
    assert long_.any() and not long_.all() and small[5] == aln_amd.E_OVERFLOW
    assert np.array_equal(small[0]["status"], np.where(long_, aln_amd.E_OVERFLOW, 0))
    assert np.array_equal(small[0]["n_pairs"], whole[0]["n_pairs"]) and np.array_equal(small[0]["score"].view(U32), whole[0]["score"].view(U32))
    for r, k in used_slots(n_hits, K):
        assert np.array_equal(small[1][r][k], whole[1][r][k][:6]), (r, k)
    cut = int(np.median(whole[4]))                                 # a line of `cut` characters needs cut + 1
    short = call(line_stride=cut)
    fits = whole[4] < cut
    assert fits.any() and not fits.all() and short[5] == aln_amd.E_OVERFLOW
    assert np.array_equal(short[0]["status"], np.where(fits, 0, aln_amd.E_OVERFLOW))
    assert np.array_equal(short[4], np.where(fits, whole[4], 0))
    for r, k in used_slots(n_hits, K):
        assert short[2][r][k] == (whole[2][r][k] if fits[r, k] else "") and np.array_equal(short[1][r][k], whole[1][r][k])
    # a slot whose score was altered
    bad = hits.copy()
    br = 10
    bk = [k for k in range(K) if interior(profiles[br], ts[hits["t"][br, k]])][-1]      # a slot the fused kernel takes
    bad["score"][br, bk] += 1.0
    got = call(bad)
    if mode == rc.LOCAL:
        assert got[5] == aln_amd.E_ARG
        want_status = np.zeros_like(whole[0]["status"])
        want_status[br, bk] = aln_amd.E_ARG
        assert np.array_equal(got[0]["status"], want_status)
        assert got[0]["n_pairs"][br, bk] == 0 and len(got[1][br][bk]) == 0 and got[2][br][bk] == "" and got[4][br, bk] == 0
        for r, k in used_slots(n_hits, K):
            if (r, k) != (br, bk):
                assert got[0][r, k].tobytes() == whole[0][r, k].tobytes()
                assert np.array_equal(got[1][r][k], whole[1][r][k]) and got[2][r][k] == whole[2][r][k] and got[3][r][k] == whole[3][r][k]
    else:
        same_results(got, whole)                                   # the non-local types do not read the score


# ---- 6. arguments ----------------------------------------------------------------------------------------------------------------------
class Raw:
    """aln_hits_align_profiles through ctypes with sentinel-filled outputs"""

    def __init__(self, profiles, letters, ts, K, pair_stride=16, line_stride=40, mode=aln_amd.LOCAL):
        self.qp = pool(profiles)
        self.cp = aln_amd.SeqPool(letters)
        self.tp = aln_amd.SeqPool(ts)
        self.g = aln_amd.AlnGap()
        self.g.model, self.g.align_type, self.g.gap_init, self.g.gap_extn = aln_amd.GAP_AFFINE_CONST, mode, 11.0, 1.0
        self.rows, self.K, self.ps, self.ls = len(profiles), K, pair_stride, line_stride
        self.fill()

    def fill(self):
        n = self.rows * self.K
        self.out = np.full(n * 16, 0x5A, dtype=np.uint8)
        self.pairs = np.full(n * self.ps * 2, 0x5A5A5A5A, dtype=np.int32)
        self.tl = C.create_string_buffer(b"\x5a" * (n * self.ls), n * self.ls)
        self.ql = C.create_string_buffer(b"\x5a" * (n * self.ls), n * self.ls)
        self.lengths = np.full(n, 0x5A5A5A5A, dtype=np.int32)

    def untouched(self):
        n = self.rows * self.K
        return ((self.out == 0x5A).all() and (self.pairs == 0x5A5A5A5A).all() and self.tl.raw == b"\x5a" * (n * self.ls) and
                self.ql.raw == b"\x5a" * (n * self.ls) and (self.lengths == 0x5A5A5A5A).all())

    def call(self, hit_array, n_array, **kw):
        ip = C.POINTER(C.c_int32)
        a = dict(prof=self.qp.c, cons=self.cp.c, templ=self.tp.c, g=self.g, hits=hit_array.ctypes.data_as(C.POINTER(aln_amd.AlnHit)),
                 n_hits=n_array.ctypes.data_as(ip), out=self.out.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)),
                 pairs=self.pairs.ctypes.data_as(ip), ps=self.ps, tl=self.tl, ql=self.ql, ls=self.ls, lengths=self.lengths.ctypes.data_as(ip),
                 K=self.K, q_begin=0, q_end=self.rows)
        a.update(kw)
        ref = lambda x: None if x is None else C.byref(x)
        return aln_amd.lib().aln_hits_align_profiles(gpu_util.ctx().h, ref(a["prof"]), ref(a["cons"]), ref(a["templ"]), ref(a["g"]),
                                                     a["q_begin"], a["q_end"], a["K"], a["hits"], a["n_hits"], a["out"], a["pairs"],
                                                     a["ps"], a["tl"], a["ql"], a["ls"], a["lengths"])

    def records(self):
        return self.out.view(aln_amd.HIT_ALIGNMENT_DTYPE).reshape(self.rows, self.K)


def test_argument_checks_leave_the_outputs_untouched():
    ctx = gpu_util.ctx()
    E = aln_amd.E_ARG
    profiles = pc.derived(["PAWHEAE", "HEAGAWGHEE"], sc.TABLES["blosum62"])
    letters = ["PAWHEAE", "HEAGAWGHEE"]
    ts = ["HEAGAWGHEE", "PAWHEAE", "AWHE"]
    K = 2
    qp = pool(profiles)
    hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, ts, 11, 1, K)
    assert (n_hits == K).all()
    raw = Raw(profiles, letters, ts, K)
    assert raw.call(hits, n_hits) == 0 and not raw.untouched()
    good = raw.records().copy()
    assert (good["status"] == 0).all() and (good["n_pairs"] > 2).any()
    raw.fill()
    assert raw.call(hits, n_hits, cons=None) == 0                      # no consensus: the placeholder
    assert np.array_equal(raw.records()["n_pairs"], good["n_pairs"]) and np.array_equal(raw.records()["score"].view(U32), good["score"].view(U32))
    raw.fill()

    def refused(want, what, **kw):
        assert raw.call(kw.pop("h_arr", hits), kw.pop("n_arr", n_hits), **kw) == want, what
        assert raw.untouched(), what

    def qprof(**kw):
        d = dict(n_seqs=qp.c.n_seqs, offsets=qp.c.offsets, rows=qp.c.rows, n=qp.c.n, alphabet=qp.c.alphabet)
        d.update(kw)
        return aln_amd.AlnQProfiles(d["n_seqs"], d["offsets"], d["rows"], d["n"], d["alphabet"])

    def gap(model=aln_amd.GAP_AFFINE_CONST, align_type=aln_amd.LOCAL):
        g = aln_amd.AlnGap()
        g.model, g.align_type, g.gap_init, g.gap_extn = model, align_type, 11.0, 1.0
        return g

    def cons(**kw):
        d = dict(n_seqs=raw.cp.c.n_seqs, offsets=raw.cp.c.offsets, residues=raw.cp.c.residues)
        d.update(kw)
        return aln_amd.AlnSeqs(d["n_seqs"], d["offsets"], d["residues"])

    bad_t = aln_amd.SeqPool(["HEAGAWGHEE", "PAW?EAE", "AWHE"]).c
    wrong_n = cons(n_seqs=1)
    # 1. NULL arguments
    for kw in (dict(prof=None), dict(templ=None), dict(g=None), dict(hits=None), dict(n_hits=None), dict(out=None)):
        refused(E, kw, **kw)
    # 2. K — before everything that follows
    for k in (0, 1025, -1):
        refused(E, ("K", k), K=k)
    refused(E, "K before the descriptor", K=0, prof=qprof(n=31), templ=bad_t)
    # 3. pairs with pair_stride < 2
    for ps in (1, 0):
        refused(E, ("pair_stride", ps), ps=ps)
    # 4. the line group given in part, line_stride < 1
    for kw in (dict(tl=None), dict(ql=None), dict(ls=0), dict(tl=None, ql=None, ls=0)):
        refused(E, kw, **kw)
    # 5. the checks of aln_score_profiles_vs_all, in its order: the row range, the gap, the descriptor ...
    refused(E, "q_begin < 0", q_begin=-1)
    refused(E, "q_end > n", q_end=3)
    refused(E, "q_begin > q_end", q_begin=1, q_end=0)
    refused(E, "gap model", g=gap(model=aln_amd.GAP_AFFINE_TPOS_MIN))
    refused(E, "align type", g=gap(align_type=5))
    for kw in (dict(n=0), dict(n=31), dict(alphabet=None), dict(rows=None), dict(offsets=None)):
        refused(E, kw, prof=qprof(**kw))
    one_row = np.array([0, 9, 10], np.int64)
    refused(E, "a profile of one row", prof=qprof(offsets=one_row.ctypes.data_as(C.POINTER(C.c_int64))))
    # 6. ... then the consensus pool, before the templates' letters
    refused(E, "consensus n_seqs", cons=wrong_n)
    off = raw.cp.offsets.copy()
    off[1] += 1
    refused(E, "one differing offset", cons=cons(offsets=off.ctypes.data_as(C.POINTER(C.c_int64))))
    last = raw.cp.offsets.copy()
    last[2] -= 1
    refused(E, "the last offset differs", cons=cons(offsets=last.ctypes.data_as(C.POINTER(C.c_int64))))
    refused(E, "consensus without offsets", cons=cons(offsets=None))
    refused(E, "consensus without residues", cons=cons(residues=None))
    refused(E, "the descriptor comes before the consensus", prof=qprof(n=31), cons=wrong_n, templ=bad_t)
    refused(E, "the consensus comes before the residues", cons=wrong_n, templ=bad_t)
    refused(aln_amd.E_RESIDUE, "a template letter outside the alphabet", templ=bad_t)
    refused(aln_amd.E_RESIDUE, "the residues come before n_hits", templ=bad_t, n_arr=np.array([3, 0], np.int32))
    # the consensus letters are not checked against the alphabet
    odd = Raw(profiles, ["PAW?EAE", "heagawghee"], ts, K)
    assert odd.call(hits, n_hits) == 0
    assert np.array_equal(odd.records()["n_pairs"], good["n_pairs"]) and np.array_equal(odd.pairs, pairs_of(raw, hits, n_hits))
    raw.fill()
    # 7. n_hits, 8. t, 9. the local end cell
    Q = [len(p) + 2 for p in profiles]
    for field, r, k, value in (("n", 0, 0, -1), ("n", 1, 0, 3), ("t", 0, 1, -1), ("t", 1, 0, len(ts)),
                               ("q_end", 0, 0, 0), ("q_end", 1, 1, Q[1] - 1), ("t_end", 0, 1, 0),
                               ("t_end", 1, 0, len(ts[hits["t"][1, 0]]) + 1)):
        h, n = hits.copy(), n_hits.copy()
        if field == "n":
            n[r] = value
        else:
            h[field][r, k] = value
        refused(E, (field, r, k, value), h_arr=h, n_arr=n)
    h, n = hits.copy(), n_hits.copy()
    n[0], h["t"][1, 0] = 3, -1
    refused(E, "n_hits and t both wrong", h_arr=h, n_arr=n)
    # q_begin == q_end: ALN_OK, nothing written
    refused(0, "empty block", q_begin=1, q_end=1)
    # a non-local align type ignores the end cell
    glob = Raw(profiles, letters, ts, K, mode=aln_amd.GLOBAL)
    h = hits.copy()
    h["q_end"], h["t_end"], h["score"] = -5, 1 << 20, -1e30
    assert glob.call(h, n_hits) == 0 and (glob.records()["status"] == 0).all()


def pairs_of(raw, hits, n_hits):
    raw.fill()
    assert raw.call(hits, n_hits) == 0
    return raw.pairs.copy()
