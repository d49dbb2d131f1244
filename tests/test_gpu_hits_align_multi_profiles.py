"""-m gpu: aln_hits_align_multi_profiles — several non-intersecting local alignments per hit of a profile search, all rounds of a
hit in one wave (align_local_multi_kernel<R, ProfileQuery>: rows staged into an LDS ring, masked sweep, 1 B/cell strip).  Every
comparison is exact: lists and lengths as integers, scores and identities as uint32, lines byte for byte.

  1  N = 1 is aln_hits_align_profiles on the hits of search_cases.CASES through derived profiles
  2  derived profiles are aln_hits_align_multi, N = 4 and 16
  3  position-specific rows at every chunk and ring edge against the int64 reference, the oracle and the detour, with a
     consensus and with the placeholder
  4  2040 columns; the routes of classes 1 .. 7 and of the fallback set
  5  chunks, rows per chunk, row blocks
  6  short strides
  7  duplicated slots and padding
  8  the argument checks, in their order, with the outputs untouched"""
import ctypes as C
import math

import numpy as np
import pytest

import aln_amd
import gpu_util
import multi_align_cases as mac
import profile_multi_cases as pm
import range_cases as rc
import search_cases as sc

pytestmark = pytest.mark.gpu

U32 = np.uint32
ALPHA = pm.ALPHA


def bits(x):
    return int(np.float32(x).view(U32))


def pool(profiles, alpha=ALPHA):
    return aln_amd.QueryProfiles([np.asarray(p, np.float32).reshape(-1, len(alpha)) for p in profiles], alpha)


def diagonal_hits(n):
    hits = np.zeros((n, 1), dtype=aln_amd.HIT_DTYPE)
    hits["t"][:, 0] = np.arange(n)
    hits["q_end"], hits["t_end"], hits["score"] = -7, 1 << 20, -1.0          # never read
    return hits, np.ones(n, np.int32)


def all_pairs_hits(nq, nt):
    hits = np.zeros((nq, nt), dtype=aln_amd.HIT_DTYPE)
    hits["t"] = np.arange(nt)[None, :]
    return hits, np.full(nq, nt, np.int32)


def same_results(a, b):
    assert a[0].tobytes() == b[0].tobytes()
    assert all(np.array_equal(x, y) for ra, rb in zip(a[1], b[1]) for ka, kb in zip(ra, rb) for x, y in zip(ka, kb))
    assert a[2] == b[2] and a[3] == b[3] and np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]) and a[6] == b[6]


def systems(cases):
    groups = {}
    for c in cases:
        groups.setdefault((c.alpha, c.gi, c.ge, c.min_score), []).append(c)
    return groups.values()


# ---- 1. N = 1 is aln_hits_align_profiles ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.CASES))
def test_one_alignment_is_hits_align_profiles(name):
    case = sc.CASES[name]
    ctx = gpu_util.ctx()
    qs, ts = sc.sequences(case)
    table = sc.TABLES[case.table]
    qp = aln_amd.profiles_from_sequences(qs, sc.ALPHA, table)
    hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, ts, case.gi, case.ge, 4)
    one = aln_amd.hits_align_profiles(ctx, qp, ts, hits, n_hits, case.gi, case.ge, consensus=qs)
    routes_one = aln_amd.hits_align_routes(ctx)
    rec, lists, tl, ql, lengths, n_found, rcode = aln_amd.hits_align_multi_profiles(ctx, qp, ts, hits, n_hits, case.gi, case.ge, 1,
                                                                                    consensus=qs)
    assert sum(aln_amd.hits_align_routes(ctx)) == sum(routes_one) == int(n_hits.sum())
    assert rcode == one[5] == 0
    assert rec[:, :, 0].tobytes() == one[0].tobytes()
    assert np.array_equal(lengths[:, :, 0], one[4])
    used = np.arange(hits.shape[1])[None, :] < n_hits[:, None]
    assert np.array_equal(n_found, used.astype(np.int32))
    for r in range(hits.shape[0]):
        for k in range(hits.shape[1]):
            assert np.array_equal(lists[r][k][0], one[1][r][k]) and tl[r][k][0] == one[2][r][k] and ql[r][k][0] == one[3][r][k], (r, k)


# ---- 2. derived profiles are aln_hits_align_multi ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 16])
def test_derived_profiles_equal_the_residue_entry(N):
    ctx = gpu_util.ctx()
    reported = 0
    for g in systems(pm.derived_small() + pm.derived_shapes()):
        c0 = g[0]
        table = c0.residue.table
        qs, ts = [c.consensus for c in g], [c.t for c in g]
        hits, n_hits = diagonal_hits(len(g))
        want = aln_amd.hits_align_multi(ctx, qs, ts, hits, n_hits, c0.alpha, table, c0.gi, c0.ge, N, min_score=c0.min_score)
        routes_want = aln_amd.hits_align_routes(ctx)
        got = aln_amd.hits_align_multi_profiles(ctx, pool([c.profile for c in g], c0.alpha), ts, hits, n_hits, c0.gi, c0.ge, N,
                                                min_score=c0.min_score, consensus=qs)
        assert aln_amd.hits_align_routes(ctx) == routes_want == (len(g), 0)
        same_results(got, want)
        assert got[6] == 0
        reported += int(got[5].sum())
        if N == 4:                                                   # and the int64 reference, once
            for i, c in enumerate(g):
                ref, _ = pm.reference(c)
                assert got[5][i, 0] == len(ref), c.name
                for a, r in enumerate(ref):
                    assert bits(got[0][i, 0, a]["score"]) == bits(r.score) and np.array_equal(got[1][i][0][a], r.pairs), (c.name, a)
    assert reported >= 60


# ---- 3. position-specific rows ------------------------------------------------------------------------------------------------------
SPECIFIC = pm.specific_cases() + [pm.stale_ring_case()]
_RUN = {}


def run_specific(N, with_consensus):
    """all position-specific cases in one call, pair (i, i); computed once per (N, consensus)"""
    key = (N, with_consensus)
    if key not in _RUN:
        ctx = gpu_util.ctx()
        hits, n_hits = diagonal_hits(len(SPECIFIC))
        res = aln_amd.hits_align_multi_profiles(ctx, pool([c.profile for c in SPECIFIC]), [c.t for c in SPECIFIC], hits, n_hits, 11, 1, N,
                                                consensus=[c.consensus for c in SPECIFIC] if with_consensus else None)
        _RUN[key] = (res, aln_amd.hits_align_routes(ctx))
    return _RUN[key]


def letters_of(case, with_consensus):
    return case.consensus if with_consensus else ALPHA[0] * len(case.profile)


def check_reference(case, rec, lists, n_found, N, letters):
    ref, _ = pm.reference(case, N)
    assert n_found == len(ref), (case.name, n_found, len(ref))
    for a, r in enumerate(ref):
        assert rec[a]["status"] == 0
        assert bits(rec[a]["score"]) == bits(r.score), (case.name, a)
        assert np.array_equal(lists[a], r.pairs), (case.name, a, lists[a].tolist(), r.pairs.tolist())
        assert bits(rec[a]["identity"]) == bits(gpu_util.identity_for(letters, case.t, r.pairs)), (case.name, a)
    for a in range(n_found, N):
        assert rec[a].tobytes() == bytes(16) and len(lists[a]) == 0, (case.name, a)


@pytest.mark.parametrize("with_consensus", [True, False], ids=["consensus", "placeholder"])
@pytest.mark.parametrize("N", [4, 16])
def test_position_specific_rows(N, with_consensus):
    ctx = gpu_util.ctx()
    (rec, lists, tl, ql, lengths, n_found, rcode), routes = run_specific(N, with_consensus)
    assert rcode == 0 and routes == (len(SPECIFIC), 0)              # classes 1, 2, 3 and 7: all fused
    for i, c in enumerate(SPECIFIC):
        check_reference(c, rec[i, 0], lists[i][0], int(n_found[i, 0]), N, letters_of(c, with_consensus))
        assert n_found[i, 0] >= 3
    if N != 4:
        return
    small = [i for i, c in enumerate(SPECIFIC) if (len(c.profile) + 2) * (len(c.t) + 2) <= 300 * 700]
    assert len(small) >= 8
    det = aln_amd.hits_align_multi_profiles_detour(ctx, pool([c.profile for c in SPECIFIC]), [c.t for c in SPECIFIC],
                                                   [(i, i) for i in small], 11, 1, N,
                                                   consensus=[c.consensus for c in SPECIFIC] if with_consensus else None)
    for p, i in enumerate(small):
        c = SPECIFIC[i]
        want = pm.oracle_rounds(c)
        assert n_found[i, 0] == len(want) == len(det[p]), c.name
        for a, (score, pl) in enumerate(want):
            assert bits(rec[i, 0, a]["score"]) == bits(score) and np.array_equal(lists[i][0][a], pl), (c.name, a)
        for a, (score, pl, ident, t_line, q_line, status) in enumerate(det[p]):
            assert status == 0 and bits(rec[i, 0, a]["score"]) == bits(score) and np.array_equal(lists[i][0][a], pl), (c.name, a)
            assert bits(rec[i, 0, a]["identity"]) == bits(ident), (c.name, a)
            assert tl[i][0][a] == t_line and ql[i][0][a] == q_line and lengths[i, 0, a] == len(t_line), (c.name, a)
        for a in range(int(n_found[i, 0]), N):
            assert tl[i][0][a] == "" and ql[i][0][a] == "" and lengths[i, 0, a] == 0


# ---- 4. 2040 columns and the routes --------------------------------------------------------------------------------------------------
def test_the_2040_column_template_matches_the_reference():
    ctx = gpu_util.ctx()
    c = pm.long_case()
    hits, n_hits = diagonal_hits(1)
    for N in (4,):
        rec, lists, tl, ql, lengths, n_found, rcode = aln_amd.hits_align_multi_profiles(ctx, pool([c.profile]), [c.t], hits, n_hits, 11, 1,
                                                                                        N, consensus=[c.consensus])
        assert rcode == 0 and sum(aln_amd.hits_align_routes(ctx)) == 1
        check_reference(c, rec[0, 0], lists[0][0], int(n_found[0, 0]), N, c.consensus)
        assert n_found[0, 0] >= 3


def check_detour(name, rec, lists, tl, ql, n_found, det, N):
    assert n_found == len(det), (name, n_found, len(det))
    for a, (score, pl, ident, t_line, q_line, status) in enumerate(det):
        assert rec[a]["status"] == status and bits(rec[a]["score"]) == bits(score), (name, a)
        if status == 0:
            assert np.array_equal(lists[a], pl) and bits(rec[a]["identity"]) == bits(ident), (name, a)
            assert tl[a] == t_line and ql[a] == q_line, (name, a)
    for a in range(n_found, N):
        assert rec[a].tobytes() == bytes(16)


def test_fallback_routes():
    """a 2100-residue template, a pair without an interior (Q = 2); then a row holding 0.5 and gap 10.5, which send every slot
    through batches"""
    ctx = gpu_util.ctx()
    base = pm.specific_cases()[5]                                    # Q = 33
    L = len(base.profile)
    body = rc.random_seq(pm.AA, 940, 2100)
    long_t = base.t[:L] + body[L:1000] + base.t[:L] + body[1000 + L:]
    assert len(long_t) == 2100
    profiles = [base.profile, np.zeros((0, len(ALPHA)), np.int64)]
    letters = [base.consensus, ""]
    ts = [long_t, base.t, ""]
    hits, n_hits = all_pairs_hits(2, 3)
    pairs_qt = [(r, k) for r in range(2) for k in range(3)]
    half = [np.asarray(p, np.float32).copy() for p in profiles]
    half[0][3, 2] = 0.5
    for prof, gi, fused, batched in ((profiles, 11, 1, 5), (half, 11, 0, 6), (profiles, 10.5, 0, 6)):
        qp = pool(prof)
        res = aln_amd.hits_align_multi_profiles(ctx, qp, ts, hits, n_hits, gi, 1, 4, consensus=letters)
        assert res[6] in (0, aln_amd.E_STARTPAIR)
        assert aln_amd.hits_align_routes(ctx) == (fused, batched), (gi, aln_amd.hits_align_routes(ctx))
        det = aln_amd.hits_align_multi_profiles_detour(ctx, qp, ts, pairs_qt, gi, 1, 4, consensus=letters)
        for p, (r, k) in enumerate(pairs_qt):
            check_detour((gi, r, k), res[0][r, k], res[1][r][k], res[2][r][k], res[3][r][k], int(res[5][r, k]), det[p], 4)
        assert (res[5][0, :2] >= 3).all() and (res[5][:, 2] == 1).all() and (res[5][1] == 1).all()


# ---- 5. chunks, rows per chunk, row blocks ----------------------------------------------------------------------------------------------
def block_set():
    cs = pm.specific_cases()
    picks = [cs[4], cs[5], cs[7], cs[0]]                             # Q = 17, 33, 67, 3
    profiles = [c.profile for c in picks] + [np.zeros((0, len(ALPHA)), np.int64)]
    letters = [c.consensus for c in picks] + [""]
    ts = [cs[4].t, cs[5].t, cs[0].t, "W"]
    return profiles, letters, ts


def test_chunks_rows_per_chunk_and_row_blocks_give_the_same_bytes():
    ctx = gpu_util.ctx()
    profiles, letters, ts = block_set()
    qp = pool(profiles)
    hits, n_hits = all_pairs_hits(len(profiles), len(ts))
    ls, ps = 67 + 402 + 6, 70
    call = lambda h=hits, n=n_hits, **kw: aln_amd.hits_align_multi_profiles(ctx, qp, ts, h, n, 11, 1, 4, consensus=letters, pair_stride=ps,
                                                                            line_stride=ls, **kw)
    whole = call()
    routes = aln_amd.hits_align_routes(ctx)
    assert whole[6] == 0 and routes == (4 * 4, 4) and (whole[5] >= 1).all() and (whole[5] >= 3).sum() >= 3
    for chunk, per_chunk in ((1, 0), (3, 0), (0, 1), (1, 1), (3, 1)):
        with ctx.hints(align_chunk_hits=chunk, align_rows_per_chunk=per_chunk):
            again = call()
        assert aln_amd.hits_align_routes(ctx) == routes
        same_results(again, whole)
    for r0, r1 in ((0, 2), (2, 5), (3, 4)):
        for per_chunk in (0, 1):
            with ctx.hints(align_rows_per_chunk=per_chunk):
                part = call(hits[r0:r1], n_hits[r0:r1], q_begin=r0)
            assert part[0].tobytes() == whole[0][r0:r1].tobytes() and part[2] == whole[2][r0:r1] and part[3] == whole[3][r0:r1]
            assert np.array_equal(part[5], whole[5][r0:r1]) and np.array_equal(part[4], whole[4][r0:r1])
            assert all(np.array_equal(x, y) for ra, rb in zip(part[1], whole[1][r0:r1]) for ka, kb in zip(ra, rb) for x, y in zip(ka, kb))
    empty = call(hits[2:2], n_hits[2:2], q_begin=2)
    assert empty[0].shape == (0, len(ts), 4) and empty[6] == 0


# ---- 6, 7. strides, slots ----------------------------------------------------------------------------------------------------------------
def test_slots_duplicates_padding_and_short_strides():
    ctx = gpu_util.ctx()
    profiles, letters, ts = block_set()
    qp = pool(profiles)
    nq, nt = len(profiles), len(ts)
    hits, n_hits = all_pairs_hits(nq, nt)
    call = lambda h=hits, n=n_hits, **kw: aln_amd.hits_align_multi_profiles(ctx, qp, ts, h, n, 11, 1, 4, consensus=letters, **kw)
    whole = call()
    h2, n2 = hits.copy(), n_hits.copy()
    h2["t"][0, 1] = 0                                            # a duplicate of slot (0, 0)
    h2["t"][1, 3] = 1                                            # ... of (1, 1)
    n2[2] = 0                                                    # a row without hits
    n2[3] = 2                                                    # unused slots that still name a template
    res = call(h2, n2)
    assert res[6] == 0
    assert res[0][0, 1].tobytes() == whole[0][0, 0].tobytes() and res[2][0][1] == whole[2][0][0]
    assert res[0][1, 3].tobytes() == whole[0][1, 1].tobytes() and all(np.array_equal(x, y) for x, y in zip(res[1][1][3], whole[1][1][1]))
    for r, k in [(2, k) for k in range(nt)] + [(3, k) for k in range(2, nt)]:
        assert res[5][r, k] == 0 and res[0][r, k].tobytes() == bytes(64) and res[2][r][k] == [""] * 4 and (res[4][r, k] == 0).all()
    assert res[0][3, :2].tobytes() == whole[0][3, :2].tobytes() and res[0][4].tobytes() == whole[0][4].tobytes()
    # a pair_stride shorter than round 0's list: that alignment overflows (its head is still written), later rounds are unchanged
    ps = 12
    short = call(pair_stride=ps)
    assert short[6] == aln_amd.E_OVERFLOW and (whole[0]["n_pairs"] > ps).any() and ((whole[0]["n_pairs"] <= ps) & (whole[0]["n_pairs"] > 0)).any()
    assert np.array_equal(short[0]["status"], np.where(whole[0]["n_pairs"] > ps, aln_amd.E_OVERFLOW, 0))
    for f in ("n_pairs", "score", "identity"):
        assert short[0][f].tobytes() == whole[0][f].tobytes()
    assert np.array_equal(short[5], whole[5])
    for r in range(nq):
        for k in range(nt):
            for a in range(4):
                assert np.array_equal(short[1][r][k][a], whole[1][r][k][a][:ps]), (r, k, a)
    ok = short[0]["status"] == 0
    assert np.array_equal(short[4][ok], whole[4][ok])
    # a line_stride too short for some lines: those alignments overflow with empty lines, the lists are untouched
    lens = whole[4]
    cut = int(np.median(lens[lens > 0]))
    tight = call(line_stride=cut)
    assert tight[6] == aln_amd.E_OVERFLOW
    over = lens >= cut
    assert over.any() and (~over & (lens > 0)).any()
    assert np.array_equal(tight[0]["status"], np.where(over, aln_amd.E_OVERFLOW, 0))
    assert np.array_equal(tight[4], np.where(over, 0, lens))
    for r in range(nq):
        for k in range(nt):
            for a in range(4):
                assert tight[2][r][k][a] == ("" if over[r, k, a] else whole[2][r][k][a])
                assert np.array_equal(tight[1][r][k][a], whole[1][r][k][a])
    bare = call(want_pairs=False, want_lines=False)
    assert bare[1] is None and bare[2] is None and bare[4] is None and bare[0].tobytes() == whole[0].tobytes()


# ---- 8. arguments --------------------------------------------------------------------------------------------------------------------------
class Raw:
    """aln_hits_align_multi_profiles through ctypes with sentinel-filled outputs"""

    def __init__(self, profiles, letters, ts, K, N, pair_stride=16, line_stride=40, mode=aln_amd.LOCAL):
        self.qp, self.cp, self.tp = pool(profiles), aln_amd.SeqPool(letters), aln_amd.SeqPool(ts)
        self.g = aln_amd.AlnGap()
        self.g.model, self.g.align_type, self.g.gap_init, self.g.gap_extn = aln_amd.GAP_AFFINE_CONST, mode, 11.0, 1.0
        self.rows, self.K, self.N, self.ps, self.ls = len(profiles), K, N, pair_stride, line_stride
        self.fill()

    def fill(self):
        n = self.rows * self.K * self.N
        self.out = np.full(n * 16, 0x5A, dtype=np.uint8)
        self.pairs = np.full(n * self.ps * 2, 0x5A5A5A5A, dtype=np.int32)
        self.tl = C.create_string_buffer(b"\x5a" * (n * self.ls), n * self.ls)
        self.ql = C.create_string_buffer(b"\x5a" * (n * self.ls), n * self.ls)
        self.lengths = np.full(n, 0x5A5A5A5A, dtype=np.int32)
        self.n_found = np.full(self.rows * self.K, 0x5A5A5A5A, dtype=np.int32)

    def untouched(self):
        n = self.rows * self.K * self.N
        return ((self.out == 0x5A).all() and (self.pairs == 0x5A5A5A5A).all() and self.tl.raw == b"\x5a" * (n * self.ls) and
                self.ql.raw == b"\x5a" * (n * self.ls) and (self.lengths == 0x5A5A5A5A).all() and (self.n_found == 0x5A5A5A5A).all())

    def call(self, hit_array, n_array, **kw):
        ip = C.POINTER(C.c_int32)
        a = dict(prof=self.qp.c, cons=self.cp.c, templ=self.tp.c, g=self.g, hits=hit_array.ctypes.data_as(C.POINTER(aln_amd.AlnHit)),
                 n_hits=n_array.ctypes.data_as(ip), N=self.N, ms=-math.inf, n_found=self.n_found.ctypes.data_as(ip),
                 out=self.out.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)), pairs=self.pairs.ctypes.data_as(ip), ps=self.ps,
                 tl=self.tl, ql=self.ql, ls=self.ls, lengths=self.lengths.ctypes.data_as(ip), K=self.K, q_begin=0, q_end=self.rows)
        a.update(kw)
        ref = lambda x: None if x is None else C.byref(x)
        return aln_amd.lib().aln_hits_align_multi_profiles(gpu_util.ctx().h, ref(a["prof"]), ref(a["cons"]), ref(a["templ"]), ref(a["g"]),
                                                           a["q_begin"], a["q_end"], a["K"], a["hits"], a["n_hits"], a["N"], a["ms"],
                                                           a["n_found"], a["out"], a["pairs"], a["ps"], a["tl"], a["ql"], a["ls"],
                                                           a["lengths"])


def test_argument_checks_in_order_leave_the_outputs_untouched():
    ctx = gpu_util.ctx()
    E = aln_amd.E_ARG
    letters = ["PAWHEAE", "HEAGAWGHEE"]
    profiles = [pm.table_rows(ALPHA, pm.BLOSUM, q) for q in letters]
    ts = ["HEAGAWGHEE", "PAWHEAE", "AWHE"]
    hits, n_hits = all_pairs_hits(2, 2)
    raw = Raw(profiles, letters, ts, 2, 3)
    assert raw.call(hits, n_hits) == 0 and not raw.untouched()
    assert aln_amd.hits_align_routes(ctx) == (4, 0)
    first = raw.out.copy()
    raw.fill()
    assert raw.call(hits, n_hits, cons=None) == 0                    # no consensus: the placeholder; scores and lists are the same
    rec0, rec1 = first.view(aln_amd.HIT_ALIGNMENT_DTYPE), raw.out.view(aln_amd.HIT_ALIGNMENT_DTYPE)
    assert np.array_equal(rec0["n_pairs"], rec1["n_pairs"]) and np.array_equal(rec0["score"].view(U32), rec1["score"].view(U32))
    raw.fill()

    def refused(want, what, **kw):
        assert raw.call(kw.pop("h_arr", hits), kw.pop("n_arr", n_hits), **kw) == want, what
        assert raw.untouched(), what

    qp = raw.qp

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
    # 1. n_found, N, and aln_hits_align_profiles' first group
    for kw in (dict(n_found=None), dict(N=0), dict(N=17), dict(N=-1), dict(prof=None), dict(templ=None), dict(g=None), dict(hits=None),
               dict(n_hits=None), dict(out=None), dict(K=0), dict(K=1025), dict(ps=1), dict(tl=None), dict(ql=None), dict(ls=0),
               dict(tl=None, ql=None, ls=0)):
        refused(E, kw, **kw)
        assert aln_amd.hits_align_routes(ctx) == (0, 0)
    refused(E, "N before the descriptor", N=0, prof=qprof(n=31), templ=bad_t)
    # 2. aln_score_profiles_vs_all's, in its order: the row range, the gap, the descriptor, the consensus, the letters
    refused(E, "q_begin < 0", q_begin=-1)
    refused(E, "q_end > n", q_end=3)
    refused(E, "q_begin > q_end", q_begin=1, q_end=0)
    refused(E, "gap model", g=gap(model=aln_amd.GAP_AFFINE_TPOS_MIN))
    refused(E, "align type", g=gap(align_type=5))
    for kw in (dict(n=0), dict(n=31), dict(alphabet=None), dict(rows=None), dict(offsets=None)):
        refused(E, kw, prof=qprof(**kw))
    one_row = np.array([0, 9, 10], np.int64)
    refused(E, "a profile of one row", prof=qprof(offsets=one_row.ctypes.data_as(C.POINTER(C.c_int64))))
    refused(E, "consensus n_seqs", cons=wrong_n)
    off = raw.cp.offsets.copy()
    off[1] += 1
    refused(E, "one differing offset", cons=cons(offsets=off.ctypes.data_as(C.POINTER(C.c_int64))))
    refused(E, "consensus without residues", cons=cons(residues=None))
    refused(E, "the descriptor comes before the consensus", prof=qprof(n=31), cons=wrong_n, templ=bad_t)
    refused(E, "the consensus comes before the residues", cons=wrong_n, templ=bad_t)
    refused(aln_amd.E_RESIDUE, "a template letter outside the alphabet", templ=bad_t)
    # 3. an align type other than local: after the score checks, before the slots are looked at
    for mode in (aln_amd.GLOBAL, aln_amd.SEMI_LOCAL, aln_amd.GLOBAL_LOCAL, aln_amd.LOCAL_GLOBAL):
        refused(E, ("mode", mode), g=gap(align_type=mode))
        refused(aln_amd.E_RESIDUE, ("mode after the residues", mode), g=gap(align_type=mode), templ=bad_t)
        refused(E, ("mode before n_hits", mode), g=gap(align_type=mode), n_arr=np.array([3, 0], np.int32))
    refused(aln_amd.E_RESIDUE, "the residues come before n_hits", templ=bad_t, n_arr=np.array([3, 0], np.int32))
    # 4. n_hits, 5. t; the end cell and the score are never read
    for field, r, k, value in (("n", 0, 0, -1), ("n", 1, 0, 3), ("t", 0, 1, -1), ("t", 1, 0, len(ts))):
        h, n = hits.copy(), n_hits.copy()
        if field == "n":
            n[r] = value
        else:
            h[field][r, k] = value
        refused(E, (field, r, k, value), h_arr=h, n_arr=n)
    refused(0, "empty block", q_begin=1, q_end=1)
    h = hits.copy()
    h["q_end"], h["t_end"], h["score"] = -3, 1 << 30, np.nan
    assert raw.call(h, n_hits) == 0 and raw.out.tobytes() == first.tobytes()
