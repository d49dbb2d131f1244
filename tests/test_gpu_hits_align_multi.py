"""-m gpu: aln_hits_align_multi — several non-intersecting local alignments per search hit, all rounds of a hit in one wave
(masked register-resident sweep, 1 B/cell strip, 1/8 B/cell plane of forbidden cells).  Every comparison is exact: lists and
lengths as integers, scores and identities as uint32, lines byte for byte.  The comparators: the int64 reference and the oracle of
multi_align_cases, and the detour the call replaces — aln_amd.hits_align_multi_detour, resident batches built by dp_simmatrix
from planes masked on the host."""
import ctypes as C
import math

import numpy as np
import pytest

import aln_amd
import gpu_util
import multi_align_cases as mc
import range_cases as rc
import search_cases as sc

pytestmark = pytest.mark.gpu

U32 = np.uint32


def bits(x):
    return int(np.float32(x).view(U32))


def diagonal_hits(n):
    hits = np.zeros((n, 1), dtype=aln_amd.HIT_DTYPE)
    hits["t"][:, 0] = np.arange(n)
    hits["q_end"], hits["t_end"], hits["score"] = -7, 1 << 20, -1.0          # never read
    return hits, np.ones(n, np.int32)


_RUN = {}


def run_cases(cases, N):
    """hits_align_multi and the detour over the cases, pair (i, i) of one pool per scoring system; computed once per (case, N)
    -> {name: (records[N], lists[N], tlines[N], qlines[N], lengths[N], n_found, detour rounds)}"""
    ctx = gpu_util.ctx()
    groups = {}
    for c in cases:
        if (c.name, N) not in _RUN:
            groups.setdefault((c.alpha, c.table.tobytes(), c.gi, c.ge, c.min_score), []).append(c)
    for g in groups.values():
        c0 = g[0]
        qs, ts = [c.q for c in g], [c.t for c in g]
        hits, n_hits = diagonal_hits(len(g))
        rec, lists, tl, ql, lengths, n_found, rcode = aln_amd.hits_align_multi(ctx, qs, ts, hits, n_hits, c0.alpha, c0.table, c0.gi,
                                                                               c0.ge, N, min_score=c0.min_score)
        assert rcode == 0
        det = aln_amd.hits_align_multi_detour(ctx, qs, ts, [(i, i) for i in range(len(g))], c0.alpha, c0.table, c0.gi, c0.ge, N,
                                              min_score=c0.min_score)
        for i, c in enumerate(g):
            _RUN[(c.name, N)] = (rec[i, 0], lists[i][0], tl[i][0], ql[i][0], lengths[i, 0], int(n_found[i, 0]), det[i])
    return {c.name: _RUN[(c.name, N)] for c in cases}


def check_against_detour(name, got, N):
    rec, lists, tl, ql, lengths, n_found, det = got
    assert n_found == len(det), (name, n_found, len(det))
    for a, (score, pl, ident, t_line, q_line, status) in enumerate(det):
        e = rec[a]
        assert status == 0 and e["status"] == 0, (name, a, e)
        assert bits(e["score"]) == bits(score), (name, a, e, score)
        assert e["n_pairs"] == len(pl) and np.array_equal(lists[a], pl), (name, a, lists[a].tolist(), pl.tolist())
        assert bits(e["identity"]) == bits(ident), (name, a, e, ident)
        assert tl[a] == t_line and ql[a] == q_line and lengths[a] == len(t_line), (name, a)
    for a in range(n_found, N):
        assert rec[a].tobytes() == bytes(16) and len(lists[a]) == 0 and tl[a] == "" and ql[a] == "" and lengths[a] == 0, (name, a)


def check_against_reference(case, got, N):
    rec, lists, tl, ql, lengths, n_found, det = got
    reported, _ = mc.reference(case, N)
    assert n_found == len(reported), (case.name, n_found, len(reported))
    for a, r in enumerate(reported):
        assert bits(rec[a]["score"]) == bits(r.score), (case.name, a)
        assert np.array_equal(lists[a], r.pairs), (case.name, a, lists[a].tolist(), r.pairs.tolist())
        assert bits(rec[a]["identity"]) == bits(gpu_util.identity_for(case.q, case.t, r.pairs)), (case.name, a)


# ---- 1. N = 1 is aln_hits_align -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.CASES))
def test_one_alignment_is_hits_align(name):
    case = sc.CASES[name]
    ctx = gpu_util.ctx()
    qs, ts = sc.sequences(case)
    table = sc.TABLES[case.table]
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, sc.ALPHA, table, case.gi, case.ge, 4)
    one = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, sc.ALPHA, table, case.gi, case.ge)
    routes_one = aln_amd.hits_align_routes(ctx)
    rec, lists, tl, ql, lengths, n_found, rcode = aln_amd.hits_align_multi(ctx, qs, ts, hits, n_hits, sc.ALPHA, table, case.gi, case.ge, 1)
    assert aln_amd.hits_align_routes(ctx) == routes_one
    assert rcode == one[5] == 0
    assert rec[:, :, 0].tobytes() == one[0].tobytes()
    assert np.array_equal(lengths[:, :, 0], one[4])
    used = np.arange(hits.shape[1])[None, :] < n_hits[:, None]
    assert np.array_equal(n_found, used.astype(np.int32))
    for r in range(hits.shape[0]):
        for k in range(hits.shape[1]):
            assert np.array_equal(lists[r][k][0], one[1][r][k]) and tl[r][k][0] == one[2][r][k] and ql[r][k][0] == one[3][r][k], (r, k)


# ---- 2. the builder's cases ------------------------------------------------------------------------------------------------------
SMALL = mc.small_cases() + [mc.cut_case()]


@pytest.mark.parametrize("N", [4, 16])
def test_builder_cases(N):
    got = run_cases(SMALL, N)
    for c in SMALL:
        check_against_reference(c, got[c.name], N)
        check_against_detour(c.name, got[c.name], N)
        if N == 4:
            rec, lists = got[c.name][0], got[c.name][1]
            want = mc.oracle_rounds(c)
            assert got[c.name][5] == len(want), c.name
            for a, (score, pl) in enumerate(want):
                assert bits(rec[a]["score"]) == bits(score) and np.array_equal(lists[a], pl), (c.name, a)


# ---- 3. shapes -------------------------------------------------------------------------------------------------------------------
def test_shapes():
    """Q = 3, 4, 17, 130 x length classes 1, 2, 3 and 7: all of them in one call, every slot through the fused kernel"""
    cases = mc.shape_cases()
    got = run_cases(cases, 4)
    for c in cases:
        check_against_reference(c, got[c.name], 4)
        check_against_detour(c.name, got[c.name], 4)
        if (len(c.q) + 2) * (len(c.t) + 2) <= 300 * 700:
            want = mc.oracle_rounds(c)
            assert got[c.name][5] == len(want)
            for a, (score, pl) in enumerate(want):
                assert bits(got[c.name][0][a]["score"]) == bits(score) and np.array_equal(got[c.name][1][a], pl), (c.name, a)
    ctx = gpu_util.ctx()
    hits, n_hits = diagonal_hits(len(cases))
    aln_amd.hits_align_multi(ctx, [c.q for c in cases], [c.t for c in cases], hits, n_hits, mc.ALPHA, mc.BLOSUM, 11, 1, 2,
                             want_pairs=False, want_lines=False)
    assert aln_amd.hits_align_routes(ctx) == (len(cases), 0)


TIE_TABLES = ("blosum62", "blosum62x9", "identity5", "constant+3", "all_zero", "all_negative")


@pytest.mark.parametrize("gi,ge", [(11, 1), (0, 0), (40, 0), (1, 5), (0, 1)])
def test_ties_under_table_and_gap_families(gi, ge):
    """three copies of a domain (rounds of equal score) in the query, in the template, and a tandem repeat against itself"""
    base = [c for c in mc.small_cases() if c.name in ("three_in_query", "three_in_template", "tandem_self")]
    fam = rc.table_families(mc.ALPHA, mc.BLOSUM)
    cases = [c._replace(name="%s_%s_%d_%d" % (c.name, tn, gi, ge), table=fam[tn], gi=gi, ge=ge, teeth=()) for tn in TIE_TABLES for c in base]
    got = run_cases(cases, 4)
    ties = 0
    for c in cases:
        check_against_reference(c, got[c.name], 4)
        check_against_detour(c.name, got[c.name], 4)
        rec, n = got[c.name][0], got[c.name][5]
        ties += sum(int(rec[a]["score"] == rec[a + 1]["score"]) for a in range(n - 1))
    assert ties >= 6, ties


# ---- 4. chunks, row blocks, strides, slots -------------------------------------------------------------------------------------------
def domain_set():
    by = {c.name: c for c in mc.small_cases()}
    qs = [by["three_in_query"].q, by["shuffled_domains"].q, by["wide_columns"].q, "W", ""]
    ts = [by["three_in_query"].t, by["shuffled_domains"].t, by["wide_columns"].t, by["three_in_template"].t, "W"]
    return qs, ts


def all_pairs_hits(nq, nt):
    hits = np.zeros((nq, nt), dtype=aln_amd.HIT_DTYPE)
    hits["t"] = np.arange(nt)[None, :]
    return hits, np.full(nq, nt, np.int32)


def same_results(a, b):
    assert a[0].tobytes() == b[0].tobytes()
    assert all(np.array_equal(x, y) for ra, rb in zip(a[1], b[1]) for ka, kb in zip(ra, rb) for x, y in zip(ka, kb))
    assert a[2] == b[2] and a[3] == b[3] and np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]) and a[6] == b[6]


def test_chunks_and_row_blocks_give_the_same_bytes():
    ctx = gpu_util.ctx()
    qs, ts = domain_set()
    hits, n_hits = all_pairs_hits(len(qs), len(ts))
    ls, ps = max(map(len, qs)) + max(map(len, ts)) + 6, min(max(map(len, qs)), max(map(len, ts))) + 5
    whole = aln_amd.hits_align_multi(ctx, qs, ts, hits, n_hits, mc.ALPHA, mc.BLOSUM, 11, 1, 4, pair_stride=ps, line_stride=ls)
    assert whole[6] == 0 and (whole[5] >= 1).all() and (whole[5] >= 3).sum() >= 3
    assert aln_amd.hits_align_routes(ctx) == (4 * 5, 5)          # the empty query has no interior
    for chunk in (1, 3):
        with ctx.hints(align_chunk_hits=chunk):
            again = aln_amd.hits_align_multi(ctx, qs, ts, hits, n_hits, mc.ALPHA, mc.BLOSUM, 11, 1, 4, pair_stride=ps, line_stride=ls)
        same_results(again, whole)
    for r0, r1 in ((0, 2), (2, 5)):
        part = aln_amd.hits_align_multi(ctx, qs, ts, hits[r0:r1], n_hits[r0:r1], mc.ALPHA, mc.BLOSUM, 11, 1, 4, q_begin=r0, pair_stride=ps,
                                        line_stride=ls)
        assert part[0].tobytes() == whole[0][r0:r1].tobytes() and part[2] == whole[2][r0:r1] and part[3] == whole[3][r0:r1]
        assert np.array_equal(part[5], whole[5][r0:r1])
        assert all(np.array_equal(x, y) for ra, rb in zip(part[1], whole[1][r0:r1]) for ka, kb in zip(ra, rb) for x, y in zip(ka, kb))
    # every slot against the detour
    det = aln_amd.hits_align_multi_detour(ctx, qs, ts, [(r, k) for r in range(len(qs)) for k in range(len(ts))], mc.ALPHA, mc.BLOSUM, 11, 1, 4)
    for r in range(len(qs)):
        for k in range(len(ts)):
            got = (whole[0][r, k], whole[1][r][k], whole[2][r][k], whole[3][r][k], whole[4][r, k], int(whole[5][r, k]), det[r * len(ts) + k])
            check_against_detour((r, k), got, 4)


def test_slots_duplicates_padding_and_short_strides():
    ctx = gpu_util.ctx()
    qs, ts = domain_set()
    hits, n_hits = all_pairs_hits(len(qs), len(ts))
    whole = aln_amd.hits_align_multi(ctx, qs, ts, hits, n_hits, mc.ALPHA, mc.BLOSUM, 11, 1, 4)
    h2, n2 = hits.copy(), n_hits.copy()
    h2["t"][0, 1] = 0                                            # a duplicate of slot (0, 0)
    h2["t"][1, 3] = 1                                            # ... of (1, 1)
    n2[2] = 0                                                    # a row without hits
    n2[3] = 2                                                    # unused slots that still name a template
    res = aln_amd.hits_align_multi(ctx, qs, ts, h2, n2, mc.ALPHA, mc.BLOSUM, 11, 1, 4)
    assert res[6] == 0
    assert res[0][0, 1].tobytes() == whole[0][0, 0].tobytes() and res[2][0][1] == whole[2][0][0]
    assert res[0][1, 3].tobytes() == whole[0][1, 1].tobytes() and all(np.array_equal(x, y) for x, y in zip(res[1][1][3], whole[1][1][1]))
    for r, k in [(2, k) for k in range(5)] + [(3, k) for k in range(2, 5)]:
        assert res[5][r, k] == 0 and res[0][r, k].tobytes() == bytes(64) and res[2][r][k] == [""] * 4 and (res[4][r, k] == 0).all()
    assert res[0][3, :2].tobytes() == whole[0][3, :2].tobytes() and res[0][4].tobytes() == whole[0][4].tobytes()
    # a pair_stride shorter than round 0's list: that alignment overflows (its head is still written), later rounds are right
    n0 = whole[0]["n_pairs"][:, :, 0]
    ps = 20
    short = aln_amd.hits_align_multi(ctx, qs, ts, hits, n_hits, mc.ALPHA, mc.BLOSUM, 11, 1, 4, pair_stride=ps)
    assert short[6] == aln_amd.E_OVERFLOW and (n0 > ps).any() and (whole[0]["n_pairs"][:, :, 1:] <= ps).any()
    assert np.array_equal(short[0]["status"], np.where(whole[0]["n_pairs"] > ps, aln_amd.E_OVERFLOW, 0))
    for f in ("n_pairs", "score", "identity"):
        assert short[0][f].tobytes() == whole[0][f].tobytes()
    assert np.array_equal(short[5], whole[5])
    for r in range(len(qs)):
        for k in range(len(ts)):
            for a in range(4):
                assert np.array_equal(short[1][r][k][a], whole[1][r][k][a][:ps]), (r, k, a)
    ok = short[0]["status"] == 0
    assert np.array_equal(short[4][ok], whole[4][ok])
    # a line_stride too short for some lines: those alignments overflow with empty lines, the lists are untouched
    lens = whole[4]
    cut = int(np.median(lens[lens > 0]))
    tight = aln_amd.hits_align_multi(ctx, qs, ts, hits, n_hits, mc.ALPHA, mc.BLOSUM, 11, 1, 4, line_stride=cut)
    assert tight[6] == aln_amd.E_OVERFLOW
    over = lens >= cut
    assert over.any() and (~over & (lens > 0)).any()
    assert np.array_equal(tight[0]["status"], np.where(over, aln_amd.E_OVERFLOW, 0))
    assert np.array_equal(tight[4], np.where(over, 0, lens))
    for r in range(len(qs)):
        for k in range(len(ts)):
            for a in range(4):
                assert tight[2][r][k][a] == ("" if over[r, k, a] else whole[2][r][k][a])
                assert np.array_equal(tight[1][r][k][a], whole[1][r][k][a])
    # outputs that are not wanted
    bare = aln_amd.hits_align_multi(ctx, qs, ts, hits, n_hits, mc.ALPHA, mc.BLOSUM, 11, 1, 4, want_pairs=False, want_lines=False)
    assert bare[1] is None and bare[2] is None and bare[4] is None and bare[0].tobytes() == whole[0].tobytes()


# ---- 5. arguments ------------------------------------------------------------------------------------------------------------------
class Raw:
    """aln_hits_align_multi through ctypes with sentinel-filled outputs"""

    def __init__(self, qs, ts, K, N, pair_stride=16, line_stride=40, mode=aln_amd.LOCAL):
        self.qp, self.tp = aln_amd.SeqPool(qs), aln_amd.SeqPool(ts)
        self.tab = np.ascontiguousarray(mc.BLOSUM, dtype=np.float32)
        self.ab = mc.ALPHA.encode()
        self.sub = aln_amd.AlnSubmatrix(len(mc.ALPHA), self.ab, self.tab.ctypes.data_as(C.POINTER(C.c_float)))
        self.g = aln_amd.AlnGap()
        self.g.model, self.g.align_type, self.g.gap_init, self.g.gap_extn = aln_amd.GAP_AFFINE_CONST, mode, 11.0, 1.0
        self.rows, self.K, self.N, self.ps, self.ls = len(qs), K, N, pair_stride, line_stride
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
        a = dict(hits=hit_array.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits=n_array.ctypes.data_as(ip), N=self.N, ms=-math.inf,
                 n_found=self.n_found.ctypes.data_as(ip), out=self.out.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)),
                 pairs=self.pairs.ctypes.data_as(ip), ps=self.ps, tl=self.tl, ql=self.ql, ls=self.ls,
                 lengths=self.lengths.ctypes.data_as(ip), K=self.K, q_begin=0, q_end=self.rows)
        a.update(kw)
        return aln_amd.lib().aln_hits_align_multi(gpu_util.ctx().h, C.byref(self.qp.c), C.byref(self.tp.c), C.byref(self.sub),
                                                  C.byref(self.g), a["q_begin"], a["q_end"], a["K"], a["hits"], a["n_hits"], a["N"],
                                                  a["ms"], a["n_found"], a["out"], a["pairs"], a["ps"], a["tl"], a["ql"], a["ls"],
                                                  a["lengths"])


def test_arguments():
    ctx = gpu_util.ctx()
    qs, ts = ["PAWHEAE", "HEAGAWGHEE"], ["HEAGAWGHEE", "PAWHEAE", "AWHE"]
    hits, n_hits = all_pairs_hits(2, 2)
    raw = Raw(qs, ts, 2, 3)
    assert raw.call(hits, n_hits) == 0 and not raw.untouched()
    assert aln_amd.hits_align_routes(ctx) == (4, 0)
    raw.fill()
    # group 1: n_found and N join aln_hits_align's first group
    for kw in (dict(n_found=None), dict(N=0), dict(N=17), dict(N=-1), dict(hits=None), dict(n_hits=None), dict(out=None), dict(K=0),
               dict(K=1025), dict(ps=1), dict(tl=None), dict(ql=None), dict(ls=0), dict(tl=None, ql=None, ls=0)):
        assert raw.call(hits, n_hits, **kw) == aln_amd.E_ARG, kw
        assert raw.untouched(), kw
        assert aln_amd.hits_align_routes(ctx) == (0, 0)
    # ... before the score checks: a residue outside the alphabet is only reported once group 1 passes
    rawj = Raw(["ACJ", "ACD"], ts, 2, 3)
    assert rawj.call(hits, n_hits, N=0) == aln_amd.E_ARG
    assert rawj.call(hits, n_hits) == aln_amd.E_RESIDUE and rawj.untouched()
    assert raw.call(hits, n_hits, q_begin=1, q_end=0) == aln_amd.E_ARG and raw.untouched()
    # an align type other than local: directly after the score checks, before the slots are looked at
    for mode in (aln_amd.GLOBAL, aln_amd.SEMI_LOCAL, aln_amd.GLOBAL_LOCAL, aln_amd.LOCAL_GLOBAL):
        rawg = Raw(qs, ts, 2, 3, mode=mode)
        assert rawg.call(hits, n_hits) == aln_amd.E_ARG and rawg.untouched()
        rawgj = Raw(["ACJ", "ACD"], ts, 2, 3, mode=mode)
        assert rawgj.call(hits, n_hits) == aln_amd.E_RESIDUE and rawgj.untouched()
    # the slots: n_hits and t; the end cell and the score are never read
    for field, r, k, value in (("n", 0, 0, -1), ("n", 1, 0, 3), ("t", 0, 1, -1), ("t", 1, 0, len(ts))):
        h, n = hits.copy(), n_hits.copy()
        if field == "n":
            n[r] = value
        else:
            h[field][r, k] = value
        assert raw.call(h, n) == aln_amd.E_ARG and raw.untouched(), (field, r, k, value)
    assert raw.call(hits, n_hits, q_begin=1, q_end=1) == 0 and raw.untouched()
    h = hits.copy()
    h["q_end"], h["t_end"], h["score"] = -3, 1 << 30, np.nan
    assert raw.call(h, n_hits) == 0
    first = raw.out.copy()
    raw.fill()
    assert raw.call(hits, n_hits) == 0 and raw.out.tobytes() == first.tobytes()


# ---- 6. the batch route ------------------------------------------------------------------------------------------------------------
def test_fallback_routes():
    """a 2100-residue template, the dropped length class (1793 .. 2048 columns), a pair without an interior; then a fractional
    gap, which sends every slot through batches"""
    ctx = gpu_util.ctx()
    d = rc.random_seq(mc.AA, 901, 30)
    def planted(n, seed):
        body = rc.random_seq(mc.AA, seed, n)
        return mc.mutated(d, seed + 1) + body[30:n - 40] + d + body[n - 10:]
    q = d + rc.random_seq(mc.AA, 902, 5) + d
    qs = [q, "W"]
    ts = [planted(2100, 910), planted(1900, 920), planted(300, 930), ""]
    assert [(len(t) + 2 + 255) // 256 for t in ts[:3]] == [9, 8, 2]
    hits, n_hits = all_pairs_hits(2, 4)
    pairs_qt = [(r, k) for r in range(2) for k in range(4)]
    for gi, fused, batched in ((11, 2, 6), (10.5, 0, 8)):
        res = aln_amd.hits_align_multi(ctx, qs, ts, hits, n_hits, mc.ALPHA, mc.BLOSUM, gi, 1, 4)
        assert res[6] in (0, aln_amd.E_STARTPAIR)
        assert aln_amd.hits_align_routes(ctx) == (fused, batched)
        det = aln_amd.hits_align_multi_detour(ctx, qs, ts, pairs_qt, mc.ALPHA, mc.BLOSUM, gi, 1, 4)
        for p, (r, k) in enumerate(pairs_qt):
            rec, n = res[0][r, k], int(res[5][r, k])
            assert n == len(det[p]) and n >= 1, (gi, r, k)
            for a, (score, pl, ident, t_line, q_line, status) in enumerate(det[p]):
                assert rec[a]["status"] == status and bits(rec[a]["score"]) == bits(score), (gi, r, k, a)
                if status == 0:
                    assert np.array_equal(res[1][r][k][a], pl) and bits(rec[a]["identity"]) == bits(ident), (gi, r, k, a)
                    assert res[2][r][k][a] == t_line and res[3][r][k][a] == q_line, (gi, r, k, a)
            for a in range(n, 4):
                assert rec[a].tobytes() == bytes(16)
        assert (res[5][0, :3] >= 3).all()                        # three domain pairings and more in the long templates
        assert res[5][0, 3] == 1 and res[5][1, 3] == 1           # no interior: round 0 only
