"""-m gpu: aln_hits_align — Optimal's alignment of every search hit, traced on the device from the end cell aln_search_topk
reported (one wave per hit: register-resident row sweep, 1 byte per cell into a transient strip, walk back through the strip).
Every comparison is exact: pair lists and lengths as integers, scores and identities as uint32, lines byte for byte.  The
comparator is the batch route the header names — one resident Batch over the same (row, template) pairs, dp_submatrix + optimal +
optimal_strings — and, for small pairs and the tie cases, the oracle's own build and traceback."""
import ctypes as C

import numpy as np
import pytest

import aln_amd
import gpu_util
import orc
from aln_amd.synth import AA20, MT19937, homolog_pair, residues

pytestmark = pytest.mark.gpu

U32 = np.uint32


def mutate(g, s, rate=0.15):
    r = g.draw(2 * len(s))
    return "".join(AA20[int(r[2 * i + 1]) % 20] if r[2 * i] % 100 < int(rate * 100) else ch for i, ch in enumerate(s))


_SET = {}


def ragged_set():
    """9 queries of 1..400 residues, 40 templates of 0..1790 residues around the 256-column class boundaries (1790 residues =
    1792 columns: the last column of the widest fused instantiation), a planted homolog of query 3, two mosaics of mutated
    pieces of the longer queries and two verbatim copies of the first mosaic."""
    if _SET:
        return _SET["qs"], _SET["ts"]
    qlens = [1, 7, 64, 200, 333, 400, 25, 90, 150]
    qs = [residues(MT19937(81000 + n), ln) for n, ln in enumerate(qlens)]
    h1, h2 = homolog_pair(81500, 200)
    qs[3] = h1
    tlens = [0, 1, 5, 40, 120, 253, 254, 255, 256, 257, 300, 509, 510, 511, 512, 513, 600, 765, 766, 767, 1021, 1022, 1023, 1024,
             1025, 1100, 1279, 1500, 1789, 1790] + [int(x) for x in np.random.RandomState(11).randint(2, 400, 5)]
    ts = [residues(MT19937(82000 + n), ln) for n, ln in enumerate(tlens)]
    ts.append(h2)
    g = MT19937(83000)
    mosaics = []
    for m in range(2):
        parts = []
        for q in qs:
            if len(q) >= 25:
                off = 3 * m if len(q) >= 40 else 0
                parts.append(mutate(g, q[off:off + 24]) + residues(g, 3))
        mosaics.append("".join(parts))
    ts += mosaics
    for at in (3, 17):
        ts.insert(at, mosaics[0])
    # a piece of the two longest queries near the END of the two longest templates: long strips, far columns
    a, b = [n for n, t in enumerate(ts) if len(t) in (1789, 1790)]
    ts[a] = ts[a][:1650] + mutate(g, qs[4][200:290]) + ts[a][1740:]
    ts[b] = ts[b][:1700] + mutate(g, qs[5][300:380]) + ts[b][1780:]
    assert len(ts) == 40 and (len(ts[a]), len(ts[b])) == (1789, 1790)
    _SET["qs"], _SET["ts"] = qs, ts
    return qs, ts


def used_slots(n_hits, K):
    return [(r, k) for r in range(len(n_hits)) for k in range(K) if k < n_hits[r]]


def batch_route(ctx, qs, ts, hits, n_hits, alpha, table, mode, gi, ge, q_begin=0):
    """the comparator: one Batch over the used slots, row-major -> per used slot (score, list, identity, tline, qline)"""
    slots = used_slots(n_hits, hits.shape[1])
    if not slots:
        return []
    b = aln_amd.Batch(ctx, qs, ts, [q_begin + r for r, k in slots], [int(hits["t"][r, k]) for r, k in slots])
    try:
        b.dp_submatrix(alpha, table, mode, gi, ge)
        scores, lists, status = b.optimal()
        s2, ident, st2, tl, ql = b.optimal_strings()
    finally:
        b.close()
    assert (status == 0).all() and (st2 == 0).all()
    assert np.array_equal(scores.view(U32), s2.view(U32))
    return [(scores[p], lists[p], ident[p], tl[p], ql[p]) for p in range(len(slots))]


def check_equal(res, hits, n_hits, ref, what=("pairs", "lines")):
    rec, lists, tl, ql, lengths, rc = res
    K = hits.shape[1]
    slots = used_slots(n_hits, K)
    assert len(slots) == len(ref)
    for p, (r, k) in enumerate(slots):
        sc, pl, idn, t_line, q_line = ref[p]
        e = rec[r, k]
        assert e["status"] == 0, (r, k, e)
        assert e["n_pairs"] == len(pl), (r, k, e, len(pl))
        assert np.float32(e["score"]).view(U32) == np.float32(sc).view(U32), (r, k, e, sc)
        assert np.float32(e["identity"]).view(U32) == np.float32(idn).view(U32), (r, k, e, idn)
        if "pairs" in what:
            assert np.array_equal(lists[r][k], pl), (r, k, lists[r][k].tolist(), pl.tolist())
        if "lines" in what:
            assert tl[r][k] == t_line and ql[r][k] == q_line, (r, k)
            assert lengths[r, k] == len(t_line), (r, k)
    for r in range(len(n_hits)):
        for k in range(n_hits[r], K):
            assert rec[r, k].tobytes() == bytes(16), (r, k)
            if "lines" in what:
                assert lengths[r, k] == 0 and tl[r][k] == "" and ql[r][k] == ""
            if "pairs" in what:
                assert len(lists[r][k]) == 0
    assert rc == 0


def same_results(a, b):
    assert a[0].tobytes() == b[0].tobytes()
    assert all(np.array_equal(x, y) for ra, rb in zip(a[1], b[1]) for x, y in zip(ra, rb))
    assert a[2] == b[2] and a[3] == b[3] and np.array_equal(a[4], b[4]) and a[5] == b[5]


_RAGGED = {}


def ragged_results(K, blosum62):
    """search + hits_align + the batch route on the ragged set, computed once per K and left unchanged"""
    if K not in _RAGGED:
        alpha, table = blosum62
        qs, ts = ragged_set()
        ctx = gpu_util.ctx()
        hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, K)
        res = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1)
        ref = batch_route(ctx, qs, ts, hits, n_hits, alpha, table, aln_amd.LOCAL, 11, 1)
        _RAGGED[K] = (hits, n_hits, res, ref)
    return _RAGGED[K]


# ---- 1. equals the batch route ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5])
def test_equals_the_batch_route(K, blosum62):
    alpha, table = blosum62
    qs, ts = ragged_set()
    ctx = gpu_util.ctx()
    hits, n_hits, res, ref = ragged_results(K, blosum62)
    assert (n_hits == K).all()
    check_equal(res, hits, n_hits, ref)
    for chunk in (1, 3):
        with ctx.hints(align_chunk_hits=chunk):
            assert ctx.get_hint("align_chunk_hits") == chunk
            again = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1)
        same_results(again, res)
    assert ctx.get_hint("align_chunk_hits") == 0
    with ctx.hints(align_list_group_slots=1):                          # groups lists read on the host: nothing here
        same_results(aln_amd.hits_align(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1), res)


def test_every_length_class_equals_the_batch_route(blosum62):
    """K = n_templates aligns every pair of two rows: every fused instantiation, the dropped class and the degenerate templates"""
    alpha, table = blosum62
    qs, ts = ragged_set()
    ctx = gpu_util.ctx()
    sub = [qs[2], qs[4]]
    hits, n_hits = aln_amd.search_topk(ctx, sub, ts, alpha, table, 11, 1, len(ts))
    assert (n_hits == len(ts)).all()
    res = aln_amd.hits_align(ctx, sub, ts, hits, n_hits, alpha, table, 11, 1)
    check_equal(res, hits, n_hits, batch_route(ctx, sub, ts, hits, n_hits, alpha, table, aln_amd.LOCAL, 11, 1))


# ---- 2. equals the oracle --------------------------------------------------------------------------------------------------
def test_equals_the_oracle(blosum62):
    alpha, table = blosum62
    qs, ts = ragged_set()
    checked = 0
    for K in (1, 5):
        hits, n_hits, res, ref = ragged_results(K, blosum62)
        rec, lists = res[0], res[1]
        for r, k in used_slots(n_hits, K):
            q, t = qs[r], ts[hits["t"][r, k]]
            if (len(q) + 2) * (len(t) + 2) >= 40000:
                continue
            S = orc.sim_submatrix(q, t, alpha, table)
            rc, D, PQ, PT = orc.dp_build(S, orc.Gap(orc.LOCAL, 11, 1))
            rc2, sc, pl = orc.optimal(D, PQ, PT, True)
            assert rc == 0 and rc2 == 0
            assert np.array_equal(lists[r][k], pl), (r, k)
            assert np.float32(rec["score"][r, k]).view(U32) == np.float32(sc).view(U32)
            checked += 1
    assert checked >= 10, checked


# ---- 3. ties ---------------------------------------------------------------------------------------------------------------
def low_complexity(seed, n, alpha):
    rs = np.random.RandomState(seed)
    if rs.randint(3) == 0:                                     # a repeat such as ACACAC... with a few point changes
        unit = "".join(alpha[x] for x in rs.randint(len(alpha), size=rs.randint(1, 4)))
        s = list((unit * (n // len(unit) + 1))[:n])
        for _ in range(rs.randint(0, 4)):
            s[rs.randint(n)] = alpha[rs.randint(len(alpha))]
        return "".join(s)
    return "".join(alpha[x] for x in rs.randint(len(alpha), size=n))


TIE_GAPS = [(0, 0), (0, 1), (1, 5), (11, 1)]     # range_cases.GAP_FAMILIES: gap_init == gap_extn, gap_init 0 and 1, the usual pair
TIE_SEEDS = range(6)                             # chosen on the CPU with the oracle: the counts asserted below hold with margin


def top_two_equal(D, i, j, gi, ge):
    """cell (i, j), i, j >= 2: do the two best of (match, best deletion, best insertion) tie?  (dpmatrix.h:607-649 restated)"""
    Di = D.astype(np.int64)
    none = -(1 << 40)
    m = Di[i - 1, j - 1]
    e = max([Di[i - 1, k] - gi - ge * (j - k - 2) for k in range(1, j - 1)] or [none])
    f = max([Di[k, j - 1] - gi - ge * (i - k - 2) for k in range(1, i - 1)] or [none])
    a = sorted([m, e, f], reverse=True)
    return a[0] == a[1]


def test_ties_equal_the_oracle_and_the_batch_route():
    ctx = gpu_util.ctx()
    n_del = n_ins = n_tie = 0
    for alpha in ("AC", "ACGT"):
        table = np.full((len(alpha), len(alpha)), -1, dtype=np.float32)
        np.fill_diagonal(table, 2)
        for gi, ge in TIE_GAPS:
            qs, ts = [], []
            for seed in TIE_SEEDS:
                rs = np.random.RandomState(1000 + seed)
                qs.append(low_complexity(5000 + seed, rs.randint(20, 121), alpha))
                ts.append(low_complexity(7000 + seed, rs.randint(20, 121), alpha))
            hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, gi, ge, len(ts))
            assert (n_hits == len(ts)).all()
            res = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, alpha, table, gi, ge)
            check_equal(res, hits, n_hits, batch_route(ctx, qs, ts, hits, n_hits, alpha, table, aln_amd.LOCAL, gi, ge))
            for r in range(len(qs)):                           # the diagonal pairs against the oracle, with the tie census
                k = int(np.nonzero(hits["t"][r] == r)[0][0])
                S = orc.sim_submatrix(qs[r], ts[r], alpha, table)
                rc, D, PQ, PT = orc.dp_build(S, orc.Gap(orc.LOCAL, gi, ge))
                rc2, sc, pl = orc.optimal(D, PQ, PT, True)
                assert rc == 0 and rc2 == 0
                assert np.array_equal(res[1][r][k], pl), (alpha, gi, ge, r)
                assert np.float32(res[0]["score"][r, k]).view(U32) == np.float32(sc).view(U32)
                path = pl[1:-1] if (pl[0] == 0).all() else pl[:-1]      # the cells the walk visited
                for a, b in zip(path[:-1], path[1:]):
                    n_del += int(b[0] - a[0] == 1 and b[1] - a[1] > 1)
                    n_ins += int(b[1] - a[1] == 1 and b[0] - a[0] > 1)
                for c in path:
                    if c[0] >= 2 and c[1] >= 2:
                        n_tie += int(top_two_equal(D, int(c[0]), int(c[1]), gi, ge))
    assert n_del >= 20 and n_ins >= 20 and n_tie >= 20, (n_del, n_ins, n_tie)


# ---- 4. route boundary and degenerate shapes --------------------------------------------------------------------------------
def test_route_boundary(blosum62):
    """1791 / 1792 columns: the widest fused instantiation; 1793 and 2047 .. 2049 columns: the class that goes the batch route;
    2602 columns: beyond the register-resident kernels altogether"""
    alpha, table = blosum62
    ctx = gpu_util.ctx()
    g = MT19937(84000)
    q64 = residues(g, 64)
    qs = [residues(g, 7), q64]
    ts = []
    for n, ln in enumerate((1789, 1790, 1791, 2045, 2046, 2047, 2600)):
        body = residues(g, ln)
        at = ln - 100 - 11 * n
        ts.append(body[:at] + mutate(g, q64) + body[at + 64:])
        assert len(ts[-1]) == ln
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, len(ts))
    assert (n_hits == len(ts)).all() and (hits["score"][1] > 100).all()
    res = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1)
    check_equal(res, hits, n_hits, batch_route(ctx, qs, ts, hits, n_hits, alpha, table, aln_amd.LOCAL, 11, 1))
    assert (res[0]["n_pairs"][1] > 40).all()


def test_degenerate_shapes(blosum62):
    alpha, table = blosum62
    ctx = gpu_util.ctx()
    qs = ["", "A", "WWWW", "WW", "W"]
    ts = ["", "C", "CCCCC", "PPPPPPP", "G", "CC"]
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, len(ts))
    assert (n_hits == len(ts)).all()
    assert (hits["score"] == 0).all()                          # every row's best score is 0 ...
    for r in range(len(qs)):                                   # ... so every hit reports find_max's seed cell (Q-2, T-2)
        for h in hits[r]:
            assert (h["q_end"], h["t_end"]) == (len(qs[r]), len(ts[h["t"]])), (r, h)
    res = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1)
    check_equal(res, hits, n_hits, batch_route(ctx, qs, ts, hits, n_hits, alpha, table, aln_amd.LOCAL, 11, 1))
    k = int(np.nonzero(hits["t"][2] == 2)[0][0])               # WWWW x CCCCC: an interior seed gets (0,0) prepended
    assert res[1][2][k].tolist() == [[0, 0], [4, 5], [5, 6]]
    k = int(np.nonzero(hits["t"][4] == 1)[0][0])               # W x C: the seed is in row 1, it points at the origin
    assert res[1][4][k].tolist() == [[1, 1], [2, 2]]


# ---- 5. non-local align types -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [aln_amd.GLOBAL_LOCAL, aln_amd.GLOBAL, aln_amd.LOCAL_GLOBAL, aln_amd.SEMI_LOCAL])
def test_non_local_align_types(mode, blosum62):
    alpha, table = blosum62
    qs, ts = ragged_set()
    qs, ts = qs[1:7], ts[2:12]
    ctx = gpu_util.ctx()
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, 4, align_type=mode)
    hits["q_end"], hits["t_end"] = -7, 1 << 20                 # ignored: Optimal starts at (Q-1, T-1)
    res = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, align_type=mode)
    check_equal(res, hits, n_hits, batch_route(ctx, qs, ts, hits, n_hits, alpha, table, mode, 11, 1))


# ---- 6. slot handling -------------------------------------------------------------------------------------------------------
def test_slot_handling(blosum62):
    alpha, table = blosum62
    qs, ts = ragged_set()
    ctx = gpu_util.ctx()
    K = 5
    full, n_full, _, _ = ragged_results(K, blosum62)
    hits, n_hits = full[2:7].copy(), n_full[2:7].copy()        # a row block: rows are queries 2 .. 6
    n_hits[1] = 0                                              # a row without hits
    n_hits[3] = 2                                              # unused slots that still hold a hit
    hits[4, 1] = hits[4, 0]                                    # duplicates
    hits[4, 3] = hits[4, 0]
    ref = batch_route(ctx, qs, ts, hits, n_hits, alpha, table, aln_amd.LOCAL, 11, 1, q_begin=2)
    res = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, q_begin=2)
    check_equal(res, hits, n_hits, ref)
    assert np.array_equal(res[1][4][1], res[1][4][0]) and res[2][4][3] == res[2][4][0]
    lines_only = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, q_begin=2, want_pairs=False)
    assert lines_only[1] is None
    check_equal(lines_only, hits, n_hits, ref, what=("lines",))
    assert lines_only[0].tobytes() == res[0].tobytes() and lines_only[2] == res[2] and lines_only[3] == res[3]
    pairs_only = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, q_begin=2, want_lines=False)
    assert pairs_only[2] is None and pairs_only[4] is None
    check_equal(pairs_only, hits, n_hits, ref, what=("pairs",))
    assert pairs_only[0].tobytes() == res[0].tobytes()
    neither = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, q_begin=2, want_pairs=False, want_lines=False)
    assert neither[0].tobytes() == res[0].tobytes()


# ---- 7. the contract of the trusted end cell --------------------------------------------------------------------------------
def test_trusted_end_cell_contract(blosum62):
    alpha, table = blosum62
    qs, ts = ragged_set()
    ctx = gpu_util.ctx()
    hits, n_hits, res, ref = ragged_results(5, blosum62)
    r, k = 6, 0                                                # query 6 has 25 residues: a small matrix for the oracle
    t = ts[hits["t"][r, k]]
    S = orc.sim_submatrix(qs[r], t, alpha, table)
    rc, D, PQ, PT = orc.dp_build(S, orc.Gap(orc.LOCAL, 11, 1))
    assert rc == 0
    Q, T = D.shape
    qe, te = int(hits["q_end"][r, k]), int(hits["t_end"][r, k])
    assert D[qe, te] == hits["score"][r, k]
    other = [i for i in range(1, Q - 1) if D[i, te] != D[qe, te]]      # in-range cells of the same column, another score
    assert other
    for moved in (other[0], other[-1]):
        bad = hits.copy()
        bad["q_end"][r, k] = moved
        got = aln_amd.hits_align(ctx, qs, ts, bad, n_hits, alpha, table, 11, 1)
        assert got[5] == aln_amd.E_ARG
        e = got[0][r, k]
        assert e["status"] == aln_amd.E_ARG and e["n_pairs"] == 0 and len(got[1][r][k]) == 0 and got[2][r][k] == ""
        keep = np.ones(hits.shape, dtype=bool)
        keep[r, k] = False
        assert got[0][keep].tobytes() == res[0][keep].tobytes()
        for rr, kk in used_slots(n_hits, 5):
            if (rr, kk) != (r, k):
                assert np.array_equal(got[1][rr][kk], res[1][rr][kk]) and got[2][rr][kk] == res[2][rr][kk]


# ---- 8. arguments -----------------------------------------------------------------------------------------------------------
class Raw:
    """aln_hits_align through ctypes with sentinel-filled outputs"""

    def __init__(self, qs, ts, blosum62, K, pair_stride=16, line_stride=40, mode=aln_amd.LOCAL):
        alpha, table = blosum62
        self.qp, self.tp = aln_amd.SeqPool(qs), aln_amd.SeqPool(ts)
        self.tab = np.ascontiguousarray(table, dtype=np.float32)
        self.ab = alpha.encode()
        self.sub = aln_amd.AlnSubmatrix(len(alpha), self.ab, self.tab.ctypes.data_as(C.POINTER(C.c_float)))
        self.g = aln_amd.AlnGap()
        self.g.model, self.g.align_type, self.g.gap_init, self.g.gap_extn = aln_amd.GAP_AFFINE_CONST, mode, 11.0, 1.0
        self.rows, self.K, self.ps, self.ls = len(qs), K, pair_stride, line_stride
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
        a = dict(hits=hit_array.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits=n_array.ctypes.data_as(ip),
                 out=self.out.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)), pairs=self.pairs.ctypes.data_as(ip), ps=self.ps,
                 tl=self.tl, ql=self.ql, ls=self.ls, lengths=self.lengths.ctypes.data_as(ip), K=self.K, q_begin=0, q_end=self.rows)
        a.update(kw)
        return aln_amd.lib().aln_hits_align(gpu_util.ctx().h, C.byref(self.qp.c), C.byref(self.tp.c), C.byref(self.sub), C.byref(self.g),
                                            a["q_begin"], a["q_end"], a["K"], a["hits"], a["n_hits"], a["out"], a["pairs"], a["ps"],
                                            a["tl"], a["ql"], a["ls"], a["lengths"])

    def records(self):
        return self.out.view(aln_amd.HIT_ALIGNMENT_DTYPE).reshape(self.rows, self.K)


def test_arguments(blosum62):
    alpha, table = blosum62
    ctx = gpu_util.ctx()
    qs, ts = ["PAWHEAE", "HEAGAWGHEE"], ["HEAGAWGHEE", "PAWHEAE", "AWHE"]
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, 2)
    assert (n_hits == 2).all()
    raw = Raw(qs, ts, blosum62, 2)
    assert raw.call(hits, n_hits) == 0 and not raw.untouched()
    good = raw.records().copy()
    assert (good["status"] == 0).all() and (good["n_pairs"] >= 2).all() and (good["n_pairs"] > 2).any()
    raw.fill()
    # group 1
    for kw in (dict(hits=None), dict(n_hits=None), dict(out=None), dict(K=0), dict(K=1025), dict(K=-1), dict(ps=1), dict(ps=0),
               dict(tl=None), dict(ql=None), dict(ls=0), dict(tl=None, ql=None, ls=0)):
        assert raw.call(hits, n_hits, **kw) == aln_amd.E_ARG, kw
        assert raw.untouched(), kw
    # ... before the score checks: a residue outside the alphabet is only reported once group 1 passes
    rawj = Raw(["ACJ", "ACD"], ts, blosum62, 2)
    assert rawj.call(hits, n_hits, K=0) == aln_amd.E_ARG
    assert rawj.call(hits, n_hits) == aln_amd.E_RESIDUE and rawj.untouched()
    assert raw.call(hits, n_hits, q_begin=1, q_end=0) == aln_amd.E_ARG and raw.untouched()
    # group 3
    Q = [len(q) + 2 for q in qs]
    for field, r, k, value in (("n", 0, 0, -1), ("n", 1, 0, 3), ("t", 0, 1, -1), ("t", 1, 0, len(ts)),
                               ("q_end", 0, 0, 0), ("q_end", 1, 1, Q[1] - 1), ("t_end", 0, 1, 0),
                               ("t_end", 1, 0, len(ts[hits["t"][1, 0]]) + 1)):
        h, n = hits.copy(), n_hits.copy()
        if field == "n":
            n[r] = value
        else:
            h[field][r, k] = value
        assert raw.call(h, n) == aln_amd.E_ARG, (field, r, k, value)
        assert raw.untouched(), (field, r, k, value)
    # q_begin == q_end: ALN_OK, nothing written
    assert raw.call(hits, n_hits, q_begin=1, q_end=1) == 0 and raw.untouched()
    # a list longer than pair_stride, a line longer than line_stride: per-slot ALN_E_OVERFLOW
    small = Raw(qs, ts, blosum62, 2, pair_stride=2)
    assert small.call(hits, n_hits) == aln_amd.E_OVERFLOW
    rec = small.records()
    assert np.array_equal(rec["status"], np.where(good["n_pairs"] > 2, aln_amd.E_OVERFLOW, 0)) and np.array_equal(rec["n_pairs"], good["n_pairs"])
    assert (small.pairs.reshape(4, 4)[:, :2] == raw_first_pairs(qs, ts, hits, n_hits, blosum62)).all()
    assert np.array_equal(small.lengths, raw_lengths(qs, ts, hits, n_hits, blosum62))
    short = Raw(qs, ts, blosum62, 2, line_stride=8)
    assert short.call(hits, n_hits) == aln_amd.E_OVERFLOW
    rec = short.records()
    assert (rec["status"] == aln_amd.E_OVERFLOW).all() and (short.lengths == 0).all()
    assert all(short.tl.raw[s * 8] == 0 and short.ql.raw[s * 8] == 0 for s in range(4))
    assert np.array_equal(rec["score"].view(U32), good["score"].view(U32))
    with pytest.raises(aln_amd.AlnError) as ei:
        ctx.set_hint("align_chunk_rows", 1)
    assert ei.value.code == aln_amd.E_ARG


def raw_lengths(qs, ts, hits, n_hits, blosum62):
    res = aln_amd.hits_align(gpu_util.ctx(), qs, ts, hits, n_hits, blosum62[0], blosum62[1], 11, 1)
    return res[4].reshape(-1)


def raw_first_pairs(qs, ts, hits, n_hits, blosum62):
    res = aln_amd.hits_align(gpu_util.ctx(), qs, ts, hits, n_hits, blosum62[0], blosum62[1], 11, 1)
    return np.array([res[1][r][k][0] for r in range(2) for k in range(2)])
