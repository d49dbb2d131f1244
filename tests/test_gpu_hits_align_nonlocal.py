"""-m gpu: aln_hits_align under the four non-local align types — hit_global_kernel<R>: one wave per hit sweeps every
row, 1 byte per cell into a transient strip, the final cell's pointer from the last row and column, a walk back to the origin.
Every comparison is exact: pair lists and lengths as integers, scores and identities as uint32, lines byte for byte.  The
comparators are the batch route (the same call with hint align_fused_nonlocal = 0, and one resident Batch over the pairs) and,
for small pairs and the tie cases, the oracle's own build and traceback."""
import numpy as np
import pytest

import aln_amd
import gpu_util
import nonlocal_cases as nc
from aln_amd.synth import AA20, MT19937, homolog_pair, residues

pytestmark = pytest.mark.gpu

U32 = np.uint32
MODES = [aln_amd.GLOBAL_LOCAL, aln_amd.GLOBAL, aln_amd.LOCAL_GLOBAL, aln_amd.SEMI_LOCAL]
FUSED_CLASSES = range(1, 9)          # ResidueQuery::kFusedGlobal (csrc/score_common.h): templates of up to 2048 columns


def fused_expected(q, t):
    """does the pair run in the fused kernel under an integer scoring system?"""
    Q, T = len(q) + 2, len(t) + 2
    return Q >= 3 and T >= 3 and T <= 2048 and (T + 255) // 256 in FUSED_CLASSES


def all_pairs_hits(n_q, n_t, garbage=True):
    """every template for every row, in template order; the slots' score and end cell are ignored by the non-local types"""
    hits = np.zeros((n_q, n_t), dtype=aln_amd.HIT_DTYPE)
    hits["t"] = np.arange(n_t, dtype=np.int32)[None, :]
    if garbage:
        hits["score"], hits["q_end"], hits["t_end"] = -1e30, -7, 1 << 20
    return hits, np.full(n_q, n_t, dtype=np.int32)


def used_slots(n_hits, K):
    return [(r, k) for r in range(len(n_hits)) for k in range(K) if k < n_hits[r]]


def batch_route(ctx, qs, ts, hits, n_hits, alpha, table, mode, gi, ge, q_begin=0):
    """one Batch over the used slots, row-major -> per used slot (score, list, identity, tline, qline)"""
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


def check_equal(res, hits, n_hits, ref):
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
        assert np.array_equal(lists[r][k], pl), (r, k, lists[r][k].tolist(), pl.tolist())
        assert tl[r][k] == t_line and ql[r][k] == q_line, (r, k)
        assert lengths[r, k] == len(t_line), (r, k)
    for r in range(len(n_hits)):
        for k in range(n_hits[r], K):
            assert rec[r, k].tobytes() == bytes(16), (r, k)
            assert lengths[r, k] == 0 and tl[r][k] == "" and ql[r][k] == "" and len(lists[r][k]) == 0
    assert rc == 0


def same_results(a, b):
    assert a[0].tobytes() == b[0].tobytes()
    assert (a[1] is None) == (b[1] is None) and (a[2] is None) == (b[2] is None)
    if a[1] is not None:
        assert all(np.array_equal(x, y) for ra, rb in zip(a[1], b[1]) for x, y in zip(ra, rb))
    if a[2] is not None:
        assert a[2] == b[2] and a[3] == b[3] and np.array_equal(a[4], b[4])
    assert a[5] == b[5]


def both_routes(ctx, qs, ts, hits, n_hits, alpha, table, gi, ge, mode, **kw):
    """the call with the fused kernel allowed and with hint align_fused_nonlocal = 0: results must be byte-identical.
    -> (results, routes of the first call, routes of the second)"""
    assert ctx.get_hint("align_fused_nonlocal") == 1
    fused = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, alpha, table, gi, ge, align_type=mode, **kw)
    rf = aln_amd.hits_align_routes(ctx)
    with ctx.hints(align_fused_nonlocal=0):
        batch = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, alpha, table, gi, ge, align_type=mode, **kw)
        rb = aln_amd.hits_align_routes(ctx)
    assert ctx.get_hint("align_fused_nonlocal") == 1
    same_results(fused, batch)
    return fused, rf, rb


def check_oracle(res, qs, ts, hits, n_hits, alpha, table, mode, gi, ge, cen=None, q_begin=0):
    rec, lists = res[0], res[1]
    for r, k in used_slots(n_hits, hits.shape[1]):
        q, t = qs[q_begin + r], ts[hits["t"][r, k]]
        D, sc, pl = nc.oracle_pair(q, t, alpha, table, mode, gi, ge)
        assert np.array_equal(lists[r][k], pl), (mode, gi, ge, r, k, lists[r][k].tolist(), pl.tolist())
        assert np.float32(rec["score"][r, k]).view(U32) == np.float32(sc).view(U32), (mode, gi, ge, r, k)
        if cen is not None:
            nc.census(D, lists[r][k], gi, ge, cen)


# ---- 1. routes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_routes(mode, blosum62):
    alpha, table = blosum62
    ctx = gpu_util.ctx()
    g = MT19937(91000)
    qs = [residues(g, n) for n in (1, 5, 64, 30)]                # Q = 3 .. 66
    ts = [residues(g, n) for n in (1, 40, 300, 600)]             # T = 3 .. 602: classes 1, 2 and 3
    hits, n_hits = all_pairs_hits(len(qs), len(ts))
    n_used = int(n_hits.sum())
    res, rf, rb = both_routes(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, mode)
    assert rf == (n_used, 0) and rb == (0, n_used)
    check_equal(res, hits, n_hits, batch_route(ctx, qs, ts, hits, n_hits, alpha, table, mode, 11, 1))
    # what the fused kernel does not take goes the batch route in both settings: a template of 2600 residues, a query without
    # an interior row, a fractional gap
    ts2 = ts + [residues(g, 2600)]
    qs2 = qs + [""]
    hits2, n2 = all_pairs_hits(len(qs2), len(ts2))
    res2, rf2, rb2 = both_routes(ctx, qs2, ts2, hits2, n2, alpha, table, 11, 1, mode)
    n_fused = sum(fused_expected(q, t) for q in qs2 for t in ts2)
    assert n_fused == len(qs) * len(ts)
    assert rf2 == (n_fused, int(n2.sum()) - n_fused) and rb2 == (0, int(n2.sum()))
    check_equal(res2, hits2, n2, batch_route(ctx, qs2, ts2, hits2, n2, alpha, table, mode, 11, 1))
    res3, rf3, rb3 = both_routes(ctx, qs, ts, hits, n_hits, alpha, table, 4.73, 0.34, mode)
    assert rf3 == (0, n_used) and rb3 == (0, n_used)
    check_equal(res3, hits, n_hits, batch_route(ctx, qs, ts, hits, n_hits, alpha, table, mode, 4.73, 0.34))
    # after a local call the counts describe that call
    lh, ln = aln_amd.search_topk(ctx, qs, ts, alpha, table, 11, 1, 2)
    aln_amd.hits_align(ctx, qs, ts, lh, ln, alpha, table, 11, 1)
    assert aln_amd.hits_align_routes(ctx) == (int(ln.sum()), 0) and int(ln.sum()) > 0


# ---- 2. ties, against the oracle and the batch route -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_ties_equal_the_oracle_and_the_batch_route(mode):
    ctx = gpu_util.ctx()
    cen = nc.new_census()
    for alpha in ("AC", "ACGT"):
        table = nc.tie_table(alpha)
        qs, ts = nc.tie_sequences(alpha)
        hits, n_hits = all_pairs_hits(len(qs), len(ts))
        for gi, ge in nc.TIE_GAPS:
            res, rf, rb = both_routes(ctx, qs, ts, hits, n_hits, alpha, table, gi, ge, mode)
            assert rf == (36, 0) and rb == (0, 36)
            assert (res[0]["status"] == 0).all() and res[5] == 0
            check_oracle(res, qs, ts, hits, n_hits, alpha, table, mode, gi, ge, cen)
    print("census", mode, cen)
    assert nc.census_ok(cen), cen


# ---- 3. every kept class and the class boundaries, against the batch route -----------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_every_length_class_equals_the_batch_route(mode, blosum62):
    alpha, table = blosum62
    ctx = gpu_util.ctx()
    g = MT19937(92000)
    qs = [residues(g, 64), residues(g, 333)]
    tlens = [1, 2, 3, 5, 40, 253, 254, 255, 256, 257, 509, 510, 511, 512, 513, 765, 766, 767, 1021, 1022, 1023, 1024, 1025,
             1277, 1278, 1279, 1533, 1534, 1535, 1789, 1790, 1791, 2045, 2046, 2047, 2600]
    ts = [residues(g, n) for n in tlens]
    hits, n_hits = all_pairs_hits(len(qs), len(ts))
    res, rf, rb = both_routes(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, mode)
    n_fused = sum(fused_expected(q, t) for q in qs for t in ts)
    assert n_fused == 2 * (len(ts) - 2)                          # all but 2049 and 2602 columns
    assert rf == (n_fused, 2 * len(ts) - n_fused) and rb == (0, 2 * len(ts))
    rec = res[0]
    assert (rec["status"] == 0).all() and res[5] == 0
    for r, q in enumerate(qs):
        for k, t in enumerate(ts):
            pl = res[1][r][k]
            assert (pl[0] == 0).all() and tuple(pl[-1]) == (len(q) + 1, len(t) + 1) and (np.diff(pl, axis=0) >= 1).all()
            assert rec["identity"][r, k].view(U32) == gpu_util.identity_for(q, t, pl).view(U32)
            tl, qls, _ = gpu_util.strings_for(q, t, [pl])
            assert (res[2][r][k], res[3][r][k]) == (tl, qls[0]) and res[4][r, k] == len(tl)


# ---- 4. degenerate and smallest shapes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_degenerate_and_smallest_shapes(mode, blosum62):
    alpha, table = blosum62
    ctx = gpu_util.ctx()
    qs, ts = ["", "A", "WW", "WWWW"], ["", "C", "CC", "CCCCC"]
    hits, n_hits = all_pairs_hits(len(qs), len(ts))
    res, rf, rb = both_routes(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, mode)
    assert rf == (9, 7) and rb == (0, 16)                        # the empty query and the empty template have no interior
    check_equal(res, hits, n_hits, batch_route(ctx, qs, ts, hits, n_hits, alpha, table, mode, 11, 1))
    # Q = 3 (one interior row: the strip has no row of its own) and T = 3, against the oracle too
    g = MT19937(93000)
    qs = ["A", residues(g, 1), residues(g, 9), residues(g, 2)]
    ts = [residues(g, 1), "A", residues(g, 12), residues(g, 2)]
    for gi, ge in ((11, 1), (0, 0), (1, 5)):
        res, rf, rb = both_routes(ctx, qs, ts, hits, n_hits, alpha, table, gi, ge, mode)
        assert rf == (16, 0) and rb == (0, 16)
        check_oracle(res, qs, ts, hits, n_hits, alpha, table, mode, gi, ge)
        check_equal(res, hits, n_hits, batch_route(ctx, qs, ts, hits, n_hits, alpha, table, mode, gi, ge))


# ---- 5. chunking and slot handling ---------------------------------------------------------------------------------------------
def mutate(g, s, rate=0.15):
    r = g.draw(2 * len(s))
    return "".join(AA20[int(r[2 * i + 1]) % 20] if r[2 * i] % 100 < int(rate * 100) else ch for i, ch in enumerate(s))


@pytest.mark.parametrize("mode", MODES)
def test_chunking_and_slot_handling(mode, blosum62):
    alpha, table = blosum62
    ctx = gpu_util.ctx()
    g = MT19937(94000)
    qs = [residues(g, n) for n in (2, 25, 64, 150, 90, 33)]
    ts = [residues(g, n) for n in (5, 40, 120, 255, 300, 513, 600)] + [mutate(g, qs[3]), mutate(g, qs[4])[10:70], qs[2] + residues(g, 250)]
    K = 5
    rs = np.random.RandomState(94)
    hits = np.zeros((len(qs), K), dtype=aln_amd.HIT_DTYPE)
    hits["t"] = rs.randint(0, len(ts), size=(len(qs), K))
    hits["t"][0, 0] = hits["t"][1, 0] = 0                        # two pairs whose list and lines are short
    hits["score"], hits["q_end"], hits["t_end"] = 12345.0, 1 << 30, -1
    n_hits = np.full(len(qs), K, dtype=np.int32)
    res, rf, rb = both_routes(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, mode)
    assert rf == (len(qs) * K, 0)
    check_equal(res, hits, n_hits, batch_route(ctx, qs, ts, hits, n_hits, alpha, table, mode, 11, 1))
    for chunk in (1, 3):
        with ctx.hints(align_chunk_hits=chunk):
            again = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, align_type=mode)
        assert aln_amd.hits_align_routes(ctx) == rf
        same_results(again, res)
    # the slots' score and end cell change nothing
    other = hits.copy()
    other["score"], other["q_end"], other["t_end"] = 0.0, 1, 1
    same_results(aln_amd.hits_align(ctx, qs, ts, other, n_hits, alpha, table, 11, 1, align_type=mode), res)
    # a row block with a row without hits, unused slots that still hold a hit, duplicates
    h2, n2 = hits[2:6].copy(), n_hits[2:6].copy()
    n2[1] = 0
    n2[2] = 2
    h2[3, 1] = h2[3, 0]
    h2[3, 4] = h2[3, 0]
    res2, rf2, rb2 = both_routes(ctx, qs, ts, h2, n2, alpha, table, 11, 1, mode, q_begin=2)
    assert rf2 == (int(n2.sum()), 0) and rb2 == (0, int(n2.sum()))
    check_equal(res2, h2, n2, batch_route(ctx, qs, ts, h2, n2, alpha, table, mode, 11, 1, q_begin=2))
    assert np.array_equal(res2[1][3][1], res2[1][3][0]) and res2[2][3][4] == res2[2][3][0]
    lines_only, _, _ = both_routes(ctx, qs, ts, h2, n2, alpha, table, 11, 1, mode, q_begin=2, want_pairs=False)
    assert lines_only[1] is None and lines_only[0].tobytes() == res2[0].tobytes()
    assert lines_only[2] == res2[2] and lines_only[3] == res2[3] and np.array_equal(lines_only[4], res2[4])
    pairs_only, _, _ = both_routes(ctx, qs, ts, h2, n2, alpha, table, 11, 1, mode, q_begin=2, want_lines=False)
    assert pairs_only[2] is None and pairs_only[4] is None and pairs_only[0].tobytes() == res2[0].tobytes()
    assert all(np.array_equal(x, y) for ra, rb_ in zip(pairs_only[1], res2[1]) for x, y in zip(ra, rb_))
    neither, _, _ = both_routes(ctx, qs, ts, h2, n2, alpha, table, 11, 1, mode, q_begin=2, want_pairs=False, want_lines=False)
    assert neither[0].tobytes() == res2[0].tobytes()
    # a pair_stride / line_stride that is too small: the slot reports ALN_E_OVERFLOW, the first pair_stride entries are written
    small, _, _ = both_routes(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, mode, pair_stride=6)
    long_ = res[0]["n_pairs"] > 6
    assert long_.any() and not long_.all() and small[5] == aln_amd.E_OVERFLOW
    assert np.array_equal(small[0]["status"], np.where(long_, aln_amd.E_OVERFLOW, 0))
    assert np.array_equal(small[0]["n_pairs"], res[0]["n_pairs"]) and np.array_equal(small[0]["score"].view(U32), res[0]["score"].view(U32))
    for r, k in used_slots(n_hits, K):
        assert np.array_equal(small[1][r][k], res[1][r][k][:6]), (r, k)
    short, _, _ = both_routes(ctx, qs, ts, hits, n_hits, alpha, table, 11, 1, mode, line_stride=60)
    fits = res[4] < 60
    assert fits.any() and not fits.all() and short[5] == aln_amd.E_OVERFLOW
    assert np.array_equal(short[0]["status"], np.where(fits, 0, aln_amd.E_OVERFLOW))
    assert np.array_equal(short[4], np.where(fits, res[4], 0))
    for r, k in used_slots(n_hits, K):
        assert short[2][r][k] == (res[2][r][k] if fits[r, k] else "") and np.array_equal(short[1][r][k], res[1][r][k])


# ---- 6. one larger scoring system ----------------------------------------------------------------------------------------------
def ragged_set():
    """9 queries of 1..400 residues, 40 templates of 0..1790 residues around the 256-column class boundaries, a planted homolog
    of query 3 and two mosaics of mutated pieces of the longer queries (the set of tests/test_gpu_hits_align.py)"""
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
    assert len(ts) == 40
    return qs, ts


@pytest.mark.parametrize("mode", MODES)
def test_a_larger_scoring_system(mode, blosum62):
    alpha, table = blosum62
    ctx = gpu_util.ctx()
    qs, ts = ragged_set()
    table3 = (3 * table).astype(np.float32)
    K = 4
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alpha, table3, 33, 3, K, align_type=mode)
    assert (n_hits == K).all()
    res, rf, rb = both_routes(ctx, qs, ts, hits, n_hits, alpha, table3, 33, 3, mode)
    n_fused = sum(fused_expected(qs[r], ts[hits["t"][r, k]]) for r, k in used_slots(n_hits, K))
    assert rf == (n_fused, len(qs) * K - n_fused) and n_fused >= len(qs) * K // 2
    assert np.array_equal(res[0]["score"].view(U32), hits["score"].view(U32))   # the search's own score of the pair
    check_equal(res, hits, n_hits, batch_route(ctx, qs, ts, hits, n_hits, alpha, table3, mode, 33, 3))
    assert (np.abs(res[0]["score"]) > 300).any()
