"""-m gpu: every kernel's value-range limit, from both sides, with scoring systems beyond BLOSUM62 11/1.

Each fast kernel is chosen by a host predicate that proves the values of a build fit a narrow representation (tagged keys with
11 or 12 tag bits, uint16 score planes, 16-bit keys, the int32 row sweep with fp32 planes, packed 16-bit score-only lanes,
int32 score-only lanes).  The predicates are restated here as arithmetic (tests/range_cases.py lhs_*), a case just inside and a
case just outside each is built, and the planes, Optimal, the gapped strings, the near-optimal sets and the score-only path are
compared bit for bit with the oracle where a pair fits it and with the int64 numpy reference (pinned to the oracle by
tests/test_value_range_reference.py) on the long pairs.  No tolerance anywhere; every case keeps |value| < 2^24 (asserted by
the reference) so fp32 is exact.

The straddle cases (tag12a, tag12b and h16 under the hint tag_bits=12: pairs this short take 12 tag bits only when asked;
Q, T with sentinels; maxs = the table's largest |entry|; k = BLOSUM62 x k):
  tag11   k=9 (99), 302 x 302, ge 8: gi 200 -> 64927 < 65536 | gi 900 -> 65627 (int kernel)
  tag11e  +-1 table, 42 x 42, ge 1: gi 65300 -> 65469 | gi 65400 -> 65569 (int kernel); H reaches -65340 in global builds
  tag12a  k=9, 302 x 302, ge 8: gi + ge max = 13500 + 2416 = 15916 < 16000 | 13600 -> 16016 (int kernel); H reaches -15920
  tag12b  k=27 (297), 302 x 302, ge 8: 297*302 + 2 gi + 24*302 + 297 = 99839 (gi 1300) | 100039 (gi 1400)
  h16     k=9, local 11/1: 659 residues 99*661 = 65439 < 65536 | 660 residues 65538; best score 65241 (top bit set)
  key16a  k=8 (88), local 11/0: 369 residues 88*371 + 88 = 32736 < 32767 | 370 residues 32824; best score 32472
  key16b  k=1, 302 x 302, local, ge 8: gi + ge L + maxs = 5500 + 2416 + 11 = 7927 < 8000 | gi 5600 -> 8027
  int     k=888 (9768), 302 x 302, ge 4096: (9768+4096)*604 + gi + 9768 = 8387624 (gi 4000) < 2^23 | 8388624 (gi 5000) (exact kernel)
  inte    +-1 table, 2030 x 3, ge 4096, gi 59000: 8388202 | gi 59500 -> 8388702; H reaches -8357496 in global builds
  int gi / ge caps: gi 65536 | 65537, ge 4096 | 4097
  packed  (score-only, local) k=9, ge 0, gi 11: 300 residues 99*302 + 99 = 29997 < 30000 | 301 residues 30096; best 29700;
          k=1, 302, ge 8: gi 5500 -> 7927 < 8000 | 5600 -> 8027;  W/W = 2047 | 2048 (maxs < 2048)
  score32 (score-only) k=888, 302 x 302, ge 4096: 8387624 | 8388624 (full builds)
"""
import functools

import numpy as np
import pytest

import aln_amd
import gpu_util
import orc
import range_cases as rc

pytestmark = pytest.mark.gpu

ALPHA, BLOSUM = rc.load_blosum62()
TABLES = rc.table_families(ALPHA, BLOSUM)
PM1 = TABLES["identity5"] / 5                         # +1 on the diagonal, -1 elsewhere
W = "W"
WORST = rc.worst_partner(ALPHA, BLOSUM, W)
SHORT = (rc.random_seq(ALPHA, 901, 23), rc.random_seq(ALPHA, 902, 31))      # the second, short pair of every straddle batch


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def K(k):
    return rc.scaled(BLOSUM, k)


@functools.lru_cache(maxsize=64)
def _oracle(q, t, tkey, mode, gi, ge):
    table = _TABLE_BY_KEY[tkey]
    S = orc.sim_submatrix(q, t, ALPHA, table)
    err, D, PQ, PT = orc.dp_build(S, orc.Gap(mode, gi, ge))
    assert err == 0
    assert np.abs(D).max() < rc.EXACT_LIMIT
    rc2, sc, pl = orc.optimal(D, PQ, PT, mode == rc.LOCAL)
    return S, D, PQ, PT, rc2, sc, pl


_TABLE_BY_KEY = {}


def oracle(q, t, table, mode, gi, ge):
    key = table.tobytes()
    _TABLE_BY_KEY[key] = table
    return _oracle(q, t, key, mode, gi, ge)


_OPEN = []


@pytest.fixture(autouse=True)
def close_batches():
    """Every batch a test built is destroyed when the test ends, whether it passed or not (close() may be called twice)."""
    yield
    while _OPEN:
        _OPEN.pop().close()


def build(pairs, table, mode, gi, ge, algo=aln_amd.DP_AUTO, **hints):
    ctx = gpu_util.ctx()
    b = aln_amd.Batch(ctx, [p[0] for p in pairs], [p[1] for p in pairs])
    _OPEN.append(b)
    with ctx.hints(**hints):
        b.dp_submatrix(ALPHA, table, mode, gi, ge, aln_amd.FWD, algo)
    return b


def check_against_oracle(b, pairs, table, mode, gi, ge, what):
    """Planes and Optimal of every pair of the batch, bit for bit -> the planes read back"""
    scores, lists, status = b.optimal()
    planes = []
    for p, (q, t) in enumerate(pairs):
        S, D0, PQ0, PT0, rc2, sc, pl = oracle(q, t, table, mode, gi, ge)
        D, PQ, PT = b.get_cells(p)
        w = (what, b.kernel_name(), p)
        assert np.array_equal(u32(D), u32(D0)), w + ("H", int(np.count_nonzero(u32(D) != u32(D0))))
        assert np.array_equal(PQ, PQ0), w + ("PQ",)
        assert np.array_equal(PT, PT0), w + ("PT",)
        assert status[p] == rc2 and u32(scores[p]) == u32(sc) and np.array_equal(lists[p], pl), w + ("optimal",)
        planes.append((D, PQ, PT))
    return planes


def same_planes(b, planes, what):
    for p, (D0, PQ0, PT0) in enumerate(planes):
        D, PQ, PT = b.get_cells(p)
        assert np.array_equal(u32(D), u32(D0)) and np.array_equal(PQ, PQ0) and np.array_equal(PT, PT0), (what, b.kernel_name(), p)


def within_1pc(lhs, limit):
    return 0.99 * limit <= lhs < limit


# ---- (a) straddle every predicate -------------------------------------------------------------------------------------------

def run300(n=300):
    return [(W * n, W * n), (W * n, WORST * n), SHORT]


def is_tag11(name):
    return ("dp_affine_tag_kernel" in name or "dp_affine_solo_kernel" in name) and "tag12" not in name


ALL = rc.ALIGN_TYPES
NONLOCAL = (rc.GLOBAL_LOCAL, rc.GLOBAL, rc.LOCAL_GLOBAL, rc.SEMI_LOCAL)

# name -> (table, pairs inside, gaps inside, pairs outside, gaps outside, modes, left side (ms, gi, ge, Q, T) -> [(lhs, limit)],
#          narrow-kernel test on the name, hints that switch the narrow form off, exercised(planes of the inside case, mode))
STRADDLE = {}


def straddle(name, table, pin, gin, pout, gout, modes, lhs, narrow, off, exercised=None, on=None):
    """on: hints of both cases (sequences of at most 2046 residues take 12 tag bits only under the hint tag_bits=12)"""
    STRADDLE[name] = dict(on=on or {}, table=table, pin=pin, gin=gin, pout=pout, gout=gout, modes=modes, lhs=lhs, narrow=narrow, off=off,
                          exercised=exercised)


def _most_negative(limit, modes, gap_only=False):
    """gap_only: the bound is on the gap constant gi + ge * length alone (a cell may lie lower by its similarities): the cell
    reached from (0,0) by the longest charged end gap, minus its own similarity, is within 1 % of it"""
    def f(planes, mode):
        if mode in modes:
            lo = min(float(D.min()) for D, _, _ in planes)
            if gap_only:
                D = planes[1][0]
                lo = max(float(D[1, -2]), float(D[-2, 1])) if mode == rc.GLOBAL else float(D[1, -2]) if mode == rc.GLOBAL_LOCAL else float(D[-2, 1])
            assert within_1pc(-lo, limit), (lo, limit)
    return f


def _best_local(limit):
    def f(planes, mode):
        hi = max(float(D.max()) for D, _, _ in planes)
        assert within_1pc(hi, limit), (hi, limit)
    return f


def _top_bit(planes, mode):
    assert max(float(D.max()) for D, _, _ in planes) >= 32768


def _largest_is(value):
    def f(planes, mode):
        assert max(float(D.max()) for D, _, _ in planes) == value
    return f


straddle("tag11", K(9), run300(), (200, 8), run300(), (900, 8), ALL,
         lambda ms, gi, ge, Q, T: [(rc.lhs_tag11(ms, gi, ge, Q, T), 65536)], is_tag11, dict(tag_bits=12), _largest_is(99.0 * 300))
straddle("tag11e", PM1, [(W * 40, W * 40), (W * 40, WORST * 40), SHORT], (65300, 1), [(W * 40, W * 40), (W * 40, WORST * 40), SHORT],
         (65400, 1), ALL, lambda ms, gi, ge, Q, T: [(rc.lhs_tag11(ms, gi, ge, Q, T), 65536)], is_tag11, dict(tag_kernel=0),
         _most_negative(65536, (rc.GLOBAL, rc.GLOBAL_LOCAL, rc.LOCAL_GLOBAL)))
straddle("tag12a", K(9), run300(), (13500, 8), run300(), (13600, 8), ALL,
         lambda ms, gi, ge, Q, T: [(rc.lhs_tag12(ms, gi, ge, Q, T)[1], 16000)], lambda n: "tag12" in n, dict(tag_kernel=0),
         _most_negative(16000, (rc.GLOBAL, rc.GLOBAL_LOCAL, rc.LOCAL_GLOBAL), gap_only=True), on=dict(tag_bits=12))
straddle("tag12b", K(27), run300(), (1300, 8), run300(), (1400, 8), ALL,
         lambda ms, gi, ge, Q, T: [(rc.lhs_tag12(ms, gi, ge, Q, T)[0], 100000)], lambda n: "tag12" in n, dict(tag_kernel=0),
         _largest_is(297.0 * 300), on=dict(tag_bits=12))
straddle("h16", K(9), [(W * 659, W * 659), SHORT], (11, 1), [(W * 660, W * 660), SHORT], (11, 1), (rc.LOCAL,),
         lambda ms, gi, ge, Q, T: [(rc.lhs_h16(ms, Q, T), 65536)], lambda n: "h16" in n, dict(h16=0), _top_bit, on=dict(tag_bits=12))
straddle("key16a", K(8), [(W * 369, W * 369), SHORT], (11, 0), [(W * 370, W * 370), SHORT], (11, 0), (rc.LOCAL,),
         lambda ms, gi, ge, Q, T: [(rc.lhs_key16(ms, gi, ge, Q, T)[0], 32767)], lambda n: "key16" in n, dict(key16=0), _best_local(32767))
straddle("key16b", K(1), run300(), (5500, 8), run300(), (5600, 8), (rc.LOCAL,),
         lambda ms, gi, ge, Q, T: [(rc.lhs_key16(ms, gi, ge, Q, T)[1], 8000)], lambda n: "key16" in n, dict(key16=0), _largest_is(11.0 * 300))
straddle("int", K(888), run300(), (4000, 4096), run300(), (5000, 4096), ALL,
         lambda ms, gi, ge, Q, T: [(rc.lhs_int(ms, gi, ge, Q, T), 1 << 23)], lambda n: "dp_affine_int_kernel" in n, dict(),
         _largest_is(9768.0 * 300))
_NARROW = [(W * 2028, W), (W * 2028, WORST), (SHORT[0], W)]
straddle("inte", PM1, _NARROW, (59000, 4096), _NARROW, (59500, 4096), ALL,
         lambda ms, gi, ge, Q, T: [(rc.lhs_int(ms, gi, ge, Q, T), 1 << 23)], lambda n: "dp_affine_int_kernel" in n, dict(),
         _most_negative(1 << 23, (rc.GLOBAL, rc.LOCAL_GLOBAL)))
_SMALL = [(W * 40, W * 40), (W * 40, WORST * 40), SHORT]
straddle("int_gi_cap", K(1), _SMALL, (65536, 1), _SMALL, (65537, 1), ALL,
         lambda ms, gi, ge, Q, T: [(gi, 65537)], lambda n: "dp_affine_int_kernel" in n, dict(), None)
straddle("int_ge_cap", K(1), _SMALL, (11, 4096), _SMALL, (11, 4097), ALL,
         lambda ms, gi, ge, Q, T: [(ge, 4097)], lambda n: "dp_affine_int_kernel" in n, dict(), None)


def _sides(c):
    ms = rc.maxs(c["table"])
    out = []
    for pairs, (gi, ge) in ((c["pin"], c["gin"]), (c["pout"], c["gout"])):
        Q = max(len(q) for q, _ in pairs) + 2
        T = max(len(t) for _, t in pairs) + 2
        out.append(c["lhs"](ms, gi, ge, Q, T))
    return out


@pytest.mark.parametrize("name", sorted(STRADDLE))
def test_straddle_construction(name):
    """The restated inequality puts the two cases on opposite sides, the inside one within 1 % of the limit."""
    inside, outside = _sides(STRADDLE[name])
    for lhs, limit in inside:
        assert within_1pc(lhs, limit), (name, lhs, limit)
    for lhs, limit in outside:
        assert lhs >= limit, (name, lhs, limit)


@pytest.mark.parametrize("name", sorted(STRADDLE))
def test_straddle(name):
    """Inside: the narrow kernel ran (its name says so), planes and Optimal equal the oracle's, the representation was really
    exercised, and the same batch with the narrow form switched off gives the same planes.  Outside: the narrow kernel did not
    run, planes and Optimal equal the oracle's."""
    c = STRADDLE[name]
    for mode in c["modes"]:
        gi, ge = c["gin"]
        algo = aln_amd.DP_FAST if c["narrow"]("dp_affine_int_kernel") else aln_amd.DP_AUTO
        hint = dict(tag_kernel=0) if algo == aln_amd.DP_FAST else c["on"]
        b = build(c["pin"], c["table"], mode, gi, ge, algo, **hint)
        print("%s mode %d inside  %s: %s" % (name, mode, _sides(c)[0], b.kernel_name()))
        assert c["narrow"](b.kernel_name()), (name, mode, "inside", b.kernel_name())
        planes = check_against_oracle(b, c["pin"], c["table"], mode, gi, ge, (name, mode, "inside"))
        if c["exercised"]:
            c["exercised"](planes[:-1], mode)
        b.close()
        for off in ([c["off"]] if c["off"] else []) + [None]:
            b = build(c["pin"], c["table"], mode, gi, ge, aln_amd.DP_AUTO if off else aln_amd.DP_EXACT, **dict(c["on"], **(off or {})))
            assert not c["narrow"](b.kernel_name()), (name, mode, off, b.kernel_name())
            same_planes(b, planes, (name, mode, off))
            b.close()
        gi, ge = c["gout"]
        if algo == aln_amd.DP_FAST:
            b = build(c["pout"], c["table"], mode, gi, ge, aln_amd.DP_AUTO)
            with pytest.raises(aln_amd.AlnError) as ei:
                build(c["pout"], c["table"], mode, gi, ge, aln_amd.DP_FAST)
            assert ei.value.code == aln_amd.E_NOT_INTEGRAL
        else:
            b = build(c["pout"], c["table"], mode, gi, ge, **c["on"])
        print("%s mode %d outside %s: %s" % (name, mode, _sides(c)[1], b.kernel_name()))
        assert not c["narrow"](b.kernel_name()), (name, mode, "outside", b.kernel_name())
        check_against_oracle(b, c["pout"], c["table"], mode, gi, ge, (name, mode, "outside"))
        b.close()


# ---- (b) degenerate scoring systems, all kernels ----------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ALL)
@pytest.mark.parametrize("family", sorted(TABLES))
def test_degenerate_scoring_systems(family, mode):
    """Every table family x gaps (0,0), (0,1), (40,0), (1,5) on 16 ragged pairs (empty, one residue, run against run, run against
    its worst partner, identical, random): planes and Optimal of DP_AUTO, of the int kernel and of DP_EXACT equal the oracle's.
    With zero gaps and a constant table every predecessor ties: match, then deletions k ascending, then insertions k ascending,
    the first arg-max wins."""
    table = TABLES[family]
    pairs = rc.ragged_batch(ALPHA, table, 500 + mode, maxlen=120)
    assert len(pairs) == 16
    for (gi, ge) in ((0, 0), (0, 1), (40, 0), (1, 5)):
        seen = set()
        for algo, hints in ((aln_amd.DP_AUTO, {}), (aln_amd.DP_FAST, dict(tag_kernel=0)), (aln_amd.DP_EXACT, {})):
            b = build(pairs, table, mode, gi, ge, algo, **hints)
            seen.add(b.kernel_name().split("<")[0])
            check_against_oracle(b, pairs, table, mode, gi, ge, (family, mode, gi, ge, algo))
            b.close()
        assert any("dp_affine_int" in s for s in seen) and any("dp_exact" in s for s in seen), seen
        ms, L = rc.maxs(table), 122
        a12, b12 = rc.lhs_tag12(ms, gi, ge, L, L)
        if rc.lhs_tag11(ms, gi, ge, L, L) < 65536 or (a12 < 100000 and b12 < 16000):
            assert any("tag" in s or "solo" in s for s in seen), seen


@pytest.mark.parametrize("mode", ALL)
def test_negative_zero_similarities(mode):
    """A -0.0 similarity (a table multiplied by a negative factor, a plane the caller computed): the reference never produces a
    -0.0 score from it, because every score starts from +0.0.  Table path (the x-1 family above) and caller-supplied planes, in
    the int kernel and the exact-order kernels, bit for bit; gaps 0/0 and 0/1 make the free and the zero-cost end gaps."""
    rng = np.random.RandomState(40 + mode)
    dims = [(42, 4), (4, 42), (30, 30), (2, 9), (9, 2), (3, 3), (70, 140)]
    planes = []
    for Q, T in dims:
        S = rng.randint(-2, 3, (Q, T)).astype(np.float32)
        S[S == 0] = -0.0
        S[0, :] = S[-1, :] = 0
        S[:, 0] = S[:, -1] = 0
        planes.append(S)
    assert any(np.signbit(S[1:-1, 1:-1]).any() and (S[1:-1, 1:-1] == 0).any() for S in planes)
    ctx = gpu_util.ctx()
    for (gi, ge) in ((0, 0), (0, 1), (3, 1)):
        for algo in (aln_amd.DP_AUTO, aln_amd.DP_EXACT):
            b = aln_amd.Batch(ctx, ["A" * (Q - 2) for Q, _ in dims], ["A" * (T - 2) for _, T in dims])
            _OPEN.append(b)
            b.dp_simmatrix(planes, mode, gi, ge, aln_amd.FWD, algo)
            assert ("dp_exact" in b.kernel_name()) == (algo == aln_amd.DP_EXACT), b.kernel_name()
            for p, S in enumerate(planes):
                err, D0, PQ0, PT0 = orc.dp_build(S, orc.Gap(mode, gi, ge))
                assert err == 0
                D, PQ, PT = b.get_cells(p)
                w = (mode, gi, ge, b.kernel_name(), p)
                assert np.array_equal(u32(D), u32(D0)), w + (int(np.count_nonzero(u32(D) != u32(D0))),)
                assert np.array_equal(PQ, PQ0) and np.array_equal(PT, PT0), w
            b.close()


# ---- (c) largest values at the kernels' largest sizes ----------------------------------------------------------------------------

def check_against_reference(b, pairs, table, mode, gi, ge, what):
    """H (every cell) and the score Optimal reports against the int64 reference; pointers by consistency -> planes"""
    scores, _, status = b.optimal(want_pairs=False)
    planes = []
    for p, (q, t) in enumerate(pairs):
        S = rc.sim_int(q, t, ALPHA, table)
        H, corner, lmax = rc.affine_reference(S, mode, gi, ge)
        D, PQ, PT = b.get_cells(p)
        w = (what, b.kernel_name(), p)
        assert np.array_equal(D, H.astype(np.float32)), w + ("H", int(np.count_nonzero(D != H.astype(np.float32))))
        assert not np.signbit(D).any() or mode != rc.LOCAL, w
        assert float(scores[p]) == rc.reference_score(H, mode), w + ("score", float(scores[p]))
        assert rc.pointers_consistent(D, PQ, PT, S, mode, gi, ge) == 0, w + ("pointers",)
        planes.append((D, PQ, PT))
    return planes


# (residues, table scale k, gi, ge, kernel name test): the scale and the gaps by the same arithmetic as the straddle cases
#   2046: (11 + 4) * 4096 + 3500 + 11 = 64951 < 65536 (11 tag bits);   2047: 12 tag bits
#   4094: 22 * 4096 + 2 * 4900 + 22 = 99934 < 100000 (12 tag bits);    4095: the int kernel
G_L = (rc.GLOBAL, rc.LOCAL)
LONG = [
    (2046, 1, 3500, 4, is_tag11, ALL),
    (2047, 1, 3500, 4, lambda n: "tag12" in n, ALL),
    (4094, 2, 4900, 0, lambda n: "tag12" in n, (rc.GLOBAL, rc.LOCAL, rc.SEMI_LOCAL)),
    (4095, 2, 4900, 0, lambda n: "dp_affine_int_kernel" in n, G_L),
]


@pytest.mark.parametrize("n,k,gi,ge,kernel,modes", LONG, ids=[str(c[0]) for c in LONG])
def test_largest_values_at_the_largest_sizes(n, k, gi, ge, kernel, modes):
    """A run against itself (largest positive values), against its worst partner (most negative global values), two identical
    random sequences and a random pair (non-uniform similarities: the ties and pointers of real data) at the tagged kernels'
    limits and one residue beyond: H and the score against the int64 reference, pointers by consistency, and up to 4094 residues
    all three planes bit-equal to the DP_EXACT build of the same batch."""
    table = K(k)
    ms = rc.maxs(table)
    if n == 2046:
        assert within_1pc(rc.lhs_tag11(ms, gi, ge, n + 2, n + 2), 65536)
    if n == 4094:
        assert within_1pc(rc.lhs_tag12(ms, gi, ge, n + 2, n + 2)[0], 100000)
    ident = rc.random_seq(ALPHA, 3000 + n, n)
    pairs = [(W * n, W * n), (W * n, WORST * n), (ident, ident), (rc.random_seq(ALPHA, 3001 + n, n), rc.random_seq(ALPHA, 3002 + n, n))]
    for mode in modes:
        b = build(pairs, table, mode, gi, ge)
        assert kernel(b.kernel_name()), b.kernel_name()
        planes = check_against_reference(b, pairs, table, mode, gi, ge, (n, mode))
        b.close()
        if n <= 4094:
            b = build(pairs, table, mode, gi, ge, aln_amd.DP_EXACT)
            assert "dp_exact" in b.kernel_name()
            same_planes(b, planes, (n, mode, "exact"))
            b.close()
        del planes


def test_largest_values_at_the_int_kernel_limit():
    """8190 residues (a row of 8192 with the sentinels): BLOSUM62 x 46 (506), ge 5, gi 15000:
    (506 + 5) * 16384 + 15000 + 506 = 8387730 < 2^23.  Score and consistency only."""
    n, table, gi, ge = 8190, K(46), 15000, 5
    assert within_1pc(rc.lhs_int(rc.maxs(table), gi, ge, n + 2, n + 2), 1 << 23)
    for mode, pair in ((rc.LOCAL, (W * n, W * n)), (rc.GLOBAL, (W * n, WORST * n))):
        b = build([pair], table, mode, gi, ge)
        assert "dp_affine_int_kernel" in b.kernel_name(), b.kernel_name()
        check_against_reference(b, [pair], table, mode, gi, ge, (n, mode))
        b.close()


def test_one_residue_beyond_the_int_kernel_limit():
    """8191 residues along the template (a row of 8193): no row-sweep kernel holds it, DP_AUTO builds it in the literal exact-order
    kernel, whose deletion scan is O(columns) per cell in ONE workgroup per pair.  A square 8191 x 8191 pair is therefore not in
    the suite: measured on the MI355X, its build had not finished after 420 s (the run was ended by its time limit), against
    22 ms for 4200 x 4200 in the int kernel.  What runs instead: the template at 8191 against 126 residues (a run pair and a
    random pair, same table and gaps as the 8190 case), H and score against the int64 reference and pointers by consistency,
    and the narrow 8191 pairs of test_long_narrow_pairs_equal_the_oracle through the oracle."""
    n, table, gi, ge = 8191, K(46), 15000, 5
    pairs = [(W * 126, W * n), (rc.random_seq(ALPHA, 8191, 126), rc.random_seq(ALPHA, 8192, n))]
    for mode in G_L:
        b = build(pairs, table, mode, gi, ge)
        assert "dp_exact" in b.kernel_name(), b.kernel_name()
        check_against_reference(b, pairs, table, mode, gi, ge, (n, mode))
        b.close()
    with pytest.raises(aln_amd.AlnError) as ei:
        build(pairs, table, rc.LOCAL, gi, ge, aln_amd.DP_FAST)
    assert ei.value.code == aln_amd.E_TOO_LONG


# (residues, gi, ge, kernel of the batch with the long queries, kernel of the batch with the long templates), BLOSUM62, L = n + 2;
# the short side has at most 4 residues (6 with the sentinels)
#   2046: (11 + 8) * (2048 + 6) + 26000 + 11 = 65037 < 65536 (11 tag bits)
#   2047: gi + ge L = 9700 + 3 * 2049 = 15847 < 16000, 11 * 6 + 2 * 9700 + 9 * 2049 + 11 = 37918 < 100000 (12 tag bits)
#   4094: 3600 + 3 * 4096 = 15888 < 16000, 11 * 6 + 7200 + 9 * 4096 + 11 = 44141 < 100000 (12 tag bits)
#   4095, 8190: the int kernel; 8191 along the template: the exact-order kernel, along the query the int kernel (its row is short)
NARROW_LONG = [
    (2046, 26000, 8, is_tag11, is_tag11),
    (2047, 9700, 3, lambda n: "tag12" in n, lambda n: "tag12" in n),
    (4094, 3600, 3, lambda n: "tag12" in n, lambda n: "tag12" in n),
    (4095, 3600, 3, lambda n: "dp_affine_int" in n, lambda n: "dp_affine_int" in n),
    (8190, 3600, 3, lambda n: "dp_affine_int" in n, lambda n: "dp_affine_int" in n),
    (8191, 3600, 3, lambda n: "dp_affine_int" in n, lambda n: "dp_exact" in n),
]


@pytest.mark.parametrize("n,gi,ge,kq,kt", NARROW_LONG, ids=[str(c[0]) for c in NARROW_LONG])
def test_long_narrow_pairs_equal_the_oracle(n, gi, ge, kq, kt):
    """A long run against 1 to 4 residues, all five align types: the largest end-gap terms gi + ge * length, through the oracle
    bit for bit.  One batch per orientation, so that the batch's smaller dimension is 6 and the tagged kernels are chosen where
    their predicates allow (the name is asserted)."""
    table = BLOSUM
    ms = rc.maxs(table)
    if n == 2046:
        assert within_1pc(rc.lhs_tag11(ms, gi, ge, n + 2, 6), 65536)
    if n in (2047, 4094):
        a12, b12 = rc.lhs_tag12(ms, gi, ge, n + 2, 6)
        assert a12 < 100000 and within_1pc(b12, 16000)
    partner = W + WORST + rc.random_seq(ALPHA, n, 2)
    long_q = [(W * n, W), (W * n, partner), (WORST * n, partner[:2])]
    long_t = [(W, W * n), (partner, W * n), (partner[:2], WORST * n)]
    for pairs, kernel in ((long_q, kq), (long_t, kt)):
        for mode in ALL:
            b = build(pairs, table, mode, gi, ge)
            assert kernel(b.kernel_name()), (n, mode, b.kernel_name())
            check_against_oracle(b, pairs, table, mode, gi, ge, (n, mode))
            b.close()


# ---- (d) the score-only path -------------------------------------------------------------------------------------------

def score_sets(n, m):
    r = rc.random_seq(ALPHA, 77, max(min(n, m), 1))
    qs = [W * n, WORST * n, r, rc.random_seq(ALPHA, 78, n), "", W]
    ts = [W * m, WORST * m, r, rc.random_seq(ALPHA, 79, m), "", W + WORST]
    return qs, ts


# name -> (table, n, m, gi, ge, the restated left sides (ms, gi, ge, Q, T) -> [(lhs, limit)], inside?)
SCORE_CASES = {
    "packed_best_in": (K(9), 300, 300, 11, 0, lambda *a: [(rc.lhs_packed(*a)[0], 30000)], True),
    "packed_best_out": (K(9), 301, 301, 11, 0, lambda *a: [(rc.lhs_packed(*a)[0], 30000)], False),
    "packed_gap_in": (K(1), 300, 300, 5500, 8, lambda *a: [(rc.lhs_packed(*a)[1], 8000)], True),
    "packed_gap_out": (K(1), 300, 300, 5600, 8, lambda *a: [(rc.lhs_packed(*a)[1], 8000)], False),
    "packed_maxs_in": (TABLES["outlier_WW_2047"], 11, 300, 11, 0, lambda *a: [(rc.lhs_packed(*a)[2], 2048)], True),
    "packed_maxs_out": (TABLES["outlier_WW_2048"], 11, 300, 11, 0, lambda *a: [(rc.lhs_packed(*a)[2], 2048)], False),
    "score32_in": (K(888), 300, 300, 4000, 4096, lambda *a: [(rc.lhs_score32(*a), 1 << 23)], True),
    "score32_out": (K(888), 300, 300, 5000, 4096, lambda *a: [(rc.lhs_score32(*a), 1 << 23)], False),
    "runs_2046": (K(1), 2046, 2046, 11, 1, None, None),
    "zero_gaps_constant": (TABLES["constant+3"], 130, 257, 0, 0, None, None),
    "all_negative": (TABLES["all_negative"], 130, 257, 0, 1, None, None),
}


@pytest.mark.parametrize("name", sorted(SCORE_CASES))
def test_score_only_path(name):
    """aln_score_all_vs_all on sets of runs, worst partners, identical and random sequences, an empty and a short one: every
    score of all five align types equals the int64 reference, with the packed kernel allowed and forbidden, and a row-block
    call equals the same rows of the full call.  Which kernel ran cannot be observed here: the inputs lie on both sides of the
    restated inequalities, and every other condition of the packed kernel holds on both sides."""
    table, n, m, gi, ge, lhs, inside = SCORE_CASES[name]
    qs, ts = score_sets(n, m)
    ms = rc.maxs(table)
    Q, T = max(map(len, qs)) + 2, max(map(len, ts)) + 2
    if lhs is not None:
        for v, limit in lhs(ms, gi, ge, Q, T):
            assert within_1pc(v, limit) if inside else v >= limit, (name, v, limit)
        if name.startswith("packed"):
            a, b2, c3 = rc.lhs_packed(ms, gi, ge, Q, T)
            assert sum([a >= 30000, b2 >= 8000, c3 >= 2048]) == (0 if inside else 1), (a, b2, c3)
            assert rc.lhs_score32(ms, gi, ge, Q, T) < 1 << 23
    ctx = gpu_util.ctx()
    S = [[rc.sim_int(q, t, ALPHA, table) for t in ts] for q in qs]
    for mode in ALL:
        want = np.array([[rc.reference_score(rc.affine_reference(S[i][j], mode, gi, ge)[0], mode) for j in range(len(ts))]
                         for i in range(len(qs))], np.float32)
        if name == "packed_best_in" and mode == rc.LOCAL:            # the 16-bit lanes really hold a score within 1 % of the limit
            assert within_1pc(float(want.max()), 30000), want.max()
        for packed in (1, 0):
            with ctx.hints(score_packed=packed):
                got = aln_amd.score_all_vs_all(ctx, qs, ts, ALPHA, table, gi, ge, align_type=mode)
                blk = aln_amd.score_all_vs_all(ctx, qs, ts, ALPHA, table, gi, ge, 1, 4, align_type=mode)
            assert np.array_equal(u32(got), u32(want)), (name, mode, packed, got.tolist(), want.tolist())
            assert np.array_equal(u32(blk), u32(want[1:4])), (name, mode, packed)


# ---- (e) downstream of a score plane with the top bit set ---------------------------------------------------------------------

def check_strings(b, pairs, what):
    sc0, lists, st0 = b.optimal()
    scores, ident, status, tl, ql = b.optimal_strings()
    for k, (q, t) in enumerate(pairs):
        assert status[k] == st0[k] == 0 and u32(scores[k]) == u32(sc0[k]), (what, k)
        assert u32(ident[k]) == u32(gpu_util.identity_for(q, t, lists[k])), (what, k)
        want_t, want_q, _ = gpu_util.strings_for(q, t, [lists[k]])
        assert tl[k] == want_t and ql[k] == want_q[0], (what, k)
    return sc0


def test_downstream_of_a_high_bit_plane_h16_case():
    """The h16 inside case (best local score 65241 in a uint16 plane): device gapped strings equal the host renderer, and the
    constrained near-optimal set equals the oracle's."""
    c = STRADDLE["h16"]
    pairs, table, (gi, ge) = c["pin"], c["table"], c["gin"]
    b = build(pairs, table, rc.LOCAL, gi, ge, **c["on"])
    assert "h16" in b.kernel_name()
    sc = check_strings(b, pairs, "h16")
    assert sc[0] == 65241.0
    for p, (q, t) in enumerate(pairs):
        S, D0, PQ0, PT0, rc2, sc0, pl = oracle(q, t, table, rc.LOCAL, gi, ge)
        gap = orc.Gap(rc.LOCAL, gi, ge)
        flags = orc.make_subopt_regions(len(t) + 2, 4)
        for nsub, delta in ((5, 0.0005), (12, 0.002)):
            s = orc.AliSet()
            s.push(pl, sc0)
            orc.enumerate_noa("cw", D0, PQ0, PT0, S, gap, flags, nsub, delta, s)
            s.identity(q, t)
            assert len(s) < 400
            got = b.enumerate(p, "cw", nsub, delta, flags, max_alignments=max(nsub, len(s)) + 2)
            assert len(got) == len(s), (p, nsub, delta, len(got), len(s))
            for k, g in enumerate(got):
                r = s.get(k)
                assert u32(g["score"]) == u32(r["score"]) and g["uid"] == r["uid"], (p, k)
                assert np.array_equal(g["pairs"], r["pairs"]) and u32(g["identity"]) == u32(r["identity"]), (p, k)
    b.close()


def test_downstream_of_a_high_bit_plane_4094_run():
    """A run of 4094 W against itself, BLOSUM62 11/1, local: 45056 in a uint16 plane (h16 legal, key16 not).  Score against the
    int64 reference, the device strings against the host renderer."""
    n = 4094
    pairs = [(W * n, W * n), SHORT]
    b = build(pairs, BLOSUM, rc.LOCAL, 11, 1)
    assert "h16" in b.kernel_name() and "key16" not in b.kernel_name() and "tag12" in b.kernel_name(), b.kernel_name()
    planes = check_against_reference(b, pairs, BLOSUM, rc.LOCAL, 11, 1, "4094 h16")
    assert planes[0][0].max() == 11.0 * n >= 32768
    sc = check_strings(b, pairs, "4094 h16")
    assert sc[0] == 11.0 * n
    b.close()
