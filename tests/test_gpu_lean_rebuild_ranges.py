"""-m gpu: lean rebuilds (dp_affine_tag_kernel<..., lean>, 2 B/cell) after gap changes, on long queries, at the value limits of
the 16-bit key layout and under the hints that reach or forbid the lean kernel.

A lean build writes flagged pointer words and, of the score plane, row Q-2 and the chunk of column T-2 only; every other score
cell is what the previous build left.  tests/test_gpu_lean_reevaluate.py rebuilds with the gaps of the build before, so those
stale cells hold the right answer there.  Here every rebuild follows a set_gap that changes the sign of thousands of the cells
a lean build leaves alone (tests/test_lean_path_checker.py proves that on the reference side), so a reader of stale scores
reports another alignment.

Every result is compared with the oracle for pairs of at most 300 x 700 residues, with the int64 reference of
tests/range_cases.py and the walk of tests/lean_cases.py for larger ones, and always with a fresh batch built by aln_batch_dp
(never lean) under the same gaps: scores bit for bit, lists and strings exactly.  Every test that means to run lean asserts the
kernel's name and 2 bytes per cell before it looks at a result."""
import functools

import numpy as np
import pytest

import aln_amd
import gpu_util
import lean_cases as lc
import orc
import range_cases as rc
from aln_amd.synth import homolog_pair

pytestmark = pytest.mark.gpu

LOCAL = aln_amd.LOCAL
ALPHA, BLOSUM = rc.load_blosum62()
TABLES = rc.table_families(ALPHA, BLOSUM)
DEGENERATE = sorted(n for n in TABLES if not n.startswith("outlier"))
W = "W"
WORST = rc.worst_partner(ALPHA, BLOSUM, W)
SHORT = (rc.random_seq(ALPHA, 901, 23), rc.random_seq(ALPHA, 902, 31))
_TABLE_BY_KEY = {}
_OPEN = []


@pytest.fixture(autouse=True)
def close_batches():
    yield
    while _OPEN:
        _OPEN.pop().close()


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def tkey(table):
    key = np.ascontiguousarray(table, np.float32).tobytes()
    _TABLE_BY_KEY[key] = table
    return key


@functools.lru_cache(maxsize=None)
def shape_pairs():
    return lc.shape_pairs(ALPHA)


@functools.lru_cache(maxsize=None)
def long_pairs():
    return lc.long_pairs(ALPHA, homolog_pair)


@functools.lru_cache(maxsize=256)
def _oracle(q, t, key, gi, ge):
    S = orc.sim_submatrix(q, t, ALPHA, _TABLE_BY_KEY[key])
    err, D, PQ, PT = orc.dp_build(S, orc.Gap(orc.LOCAL, gi, ge))
    assert err == 0
    err, sc, pl = orc.optimal(D, PQ, PT, True)
    assert err == 0
    return D, PQ, PT, sc, pl


@functools.lru_cache(maxsize=4)
def _sim(q, t, key):
    return rc.sim_int(q, t, ALPHA, _TABLE_BY_KEY[key])


@functools.lru_cache(maxsize=8)
def _reference(q, t, key, gi, ge):
    """-> S, H, corner, Optimal's list (int64 reference; one 2046 x 2046 plane takes 0.3 s, so it is kept per pair and gaps)"""
    S = _sim(q, t, key)
    H, corner, _ = rc.affine_reference(S, rc.LOCAL, gi, ge)
    return S, H, corner, lc.reference_list(H, gi, ge)


assert_lean, assert_full, same_optimal = lc.assert_lean, lc.assert_full, lc.same_optimal


def hints(variant=True, **extra):
    """The hints of a test: the lean instantiation's shape (2 waves x 2 groups x 8 columns), which pairs of at most 1024 columns
    take only when asked, plus the test's own"""
    return gpu_util.ctx().hints(**dict(lc.VARIANT if variant else {}, **extra))


def new_batch(pairs, table, gi, ge):
    b = aln_amd.Batch(gpu_util.ctx(), [p[0] for p in pairs], [p[1] for p in pairs])
    _OPEN.append(b)
    b.dp_submatrix(ALPHA, table, LOCAL, gi, ge)
    return b


def fresh_results(pairs, table, gi, ge):
    """Optimal and the strings of a batch built by aln_batch_dp under these gaps and the caller's hints: never lean"""
    with gpu_util.ctx().hints(lean_reevaluate=0):
        b = new_batch(pairs, table, gi, ge)
        assert_full(b, b.plane_bytes_per_cell())
        res = b.optimal(), b.optimal_strings()
        b.close()
    return res


def same_strings(got, want):
    assert np.array_equal(u32(got[0]), u32(want[0])) and np.array_equal(u32(got[1]), u32(want[1]))
    assert np.array_equal(got[2], want[2])
    assert got[3] == want[3] and got[4] == want[4]


def check_optimal(res, pairs, table, gi, ge, what=None):
    """Optimal of every pair against the oracle (short pairs) or the int64 reference and the checker (long pairs)"""
    scores, lists, status = res
    key = tkey(table)
    for p, (q, t) in enumerate(pairs):
        w = (what, p, len(q), len(t), gi, ge)
        assert status[p] == 0, w
        if lc.fits_oracle(q, t):
            D, PQ, PT, sc, pl = _oracle(q, t, key, gi, ge)
            assert u32(scores[p]) == u32(sc), w + (float(scores[p]), float(sc))
            assert np.array_equal(lists[p], pl), w
        else:
            S, H, corner, pl = _reference(q, t, key, gi, ge)
            assert float(scores[p]) == float(H[lc.find_max_cell(H)]), w + (float(scores[p]),)
            assert not np.signbit(scores[p]), w
            lc.check_local_list(S, H, lists[p], gi, ge)
            assert np.array_equal(lists[p], pl), w


def check_cells(b, p, q, t, table, gi, ge):
    key = tkey(table)
    D, PQ, PT = b.get_cells(p)
    if lc.fits_oracle(q, t):
        D0, PQ0, PT0, sc, pl = _oracle(q, t, key, gi, ge)
        assert np.array_equal(u32(D), u32(D0)), (p, int(np.count_nonzero(u32(D) != u32(D0))))
        assert np.array_equal(PQ, PQ0) and np.array_equal(PT, PT0), p
    else:
        S, H, corner, pl = _reference(q, t, key, gi, ge)
        assert np.array_equal(u32(D), u32(H.astype(np.float32))), (p, int(np.count_nonzero(D != H.astype(np.float32))))
        assert rc.pointers_consistent(D, PQ, PT, S, rc.LOCAL, gi, ge) == 0, p


def check_all(b, pairs, table, gi, ge, what=None, strings=True):
    """Optimal (and the strings) of the resident build against the references and against a fresh full build"""
    fresh_opt, fresh_str = fresh_results(pairs, table, gi, ge)
    res = b.optimal()
    check_optimal(res, pairs, table, gi, ge, what)
    same_optimal(res, fresh_opt)
    if strings:
        same_strings(b.optimal_strings(), fresh_str)
    return res


# ---- (a) + (b): rounds with changing gaps, short shapes and long queries ---------------------------------------------------------

def round_batches():
    lp = long_pairs()
    return [("shapes", shape_pairs(), None)] + [("+".join(names), [lp[n] for n in names], "1030x1030" if "1030x1030" in names else None)
                                               for names in lc.LONG_BATCHES]


@pytest.mark.parametrize("k", range(4), ids=[b[0] for b in round_batches()])
def test_rounds_with_changing_gaps(k):
    """dp(11/1), optimal; then set_gap, reevaluate (lean), optimal, optimal_strings for 3/0, 40/3 and 11/1 again.  Where the batch
    holds pairs the oracle reaches, get_cells in the middle (after 3/0): the next rebuild is full, the one after it lean again.
    After the last round get_cells gives the planes of the last setting and the batch is full."""
    name, pairs, cells_of = round_batches()[k]
    short = [p for p, (q, t) in enumerate(pairs) if lc.fits_oracle(q, t)]
    with hints():
        gi, ge = lc.ROUNDS[0]
        b = new_batch(pairs, BLOSUM, gi, ge)
        assert_full(b)
        full_name = b.kernel_name()
        assert "key16" in full_name and "h16" in full_name, full_name
        check_all(b, pairs, BLOSUM, gi, ge, (name, 0), strings=False)
        full_next = False
        for r, (gi, ge) in enumerate(lc.ROUNDS[1:], 1):
            b.set_gap(LOCAL, gi, ge)
            b.reevaluate()
            if full_next:
                assert_full(b)
                assert b.kernel_name() == full_name
            else:
                assert_lean(b)
                assert b.kernel_name().replace(",lean", "") == full_name
            check_all(b, pairs, BLOSUM, gi, ge, (name, r))
            assert ("lean" in b.kernel_name()) == (not full_next)      # Optimal and the strings work on the lean build as it is
            full_next = False
            if r == 1 and short:
                for p in short:
                    check_cells(b, p, pairs[p][0], pairs[p][1], BLOSUM, gi, ge)
                assert_full(b)
                same_optimal(b.optimal(), fresh_results(pairs, BLOSUM, gi, ge)[0])
                full_next = True
        assert_lean(b)
        for p, (q, t) in enumerate(pairs):
            if (short and cells_of is None) or (cells_of is not None and (q, t) == long_pairs()[cells_of]):
                check_cells(b, p, q, t, BLOSUM, gi, ge)
        if short or cells_of is not None:
            assert_full(b)
            assert b.kernel_name() == full_name
            check_all(b, pairs, BLOSUM, gi, ge, (name, "after get_cells"))


def test_the_gap_jump_shapes_jump_on_the_device():
    """The lists the device reports for ins60 / del70 under 3/0 really hold the jumps the shapes were made for (>= 20 rows,
    >= 20 columns across column 1024)"""
    lp = long_pairs()
    pairs = [lp["ins60"], lp["del70"]]
    gi, ge = 3, 0
    with hints(lean_reevaluate=2):
        b = new_batch(pairs, BLOSUM, 11, 1)
        b.set_gap(LOCAL, gi, ge)
        b.reevaluate()
        assert_lean(b)
        scores, lists, status = b.optimal()
        check_optimal((scores, lists, status), pairs, BLOSUM, gi, ge)
    assert lc.longest_jumps(lists[0])[1] >= 20 and lc.longest_jumps(lists[1])[0] >= 20
    inner = lists[1][1:-1]
    assert any(c[1] - a[1] > 20 and a[1] < 1024 <= c[1] for a, c in zip(inner[:-1], inner[1:]))


# ---- (c) the value limits of the 16-bit key layout ------------------------------------------------------------------------------

def K(k):
    return rc.scaled(BLOSUM, k)


def run300():
    return [(W * 300, W * 300), (W * 300, WORST * 300), SHORT]


def hom_batch():
    return [long_pairs()["hom2046"], SHORT]


# name -> (table, pairs, gi, ge, inside?, the restated left side of tag_key16_legal and its limit)
LIMITS = {
    "key16a_in": (K(8), [(W * 369, W * 369), SHORT], 11, 0, True, 0, 32767),
    "key16a_out": (K(8), [(W * 370, W * 370), SHORT], 11, 0, False, 0, 32767),
    "key16b_in": (K(1), run300(), 5500, 8, True, 1, 8000),
    "key16b_out": (K(1), run300(), 5600, 8, False, 1, 8000),
    "2046_in": (K(1), None, 11, 3, True, 1, 8000),
    "2046_out": (K(1), None, 11, 4, False, 1, 8000),
}
PREDICATE = {"key16a_in": 32736, "key16a_out": 32824, "key16b_in": 7927, "key16b_out": 8027, "2046_in": 6166, "2046_out": 8214}


@pytest.mark.parametrize("name", sorted(LIMITS))
def test_key16_limits_under_lean(name):
    """lean_reevaluate=2 asks for a lean build at every reevaluate.  Inside tag_key16_legal the rebuild is lean and right (the
    flag is (score + 0x7FFF) & 0x8000 on packed halves: a score of 2^15 or more would carry into the neighbour's half); outside
    the launch keeps the batch full, without the 16-bit keys."""
    table, pairs, gi, ge, inside, which, limit = LIMITS[name]
    pairs = pairs or hom_batch()
    Q, T = max(len(q) for q, _ in pairs) + 2, max(len(t) for _, t in pairs) + 2
    lhs = rc.lhs_key16(rc.maxs(table), gi, ge, Q, T)
    assert lhs[which] == PREDICATE[name] and (lhs[which] < limit) == inside and lhs[1 - which] < (8000 if which == 0 else 32767)
    with hints(lean_reevaluate=2):
        b = new_batch(pairs, table, gi, ge)
        assert "lean" not in b.kernel_name() and ("key16" in b.kernel_name()) == inside, b.kernel_name()
        b.reevaluate()
        if inside:
            assert_lean(b)
        else:                                        # (370 W also leave the 11-bit tags: that batch is built by the int kernel)
            assert "lean" not in b.kernel_name() and "key16" not in b.kernel_name(), b.kernel_name()
            assert b.plane_bytes_per_cell() >= 4
        res = check_all(b, pairs, table, gi, ge, name)
        if name == "key16a_in":
            assert res[0][0] == 32472.0 > 32000
        if inside:
            assert_lean(b)
            check_cells(b, len(pairs) - 1, SHORT[0], SHORT[1], table, gi, ge)         # ensure_full at the limit: the short pair's planes
            assert_full(b)


def test_set_gap_crosses_the_limits_on_one_resident_batch():
    """2046 x 2046, BLOSUM62: lean at 11/1; 11/4 leaves the 16-bit keys (8214 >= 8000): full; 20000/1 leaves the tagged kernels
    (49152 + 20000 + 11 >= 65536 with 11 tag bits, gi + ge L >= 16000 with 12); 11/1: lean again.  Without the shape hints:
    beyond 1024 columns the dispatch takes the lean instantiation's shape by itself, and the int kernel of step 3 has its own."""
    pairs = hom_batch()
    ms = rc.maxs(BLOSUM)
    assert rc.lhs_key16(ms, 11, 4, 2048, 2048)[1] == 8214 and rc.lhs_tag11(ms, 11, 4, 2048, 2048) < 65536
    assert rc.lhs_tag11(ms, 20000, 1, 2048, 2048) >= 65536 and rc.lhs_tag12(ms, 20000, 1, 2048, 2048)[1] >= 16000
    with hints(variant=False, lean_reevaluate=2):
        b = new_batch(pairs, BLOSUM, 11, 1)
        b.reevaluate()
        assert_lean(b)
        check_all(b, pairs, BLOSUM, 11, 1, "lean 11/1")
        b.set_gap(LOCAL, 11, 4)
        b.reevaluate()
        assert_full(b)
        assert "key16" not in b.kernel_name() and "dp_affine_tag_kernel" in b.kernel_name(), b.kernel_name()
        check_all(b, pairs, BLOSUM, 11, 4, "full 11/4")
        b.set_gap(LOCAL, 20000, 1)
        b.reevaluate()
        assert "tag" not in b.kernel_name() and "solo" not in b.kernel_name() and "lean" not in b.kernel_name(), b.kernel_name()
        assert b.plane_bytes_per_cell() == 8
        check_all(b, pairs, BLOSUM, 20000, 1, "untagged 20000/1")
        b.set_gap(LOCAL, 11, 1)
        b.reevaluate()
        assert_lean(b)
        check_all(b, pairs, BLOSUM, 11, 1, "lean again")
        assert_lean(b)


@pytest.mark.parametrize("gaps", rc.GAP_FAMILIES, ids=["%d_%d" % g for g in rc.GAP_FAMILIES])
@pytest.mark.parametrize("family", DEGENERATE)
def test_degenerate_systems_under_lean(family, gaps):
    """Scaled, negated, all-negative, all-zero, constant and identity tables with zero, gi = 0, ge = 0, ge > gi and usual gaps:
    full build, optimal, reevaluate (lean), optimal against the oracle for every pair.  With nothing positive every flag is
    clear and every list is the seed's; with a constant table and zero gaps every predecessor ties."""
    table = TABLES[family]
    gi, ge = gaps
    pairs = rc.ragged_batch(ALPHA, table, 700, maxlen=200)
    assert len(pairs) == 16 and all(lc.fits_oracle(q, t) for q, t in pairs)
    with hints(lean_reevaluate=2):
        b = new_batch(pairs, table, gi, ge)
        assert_full(b)
        full = b.optimal()
        check_optimal(full, pairs, table, gi, ge, (family, "full"))
        b.reevaluate()
        assert_lean(b)
        lean = b.optimal()
        same_optimal(lean, full)
        check_optimal(lean, pairs, table, gi, ge, (family, "lean"))
        assert_lean(b)
    if family in ("all_zero", "all_negative"):
        for p, (q, t) in enumerate(pairs):
            Q, T = len(q) + 2, len(t) + 2
            head = [[0, 0]] if ((Q > 3 and T > 3) or (T == 2 and Q > 2)) else []
            assert lean[0][p] == 0 and lean[1][p].tolist() == head + [[Q - 2, T - 2], [Q - 1, T - 1]], (p, lean[1][p].tolist())


# ---- (d) hints ----------------------------------------------------------------------------------------------------------------

def hint_batch():
    return shape_pairs() + [long_pairs()["1030x1030"]]


_LAG0 = {}


def lean_rebuild(gi, ge):
    """dp(11/1); optimal; set_gap; reevaluate -> the batch, for the caller to assert on"""
    b = new_batch(hint_batch(), BLOSUM, 11, 1)
    b.optimal()
    b.set_gap(LOCAL, gi, ge)
    b.reevaluate()
    return b


def lag0_results():
    if not _LAG0:
        with hints(tag_lag=0):
            b = lean_rebuild(3, 0)
            assert_lean(b)
            _LAG0["res"] = (b.optimal(), b.optimal_strings())
            b.close()
    return _LAG0["res"]


@pytest.mark.parametrize("lag", [1, 2, 4])
def test_tag_lag_reaches_the_lean_kernel(lag):
    """The skewed exchange (wave w runs tag_lag rows behind wave w-1) in the lean instantiation: same results as tag_lag=0 and
    as the references, after a gap change"""
    want_opt, want_str = lag0_results()
    with hints(tag_lag=lag):
        b = lean_rebuild(3, 0)
        assert_lean(b)
        res = check_all(b, hint_batch(), BLOSUM, 3, 0, ("lag", lag))
        same_optimal(res, want_opt)
        same_strings(b.optimal_strings(), want_str)
        assert_lean(b)


@pytest.mark.parametrize("hint,marker", [("tag_segments", "+segq"), ("tag_bits", "tag12")])
def test_hints_that_keep_a_batch_full(hint, marker):
    """The segment queue (tag_segments=-4: the 1030-row pair is cut into segments) and 12 tag bits have no lean form: with
    lean_reevaluate=2 the rebuild stays full and right"""
    value = {"tag_segments": -4, "tag_bits": 12}[hint]
    with hints(lean_reevaluate=2, **{hint: value}):
        b = lean_rebuild(3, 0)
        assert_full(b)
        assert marker in b.kernel_name(), b.kernel_name()
        check_all(b, hint_batch(), BLOSUM, 3, 0, hint)
        assert_full(b)


# ---- (e) two more readers after a lean build -----------------------------------------------------------------------------------

def outcome(f):
    try:
        return "ok", f()
    except aln_amd.AlnError as e:
        return "error", e.code


def test_optimal_subali_after_a_lean_build():
    """Optimal_Subali needs a sub-rectangle build (have_sub), and a batch with one is never built tagged, let alone lean: the
    ensure_full call in aln_batch_optimal_subali cannot meet a lean build.  What can be pinned: on a lean build the call is
    refused with E_STATE exactly as on a fresh batch and leaves the lean build as it was; after dp_sub on the once-lean batch
    (no lean code runs there) it equals a fresh batch's."""
    pairs = [shape_pairs()[k] for k in (3, 4, 7)]
    bounds = [(2, 3, len(q) - 1, len(t) - 2) for q, t in pairs]
    with hints():
        fresh = new_batch(pairs, BLOSUM, 3, 0)
        b = new_batch(pairs, BLOSUM, 11, 1)
        b.optimal()
        b.set_gap(LOCAL, 3, 0)
        b.reevaluate()
        assert_lean(b)
        got, want = outcome(lambda: b.optimal(subali=True)), outcome(lambda: fresh.optimal(subali=True))
        assert got == want == ("error", aln_amd.E_STATE)
        assert_lean(b)
        check_all(b, pairs, BLOSUM, 3, 0, "after the refused call")
        assert_lean(b)
        for x in (fresh, b):
            x.dp_sub_submatrix(ALPHA, BLOSUM, aln_amd.GLOBAL, 3, 0, aln_amd.FWD, bounds)
        assert "lean" not in b.kernel_name()
        same_optimal(b.optimal(subali=True), fresh.optimal(subali=True))


def test_corner_scores_after_a_lean_build():
    """dp_corner_kernel reads row Q-2 and column T-2 of the score plane, which a lean build writes: after a gap change its result
    is the reference's corner, and reading it does not cost the lean build"""
    pairs = hint_batch()
    key = tkey(BLOSUM)
    with hints():
        b = lean_rebuild(3, 0)
        assert_lean(b)
        got = b.corner_scores()
        assert_lean(b)
        for p, (q, t) in enumerate(pairs):
            if lc.fits_oracle(q, t):
                corner = rc.affine_reference(rc.sim_int(q, t, ALPHA, BLOSUM), rc.LOCAL, 3, 0)[1]
            else:
                corner = _reference(q, t, key, 3, 0)[2]
            assert float(got[p]) == float(corner) and not np.signbit(got[p]), (p, float(got[p]), corner)
        check_all(b, pairs, BLOSUM, 3, 0, "after corner_scores")
        assert_lean(b)
        b.reevaluate()
        assert_lean(b)
