"""-m gpu: the zero mark of lean rebuilds (dp_affine_tag_kernel<..., lean>: clip key ZKEY | 1, bit 15 in row 1 and column 1) on
pairs whose walk has to read "this cell scores 0" from a pointer word at every place the kernel treats differently.

tests/lean_zero_cases.py builds the pairs and says what each is for; tests/test_lean_zero_mark_rules.py proves on the oracle that
each holds it.  Every result of a lean build (lists, optimal_strings, corner scores) is compared bit for bit with a fresh batch
built by aln_batch_dp under the same gaps (never lean), with the int64 reference of tests/range_cases.py, and with the oracle where
the pair is small enough.  Every test asserts the kernel's name and 2 bytes per cell before it looks at a result."""
import functools

import numpy as np
import pytest

import aln_amd
import gpu_util
import lean_cases as lc
import lean_zero_cases as z
import orc

pytestmark = pytest.mark.gpu

LOCAL = aln_amd.LOCAL
_OPEN = []


@pytest.fixture(autouse=True)
def close_batches():
    yield
    while _OPEN:
        _OPEN.pop().close()


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def new_batch(pairs, table, gi, ge):
    b = aln_amd.Batch(gpu_util.ctx(), [p[0] for p in pairs], [p[1] for p in pairs])
    _OPEN.append(b)
    b.dp_submatrix(z.ALPHA, z.TABLES[table], LOCAL, gi, ge)
    return b


@functools.lru_cache(maxsize=None)
def fresh_results(pairs, table, gi, ge):
    """Optimal, the strings and the corner scores of a batch built by aln_batch_dp with the default hints: never lean.  Computed
    once per batch and setting, shared by the tests (hints never change a result)"""
    b = new_batch(pairs, table, gi, ge)
    lc.assert_full(b, b.plane_bytes_per_cell())
    res = b.optimal(), b.optimal_strings(), b.corner_scores()
    b.close()
    return res


def same_strings(got, want):
    assert np.array_equal(u32(got[0]), u32(want[0])) and np.array_equal(u32(got[1]), u32(want[1]))
    assert np.array_equal(got[2], want[2])
    assert got[3] == want[3] and got[4] == want[4]


@functools.lru_cache(maxsize=None)
def oracle_list(q, t, table, gi, ge):
    S = orc.sim_submatrix(q, t, z.ALPHA, z.TABLES[table])
    err, D, PQ, PT = orc.dp_build(S, orc.Gap(orc.LOCAL, gi, ge))
    assert err == 0
    err, sc, pl = orc.optimal(D, PQ, PT, True)
    assert err == 0
    return sc, pl


def check_lean(pairs, table, gi, ge, what=None):
    """full build, Optimal, lean rebuild -> Optimal, strings, corner scores against the fresh batch and the references"""
    pairs = tuple(pairs)
    want_opt, want_str, want_corner = fresh_results(pairs, table, gi, ge)
    b = new_batch(pairs, table, gi, ge)
    full_name = b.kernel_name()
    lc.same_optimal(b.optimal(), want_opt)
    b.reevaluate()
    lc.assert_lean(b)
    assert b.kernel_name().replace(",lean", "") == full_name, (b.kernel_name(), full_name)
    res = b.optimal()
    lc.same_optimal(res, want_opt)
    same_strings(b.optimal_strings(), want_str)
    assert np.array_equal(u32(b.corner_scores()), u32(want_corner))
    lc.assert_lean(b)
    scores, lists, status = res
    for p, (q, t) in enumerate(pairs):
        w = (what, p, len(q), len(t))
        S, H, L = z.reference(q, t, table, gi, ge)
        assert status[p] == 0, w
        assert float(scores[p]) == float(H[lc.find_max_cell(H)]) and not np.signbit(scores[p]), w
        assert np.array_equal(lists[p], L), w
        assert float(want_corner[p]) == float(H[-1, -1]), w
        if lc.fits_oracle(q, t):
            sc, pl = oracle_list(q, t, table, gi, ge)
            assert u32(scores[p]) == u32(sc) and np.array_equal(lists[p], pl), w
    return b, res


def variant(**extra):
    return gpu_util.ctx().hints(**dict(lc.VARIANT, **extra))


@pytest.mark.parametrize("name", [c.name for c in z.cases()])
def test_each_case_alone(name):
    """the walk stops on the diagonal at a zero cell in each column the kernel treats differently and in row 1; after a deletion
    or an insertion jump that lands in column 1, in row 1, in column 1024; at once on an all-negative table"""
    c = z.case(name)
    S, H, L = z.reference(c.q, c.t, c.table, c.gi, c.ge)
    z.check_purpose(c, H, L)
    with variant():
        b, res = check_lean([(c.q, c.t)], c.table, c.gi, c.ge, name)
        z.check_purpose(c, H, res[1][0])


def groups():
    """the cases as batches: one per (table, gaps)"""
    out = {}
    for c in z.cases():
        out.setdefault((c.table, c.gi, c.ge), []).append((c.q, c.t))
    return sorted(out.items())


@pytest.mark.parametrize("occ", [2, 3])
@pytest.mark.parametrize("g", range(3), ids=["%s_%d_%d" % k for k, _ in groups()])
def test_case_batches_at_both_occupancies(g, occ):
    (table, gi, ge), pairs = groups()[g]
    with variant(tag_occupancy=occ):
        b, res = check_lean(pairs, table, gi, ge, (table, occ))
        assert ("occ3" in b.kernel_name()) == (occ == 3), b.kernel_name()


@pytest.mark.parametrize("occ", [2, 3])
def test_ragged_batch(occ):
    """T in {10, 515, 1026, 1031, 1537, 2046} beside one 2046-column pair: the owner of the chunk of column T-2 in each group of
    each wave, at both ends of a chunk"""
    pairs = z.ragged_pairs()
    assert [len(t) + 2 for _, t in pairs] == list(z.RAGGED_T) + [2046]
    with variant(tag_occupancy=occ):
        check_lean(pairs, "blosum62", 11, 1, ("ragged", occ))


HINTS = [("tag_lag", v) for v in (1, 2, 4)] + [("tag_alt_prio", v) for v in (0, 1, 2, 3, 0x111)]


@pytest.mark.parametrize("hint,value", HINTS, ids=["%s_%x" % h for h in HINTS])
def test_hints_leave_the_kernel_lean_and_the_results_equal(hint, value):
    """the lean form has no skewed exchange and one priority form: tag_lag is accepted and ignored, every tag_alt_prio but 1 is off"""
    (table, gi, ge), pairs = groups()[1]
    assert table == "blosum62" and (gi, ge) == (3, 1)
    with variant(**{hint: value}):
        check_lean(pairs + z.ragged_pairs()[:3], table, gi, ge, (hint, value))
    (table, gi, ge), pairs = groups()[2]
    assert table == "blosum62" and (gi, ge) == (11, 1)
    with variant(**{hint: value}):
        check_lean(pairs[4:8] + pairs[10:12], table, gi, ge, (hint, value))
