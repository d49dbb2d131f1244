"""The int64 numpy reference of tests/range_cases.py, pinned to the oracle (the literal O(n^3) restatement) on every scoring
family of the value-range tests, all five align types, small pairs and a few narrow ones.  The oracle computes in fp32; every
case keeps |value| < 2^24 (asserted by the reference for every cell and candidate, and here for the oracle's plane) so fp32 is
exact and the comparison is a comparison of integers.  This is what entitles tests/test_gpu_value_ranges.py to trust the numpy
reference on the long pairs the oracle cannot reach."""
import numpy as np
import pytest

import orc
import range_cases as rc

ALPHA, BLOSUM = rc.load_blosum62()
TABLES = rc.table_families(ALPHA, BLOSUM)


def check_pair(q, t, table, mode, gi, ge, what):
    S32 = orc.sim_submatrix(q, t, ALPHA, table)
    S = rc.sim_int(q, t, ALPHA, table)
    assert np.array_equal(S, S32.astype(np.int64)) and np.array_equal(S.astype(np.float32), S32), what
    err, D, PQ, PT = orc.dp_build(S32, orc.Gap(mode, gi, ge))
    assert err == 0, what
    H, corner, lmax = rc.affine_reference(S, mode, gi, ge)
    assert np.abs(D).max() < rc.EXACT_LIMIT, what
    D64 = D.astype(np.int64)
    assert np.array_equal(D64.astype(np.float32), D), what               # integral
    assert np.array_equal(H, D64), "%s: %d cells differ" % (what, np.count_nonzero(H != D64))
    score = orc.optimal(D, PQ, PT, mode == rc.LOCAL)[1]
    assert float(score) == rc.reference_score(H, mode), what
    assert (corner, lmax) == (int(H[-1, -1]), int(H[:-1, :-1].max())), what
    assert rc.pointers_consistent(D, PQ, PT, S, mode, gi, ge) == 0, what
    return PQ, PT, S, D


def test_the_modes_and_the_parser_agree_with_the_oracle(blosum62):
    assert (rc.GLOBAL_LOCAL, rc.GLOBAL, rc.LOCAL_GLOBAL, rc.LOCAL, rc.SEMI_LOCAL) == (
        orc.GLOBAL_LOCAL, orc.GLOBAL, orc.LOCAL_GLOBAL, orc.LOCAL, orc.SEMI_LOCAL)
    assert blosum62[0] == ALPHA and np.array_equal(blosum62[1], BLOSUM)
    assert rc.maxs(BLOSUM) == 11 and rc.best_residue(ALPHA, BLOSUM) == "W"
    for mode in rc.ALIGN_TYPES:
        fdel, fins = rc.free_ends(mode)
        for (a, b, last) in [(0, 1, 9), (0, 5, 9), (3, 9, 9), (2, 6, 9), (0, 9, 9), (4, 5, 9)]:
            g = orc.Gap(mode, 7, 2)
            assert float(orc.deletion(g, 10, 10, 0, 1, a, b)) == float(rc.gap_cost(a, b, last, fdel, 7, 2))
            assert float(orc.insertion(g, 10, 10, a, b, 0, 1)) == float(rc.gap_cost(a, b, last, fins, 7, 2))


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
@pytest.mark.parametrize("family", sorted(TABLES))
def test_reference_equals_oracle(family, mode):
    """Every table family x every gap family x the sequence shapes (runs, worst partners, identical, random, run against one or
    two residues, empties) at 40 x 57, the run and random shapes again at 120 x 120."""
    table = TABLES[family]
    for (gi, ge) in rc.GAP_FAMILIES + [(2500, 3)]:
        for name, q, t in rc.shaped_pairs(ALPHA, table, 40, 57, seed=7):
            check_pair(q, t, table, mode, gi, ge, "%s %s mode %d gaps %d/%d" % (family, name, mode, gi, ge))
    for (gi, ge) in [(0, 0), (1, 5), (11, 1)]:
        for name, q, t in rc.shaped_pairs(ALPHA, table, 120, 120, seed=11)[:4]:
            check_pair(q, t, table, mode, gi, ge, "%s %s 120 mode %d gaps %d/%d" % (family, name, mode, gi, ge))


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_reference_equals_oracle_on_narrow_pairs(mode):
    """600 x 6 and 6 x 600: the largest end-gap terms gi + ge * length, BLOSUM62 x 9 and the all-negative table."""
    for family in ("blosum62x9", "all_negative", "constant+3"):
        table = TABLES[family]
        a = rc.best_residue(ALPHA, table)
        w = rc.worst_partner(ALPHA, table, a)
        for (gi, ge) in [(0, 1), (900, 8), (1, 5)]:
            for q, t in [(rc.run(a, 600), rc.run(a, 6)), (rc.run(a, 6), rc.run(w, 600)), (rc.random_seq(ALPHA, 3, 600), a + w),
                         (rc.run(a, 2), rc.random_seq(ALPHA, 4, 600))]:
                check_pair(q, t, table, mode, gi, ge, "%s narrow %dx%d mode %d gaps %d/%d" % (family, len(q), len(t), mode, gi, ge))


def test_pointer_check_notices_a_wrong_pointer_and_a_wrong_score():
    """pointers_consistent is itself a judge on the long pairs: one moved pointer or one changed score must count."""
    table = TABLES["blosum62"]
    q, t = rc.random_seq(ALPHA, 21, 50), rc.random_seq(ALPHA, 22, 61)
    for mode in (rc.GLOBAL, rc.LOCAL):
        PQ, PT, S, D = check_pair(q, t, table, mode, 11, 1, "pointer check")
        P2 = PT.copy()
        P2[30, 40] = PT[30, 40] - 1 if PT[30, 40] > 1 else PT[30, 40] + 1
        assert rc.pointers_consistent(D, PQ, P2, S, mode, 11, 1) > 0
        D2 = D.copy()
        D2[30, 40] += 1
        assert rc.pointers_consistent(D2, PQ, PT, S, mode, 11, 1) > 0
    # a local start must keep the diagonal pointer: any other in-bounds pointer with a candidate <= 0 is wrong too
    zi, zj = [(i, j) for i, j in zip(*np.nonzero(D[2:-1, 3:-1] == 0))][0]
    zi, zj = zi + 2, zj + 3
    assert (PQ[zi, zj], PT[zi, zj]) == (zi - 1, zj - 1)
    P2 = PT.copy()
    P2[zi, zj] = zj - 2                                       # a deletion from (zi-1, zj-2): candidate D - 11 + S, clipped to 0 as well
    assert D[zi - 1, zj - 2] - 11 + S[zi, zj] <= 0
    assert rc.pointers_consistent(D, PQ, P2, S, rc.LOCAL, 11, 1) > 0


def test_reference_refuses_values_beyond_fp32_exact_range():
    table = rc.scaled(BLOSUM, 20000)
    with pytest.raises(AssertionError):
        rc.affine_reference(rc.sim_int(rc.run("W", 100), rc.run("W", 100), ALPHA, table), rc.GLOBAL, 0, 0)
