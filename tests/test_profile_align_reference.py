"""No GPU: the references of aln_hits_align_profiles (tests/profile_align_cases.py).  On the tie profiles the restated rules —
lean_cases.reference_list for local builds, nonlocal_cases.walk for the four other align types, both on the int64 plane — give
the list and the score of orc.dp_build + orc.optimal over the float plane, for all 6 x 6 pairs, both alphabets, the four gap
systems and all five align types; every profile differs from the table rows it was made from; and the inputs meet the census
floors the GPU test asserts on what the device returns."""
import numpy as np
import pytest

import nonlocal_cases as nc
import profile_align_cases as pac
import range_cases as rc

U32 = np.uint32


@pytest.fixture(autouse=True, scope="module")
def the_entry_these_references_are_for():
    """references of an entry the package does not have pin nothing"""
    import aln_amd
    assert "aln_hits_align_profiles" in aln_amd.EXPORTS and callable(aln_amd.hits_align_profiles)


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_restated_rules_reproduce_the_oracle_on_the_tie_profiles(mode):
    local = mode == rc.LOCAL
    cen = pac.new_local_census() if local else nc.new_census()
    pairs = 0
    for alpha in pac.TIE_ALPHAS:
        profiles, qs, ts = pac.tie_profiles(alpha)
        assert len(profiles) == 6 and len(ts) == 6
        for gi, ge in pac.TIE_GAPS:
            for p in profiles:
                for t in ts:
                    D, sc, pl = pac.oracle_pair(p, t, alpha, mode, gi, ge)
                    score, got = pac.restated(p, t, alpha, mode, gi, ge)
                    assert np.array_equal(got, pl), (mode, alpha, gi, ge, t, got.tolist(), pl.tolist())
                    assert np.float32(score).view(U32) == np.float32(sc).view(U32), (mode, alpha, gi, ge, t)
                    if local:
                        pac.local_census(D, pl, gi, ge, cen)
                    else:
                        nc.census(D, pl, gi, ge, cen)
                    pairs += 1
    assert pairs == 2 * 4 * 36
    print("census", mode, cen)
    assert pac.meets(cen, pac.LOCAL_FLOORS if local else pac.NONLOCAL_FLOORS), cen


def test_every_tie_profile_differs_from_its_table_rows():
    n = 0
    for alpha in pac.TIE_ALPHAS:
        profiles, qs, ts = pac.tie_profiles(alpha)
        for p, q in zip(profiles, qs):
            rows = pac.table_rows(alpha, q)
            assert p.shape == rows.shape == (len(q), len(alpha))
            assert (p != rows).any() and np.abs(p - rows).max() == 1
            n += 1
    assert n == 12


def test_the_plane_is_a_gather_of_rows_by_letters():
    p = np.array([[1, 2], [3, 4], [5, 6]])
    S = pac.plane(p, "CAAC", "AC")
    assert S.shape == (5, 6) and (S[0] == 0).all() and (S[-1] == 0).all() and (S[:, 0] == 0).all() and (S[:, -1] == 0).all()
    assert S[1:-1, 1:-1].tolist() == [[2, 1, 1, 2], [4, 3, 3, 4], [6, 5, 5, 6]]
    assert pac.plane(p, "", "AC").shape == (5, 2) and pac.plane(np.zeros((0, 2)), "AC", "AC").shape == (2, 4)
