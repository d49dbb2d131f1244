"""CPU only: aln_hits_align_multi_profiles at the ABI boundary, and the reference its GPU test uses — multi_align_cases.rounds on
the int64 plane of a profile — against the oracle's own build and traceback on the same masked planes, round by round, against
the residue reference for derived profiles, with the properties the header promises and the situations the cases were built for."""
import ctypes
import os
import re

import numpy as np
import pytest

import multi_align_cases as mac
import profile_multi_cases as pm

U32 = np.uint32
SPECIFIC = pm.specific_cases() + [pm.stale_ring_case()]
DERIVED = pm.derived_small()
ORACLE = [c for c in SPECIFIC + DERIVED if (len(c.profile) + 2) * (len(c.t) + 2) <= 300 * 700]
ALL = SPECIFIC + [pm.long_case()] + DERIVED + pm.derived_shapes()


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_hits_align_multi_profiles_is_declared_exported_and_bound():
    import aln_amd
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "aln_hip.h")).read()
    assert re.search(r"\bint\s+aln_hits_align_multi_profiles\s*\(", header)
    if not os.path.exists(aln_amd.LIB_PATH):
        aln_amd.build_library()
    L = ctypes.CDLL(aln_amd.LIB_PATH)
    assert hasattr(L, "aln_hits_align_multi_profiles")
    assert "aln_hits_align_multi_profiles" in aln_amd.EXPORTS
    assert callable(aln_amd.hits_align_multi_profiles) and callable(aln_amd.hits_align_multi_profiles_detour)
    assert len(aln_amd.lib().aln_hits_align_multi_profiles.argtypes) == 20


# ---- the rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ORACLE, ids=[c.name for c in ORACLE])
def test_reference_equals_the_oracle_round_by_round(case):
    reported, ender = pm.reference(case)                       # asserts the case's teeth
    want = pm.oracle_rounds(case)
    assert len(reported) == len(want)
    for a, (r, (sc, pl)) in enumerate(zip(reported, want)):
        assert np.float32(r.score).view(U32) == np.float32(sc).view(U32), (case.name, a)
        assert np.array_equal(r.pairs, pl), (case.name, a, r.pairs.tolist(), pl.tolist())


@pytest.mark.parametrize("case", DERIVED + pm.derived_shapes(), ids=lambda c: c.name)
def test_derived_reference_is_the_residue_reference(case):
    reported, ender = pm.reference(case)
    want, wender = mac.reference(case.residue)
    assert pm.same_rounds(reported, want), case.name
    assert (ender is None) == (wender is None)
    assert np.array_equal(pm.plane(case), mac.sim(case.residue))


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_rounds_are_disjoint_and_scores_do_not_increase(case):
    reported, ender = pm.reference(case)
    Q, T = len(case.profile) + 2, len(case.t) + 2
    seen = set()
    for a, r in enumerate(reported):
        cells = mac.interior(r.pairs, Q, T)
        assert len(set(cells)) == len(cells) and not (seen & set(cells)), (case.name, a)
        seen |= set(cells)
        if a:
            assert r.score <= reported[a - 1].score and r.score > 0
    if ender is not None and reported:
        assert ender.score <= reported[-1].score


# ---- the situations --------------------------------------------------------------------------------------------------------------
def test_every_situation_has_a_case():
    found = set()
    for c in SPECIFIC + [pm.long_case()]:
        reported, ender = pm.reference(c)
        assert len(reported) >= 3, c.name
        found |= pm.census(c, reported, ender)
    need = {"rounds3", "stale_ring"} | {"row%d" % r for r in pm.ROW_TEETH} | {"col%d" % c for c in pm.COL_TEETH}
    assert need <= found, sorted(need - found)
    assert tuple(len(c.profile) + 2 for c in pm.specific_cases()) == pm.QUERY_SIZES
    assert sorted({(len(c.t) + 2 + 255) // 256 for c in SPECIFIC + [pm.long_case()]}) == [1, 2, 3, 7, 8]
    assert len(pm.long_case().t) + 2 == 2040 and len(pm.long_case().profile) + 2 == 130


def test_position_specific_rows_differ_from_the_consensus_rows_everywhere():
    """so the residue kernel over the consensus cannot pass: reference() has asserted that its lists differ; here the inputs"""
    for c in SPECIFIC + [pm.long_case()]:
        rows = pm.table_rows(pm.ALPHA, pm.BLOSUM, c.consensus)
        assert rows.shape == c.profile.shape and (rows != c.profile).any(axis=1).all(), c.name


def test_the_stale_ring_case_reenters_low_rows_after_high_ones():
    c = pm.stale_ring_case()
    reported, _ = pm.reference(c)
    Q, T = len(c.profile) + 2, len(c.t) + 2
    assert Q == 67
    for a in (1, 2):
        assert reported[a - 1].end[0] > 40 and min(i for i, j in mac.interior(reported[a].pairs, Q, T)) < 8
