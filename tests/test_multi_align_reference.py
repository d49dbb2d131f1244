"""CPU only: aln_hits_align_multi at the ABI boundary, and the rule it implements — the int64 reference of
multi_align_cases against the oracle's own build and traceback on the same masked planes, round by round, with the properties the
header promises and the situations every case was built for."""
import ctypes
import os

import numpy as np
import pytest

import multi_align_cases as mc

U32 = np.uint32
SMALL = mc.small_cases() + [mc.cut_case()]
IDS = [c.name for c in SMALL]


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_hits_align_multi_is_exported_and_bound():
    import aln_amd
    if not os.path.exists(aln_amd.LIB_PATH):
        aln_amd.build_library()
    L = ctypes.CDLL(aln_amd.LIB_PATH)
    assert hasattr(L, "aln_hits_align_multi")
    assert "aln_hits_align_multi" in aln_amd.EXPORTS
    assert callable(aln_amd.hits_align_multi)
    assert len(aln_amd.lib().aln_hits_align_multi.argtypes) == 20


# ---- the rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL, ids=IDS)
def test_reference_equals_the_oracle_round_by_round(case):
    reported, ender = mc.reference(case)                       # asserts the case's teeth
    want = mc.oracle_rounds(case)
    assert len(reported) == len(want)
    for a, (r, (sc, pl)) in enumerate(zip(reported, want)):
        assert np.float32(r.score).view(U32) == np.float32(sc).view(U32), (case.name, a)
        assert np.array_equal(r.pairs, pl), (case.name, a, r.pairs.tolist(), pl.tolist())


@pytest.mark.parametrize("case", SMALL, ids=IDS)
def test_rounds_are_disjoint_and_scores_do_not_increase(case):
    reported, ender = mc.reference(case)
    Q, T = len(case.q) + 2, len(case.t) + 2
    seen = set()
    for a, r in enumerate(reported):
        cells = mc.interior(r.pairs, Q, T)
        assert len(set(cells)) == len(cells) and not (seen & set(cells)), (case.name, a)
        seen |= set(cells)
        if a:
            assert r.score <= reported[a - 1].score and r.score > 0
    if ender is not None and reported:
        assert ender.score <= reported[-1].score


@pytest.mark.parametrize("case", SMALL, ids=IDS)
def test_round_0_is_the_unmasked_optimal_list(case):
    import lean_cases as lc
    import range_cases as rc
    reported, _ = mc.reference(case)
    H = rc.affine_reference(mc.sim(case), rc.LOCAL, case.gi, case.ge)[0]
    if reported:
        assert np.array_equal(reported[0].pairs, lc.reference_list(H, case.gi, case.ge))
        assert reported[0].score == rc.reference_score(H, rc.LOCAL)
    else:
        assert rc.reference_score(H, rc.LOCAL) < case.min_score


# ---- teeth ---------------------------------------------------------------------------------------------------------------------
def test_every_situation_has_a_case():
    found = set()
    group = set()
    for c in SMALL:
        reported, ender = mc.reference(c)
        f = mc.census(c, reported, ender)
        found |= f | (set(c.teeth) & {"min_score_cut"})
        if c.name.startswith("tie_"):
            group |= f
    need = {"rounds3", "stop_diag", "stop_after_del", "stop_after_ins", "jump_over", "row1", "col1", "col31", "col32", "col255",
            "col256", "col257", "tie_rounds", "seed_zero_end", "min_score_cut"}
    assert need <= found, sorted(need - found)
    assert set(mc.TIE_GROUP_TEETH) <= group, sorted(set(mc.TIE_GROUP_TEETH) - group)
    fams = {(c.gi, c.ge) for c in SMALL if c.name.startswith("tie_") and "tie_rounds" in mc.census(c, *mc.reference(c))}
    assert {(11, 1), (0, 0), (40, 0), (1, 5)} <= fams, fams


def test_a_walk_never_stops_at_a_forbidden_gap_source():
    """census() asserts it for every stop it classifies (a forbidden predecessor is always the diagonal one); here the count of
    such stops, so that the assertion is known to have run"""
    n = 0
    for c in SMALL:
        reported, ender = mc.reference(c)
        n += "stop_diag" in mc.census(c, reported, ender)
    assert n >= 3, n


def test_shape_cases_cover_the_classes_and_report_several_rounds():
    cases = mc.shape_cases()
    assert sorted({(len(c.t) + 2 + 255) // 256 for c in cases}) == [1, 2, 3, 7]
    assert sorted({len(c.q) + 2 for c in cases}) == [3, 4, 17, 130]
    for c in cases:
        reported, _ = mc.reference(c)
        assert len(reported) >= 2, c.name


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------
def differs(case, variant):
    reported, _ = mc.reference(case)
    other, _ = mc.rounds(mc.sim(case), case.gi, case.ge, case.N, case.min_score, variant)
    return not (len(other) == len(reported) and
                all(a.score == b.score and np.array_equal(a.pairs, b.pairs) for a, b in zip(reported, other)))


def test_forgetting_the_mask_in_row_1_and_column_1_changes_the_lists():
    by = {c.name: c for c in SMALL}
    for name in ("single_cell", "tie_AC_0_0_1", "tie_ACGT_0_0_1"):
        f = mc.census(by[name], *mc.reference(by[name]))
        assert {"row1", "col1"} <= f, name
        assert differs(by[name], "forget_borders"), name


def test_walking_on_through_forbidden_cells_changes_the_lists():
    by = {c.name: c for c in SMALL}
    for name in ("tie_ACGT_0_0_40", "tie_ACGT_0_0_54", "tie_AC_0_1_1"):
        assert "stop_diag" in mc.census(by[name], *mc.reference(by[name])), name
        assert differs(by[name], "walk_through"), name
