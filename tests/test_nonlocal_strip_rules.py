"""No GPU: the rules of hit_global_kernel (csrc/search_align.h) — strip byte, final cell, walk — restated in numpy from
the oracle's D plane (tests/nonlocal_cases.py) reproduce orc.optimal's list on the tie inputs, for the four non-local align
types and the four gap families, and those inputs meet every case the GPU test's census asks for."""
import numpy as np
import pytest

import nonlocal_cases as nc

U32 = np.uint32


@pytest.mark.parametrize("mode", nc.NONLOCAL)
def test_rules_reproduce_the_oracle_on_the_tie_inputs(mode):
    free_del, free_ins = nc.free_ends(mode)
    cen = nc.new_census()
    pairs = 0
    for alpha in ("AC", "ACGT"):
        table = nc.tie_table(alpha)
        qs, ts = nc.tie_sequences(alpha)
        for gi, ge in nc.TIE_GAPS:
            for q in qs:
                for t in ts:
                    D, sc, pl = nc.oracle_pair(q, t, alpha, table, mode, gi, ge)
                    score, got = nc.walk(D, gi, ge, free_del, free_ins)
                    assert np.array_equal(got, pl), (mode, alpha, gi, ge, q, t, got.tolist(), pl.tolist())
                    assert score.view(U32) == np.float32(sc).view(U32)
                    nc.census(D, pl, gi, ge, cen)
                    pairs += 1
    assert pairs == 2 * 4 * 36
    print("census", mode, cen)
    assert nc.census_ok(cen), cen


@pytest.mark.parametrize("mode", nc.NONLOCAL)
def test_rules_on_the_smallest_shapes(mode):
    """Q = 3 (no strip row at all), T = 3, and both"""
    free_del, free_ins = nc.free_ends(mode)
    alpha = "ACGT"
    table = nc.tie_table(alpha)
    for q in ("A", "C", "AC", "ACGTA"):
        for t in ("A", "G", "CA", "GTACA"):
            for gi, ge in nc.TIE_GAPS:
                D, sc, pl = nc.oracle_pair(q, t, alpha, table, mode, gi, ge)
                score, got = nc.walk(D, gi, ge, free_del, free_ins)
                assert np.array_equal(got, pl), (mode, q, t, gi, ge, got.tolist(), pl.tolist())
                assert score.view(U32) == np.float32(sc).view(U32)
