"""The int64 restatement of position-specific gap penalties (qgap_cases.qgap_planes) pinned without a GPU: constant rows give
the constant-affine reference, a hand-worked example, the entries that are never read, and what one row's price can change.

The hand-worked example (test_worked_example).  Profile of 3 interior rows (Q = 5): row 1 scores A +5, row 2 scores C +5,
row 3 scores D +5, every other letter -2.  Template "ACWD" (T = 6).  ALN_GLOBAL, del_init = [7, 7, 4, 1] for rows 0..3,
del_extn = 1, ins_init = 6, ins_extn = 1.  D, interior rows x interior columns:

            A    C    W    D
   row 1    5   -9  -10  -11      row 1, column j: S - del(0, j-1), the head deletion priced by row 0: 7, 8, 9
   row 2   -8   10   -4   -5      (2,W): (1,A) 5 - del(1, 1) = 5 - 7, + S = -2 -> -4
   row 3   -9   -3    8   11      (3,C): (1,A) 5 - ins(2, 2) = 5 - 6, + S = -2 -> -3;  (3,W): diagonal (2,C) 10 - 2;  (3,D): (2,C) 10 - del(2, 1) = 10 - 4, + 5 = 11

final cell = max( D[3][D] = 11,  (3,W) 8 - del(3, 1) = 8 - 1 = 7, ... ) = 11: A-1, C-2, W skipped at row 2's price, D-3.
With del_init[2] raised to 9 the skip of W costs 9 and (3,D) falls to max(10 - 9, -4) + 5 = 6, so the best path becomes
A-1, C-2, W-3 (-2) with D skipped at the tail, priced by row 3, the row the gap LEAVES: 8 - 1 = 7.
"""
import numpy as np
import pytest

import lean_cases as lc
import profile_cases as pc
import qgap_cases as qg
import range_cases as rc

IDX = {ch: k for k, ch in enumerate(qg.ALPHA)}


def rows_scoring(letters, hit, miss):
    p = np.full((len(letters), qg.N), miss, np.int64)
    for i, ch in enumerate(letters):
        if ch != ".":
            p[i, IDX[ch]] = hit
    return p


def small_members():
    profiles, ts = pc.length_set()
    profiles = [p for p in profiles if len(p) <= 9]
    ts = sorted(set(t for t in ts if len(t) <= 40) | {"", "W", "AC"}, key=lambda t: (len(t), t))
    assert {len(p) for p in profiles} >= {0, 1, 2, 7, 8, 9} and {len(t) for t in ts} >= {0, 1, 2}
    return profiles, ts


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
@pytest.mark.parametrize("gi,ge", [(11, 1), (3, 2), (0, 0)])
def test_constant_rows_are_the_constant_affine_recurrence(mode, gi, ge):
    """every cell, the score and the end cell; the degenerate shapes Q in {2, 3} x T in {2, 3} are among the members"""
    profiles, ts = small_members()
    for p in profiles:
        for t in ts:
            S = pc.plane(p, t)
            H = rc.affine_reference(S, mode, gi, ge)[0]
            G = qg.qgap_planes(S, mode, *[qg.with_tail(g) for g in qg.constant(len(p), gi, ge)])
            assert np.array_equal(G, H), (len(p), t, mode)
            assert qg.pair_reference(p, t, mode, qg.constant(len(p), gi, ge)) == pc.pair_reference(p, t, mode, gi, ge)
            assert rc.reference_score(G, mode) == rc.reference_score(H, mode) and lc.find_max_cell(G) == lc.find_max_cell(H)


def test_worked_example():
    p = rows_scoring("ACD", 5, -2)
    gaps = [[7, 7, 4, 1], [1] * 4, [6] * 4, [1] * 4]
    H = qg.qgap_planes(pc.plane(p, "ACWD"), rc.GLOBAL, *[qg.with_tail(g) for g in gaps])
    assert H[1:4, 1:5].tolist() == [[5, -9, -10, -11], [-8, 10, -4, -5], [-9, -3, 8, 11]]
    assert H[4, 5] == 11
    gaps[0][2] = 9
    H = qg.qgap_planes(pc.plane(p, "ACWD"), rc.GLOBAL, *[qg.with_tail(g) for g in gaps])
    assert H[3, 4] == 6 and H[3, 3] == 8 and H[4, 5] == 7


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_entries_never_read_may_be_nan(mode):
    """del_* at row Q-1, ins_* at rows 0 and Q-1: the reference reads entries through int(), which a NaN does not survive"""
    profiles, ts = qg.small_set()
    for s, p in enumerate(profiles):
        L = len(p)
        g = qg.random_rows(L, 77 + s)
        full = [list(map(float, a)) + [qg.NAN] for a in g]
        full[2][0] = full[3][0] = qg.NAN
        for t in ts:
            H = qg.qgap_planes(pc.plane(p, t), mode, *full)
            zeroed = [a[:-1] + [0.0] for a in full]
            zeroed[2][0] = zeroed[3][0] = 0.0
            assert np.array_equal(H, qg.qgap_planes(pc.plane(p, t), mode, *zeroed))
    with pytest.raises(ValueError):                              # ... and an entry that IS read does not pass as NaN
        bad = [list(map(float, a)) + [qg.NAN] for a in qg.constant(6, 11, 1)]
        bad[0][0] = qg.NAN
        qg.qgap_planes(pc.plane(profiles[0], ts[1]), rc.GLOBAL, *bad)


def test_one_ins_extn_changes_only_alignments_that_skip_its_row():
    """Rows 1-3 score A, C, D +10, rows 4-6 score every letter -5, rows 7-8 score E, F +10; the template is ACDEF.  The global
    optimum skips rows 4..6: ins(4, 6) = ins_init[4] + ins_extn[5] + ins_extn[6] = 8, score 50 - 8."""
    p = rows_scoring("ACD...EF", 10, -5)
    base = qg.constant(8, 6, 1)

    def score(row=None, by=0, mode=rc.GLOBAL):
        g = [list(a) for a in base]
        if row is not None:
            g[3][row] += by
        return qg.pair_reference(p, "ACDEF", mode, g)[0]

    assert score() == 42
    assert score(5, 3) == 39 and score(6, 3) == 39              # a skipped position behind the first pays its own ins_extn
    assert score(4, 3) == 42                                    # the first skipped position pays ins_init, never its ins_extn
    for row in (1, 2, 3, 7, 8):                                 # rows the optimum aligns
        assert score(row, 3) == 42
    # a local alignment takes the same bridge, and drops it (ACD alone, 30) once it costs more than EF brings
    assert score(mode=rc.LOCAL) == 42 and score(5, 40, mode=rc.LOCAL) == 30
