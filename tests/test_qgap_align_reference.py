"""The alignment under position-specific gap penalties (include/aln_hip.h, aln_hits_align_profiles_gaps) pinned without a GPU:
the int64 restatement of qgap_align_cases against the existing restatements under constant rows, its path scorer, the
conditions on the inputs of tests/test_gpu_qgap_align.py, and an example worked by hand.

The hand-worked example (test_worked_tie).  Profile of 4 interior rows (Q = 6) that like C, A, D, E in turn (+5, every other
letter -4); template "ACDEF" (T = 7); ALN_SEMI_LOCAL (every end gap free); all four prices 3 / 1.  Row 1 and column 1 hold S:

            A    C    D    E    F
   row 1   -4    5   -4   -4   -4
   row 2    5   -8    .    .    .        (2,C): -4 + D[1][A] = -8
   row 3   -4    .    7    .    .        (3,D): match (2,C) -8;  deletion from (2,A): 5 - del(2, 1) = 2;  insertion from (1,C):
   row 4   -4    .    .   12    .                5 - ins(2, 2) = 2.  A tie: the deletion comes first and stays.  +5 = 7

The final cell takes (4,E) = 12 by a free tail deletion, so the list is (0,0) (2,1) (3,3) (4,4) (5,6), score 12.  With
ins_init[2] lowered to 2 the insertion is strictly greater (3 > 2): (0,0) (1,2) (3,3) (4,4) (5,6), score 13.  With del_init[2]
raised to 4 instead the insertion wins as well, at the old score 12.
"""
import numpy as np
import pytest

import profile_align_cases as pac
import profile_cases as pc
import qgap_align_cases as qa
import qgap_cases as qg
import range_cases as rc

IDX = {ch: k for k, ch in enumerate(qg.ALPHA)}


def small_members():
    profiles, ts = pc.length_set()
    profiles = [p for p in profiles if len(p) <= 9]
    ts = sorted(set(t for t in ts if len(t) <= 40) | {"", "W", "AC"}, key=lambda t: (len(t), t))
    assert {len(p) for p in profiles} >= {0, 1, 2, 7, 8, 9} and {len(t) for t in ts} >= {0, 1, 2}
    return profiles, ts


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
@pytest.mark.parametrize("gi,ge", [(11, 1), (4, 1), (1, 0)])
def test_constant_rows_give_the_existing_lists(mode, gi, ge):
    """profile_align_cases.restated: lean_cases.reference_list (local) and nonlocal_cases.walk; Q, T in {2, 3} among the members"""
    profiles, ts = small_members()
    for p in profiles:
        for t in ts:
            score, pl = qa.restated(p, t, mode, qg.constant(len(p), gi, ge))
            want_score, want = pac.restated(p, t, qg.ALPHA, mode, gi, ge)
            assert score == want_score, (len(p), t, mode)
            if want is None:                                   # a non-local pair without an interior
                want = np.array([(0, 0), (len(p) + 1, len(t) + 1)], np.int32)
            assert np.array_equal(pl, want), (len(p), t, mode, pl.tolist(), want.tolist())


def test_constant_rows_on_the_tie_profiles():
    """the tie inputs under the existing tie gaps: ties everywhere, and still the existing lists"""
    profiles, qs, ts = pac.tie_profiles(qa.TIE_ALPHA)
    for mode in rc.ALIGN_TYPES:
        for gi, ge in ((0, 1), (1, 5)):
            for p, t in zip(profiles[:3], ts[:3]):
                score, pl = qa.restated(p, t, mode, qg.constant(len(p), gi, ge), alpha=qa.TIE_ALPHA)
                want_score, want = pac.restated(p, t, qa.TIE_ALPHA, mode, gi, ge)
                assert score == want_score and np.array_equal(pl, want), (mode, gi, ge)


def gpu_sets():
    """(key, profiles, gaps, templates, alphabet) of the sets the GPU test compares with the restatement"""
    profiles, ts = qg.small_set()
    out = [("small-" + kind, profiles, qg.small_gaps(kind, profiles), ts, qg.ALPHA) for kind in qg.SMALL_KINDS]
    tp, _, tt, tg = qa.tie_set()
    out.append(("tie", tp, tg, tt, qa.TIE_ALPHA))
    return out


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_path_scorer_and_census_on_the_gpu_sets(mode):
    """every list's score by the path scorer equals the plane's, and the lists go through every case the census counts: the GPU
    tests cannot pass vacuously"""
    cen = qa.new_census()
    for key, profiles, gaps, ts, alpha in gpu_sets():
        ref = qa.reference_lists(key, profiles, gaps, ts, mode, alpha)
        for (r, c), (score, pl) in ref.items():
            qa.check_path(profiles[r], ts[c], mode, gaps[r], pl, score, alpha)
            qa.census(profiles[r], ts[c], mode, gaps[r], pl, cen, alpha)
    print("census", mode, cen)
    for k in qa.applies(mode):
        assert cen[k] > 0, (mode, k, cen)


def rows_liking(letters, hit=5, miss=-4):
    p = np.full((len(letters), qg.N), miss, np.int64)
    for i, ch in enumerate(letters):
        p[i, IDX[ch]] = hit
    return p


def test_worked_tie():
    p, t = rows_liking("CADE"), "ACDEF"
    g = qg.constant(4, 3, 1)
    H, gt = qa.planes(p, t, rc.SEMI_LOCAL, g)
    assert H[1:5, 1:6].tolist()[0] == [-4, 5, -4, -4, -4] and H[2, 1] == 5 and H[2, 2] == -8 and H[3, 3] == 7 and H[4, 4] == 12
    c = qa.candidates(H, gt, 3, 3)
    assert c == [(-8, (2, 2)), (2, (2, 1)), (2, (1, 2))] and qa.tied(c) and qa.pointer(H, gt, 3, 3) == (2, 1)
    score, pl = qa.restated(p, t, rc.SEMI_LOCAL, g)
    assert score == 12 and pl.tolist() == [[0, 0], [2, 1], [3, 3], [4, 4], [5, 6]]
    assert qa.path_score(p, t, rc.SEMI_LOCAL, g, pl) == 12
    g2 = [list(a) for a in g]
    g2[2][2] = 2                                               # ins_init[2]: the insertion is now strictly greater
    score, pl = qa.restated(p, t, rc.SEMI_LOCAL, g2)
    assert score == 13 and pl.tolist() == [[0, 0], [1, 2], [3, 3], [4, 4], [5, 6]]
    g3 = [list(a) for a in g]
    g3[0][2] = 4                                               # del_init[2]: the deletion falls behind
    score, pl = qa.restated(p, t, rc.SEMI_LOCAL, g3)
    assert score == 12 and pl.tolist() == [[0, 0], [1, 2], [3, 3], [4, 4], [5, 6]]
    # a wrong but self-consistent rule that priced the deletion by the row it ENTERS would not see the tie
    g4 = [list(a) for a in g]
    g4[0][3] = 9                                               # del_init[3] is not read by a gap that leaves row 2
    assert qa.restated(p, t, rc.SEMI_LOCAL, g4)[1].tolist() == [[0, 0], [2, 1], [3, 3], [4, 4], [5, 6]]


def test_final_pointer_cases():
    """the pairs the GPU test runs for the final cell's pointer do what they are built for"""
    cases = {what: (p, g, t, mode) for p, g, t, mode, what in qa.final_pointer_cases()}
    last = {}
    for what, (p, g, t, mode) in cases.items():
        score, pl = qa.restated(p, t, mode, g)
        assert qa.path_score(p, t, mode, g, pl) == score, what
        last[what] = (tuple(pl[-2]), len(p) + 2, len(t) + 2, score)
    cell, Q, T, score = last["del_row_Q-2"]
    assert cell == (Q - 2, 4) and score == 19                  # 4 matches, then 6 residues skipped at row Q-2's 1 / 0
    p, g, t, mode = cases["del_row_Q-2"]
    dear = [list(a) for a in g]
    dear[0][4] = dear[1][4] = 50                               # row Q-2 as dear as the rest: the tail costs 50 + 50 * 5
    assert qa.restated(p, t, mode, dear)[0] == 20 - 300
    other = [list(a) for a in g]
    other[0][3] = other[1][3] = 0                              # row Q-3's prices are not the tail deletion's
    assert qa.restated(p, t, mode, other)[0] == 19 and tuple(qa.restated(p, t, mode, other)[1][-2]) == cell
    a, b = last["ins_cheap"], last["ins_dear"]
    assert a[0][1] == a[2] - 2 and b[0][1] == b[2] - 2 and a[0][0] < a[1] - 2 and b[0][0] < b[1] - 2   # both insertions
    assert a[0] != b[0], (a, b)                                # ... and one ins_extn[p] moved the winner
    cell, Q, T, score = last["free_tail_tie"]
    assert cell == (2, T - 2)                                  # rows 2 and 4 tie: the smallest row
    p, g, t, mode = cases["free_tail_tie"]
    H, gt = qa.planes(p, t, mode, g)
    assert H[2, T - 2] == H[4, T - 2] > H[Q - 2, T - 2]
