"""The reference of aln_hits_column_counts on its own (no GPU): the case sets show what the tally exists for — lists with
deletion and insertion jumps, positions passed opposite a gap — before any kernel is compared with them, and
aln_amd.pssm_from_counts is pinned on numbers worked out by hand."""
import numpy as np

import aln_amd
import column_count_cases as cc


def test_the_case_sets_meet_their_conditions():
    seen = cc.check_sets()
    print(seen)
    assert seen["del_jumps"] >= 1 and seen["ins_jumps"] >= 1 and seen["gap_rows"] >= 1


def test_the_tally_on_a_hand_made_list():
    # query ^AC$ ... of 4 residues, template of 5: entries (1,1) (2,2) (4,3) = a jump over query row 3, then the end (5,6)
    qs_len, ts = [4], ["ARNDC"]
    pl = np.array([[0, 0], [1, 1], [2, 2], [4, 3], [5, 6]], np.int32)
    counts, covered = cc.tally(qs_len, ts, [(0, 0), (0, 0)], [(7.0, pl), (0.0, pl)], [3, 5], local=True)
    want = np.zeros((6, cc.N), np.int64)
    want[1, cc.ALPHA.index("A")] = want[2, cc.ALPHA.index("R")] = want[4, cc.ALPHA.index("N")] = 3
    assert np.array_equal(counts[0], want)                            # the score-0 local slot adds nothing
    assert covered.tolist() == [0, 3, 3, 3, 3, 0]                     # row 3 is covered and counts nothing
    counts, covered = cc.tally(qs_len, ts, [(0, 0), (0, 0)], [(7.0, pl), (0.0, pl)], [3, 5], local=False)
    assert np.array_equal(counts[0], want * 8 // 3) and covered.tolist() == [0, 8, 8, 8, 8, 0]
    counts, covered = cc.tally(qs_len, ts, [(0, 0)], [(7.0, pl)], [0], local=False)
    assert not counts[0].any() and not covered.any()


def test_the_class_set_covers_every_class_and_both_routes():
    qs, ts = cc.class_set()
    assert tuple(len(q) for q in qs) == cc.Q_INTERIOR
    assert sorted(set(cc.class_of(t) for t in ts[:-1])) == list(range(1, 9)) and len(ts[-1]) == cc.LONG_T
    t, n = cc.class_hits()
    used = [int(t[r, k]) for r in range(len(n)) for k in range(n[r])]
    assert set(used) == set(range(len(ts))) and used.count(len(ts) - 1) == 2
    assert all(t[r, 3] == t[r, 0] for r in range(len(n))) and n[cc.LONG_ROW] == 5 and len(qs[cc.LONG_ROW]) == 63


def test_pssm_from_counts_on_a_hand_computed_example():
    # 3 x 4, uniform background, pseudo 1, scale 2.  Row 0: N = 2, (2 + .25) / (3 * .25) = 3 -> 2 log2 3 = 3.17 -> 3;
    # (0 + .25) / .75 = 1/3 -> -3.17 -> -3.  Row 1: N = 0 -> the fallback.  Row 2: N = 2, 1.25 / .75 = 5/3 -> 1.47 -> 1.
    counts = np.array([[2, 0, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0]])
    fallback = np.array([[9, 9, 9, 9], [4, -1, -2, 0], [9, 9, 9, 9]])
    got = aln_amd.pssm_from_counts(counts, [0.25] * 4, fallback)
    assert got.dtype == np.float32
    assert got.tolist() == [[3, -3, -3, -3], [4, -1, -2, 0], [1, 1, -3, -3]]
    # a skewed background and another scale: row 0, letter 0: (2 + .5) / (3 * .5) = 5/3 -> 3 log2(5/3) = 2.21 -> 2;
    # letter 1: (0 + .25) / (3 * .25) = 1/3 -> -4.75 -> -5; letters 2, 3 (bg .125): the same ratio 1/3 -> -5
    got = aln_amd.pssm_from_counts(counts, [0.5, 0.25, 0.125, 0.125], fallback, pseudo=1.0, scale=3.0)
    assert got[0].tolist() == [2, -5, -5, -5] and got[1].tolist() == [4, -1, -2, 0]
    assert np.array_equal(got, np.rint(got))


def test_pssm_rows_without_counts_keep_the_fallback():
    fallback = np.arange(8, dtype=np.float64).reshape(2, 4) - 3
    got = aln_amd.pssm_from_counts(np.zeros((2, 4), np.int32), [0.25] * 4, fallback)
    assert np.array_equal(got, fallback.astype(np.float32))
