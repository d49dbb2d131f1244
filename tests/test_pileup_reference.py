"""The reference of aln_hits_pileup on its own (no GPU): the case sets hold what a pileup exists for — deletion and insertion
jumps, '-' and '.' positions, never a double jump — a hand example, and the two numpy helpers on a hand-made row."""
import numpy as np

import aln_amd
import pileup_cases as pu
import range_cases as rc


def test_the_sets_hold_jumps_gaps_and_unaligned_positions():
    seen = pu.check_sets()
    assert len(seen) == 2 * len(rc.ALIGN_TYPES)
    for key, s in seen.items():
        print(key, s)
        assert s["double_jumps"] == 0 and min(s["del_jumps"], s["ins_jumps"], s["dashes"], s["dots"]) >= 1, (key, s)


HAND_Q, HAND_T = "PAWHEAE", "HEAGAWGHEE"
HAND_LIST = np.array([(0, 0), (2, 5), (3, 6), (4, 7), (5, 8), (6, 9), (7, 10), (8, 11)], np.int32)


def test_the_hand_example():
    letters, tpos, spans = pu.pileup([len(HAND_Q)], [HAND_T], [(0, 0)], [(28.0, HAND_LIST)], True, 9)
    assert letters[0].tobytes() == b".AWGHEE\0\0"
    assert tpos[0].tolist() == [0, 5, 6, 7, 8, 9, 10, 0, 0]
    assert spans[0].tolist() == [2, 7, 5, 10]
    # a local score of 0: the seed cell's list is no alignment
    letters, tpos, spans = pu.pileup([len(HAND_Q)], [HAND_T], [(0, 0)], [(0.0, HAND_LIST)], True, 7)
    assert letters[0].tobytes() == b"......." and not tpos.any() and spans[0].tolist() == [0, 0, 0, 0]
    # ... but under a non-local type it is one
    letters, tpos, spans = pu.pileup([len(HAND_Q)], [HAND_T], [(0, 0)], [(0.0, HAND_LIST)], False, 7)
    assert letters[0].tobytes() == b".AWGHEE" and spans[0].tolist() == [2, 7, 5, 10]


def test_the_helpers_on_a_hand_made_row():
    # query of 7 positions; template ACDEFGHIK: (2,1) (3,2) then an insert of template 3..4, (4,5), query 5 opposite a gap, (6,6)
    template = "ACDEFGHIK"
    line = np.frombuffer(b".ACF-G.\0", np.uint8)
    tpos = np.array([0, 1, 2, 5, 0, 6, 0, 0], np.uint16)
    assert aln_amd.a3m_from_pileup(template, line[:7], tpos[:7]) == "-ACdeF-G-"
    a3m = aln_amd.a3m_from_pileup(template, line[:7], tpos[:7])
    assert len([c for c in a3m if not c.islower()]) == 7
    assert a3m.replace("-", "").upper() == template[0:6]
    other = np.frombuffer(b"..CF.\0\0\0", np.uint8)                    # a shorter range; '.' is no coverage
    alphabet = "ACFG"
    counts, covered = aln_amd.counts_from_pileup(np.stack([line, other]), alphabet)
    assert counts.dtype == np.int64 and counts.shape == (8, 4) and covered.dtype == np.int64
    assert counts.tolist() == [[0, 0, 0, 0], [1, 0, 0, 0], [0, 2, 0, 0], [0, 0, 2, 0], [0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert covered.tolist() == [0, 1, 2, 2, 1, 1, 0, 0]
    counts, covered = aln_amd.counts_from_pileup(np.stack([line, other]), alphabet, weights=[3, 5])
    assert counts[2].tolist() == [0, 8, 0, 0] and covered.tolist() == [0, 3, 8, 8, 3, 3, 0, 0]
