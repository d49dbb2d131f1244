"""The reference of aln_hits_weights on its own (no GPU): the case sets hold what position-based weights exist for — positions
with three letters and repeated letters, rows whose slots weigh differently, the clamp to 1, a muted row, a duplicated slot,
counts that the weights change — a hand example with its raw values written out, and the numpy restatement
aln_amd.weights_from_pileup against the reference's integer loops."""
import numpy as np

import aln_amd
import column_count_cases as cc
import pileup_cases as pu
import range_cases as rc
import weight_cases as wc


def test_the_sets_meet_every_condition():
    seen = wc.check_sets()
    assert len(seen) == 3 * len(rc.ALIGN_TYPES) + 1
    for key, s in seen.items():
        print(key, s)
    assert seen[("muted", rc.LOCAL)]["muted_rows"] == 2


# three slots, four positions, alphabet AC
#   p0  A A .   n_A = 2, k = 1          A: 2^24 / 2 = 8388608
#   p1  A C C   n_A = 1, n_C = 2, k = 2 A: 2^24 / 2 = 8388608, C: 2^24 / 4 = 4194304
#   p2  C - C   n_C = 2, k = 1          C: 8388608
#   p3  . . A   n_A = 1, k = 1          A: 16777216
HAND = np.array([list(b"AAC."), list(b"AC-."), list(b".CCA")], np.uint8)
HAND_RAW = [8388608 + 8388608 + 8388608, 8388608 + 4194304, 4194304 + 8388608 + 16777216]


def test_the_hand_example():
    assert HAND_RAW == [25165824, 12582912, 29360128]
    for f in (wc.slot_weights, aln_amd.weights_from_pileup):
        w, raw = f(HAND, "AC", 1000)
        assert list(raw) == HAND_RAW and list(w) == [857, 428, 1000], f       # 1000 * 25165824 // 29360128 = 857
        w, raw = f(HAND, "AC", 1)
        assert list(w) == [1, 1, 1] and list(raw) == HAND_RAW                 # 0 < raw < M: clamped up to 1
        w, raw = f(HAND, "AC", 65535)
        assert list(w) == [56172, 28086, 65535]
        # a row of '.' and a row of NUL weigh nothing and change nothing
        more = np.concatenate([HAND, np.full((1, 4), ord("."), np.uint8), np.zeros((1, 4), np.uint8)])
        w, raw = f(more, "AC", 1000)
        assert list(raw) == HAND_RAW + [0, 0] and list(w) == [857, 428, 1000, 0, 0]
        # letters outside the alphabet never count
        w, raw = f(HAND, "C", 1000)
        assert list(raw) == [1 << 23, 1 << 23, 1 << 24] and list(w) == [500, 500, 1000]
        w, raw = f(np.full((2, 3), ord("."), np.uint8), "AC", 1000)
        assert list(w) == [0, 0] and list(raw) == [0, 0]
    w, raw = aln_amd.weights_from_pileup(HAND, "AC", 1000)
    assert w.dtype == np.int64 and raw.dtype == np.int64


def test_the_numpy_restatement_agrees_with_the_reference():
    for name in ("class", "homolog65"):
        qs, ts, t_idx, n_hits, _ = wc.sets()[name]
        q_lens = [len(q) for q in qs]
        for mode in (rc.LOCAL, rc.GLOBAL):
            lists = wc.set_lists(name, mode)
            for w_max in wc.W_MAXES:
                ref = wc.reference(q_lens, ts, t_idx, n_hits, lists, mode == rc.LOCAL, w_max)
                off = np.concatenate(([0], np.cumsum([n + 2 for n in q_lens])))
                for r, L in enumerate(q_lens):
                    mine = [s for s, (rr, k) in enumerate(ref["slots"]) if rr == r]
                    if not mine:
                        continue
                    rows = ref["letters"][mine]
                    w, raw = aln_amd.weights_from_pileup(rows, wc.ALPHA, w_max)
                    assert np.array_equal(w, ref["weights"][r, :len(mine)]) and np.array_equal(raw, ref["raw"][r, :len(mine)]), (name, mode, r)
                    counts, covered = aln_amd.counts_from_pileup(rows, wc.ALPHA, w)
                    assert np.array_equal(counts[:L], ref["counts"][r][1:-1]) and not counts[L:].any(), (name, mode, r)
                    assert np.array_equal(covered[:L], ref["covered"][off[r] + 1:off[r + 1] - 1]), (name, mode, r)
