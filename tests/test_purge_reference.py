"""The reference of aln_hits_purge on its own (no GPU): the case sets hold what purging exists for — a slot purged at 90 % and
kept at 100 %, an exact duplicate, a slot near a purged slot only (kept), a slot near two kept slots (the smaller keeps it), a
slot the overlap bound decides, rows in which nothing and in which everything but slot 0 is purged, weights that the purge
changes — the header's hand example with both parameter pairs, and the numpy restatement aln_amd.purge_from_pileup against the
reference's integer loops."""
import numpy as np

import aln_amd
import purge_cases as pg
import range_cases as rc


def test_the_sets_meet_every_condition():
    seen = pg.check_sets()
    assert len(seen) == len(rc.ALIGN_TYPES)
    for key, s in seen.items():
        print(key, s)


def test_the_hand_example():
    for (max_identity, min_overlap), want in pg.HAND_RECORDS.items():
        assert pg.slot_purge(pg.HAND, "AC", max_identity, min_overlap) == want
        keeper, same, overlap, letters = aln_amd.purge_from_pileup(pg.HAND, "AC", max_identity, min_overlap)
        assert all(x.dtype == np.int64 for x in (keeper, same, overlap, letters))
        assert list(zip(keeper.tolist(), same.tolist(), overlap.tolist(), letters.tolist())) == want
    # row 2 against row 0: 2 of 3 equal, 200 < 225 — kept at 75, and at 66 purged by row 0
    assert pg.slot_purge(pg.HAND, "AC", 66, 50)[2] == (0, 2, 3, 3)
    # 101 can never be met; rows of '.', '-' and NUL show no letter; letters outside the alphabet are none
    assert [r[0] for r in pg.slot_purge(pg.HAND, "AC", 101, 0)] == [0, 1, 2, 3]
    more = np.concatenate([pg.HAND, np.array([list(b".-.-."), [0] * 5], np.uint8), pg.HAND[:1]])
    for f in (lambda *a: pg.slot_purge(*a), lambda *a: list(zip(*(x.tolist() for x in aln_amd.purge_from_pileup(*a))))):
        got = f(more, "AC", 100, 50)
        assert got == pg.HAND_RECORDS[(100, 50)] + [(-1, 0, 0, 0), (-1, 0, 0, 0), (0, 5, 5, 5)]
        assert f(pg.HAND, "C", 100, 0) == [(0, 0, 0, 2), (0, 1, 1, 1), (0, 1, 1, 1), (0, 1, 1, 1)]
        # min_overlap: row 3 shows 2 letters, both under row 0's; row 0 under 100 needs all 5 of its letters under the keeper
        assert f(pg.HAND[[3, 0]], "AC", 50, 100) == [(0, 0, 0, 2), (1, 0, 0, 5)]
        assert f(pg.HAND[[3, 0]], "AC", 50, 40) == [(0, 0, 0, 2), (0, 2, 2, 5)]


def test_the_numpy_restatement_agrees_with_the_reference():
    for name in pg.sets():
        qs, ts, t_idx, n_hits, _ = pg.sets()[name]
        for mode in (rc.LOCAL, rc.GLOBAL):
            for par in pg.PARAMS:
                ref = pg.set_reference(name, mode, *par)
                for r in range(len(qs)):
                    mine = [s for s, (rr, k) in enumerate(ref["slots"]) if rr == r]
                    if not mine:
                        continue
                    got = aln_amd.purge_from_pileup(ref["all_letters"][mine], pg.ALPHA, *par)
                    assert np.array_equal(np.stack(got, axis=1), ref["purge"][r, :len(mine)]), (name, mode, par, r)
                    # the survivors' weights: weights_from_pileup over the rows muted as the definition says
                    muted = ref["all_letters"][mine].copy()
                    muted[got[0] != np.arange(len(mine))] = ord(".")
                    w, raw = aln_amd.weights_from_pileup(muted, pg.ALPHA, pg.W_MAX)
                    assert np.array_equal(w, ref["weights"][r, :len(mine)]) and np.array_equal(raw, ref["raw"][r, :len(mine)])
