"""The reference of tests/test_gpu_qprofile_search.py (tests/profile_cases.py), pinned on the CPU: the plane of a profile
derived from a sequence is the sequence's own similarity plane, and the int64 recurrence over a position-specific plane agrees
with the oracle's build and traceback (orc.dp_build + orc.optimal) on the same plane.  No GPU."""
import numpy as np
import pytest

import orc
import profile_cases as pc
import range_cases as rc
import search_cases as sc

PAIRS = [(7, "blosum62", 11, 1), (16, "blosum62x-1", 1, 5), (33, "identity5", 40, 0)]     # (rows, table, gi, ge)


def test_the_plane_of_a_derived_profile_is_the_sequence_plane():
    for name in ("blosum62", "blosum62x-1", "constant+3"):
        table = sc.TABLES[name]
        qs, ts = sc.sequences(sc.Case("small", None, 0, 0, 40, 57))
        for q, p in zip(qs, pc.derived(qs, table)):
            assert p.shape == (len(q), pc.N)
            for t in ts[:8]:
                assert np.array_equal(pc.plane(p, t), rc.sim_int(q, t, pc.ALPHA, table)), (name, q, t)


def test_plane_sentinels_and_gather():
    p = np.arange(3 * pc.N, dtype=np.int64).reshape(3, pc.N)
    t = pc.ALPHA[5] + pc.ALPHA[0] + pc.ALPHA[5]
    S = pc.plane(p, t)
    assert S.shape == (5, 5) and not S[0].any() and not S[-1].any() and not S[:, 0].any() and not S[:, -1].any()
    assert S[1:-1, 1:-1].tolist() == [[5, 0, 5], [pc.N + 5, pc.N, pc.N + 5], [2 * pc.N + 5, 2 * pc.N, 2 * pc.N + 5]]
    assert pc.plane(np.zeros((0, pc.N)), t).shape == (2, 5) and pc.plane(p, "").shape == (5, 2)


def test_perturbed_rows_are_position_specific():
    """the perturbed sets are not expressible as a residue string: some row equals no table row"""
    profiles, _ = pc.length_set()
    table = np.asarray(sc.TABLES[pc.LENGTH_SYSTEM[0]]).astype(np.int64)
    assert [len(p) for p in profiles[:len(pc.INTERIOR_ROWS)]] == list(pc.INTERIOR_ROWS)
    for p in profiles[:len(pc.INTERIOR_ROWS)]:
        assert all(not (table == row).all(axis=1).any() for row in p)
        assert np.abs(p - pc.derived([rc.random_seq(pc.ALPHA, 300 + len(p), len(p))], table)[0]).max() <= 6 if len(p) else True
    assert (profiles[-2][23] == table.max()).all() and (np.delete(profiles[-2], 23, axis=0) < 0).all()
    assert not profiles[-1].any()


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_reference_equals_the_oracle(mode):
    """three small pairs per align type: score and, local, the end cell (the entry before the closing pair of Optimal's list)"""
    for rows, tname, gi, ge in PAIRS:
        prof = pc.perturbed([rc.random_seq(pc.ALPHA, 600 + rows, rows)], sc.TABLES[tname], 17)[0]
        t = rc.random_seq(pc.ALPHA, 700 + rows, rows + 9)
        score, end = pc.pair_reference(prof, t, mode, gi, ge)
        err, D, PQ, PT = orc.dp_build(pc.plane(prof, t).astype(np.float32), orc.Gap(mode, gi, ge))
        err2, sc0, pl = orc.optimal(D, PQ, PT, mode == rc.LOCAL)
        assert err == 0 and err2 == 0
        assert float(score) == float(sc0), (rows, tname, mode)
        if mode == rc.LOCAL:
            assert tuple(int(v) for v in pl[-2]) == end, (rows, tname)
        else:
            assert end == (rows + 1, len(t) + 1)
