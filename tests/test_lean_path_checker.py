"""No GPU: the checker the lean-rebuild GPU tests rely on (tests/lean_cases.py) against the oracle, and the precondition of their
gap rounds on the reference side alone.

check_local_list / reference_list restate Optimal's local walk on the int64 planes of range_cases.affine_reference.  Here they
are pinned to orc.dp_build + orc.optimal on every shape the oracle can build quickly, under every gap setting of ROUNDS; the
checker must refuse the oracle's list once it is damaged.  The rounds of the GPU tests mean something only if a score plane left
over from the previous setting is WRONG where a lean build does not write it: for every shape and every consecutive pair of
settings the two reference planes must differ in the sign of such a cell."""
import functools

import numpy as np
import pytest

import lean_cases as lc
import orc
import range_cases as rc
from aln_amd.synth import homolog_pair

ALPHA, BLOSUM = rc.load_blosum62()
SETTINGS = sorted(set(lc.ROUNDS))

# the maximum twice: in two rows (the first in row-major order wins), and in the seed as well (the seed wins)
TIES = {"tie_rows": ("WCWPPPPWCWPP", "WCW"), "tie_seed": ("WCW", "WCWPPPPWCW")}


@functools.lru_cache(maxsize=None)
def all_shapes():
    out = {"shape%02d_%dx%d" % (k, len(q), len(t)): (q, t) for k, (q, t) in enumerate(lc.shape_pairs(ALPHA))}
    out.update(lc.long_pairs(ALPHA, homolog_pair))
    return out


def oracle_shapes():
    out = {n: p for n, p in all_shapes().items() if lc.fits_oracle(*p)}
    out.update(TIES)
    out["hom300"] = homolog_pair(77, 300)
    out["empty_t"] = ("ACD", "")
    out["empty_both"] = ("", "")
    out["one_residue"] = ("W", "W")
    out["nothing_scores"] = ("PPP", "WWWW")
    return out


@functools.lru_cache(maxsize=None)
def reference(name, gi, ge):
    q, t = all_shapes()[name]
    S = rc.sim_int(q, t, ALPHA, BLOSUM)
    return S, rc.affine_reference(S, rc.LOCAL, gi, ge)[0]


@functools.lru_cache(maxsize=None)
def oracle(q, t, gi, ge):
    S = orc.sim_submatrix(q, t, ALPHA, BLOSUM)
    err, D, PQ, PT = orc.dp_build(S, orc.Gap(orc.LOCAL, gi, ge))
    assert err == 0
    err, sc, pl = orc.optimal(D, PQ, PT, True)
    assert err == 0
    Si = rc.sim_int(q, t, ALPHA, BLOSUM)
    H = rc.affine_reference(Si, rc.LOCAL, gi, ge)[0]
    assert np.array_equal(H.astype(np.float32), D)
    return Si, H, sc, pl


def refused(S, H, lst, gi, ge):
    try:
        lc.check_local_list(S, H, np.asarray(lst, np.int32).reshape(-1, 2), gi, ge)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", sorted(oracle_shapes()))
def test_checker_accepts_the_oracles_list(name):
    q, t = oracle_shapes()[name]
    for gi, ge in SETTINGS:
        S, H, sc, pl = oracle(q, t, gi, ge)
        assert H[lc.find_max_cell(H)] == sc or min(len(q), len(t)) == 0
        assert np.array_equal(lc.reference_list(H, gi, ge), pl), (name, gi, ge)
        lc.check_local_list(S, H, pl, gi, ge)


def test_find_max_cell_ties():
    for name, want in (("tie_rows", (3, 3)), ("tie_seed", (3, 10))):
        q, t = TIES[name]
        S, H, sc, pl = oracle(q, t, 11, 1)
        assert np.count_nonzero(H[1:-1, 1:-1] == H[1:-1, 1:-1].max()) == 2
        assert lc.find_max_cell(H) == want == tuple(pl[-2])
    H = np.zeros((6, 7), np.int64)
    assert lc.find_max_cell(H) == (4, 5)


def test_checker_refuses_damaged_lists():
    done = {"shift": 0, "drop_first": 0, "drop_first_aligned": 0, "other_max": 0, "origin_removed": 0, "origin_added": 0}
    for name, (q, t) in sorted(oracle_shapes().items()):
        for gi, ge in SETTINGS:
            S, H, sc, pl = oracle(q, t, gi, ge)
            L = [tuple(x) for x in pl.tolist()]
            Q, T = H.shape
            has_origin = L[0] == (0, 0)
            first = 1 if has_origin else 0                      # index of the first aligned cell
            n_aligned = len(L) - 1 - first
            if min(Q, T) > 2 and sc > 0:
                k = first + n_aligned // 2                      # one cell, one column to the right
                assert refused(S, H, L[:k] + [(L[k][0], L[k][1] + 1)] + L[k + 1:], gi, ge), (name, gi, ge, "shift", k)
                done["shift"] += 1
                assert refused(S, H, L[1:], gi, ge), (name, gi, ge, "drop_first")
                done["drop_first"] += 1
                if n_aligned >= 2:
                    assert refused(S, H, L[:first] + L[first + 1:], gi, ge), (name, gi, ge, "drop_first_aligned")
                    done["drop_first_aligned"] += 1
                best = H[1:Q - 1, 1:T - 1]
                others = [(int(i) + 1, int(j) + 1) for i, j in zip(*np.nonzero(best == best.max())) if (i + 1, j + 1) != L[-2]]
                for c in others[:2]:
                    assert refused(S, H, L[:-2] + [c, L[-1]], gi, ge), (name, gi, ge, "other_max", c)
                    done["other_max"] += 1
            if has_origin:
                assert refused(S, H, L[1:], gi, ge), (name, gi, ge, "origin_removed")
                done["origin_removed"] += 1
            else:
                assert refused(S, H, [(0, 0)] + L, gi, ge), (name, gi, ge, "origin_added")
                done["origin_added"] += 1
    print(done)
    assert all(v > 0 for v in done.values()), done


@pytest.mark.parametrize("name", sorted(all_shapes()))
def test_checker_accepts_the_reference_walk(name):
    """reference_list, which the pairs beyond the oracle's reach are compared with, passes the checker on every shape"""
    for gi, ge in SETTINGS:
        S, H = reference(name, gi, ge)
        lc.check_local_list(S, H, lc.reference_list(H, gi, ge), gi, ge)


@pytest.mark.parametrize("name", sorted(n for n, (q, t) in all_shapes().items() if len(q) >= 7))
def test_stale_planes_are_wrong_between_rounds(name):
    """A score plane left by the previous setting differs in sign from the right one in at least one interior cell that a lean
    build leaves alone (outside row Q-2, outside the chunk of column T-2): a reader of stale scores cannot pass the rounds."""
    for (a, b) in zip(lc.ROUNDS[:-1], lc.ROUNDS[1:]):
        n = lc.stale_sign_cells(reference(name, *a)[1], reference(name, *b)[1])
        print(name, a, b, n)
        assert n >= 1, (name, a, b)


def test_the_gap_jump_shapes_jump():
    """ins60 holds an insertion jump and del70 a deletion jump of at least 20 under at least one setting, del70's across column 1024"""
    ins = max(lc.longest_jumps(lc.reference_list(reference("ins60", gi, ge)[1], gi, ge))[1] for gi, ge in SETTINGS)
    dele = max(lc.longest_jumps(lc.reference_list(reference("del70", gi, ge)[1], gi, ge))[0] for gi, ge in SETTINGS)
    assert ins >= 20 and dele >= 20, (ins, dele)
    crossed = False
    for gi, ge in SETTINGS:
        p = lc.reference_list(reference("del70", gi, ge)[1], gi, ge)[1:-1]
        for (a, b) in zip(p[:-1], p[1:]):
            crossed |= bool(b[1] - a[1] > 20 and a[1] < 1024 <= b[1])
    assert crossed


def test_the_end_shape_ends_in_the_seed():
    for gi, ge in SETTINGS:
        H = reference("end700", gi, ge)[1]
        assert lc.find_max_cell(H) == (H.shape[0] - 2, H.shape[1] - 2) and H[-2, -2] > 0


def _round_batches():
    shapes = [n for n in sorted(all_shapes()) if n.startswith("shape")]
    return [("shapes", shapes)] + [("+".join(names), list(names)) for names in lc.LONG_BATCHES]


@pytest.mark.parametrize("batch", [b[0] for b in _round_batches()])
def test_a_reader_of_stale_scores_is_caught_in_every_batch(batch):
    """That stale cells differ somewhere is not enough: a walk has to meet one.  For every batch of the GPU rounds, with the plane
    the rounds really leave behind (lean_cases.stale_settings), a traceback that took its stop test from the score plane
    (lean_cases.stale_list) reports another list than Optimal for at least one pair in at least one lean round."""
    names = dict(_round_batches())[batch]
    has_short = any(lc.fits_oracle(*all_shapes()[n]) for n in names)
    caught = []
    for r, stale in lc.stale_settings(has_short).items():
        gi, ge = lc.ROUNDS[r]
        if stale is None or stale == (gi, ge):
            continue
        for n in names:
            if min(len(s) for s in all_shapes()[n]) == 0:
                continue
            H, Hs = reference(n, gi, ge)[1], reference(n, *stale)[1]
            if not np.array_equal(lc.reference_list(H, gi, ge), lc.stale_list(H, Hs, gi, ge)):
                caught.append((n, r))
    print(batch, caught)
    assert caught, batch
