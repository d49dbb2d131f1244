"""-m gpu: lean rebuilds (aln_batch_reevaluate -> dp_affine_tag_kernel<..., lean>, 2 B/cell) against the full build and the oracle.

A lean build writes flagged pointer words and, of the score plane, only what the corner kernel reads (row Q-2 and the chunk of
column T-2).  Optimal works on it as it is; every other reader gets the full planes back first (ensure_full).  The shapes put
column T-2 into every (wave, group) of the 2 x 2 x 8 layout and on their edges; the kernel is forced on these small pairs with the
dp_variant hints.  Every test that means to run the lean path asserts the kernel's name and 2 bytes per cell first."""
import numpy as np
import pytest

import aln_amd
import gpu_util
import orc
from lean_cases import SHAPES, VARIANT, assert_full, assert_lean, same_optimal
from aln_amd.synth import MT19937, homolog_pair, residues

pytestmark = pytest.mark.gpu

LOCAL = aln_amd.LOCAL
_ORACLE = {}


def oracle(blosum62, q, t, gi=11, ge=1):
    key = (q, t, gi, ge)
    if key not in _ORACLE:
        alpha, table = blosum62
        S = orc.sim_submatrix(q, t, alpha, table)
        rc, D, PQ, PT = orc.dp_build(S, orc.Gap(orc.LOCAL, gi, ge))
        assert rc == 0
        rc, sc, pl = orc.optimal(D, PQ, PT, True)
        assert rc == 0
        _ORACLE[key] = (S, D, PQ, PT, sc, pl)
    return _ORACLE[key]


def make_pair(seed, qlen, tlen, at_end):
    """template random; query = a noisy piece of it (one deletion) from its end or its middle, so the walk is long and, at the
    end, runs through column T-2"""
    g = MT19937(seed)
    t = residues(g, tlen)
    if qlen == 0:
        return "", t
    start = tlen - qlen if at_end else (tlen - qlen) // 2
    q = list(t[start:start + qlen])
    noise = residues(g, qlen)
    for k in range(3, qlen, 6):
        q[k] = noise[k]
    if qlen > 12:
        q = q[:qlen // 2] + q[qlen // 2 + 2:] + list(noise[:2])
    return "".join(q), t


# SHAPES (tests/lean_cases.py): column T-2 in every (wave, group) of the layout and on their edges.  The sequences of this file are
# its own (make_pair below draws them from MT19937; lean_cases.make_pair gives the same shapes a weak head instead)


def shape_pairs():
    out = []
    for k, (ql, T) in enumerate(SHAPES):
        out.append(("", "ACD") if (ql, T) == (0, 5) else make_pair(9100 + k, ql, T - 2, at_end=(k % 2 == 0)))
    return out


def lean_name_ok(name, full_name):
    return "lean" in name and name.replace(",lean", "") == full_name


def new_batch(pairs, blosum62, gi=11, ge=1, mode=LOCAL):
    alpha, table = blosum62
    b = aln_amd.Batch(gpu_util.ctx(), [p[0] for p in pairs], [p[1] for p in pairs])
    b.dp_submatrix(alpha, table, mode, gi, ge)
    return b


def check_against_oracle(blosum62, pairs, res, gi=11, ge=1):
    scores, lists, status = res
    for p, (q, t) in enumerate(pairs):
        S, D, PQ, PT, sc, pl = oracle(blosum62, q, t, gi, ge)
        assert status[p] == 0
        assert np.float32(scores[p]).view(np.uint32) == np.float32(sc).view(np.uint32), (p, scores[p], sc)
        assert np.array_equal(lists[p], pl), (p, len(q), len(t))


def check_cells(blosum62, b, pairs, gi=11, ge=1):
    for p, (q, t) in enumerate(pairs):
        S, D0, PQ0, PT0, sc, pl = oracle(blosum62, q, t, gi, ge)
        D, PQ, PT = b.get_cells(p)
        assert np.array_equal(D.view(np.uint32), D0.view(np.uint32)), p
        assert np.array_equal(PQ, PQ0) and np.array_equal(PT, PT0), p


def full_then_lean(blosum62, pairs, check_strings=True):
    """dp; optimal; reevaluate (lean); optimal -> checks (a), (b), (g) on one batch"""
    b = new_batch(pairs, blosum62)
    assert_full(b)
    full_name = b.kernel_name()
    full = b.optimal()
    full_str = b.optimal_strings() if check_strings else None
    b.reevaluate()
    assert_lean(b)
    assert lean_name_ok(b.kernel_name(), full_name), (b.kernel_name(), full_name)
    lean = b.optimal()
    same_optimal(lean, full)                                   # (a)
    check_against_oracle(blosum62, pairs, lean)
    if check_strings:                                          # (g)
        lean_str = b.optimal_strings()
        assert_lean(b)
        for x, y in zip(lean_str, full_str):
            assert np.array_equal(np.asarray(x), np.asarray(y))
    check_cells(blosum62, b, pairs)                            # (b): the full planes are back, bit for bit
    assert_full(b)
    assert b.kernel_name() == full_name
    same_optimal(b.optimal(), full)
    b.close()


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_each_shape_alone(k, blosum62):
    with gpu_util.ctx().hints(**VARIANT):
        full_then_lean(blosum62, [shape_pairs()[k]])


def test_ragged_batch(blosum62):
    with gpu_util.ctx().hints(**VARIANT):
        full_then_lean(blosum62, shape_pairs())


def test_homolog_700(blosum62):
    """the default dispatch picks the instantiation by itself beyond 1024 columns; 700 columns need the hints"""
    with gpu_util.ctx().hints(**VARIANT):
        full_then_lean(blosum62, [homolog_pair(4242, 700)])


def small_pairs():
    sp = shape_pairs()
    return [sp[3], sp[4], sp[7], sp[0]]


def test_enqueued_slots_survive_the_rebuild(blosum62):
    """optimal_enqueue -> lean reevaluate -> optimal_enqueue -> get_cells -> both collects"""
    pairs = small_pairs()
    with gpu_util.ctx().hints(**VARIANT):
        b = new_batch(pairs, blosum62)
        b.optimal_enqueue()
        b.reevaluate()
        assert_lean(b)
        b.optimal_enqueue()
        check_cells(blosum62, b, pairs)
        assert_full(b)
        for _ in range(2):
            sc, cnt, st = b.optimal_collect()
            for p, (q, t) in enumerate(pairs):
                want = oracle(blosum62, q, t)
                assert st[p] == 0 and sc[p] == want[4] and cnt[p] == len(want[5])
        b.close()


def test_enumerate_after_lean(blosum62):
    pairs = small_pairs()[:3]
    with gpu_util.ctx().hints(**VARIANT):
        fresh = new_batch(pairs, blosum62)
        b = new_batch(pairs, blosum62)
        b.optimal()
        b.reevaluate()
        assert_lean(b)
        for p, (q, t) in enumerate(pairs):
            flags = orc.make_subopt_regions(len(t) + 2, 3)
            want = fresh.enumerate(p, "cw", 5, 0.3, flags)
            got = b.enumerate(p, "cw", 5, 0.3, flags)
            assert_full(b)
            assert len(got) == len(want) and len(got) >= 1
            for g, w in zip(got, want):
                assert np.float32(g["score"]).view(np.uint32) == np.float32(w["score"]).view(np.uint32)
                assert np.array_equal(g["pairs"], w["pairs"])
        # the build was read: the next reevaluate is full, and one Optimal later it is lean again
        b.reevaluate()
        assert_full(b)
        b.optimal()
        b.reevaluate()
        assert_lean(b)
        b.close()
        fresh.close()


def test_enumerate_all_after_lean(blosum62):
    pairs = small_pairs()[:3]
    maxT = max(len(t) for _, t in pairs) + 2
    flags = np.zeros((len(pairs), maxT), dtype=np.uint8)
    for p, (q, t) in enumerate(pairs):
        flags[p, :len(t) + 2] = orc.make_subopt_regions(len(t) + 2, 3)
    with gpu_util.ctx().hints(**VARIANT):
        fresh = new_batch(pairs, blosum62)
        want = fresh.enumerate_all("cw", 5, 0.3, flags)
        b = new_batch(pairs, blosum62)
        b.optimal()
        b.reevaluate()
        assert_lean(b)
        got = b.enumerate_all("cw", 5, 0.3, flags)
        assert_full(b)
        n_out, scores, lengths, lists, status = got
        w_n, w_scores, w_lengths, w_lists, w_status = want
        assert np.array_equal(n_out, w_n) and np.array_equal(status, w_status) and (n_out >= 1).all()
        for p in range(len(pairs)):                    # (slots past n_out / rows past a list's length are not written)
            for k in range(n_out[p]):
                assert scores[p, k].view(np.uint32) == w_scores[p, k].view(np.uint32)
                assert lengths[p, k] == w_lengths[p, k]
                assert np.array_equal(lists[p, k, :lengths[p, k]], w_lists[p, k, :lengths[p, k]])
        b.close()
        fresh.close()


def test_set_gap_between_lean_builds(blosum62):
    """a lean build after another with different gaps: nothing of the earlier planes may be used"""
    pairs = small_pairs()
    with gpu_util.ctx().hints(**VARIANT):
        b = new_batch(pairs, blosum62)
        b.optimal()
        b.reevaluate()
        assert_lean(b)
        check_against_oracle(blosum62, pairs, b.optimal())
        b.set_gap(LOCAL, 5, 2)
        b.reevaluate()
        assert_lean(b)
        check_against_oracle(blosum62, pairs, b.optimal(), 5, 2)
        check_cells(blosum62, b, pairs, 5, 2)
        b.close()


def test_dp_sub_after_lean(blosum62):
    pairs = small_pairs()[:3]
    alpha, table = blosum62
    bounds = [(1, 1, len(q), len(t)) for q, t in pairs]
    with gpu_util.ctx().hints(**VARIANT):
        fresh = aln_amd.Batch(gpu_util.ctx(), [p[0] for p in pairs], [p[1] for p in pairs])
        fresh.dp_sub_submatrix(alpha, table, aln_amd.GLOBAL, 11, 1, aln_amd.FWD, bounds)
        want = fresh.optimal(subali=True)
        b = new_batch(pairs, blosum62)
        b.optimal()
        b.reevaluate()
        assert_lean(b)
        b.dp_sub_submatrix(alpha, table, aln_amd.GLOBAL, 11, 1, aln_amd.FWD, bounds)
        assert "lean" not in b.kernel_name()
        same_optimal(b.optimal(subali=True), want)
        for p in range(len(pairs)):
            for x, y in zip(b.get_cells(p), fresh.get_cells(p)):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        b.close()
        fresh.close()


def test_reevaluate_without_optimal_stays_full(blosum62):
    pairs = small_pairs()
    with gpu_util.ctx().hints(**VARIANT):
        b = new_batch(pairs, blosum62)
        b.reevaluate()
        assert_full(b)
        b.optimal()
        b.reevaluate()
        assert_lean(b)
        b.reevaluate()                         # the lean build served nobody
        assert_full(b)
        check_against_oracle(blosum62, pairs, b.optimal())
        b.optimal()
        b.corner_scores()                      # reads d_res only
        b.reevaluate()
        assert_lean(b)
        b.close()


def test_hint_values(blosum62):
    pairs = small_pairs()
    with gpu_util.ctx().hints(lean_reevaluate=0, **VARIANT):
        b = new_batch(pairs, blosum62)
        for _ in range(2):
            b.optimal()
            b.reevaluate()
            assert_full(b)
        check_against_oracle(blosum62, pairs, b.optimal())
        b.close()
    with gpu_util.ctx().hints(lean_reevaluate=2, **VARIANT):
        b = new_batch(pairs, blosum62)
        assert_full(b)                         # aln_batch_dp is never lean
        b.reevaluate()
        assert_lean(b)
        check_against_oracle(blosum62, pairs, b.optimal())
        check_cells(blosum62, b, pairs)
        b.close()


@pytest.mark.parametrize("occ", [2, 3])
@pytest.mark.parametrize("alt", [0, 1])
def test_occupancy_and_priority_variants(occ, alt, blosum62):
    pairs = shape_pairs()
    with gpu_util.ctx().hints(tag_occupancy=occ, tag_alt_prio=alt, **VARIANT):
        b = new_batch(pairs, blosum62)
        full = b.optimal()
        b.reevaluate()
        assert_lean(b)
        assert ("occ3" in b.kernel_name()) == (occ == 3)
        lean = b.optimal()
        same_optimal(lean, full)
        check_against_oracle(blosum62, pairs, lean)
        b.close()


@pytest.mark.parametrize("case", ["global", "h16", "key16", "dispatch"])
def test_ineligible_batches_stay_full(case, blosum62):
    pairs = small_pairs()[:2]                  # ld <= 1024: the default dispatch takes another instantiation
    hints = dict(VARIANT)
    mode, bpc = LOCAL, 4
    if case == "global":
        mode, bpc = aln_amd.GLOBAL, 6
    elif case == "h16":
        hints["h16"], bpc = 0, 6
    elif case == "key16":
        hints["key16"] = 0
    elif case == "dispatch":
        hints = {}
    alpha, table = blosum62
    with gpu_util.ctx().hints(lean_reevaluate=2, **hints):
        b = new_batch(pairs, blosum62, mode=mode)
        name = b.kernel_name()
        first = b.optimal()
        cells = [b.get_cells(p) for p in range(len(pairs))]
        b.optimal()
        b.reevaluate()
        assert_full(b, bpc)
        assert b.kernel_name() == name
        same_optimal(b.optimal(), first)
        for p in range(len(pairs)):
            for x, y in zip(b.get_cells(p), cells[p]):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        b.close()
