"""-m gpu: hmap2_sim_kernel, hmap2_stats_kernel and hmap2_apply_kernel (csrc/sim_hmap2.hip) off the default parameters and off
the few shapes the other suites use — tests/hmap2_cases.py builds the inputs, tests/test_hmap2_reference.py pins the oracle they
are judged against to the real reference.  Everything is compared bit for bit (uint32 patterns); the only allowance is
hmap2_cases.same_bits_or_nan on planes the oracle itself makes NaN."""
import numpy as np
import pytest

import aln_amd
import gpu_util
import hmap2_cases as hc
from test_oracle_profile import inputs, load_profile_cases

pytestmark = pytest.mark.gpu

D = hc.DEFAULTS


def build(ctx, rg, mode, params=None, normalize=True):
    """one dp_hmap2 launch over a hmap2_cases.Ragged batch -> (Batch, tgi, tge over the template pool)"""
    pr = D if params is None else params
    qs, ts = rg.strings()
    qpool, tpool = rg.pools()
    b = aln_amd.Batch(ctx, qs, ts, rg.q_idx, rg.t_idx)
    tgi, tge = b.dp_hmap2(qpool, tpool, mode, pr["gi"], pr["ge"], pr["alpha"], pr["beta"], pr["zero_shift"], normalize)
    return b, tgi, tge


def build_own(ctx, items, mode, params=None, normalize=True, alpha=None):
    """the same for pairs that share nothing: items = [(qp, tp), ...]"""
    pr = D if params is None else params
    qs, ts, qpool, tpool = hc.own_pools(items)
    b = aln_amd.Batch(ctx, qs, ts)
    tgi, tge = b.dp_hmap2(qpool, tpool, mode, pr["gi"], pr["ge"], pr["alpha"] if alpha is None else alpha, pr["beta"],
                          pr["zero_shift"], normalize)
    return b, tgi, tge


def assert_pair(b, p, ref, optimal, where):
    """S, D, PQ, PT and (optimal = b.optimal()'s result, or None) the optimal score and list of pair p against the oracle's"""
    assert hc.bits_equal(b.get_sim(p), ref["S"]), ("S",) + where
    Dp, PQ, PT = b.get_cells(p)
    assert hc.bits_equal(Dp, ref["D"]), ("D",) + where
    assert np.array_equal(PQ, ref["PQ"]) and np.array_equal(PT, ref["PT"]), ("P",) + where
    if optimal is not None:
        scores, lists, status = optimal
        assert status[p] == 0 and ref["status"] == 0, ("status",) + where
        assert np.float32(scores[p]).view(np.uint32) == ref["score"].view(np.uint32), ("score",) + where
        assert np.array_equal(lists[p], ref["pairs"]), ("list",) + where


@pytest.mark.parametrize("mode", [1, 3, 4])
def test_shapes_against_the_oracle(mode):
    """The whole ragged batch in one launch: T one below, at and one above 256, 512 and 1024 (the sim kernel's column blocks and
    the apply kernel's), 1030; Q around 16, 32 and 64 (the row chunks); statistics chains of exactly 63 .. 1025 cells; pairs far
    smaller than maxQ, maxT and maxld — then once more in reversed order, which moves the pair that owns maxld."""
    ctx = gpu_util.ctx()
    sb = hc.shape_batch()
    results = []
    for rg in (sb, sb.reversed()):
        b, tgi, tge = build(ctx, rg, mode)
        assert "dp_exact" in b.kernel_name()
        opt = b.optimal()
        toff = np.concatenate([[0], np.cumsum([n + 2 for n in rg.tlens])])
        for p in range(len(rg.pairs)):
            qp, tp = rg.profiles(p)
            ref = hc.reference(rg.key(p), qp, tp, mode)
            assert not np.isnan(ref["S"]).any()
            t0 = toff[rg.t_idx[p]]
            assert hc.bits_equal(tgi[t0:t0 + len(ref["tgi"])], ref["tgi"]) and hc.bits_equal(tge[t0:t0 + len(ref["tge"])], ref["tge"])
            assert_pair(b, p, ref, opt, (mode, rg.pairs[p], rg is sb))
        results.append((opt[0].copy(), [b.get_sim(p) for p in range(len(rg.pairs))]))
        b.close()
    n = len(sb.pairs)
    assert hc.bits_equal(results[0][0], results[1][0][::-1].copy())
    assert all(hc.bits_equal(results[0][1][p], results[1][1][n - 1 - p]) for p in range(n))


_PARAM_ITEMS = {}


def param_items():
    """-> [(key, qp, tp)]: the 19 x 14 and the 66 x 72 inputs of tests/golden/profile_cases.npz and one 40 x 300 pair"""
    if not _PARAM_ITEMS:
        _, z = load_profile_cases()
        for key in ("in02", "in04"):
            _PARAM_ITEMS[key] = inputs(z, key)
        _PARAM_ITEMS["40x300"] = (hc.query_profile(38), hc.template_profile(298))
    return [(k,) + v for k, v in _PARAM_ITEMS.items()]


@pytest.mark.parametrize("params", sorted(hc.PARAMS))
def test_parameter_sets(params):
    pr = hc.PARAMS[params]
    items = param_items()
    assert [(len(q["conf"]), len(t["conf"])) for _, q, t in items] == [(19, 14), (66, 72), (40, 300)]
    for mode in (1, 3):
        b, tgi, tge = build_own(gpu_util.ctx(), [(q, t) for _, q, t in items], mode, pr)
        opt = b.optimal()
        t0 = 0
        for p, (key, qp, tp) in enumerate(items):
            ref = hc.reference(("param", key), qp, tp, mode, pr)
            n = len(ref["tgi"])
            assert hc.bits_equal(tgi[t0:t0 + n], ref["tgi"]) and hc.bits_equal(tge[t0:t0 + n], ref["tge"]), (params, key)
            t0 += n
            assert_pair(b, p, ref, opt, (params, mode, key))
        b.close()


def test_parameter_sets_against_the_goldens():
    """the 19 x 14 pair of test_parameter_sets against the real reference's own planes (no oracle in between)"""
    from test_hmap2_reference import load_param_cases
    meta, z = load_param_cases()
    _, zin = load_profile_cases()
    qp, tp = inputs(zin, "in02")
    for m in meta:
        if m["inputs"] != "in02":
            continue
        b, tgi, tge = build_own(gpu_util.ctx(), [(qp, tp)], m["mode"], hc.PARAMS[m["params"]])
        name = m["name"]
        assert hc.bits_equal(tgi, z[name + "/TGI"]) and hc.bits_equal(tge, z[name + "/TGE"]), name
        assert hc.bits_equal(b.get_sim(0), z[name + "/S"]), name
        Dp, PQ, PT = b.get_cells(0)
        assert hc.bits_equal(Dp, z[name + "/H"]) and np.array_equal(PQ, z[name + "/PQ"]) and np.array_equal(PT, z[name + "/PT"]), name
        scores, lists, status = b.optimal()
        assert status[0] == 0 and int(np.float32(scores[0]).view(np.uint32)) == m["opt"]["score"], name
        assert lists[0].reshape(-1).tolist() == m["opt"]["pairs"], name
        b.close()


UNNORMALISED = ((3, 1028), (16, 64), hc.WIDE, (40, 5))


def test_unnormalised_planes():
    """normalize = False: only hmap2_sim_kernel runs, no max|S| is left with the plane, and the tiled exact kernel (a template
    of 1030 columns is in the batch) has to take its rounding margin from plane_absmax_kernel."""
    ctx = gpu_util.ctx()
    rg = hc.Ragged(UNNORMALISED)
    assert set(UNNORMALISED) <= set(hc.SHAPE_PAIRS)
    for mode in (1, 3):
        b, tgi, tge = build(ctx, rg, mode, normalize=False)
        assert "dp_exact_tiled" in b.kernel_name()
        opt = b.optimal()
        for p in range(len(rg.pairs)):
            qp, tp = rg.profiles(p)
            ref = hc.reference(rg.key(p), qp, tp, mode, normalize=False)
            assert hc.bits_equal(ref["S"], hc.sim_reference(rg.key(p), qp, tp, D["alpha"], None))
            assert_pair(b, p, ref, opt, (mode, rg.pairs[p]))
        b.close()


def test_a_raw_build_forgets_the_last_normalised_max():
    """One resident batch, built normalised from a query whose flat sse triple makes the wide pair's plane (and the max|S| that
    hmap2_apply_kernel leaves with it) NaN, then built again with normalize = False from ordinary profiles: the second build must
    not prune with the first one's max|S|.  The planes are the oracle's, and the tiled kernel's chunk counters (hint exact_debug;
    they repeat exactly from build to build) are those of a fresh batch."""
    ctx = gpu_util.ctx()
    rg = hc.Ragged(ABSMAX)
    qs, ts = rg.strings()
    qpool, tpool = rg.pools()
    flat = {k: v.copy() for k, v in qpool.items()}
    q0 = sum(n + 2 for n in rg.qlens[:rg.qlens.index(hc.WIDE[0])])
    flat["sse"][q0 + 4] = 0.5
    wide = rg.pairs.index(hc.WIDE)
    with ctx.hints(exact_debug=1):
        for mode in (1, 3):
            fresh, _, _ = build(ctx, rg, mode, normalize=False)
            want = fresh.last_exact_stats()
            fresh.close()
            b = aln_amd.Batch(ctx, qs, ts, rg.q_idx, rg.t_idx)
            b.dp_hmap2(flat, tpool, mode, D["gi"], D["ge"], D["alpha"], D["beta"], D["zero_shift"], True)
            assert np.isnan(b.get_sim(wide)[1:-1, 1:-1]).all()
            b.dp_hmap2(qpool, tpool, mode, D["gi"], D["ge"], D["alpha"], D["beta"], D["zero_shift"], False)
            assert "dp_exact_tiled" in b.kernel_name()
            assert want[1] > 0 and b.last_exact_stats() == want, (mode, b.last_exact_stats(), want)
            for p in range(len(rg.pairs)):
                qp, tp = rg.profiles(p)
                assert_pair(b, p, hc.reference(rg.key(p), qp, tp, mode, normalize=False), None, (mode, rg.pairs[p]))
            b.close()


def test_exp_argument_bands():
    """alpha = 105 on confidences near 1: exp() arguments below -103.98 (+0), down to -88 and between -88 and -87.34 (denormal),
    ordinary, in [88, 88.7228] (large finite) and above (+inf) — glibc's expf over its whole range, bit for bit."""
    qp, tp = hc.exp_sweep()
    b, _, _ = build_own(gpu_util.ctx(), [(qp, tp)], 1, normalize=False, alpha=hc.EXP_ALPHA)
    S = b.get_sim(0)
    b.close()
    ref = hc.sim_reference("exp_sweep", qp, tp, hc.EXP_ALPHA, None)
    masks = hc.exp_band_masks(hc.exp_arguments(qp, tp, hc.EXP_ALPHA))
    differ = S.view(np.uint32) != ref.view(np.uint32)
    per_band = {k: "%d of %d" % (int((differ & m).sum()), int(m.sum())) for k, m in masks.items()}
    if differ.any():
        print("cells that differ from the oracle, per band of the exp() argument:", per_band)
    assert not differ.any(), per_band


@pytest.mark.parametrize("normalize", [True, False])
def test_degenerate_profiles(normalize):
    """Flat sse triples, interiors of one cell, one row and one column, pairs without interior, zero confidences: the planes
    are the oracle's, NaN where the oracle's are, and the call succeeds (dp_hmap2 raises on anything but ALN_OK)."""
    cases = hc.degenerate_cases()
    for c in cases:
        b, tgi, tge = build_own(gpu_util.ctx(), [(c["qp"], c["tp"])], 1, normalize=normalize, alpha=c["alpha"])
        ref = hc.sim_reference(("deg", c["name"]), c["qp"], c["tp"], c["alpha"], D["zero_shift"] if normalize else None)
        S = b.get_sim(0)
        assert hc.same_bits_or_nan(S, ref), c["name"]
        assert int(np.isnan(S).sum()) == (c["nan_norm"] if normalize else c["nan_raw"]), c["name"]
        gi0, ge0 = hc.gap_reference(("deg", c["name"]), c["tp"], D["gi"], D["ge"], D["beta"])
        assert hc.bits_equal(tgi, gi0) and hc.bits_equal(tge, ge0), c["name"]
        if not np.isnan(ref).any():
            r = hc.reference(("deg", c["name"]), c["qp"], c["tp"], 1, hc.params_with(alpha=c["alpha"]), normalize)
            assert_pair(b, 0, r, None, (c["name"], normalize))
        b.close()
    # and all of them in one launch
    b, _, _ = build_own(gpu_util.ctx(), [(c["qp"], c["tp"]) for c in cases if c["alpha"] == D["alpha"]], 1, normalize=normalize)
    for p, c in enumerate(c for c in cases if c["alpha"] == D["alpha"]):
        ref = hc.sim_reference(("deg", c["name"]), c["qp"], c["tp"], c["alpha"], D["zero_shift"] if normalize else None)
        assert hc.same_bits_or_nan(b.get_sim(p), ref), c["name"]
    b.close()


NEIGHBOURS = ((16, 64), (30, 1021), (40, 5), (25, 41))


@pytest.mark.parametrize("mode", [1, 3])
def test_a_nan_pair_leaves_its_neighbours_alone(mode):
    """Two pairs whose normalised planes are NaN (a flat sse triple; an interior of one cell) at positions 0 and 3 of a batch of
    six: the other four are the oracle's, and what the same four give in a batch of their own."""
    ctx = gpu_util.ctx()
    assert set(NEIGHBOURS) <= set(hc.SHAPE_PAIRS)
    ordinary = [(hc.query_profile(q), hc.template_profile(t)) for q, t in NEIGHBOURS]
    nan_a, nan_b = hc.degenerate("flat_half"), hc.degenerate("one_cell")
    mixed = [(nan_a["qp"], nan_a["tp"]), ordinary[0], ordinary[1], (nan_b["qp"], nan_b["tp"]), ordinary[2], ordinary[3]]
    where = (1, 2, 4, 5)
    alone, _, _ = build_own(ctx, ordinary, mode)
    both, _, _ = build_own(ctx, mixed, mode)
    assert np.isnan(both.get_sim(0)[1:-1, 1:-1]).all() and np.isnan(both.get_sim(3)[1, 1])
    opt_alone, opt_both = alone.optimal(), both.optimal()
    for k, (q, t) in enumerate(NEIGHBOURS):
        ref = hc.reference(("shape", q, t), ordinary[k][0], ordinary[k][1], mode)
        assert_pair(both, where[k], ref, opt_both, (mode, (q, t), "beside NaN pairs"))
        assert_pair(alone, k, ref, opt_alone, (mode, (q, t), "alone"))
        assert hc.bits_equal(both.get_sim(where[k]), alone.get_sim(k))
        for x, y in zip(both.get_cells(where[k]), alone.get_cells(k)):
            assert hc.bits_equal(x, y)
        assert opt_both[2][where[k]] == 0
    alone.close()
    both.close()


ABSMAX = (hc.WIDE, (3, 1028), (40, 5))


def test_both_absmax_routes_build_the_same_planes():
    """max|S| for the pruned exact kernel's rounding margin comes from hmap2_apply_kernel (dp_hmap2) or from plane_absmax_kernel
    (planes a caller uploads): both routes, with and without pruning, build the oracle's planes."""
    ctx = gpu_util.ctx()
    rg = hc.Ragged(ABSMAX)
    assert set(ABSMAX) <= set(hc.SHAPE_PAIRS)
    qs, ts = rg.strings()
    for mode in (1, 3):
        built, counters = {}, {}
        for prune in (1, 0):
            with ctx.hints(exact_prune=prune, exact_debug=1):
                b, tgi, tge = build(ctx, rg, mode)
                assert "dp_exact_tiled" in b.kernel_name()
                planes = [b.get_sim(p) for p in range(len(rg.pairs))]
                built[("hmap2", prune)] = [b.get_cells(p) for p in range(len(rg.pairs))]
                counters[("hmap2", prune)] = b.last_exact_stats()
                b.close()
                b = aln_amd.Batch(ctx, qs, ts, rg.q_idx, rg.t_idx)
                b.dp_simmatrix(planes, mode, 0, 0, tgi=tgi, tge=tge)
                assert "dp_exact_tiled" in b.kernel_name()
                built[("simmatrix", prune)] = [b.get_cells(p) for p in range(len(rg.pairs))]
                counters[("simmatrix", prune)] = b.last_exact_stats()
                b.close()
        # far chunks tested / skipped: the counters repeat exactly from build to build, so both routes' max|S| must give the same
        assert counters[("hmap2", 1)] == counters[("simmatrix", 1)] and counters[("hmap2", 1)][1] > 0, counters
        assert counters[("hmap2", 0)] == counters[("simmatrix", 0)] and counters[("hmap2", 0)][1] == 0, counters
        for p in range(len(rg.pairs)):
            qp, tp = rg.profiles(p)
            ref = hc.reference(rg.key(p), qp, tp, mode)
            assert hc.bits_equal(planes[p], ref["S"])
            for route, cells in built.items():
                assert hc.bits_equal(cells[p][0], ref["D"]), (mode, route, rg.pairs[p])
                assert np.array_equal(cells[p][1], ref["PQ"]) and np.array_equal(cells[p][2], ref["PT"]), (mode, route, rg.pairs[p])
