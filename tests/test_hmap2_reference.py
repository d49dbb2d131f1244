"""The oracle's Hmap2Eval path off the default parameters, pinned to the REAL reference before tests/test_gpu_hmap2_ranges.py
judges the device against it, and the construction of tests/hmap2_cases.py's inputs.  CPU only.

tests/golden/profile_param_cases.* come from oracle/gen_golden.py (gen_profile_params) through oracle/_ref/ref_profile: every
parameter set of hmap2_cases.PARAMS on the 5 x 11 and the 19 x 14 inputs of profile_cases.npz, global and local."""
import json
import os

import numpy as np

import hmap2_cases as hc
import orc
from test_oracle_profile import GOLD, inputs, load_profile_cases


def load_param_cases():
    meta = json.load(open(os.path.join(GOLD, "profile_param_cases.json")))["cases"]
    z = np.load(os.path.join(GOLD, "profile_param_cases.npz"), allow_pickle=False)
    return meta, z


def test_goldens_cover_every_parameter_set():
    meta, z = load_param_cases()
    assert {(m["inputs"], m["params"], m["mode"]) for m in meta} == {(i, p, m) for i in ("in01", "in02") for p in hc.PARAMS for m in (1, 3)}
    for m in meta:
        pr = hc.PARAMS[m["params"]]
        assert all(m[k] == pr[k] for k in pr) and m["dir"] == 1
    _, zin = load_profile_cases()
    assert zin["in01/q_conf"].shape == (5,) and zin["in01/t_conf"].shape == (11,)
    assert zin["in02/q_conf"].shape == (19,) and zin["in02/t_conf"].shape == (14,)
    here = os.path.getsize(os.path.join(GOLD, "profile_param_cases.npz")) + os.path.getsize(os.path.join(GOLD, "profile_param_cases.json"))
    assert 2 * here < os.path.getsize(os.path.join(GOLD, "profile_cases.npz"))
    # every alpha, shift and gap set moves the golden it is meant to move (a generator that dropped a parameter would not)
    by = {(m["inputs"], m["params"], m["mode"]): m["name"] for m in meta}
    for i in ("in01", "in02"):
        base = by[(i, "gap4.73", 1)]
        for p in hc.PARAMS:
            other = by[(i, p, 1)]
            field = "S" if p.startswith(("alpha", "shift")) else "TGI"
            same = np.array_equal(z[base + "/" + field].view(np.uint32), z[other + "/" + field].view(np.uint32))
            assert same == (p == "gap4.73"), (i, p)


def test_oracle_matches_the_reference_off_the_defaults():
    meta, z = load_param_cases()
    _, zin = load_profile_cases()
    for m in meta:
        qp, tp = inputs(zin, m["inputs"])
        name = m["name"]
        S = orc.hmap2_sim(qp, tp, m["alpha"], m["zero_shift"])
        assert hc.bits_equal(S, z[name + "/S"]), name
        tgi, tge = orc.hmap2_precalc(tp, m["gi"], m["ge"], m["beta"])
        assert hc.bits_equal(tgi, z[name + "/TGI"]) and hc.bits_equal(tge, z[name + "/TGE"]), name
        rc, D, PQ, PT = orc.dp_build(S, orc.Gap(m["mode"], tgi=tgi, tge=tge), m["dir"], bug_b4=True)
        assert hc.bits_equal(D, z[name + "/H"]), name
        assert np.array_equal(PQ, z[name + "/PQ"]) and np.array_equal(PT, z[name + "/PT"]), name
        rc2, sc, pairs = orc.optimal(D, PQ, PT, m["mode"] == 3)
        assert int(sc.view(np.uint32)) == m["opt"]["score"] and pairs.reshape(-1).tolist() == m["opt"]["pairs"], name


def test_raw_plane_then_norm_shift_is_the_normalised_plane():
    """ref_profile always normalises; normalize = False is pinned through the split: the oracle's raw plane, then orc_norm_shift
    alone, must give the golden plane."""
    meta, z = load_param_cases()
    _, zin = load_profile_cases()
    for m in meta:
        qp, tp = inputs(zin, m["inputs"])
        raw = orc.hmap2_sim(qp, tp, m["alpha"], None)
        assert not hc.bits_equal(raw, z[m["name"] + "/S"])
        Q, T = raw.shape
        assert raw[0].tolist() == [0.0] * T and raw[-1].tolist() == [0.0] * T and not raw[:, 0].any() and not raw[:, -1].any()
        orc.lib().orc_norm_shift(Q, T, orc._fp(raw), orc.C.c_float(float(np.float32(m["zero_shift"]))))
        assert hc.bits_equal(raw, z[m["name"] + "/S"]), m["name"]


def test_shape_batch_construction():
    sb = hc.shape_batch()
    Ts = {t + 2 for _, t in sb.pairs}
    Qs = {q + 2 for q, _ in sb.pairs}
    assert set(hc.T_EDGES) <= Ts and hc.T_EDGES == (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1030)
    assert set(hc.Q_EDGES) <= Qs and hc.Q_EDGES == (15, 16, 17, 31, 32, 33, 63, 64, 65)
    for q, t in sb.pairs:
        if t + 2 >= 255:
            assert q <= 40                          # the O(Q T (Q + T)) oracle stays quick
    for Q in hc.Q_EDGES:
        assert any(q + 2 == Q and t <= 41 for q, t in sb.pairs)          # every Q edge against a short template
    assert hc.DWARFED == ((3, 1028), (40, 5)) and set(hc.DWARFED) <= set(sb.pairs) and hc.WIDE in sb.pairs
    assert max(Ts) == 1030 and max(Qs) == 65
    assert [q * t for q, t in hc.N_SHAPES] == [63, 64, 65, 511, 512, 513, 1024, 1025] == list(hc.N_LIST)
    assert set(hc.N_SHAPES) <= set(sb.pairs)
    assert hc.degenerate("one_cell")["qp"]["conf"].shape == (3,) and hc.degenerate("one_cell")["tp"]["conf"].shape == (3,)   # N = 1
    # the pools are shared: fewer sequences than pairs, and the reversed batch is the same pairs in the other order
    assert len(sb.qlens) < len(sb.pairs) and len(sb.tlens) < len(sb.pairs)
    rv = sb.reversed()
    assert rv.pairs == sb.pairs[::-1] and rv.pairs[0] != sb.pairs[0]
    for p in range(len(sb.pairs)):
        qp, tp = sb.profiles(p)
        assert (len(qp["conf"]) - 2, len(tp["conf"]) - 2) == sb.pairs[p]
        assert rv.profiles(len(sb.pairs) - 1 - p)[0] is qp
    qpool, tpool = sb.pools()
    assert len(qpool["conf"]) == sum(n + 2 for n in sb.qlens) and tpool["aa"].shape == (sum(n + 2 for n in sb.tlens), 20)


def test_shape_batch_planes_hold_no_nan():
    sb = hc.shape_batch()
    for p in range(len(sb.pairs)):
        qp, tp = sb.profiles(p)
        for zs in (hc.DEFAULTS["zero_shift"], None):
            assert np.isfinite(hc.sim_reference(sb.key(p), qp, tp, hc.DEFAULTS["alpha"], zs)).all(), sb.pairs[p]


EXP_BAND_COUNTS = {"underflow": 114, "denormal_far": 342, "denormal_table": 114, "normal": 304, "large": 114, "overflow": 342}


def test_exp_sweep_bands():
    qp, tp = hc.exp_sweep()
    assert len(qp["conf"]) <= 40 and len(tp["conf"]) <= 40
    arg = hc.exp_arguments(qp, tp, hc.EXP_ALPHA)
    masks = hc.exp_band_masks(arg)
    counts = {k: int(m.sum()) for k, m in masks.items()}
    assert counts == EXP_BAND_COUNTS
    assert all(c >= 20 for c in counts.values())
    # what the host libm makes of the bands: +0 below -103.98, denormal factors down to there, +inf above 88.7228
    S = hc.sim_reference("exp_sweep", qp, tp, hc.EXP_ALPHA, None)
    tiny = np.float32(np.finfo(np.float32).tiny)
    assert not np.isnan(S).any()
    assert (S[masks["underflow"]].view(np.uint32) == 0).all()
    assert np.isposinf(S[masks["overflow"]]).all()
    assert np.isfinite(S[masks["large"]]).all() and (S[masks["large"]] > 1e36).all()
    assert (S[masks["denormal_table"]] < tiny).all() and (S[masks["denormal_table"]] > 0).all()
    assert (S[masks["denormal_far"]] < tiny).all() and (S[masks["denormal_far"]] > 0).sum() >= 20
    assert (S[masks["normal"]] > 0).all() and np.isfinite(S[masks["normal"]]).all()


def test_degenerate_planes():
    names = [c["name"] for c in hc.degenerate_cases()]
    assert names == ["flat_third", "flat_half", "one_cell", "one_row", "one_column", "no_query", "no_template", "conf0_alpha0"]
    want = {"flat_third": (0, 0), "flat_half": (53, 130), "one_cell": (0, 1), "one_row": (0, 0), "one_column": (0, 0),
            "no_query": (0, 14), "no_template": (0, 14), "conf0_alpha0": (0, 0)}
    third = np.float32(1.0) / np.float32(3.0)
    for c in hc.degenerate_cases():
        raw = hc.sim_reference(("deg", c["name"]), c["qp"], c["tp"], c["alpha"], None)
        nrm = hc.sim_reference(("deg", c["name"]), c["qp"], c["tp"], c["alpha"], 0.12)
        assert (int(np.isnan(raw).sum()), int(np.isnan(nrm).sum())) == want[c["name"]] == (c["nan_raw"], c["nan_norm"]), c["name"]
        assert not np.isinf(raw).any() and not np.isinf(nrm).any()
    c = hc.degenerate("flat_third")
    assert c["qp"]["conf"].shape == (12,) and c["tp"]["conf"].shape == (15,)
    assert [i for i in range(12) if (c["qp"]["sse"][i] == third).all()] == [1, 5, 10]
    assert [j for j in range(15) if (c["tp"]["sse"][j] == third).all()] == [2, 13]
    c = hc.degenerate("flat_half")
    raw = hc.sim_reference(("deg", "flat_half"), c["qp"], c["tp"], c["alpha"], None)
    assert np.isnan(raw[[1, 5, 10], 1:-1]).all() and np.isnan(raw[1:-1, [2, 13]]).all()
    nrm = hc.sim_reference(("deg", "flat_half"), c["qp"], c["tp"], c["alpha"], 0.12)
    assert np.isnan(nrm[1:-1, 1:-1]).all() and not nrm[0].any() and not nrm[:, 0].any()
    for name in ("no_query", "no_template"):
        c = hc.degenerate(name)
        assert np.isnan(hc.sim_reference(("deg", name), c["qp"], c["tp"], c["alpha"], 0.12)).all()
        assert not hc.sim_reference(("deg", name), c["qp"], c["tp"], c["alpha"], None).any()
    c = hc.degenerate("conf0_alpha0")
    raw = hc.sim_reference(("deg", "conf0_alpha0"), c["qp"], c["tp"], 0.0, None)
    dot = np.float32(orc.lib().orc_dot(orc._fp(np.ascontiguousarray(c["qp"]["aa"][2])), orc._fp(np.ascontiguousarray(c["tp"]["aa"][3])), 20))
    assert raw[2, 3].view(np.uint32) == dot.view(np.uint32)                  # exp(0) = 1


def test_same_bits_or_nan():
    f = np.float32
    a = np.array([[1.5, 0.0, np.inf], [np.nan, -2.0, 3.0]], f)
    assert hc.same_bits_or_nan(a, a.copy())
    b = a.copy(); b[1, 2] = np.nextafter(f(3.0), f(4.0))
    assert not hc.same_bits_or_nan(a, b)                                     # a differing finite cell
    b = a.copy(); b[1, 0] = 7.0
    assert not hc.same_bits_or_nan(a, b) and not hc.same_bits_or_nan(b, a)   # NaN against a number
    b = a.copy(); b[0, 1] = -0.0
    assert not hc.same_bits_or_nan(a, b)                                     # +0 against -0
    b = a.copy(); b[0, 2] = -np.inf
    assert not hc.same_bits_or_nan(a, b)                                     # +inf against -inf
    b = a.copy(); b.view(np.uint32)[1, 0] = 0xFFC00001
    assert np.isnan(b[1, 0]) and b.view(np.uint32)[1, 0] != a.view(np.uint32)[1, 0]
    assert hc.same_bits_or_nan(a, b)                                         # NaNs of another payload and sign
    b = a.copy(); b.view(np.uint32)[1, 0] = 0x7F800001
    assert hc.same_bits_or_nan(a, b)                                         # a signalling NaN
    assert not hc.same_bits_or_nan(a, a[:, :2])
