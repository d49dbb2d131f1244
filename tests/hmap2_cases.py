"""Shared by tests/test_hmap2_reference.py (CPU) and tests/test_gpu_hmap2_ranges.py (GPU): the inputs that take the three
similarity kernels of csrc/sim_hmap2.hip off the default parameters and off the few shapes the other suites use, and the
oracle's answers for them, computed once and read-only.  numpy, orc (the CPU restatement) and aln_amd.synth (the seeded profile
generator) only; the library under test is never loaded here.

Sizes: a profile of n INTERIOR positions has n + 2 rows (the sentinels), so a pair of interiors (q, t) is a Q x T = (q+2) x (t+2)
plane whose normalised part holds N = q t cells.

  same_bits_or_nan   the one comparison that tolerates anything: cells where BOTH sides are NaN
  PARAMS             parameter sets, each one step away from the defaults
  shape_batch        one ragged batch whose pairs sit on every block, chunk and prefetch boundary of the three kernels
  exp_sweep          one pair whose exp() arguments fall in every band of glibc's expf, the out-of-range ones included
  degenerate_cases   inputs whose planes are NaN in the reference too, and their finite neighbours
  reference          the oracle's planes for a (query, template, parameters) triple
"""
import numpy as np

import orc
from aln_amd.synth import random_profile

DEFAULTS = dict(alpha=0.5, beta=1.0, zero_shift=0.12, gi=4.73, ge=0.34)


def same_bits_or_nan(a, b):
    """True iff a and b (float32, same shape) have equal NaN masks and equal uint32 patterns everywhere else: infinities and the
    sign of zero count, the payload and the sign of a NaN do not."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return bool(np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def params_with(**kv):
    p = dict(DEFAULTS)
    p.update(kv)
    return p


# every set keeps the other values at the defaults
PARAMS = {
    "alpha0": params_with(alpha=0.0),
    "alpha-0.5": params_with(alpha=-0.5),
    "alpha2": params_with(alpha=2.0),
    "alpha8": params_with(alpha=8.0),
    "shift0": params_with(zero_shift=0.0),
    "shift-0.3": params_with(zero_shift=-0.3),
    "shift1.5": params_with(zero_shift=1.5),
    "beta0": params_with(beta=0.0),
    "beta2.5": params_with(beta=2.5),
    "gap4.73": params_with(gi=4.73, ge=0.34),
    "gap11": params_with(gi=11.0, ge=1.0),
}


def pool(profiles):
    """the profiles of a sequence pool, concatenated in pool order (what Batch.dp_hmap2 takes)"""
    return {k: np.concatenate([p[k] for p in profiles]) for k in ("aa", "sse", "conf")}


# --- the ragged batch ------------------------------------------------------------------------------------------------------
# hmap2_sim_kernel: 256 columns per block, 32 rows per chunk; hmap2_apply_kernel: 1024 columns per block (256 threads x float4),
# 16 rows per workgroup; hmap2_stats_kernel: 64 elements per step (full-64 path / tail path), 8 x 64 = 512 per prefetch.
T_EDGES = (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1030)      # T, sentinels included
Q_EDGES = (15, 16, 17, 31, 32, 33, 63, 64, 65)                        # Q, sentinels included
N_SHAPES = ((1, 63), (1, 64), (1, 65), (7, 73), (8, 64), (19, 27), (16, 64), (25, 41))   # interiors
N_LIST = (63, 64, 65, 511, 512, 513, 1024, 1025)
# N = 1 is the 1 x 1 interior: its variance is 0 and its plane NaN in the reference too, so it is degenerate_cases()'s "one_cell"
# (shape_batch's planes must hold no NaN: they are compared without any allowance)

# (query interior, template interior): every T edge against a short query (the oracle's DP is O(Q T (Q + T))), every Q edge against
# a short template, the two pairs that maxT / maxQ / maxld dwarf, the N list
_T_QUERIES = (5, 7, 8, 16, 19, 25, 30, 40, 13, 3)
_Q_TEMPLATES = (9, 27, 41, 5, 9, 27, 41, 5, 9)
SHAPE_PAIRS = (tuple(zip(_T_QUERIES, (t - 2 for t in T_EDGES)))
               + tuple(zip((q - 2 for q in Q_EDGES), _Q_TEMPLATES))
               + ((40, 5), (30, 1028))
               + N_SHAPES)
DWARFED = ((3, 1028), (40, 5))
WIDE = (30, 1028)                                                     # the absmax test's wide pair

_CACHE = {}


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _freeze(p):
    for v in p.values():
        v.setflags(write=False)
    return p


def query_profile(n):
    return _memo(("q", n), lambda: _freeze(random_profile(81000 + n, n)))


def template_profile(n):
    return _memo(("t", n), lambda: _freeze(random_profile(82000 + n, n)))


class Ragged:
    """pairs over shared pools: .qlens / .tlens (interiors, pool order), .qps / .tps (profiles), .q_idx / .t_idx, .pairs"""

    def __init__(self, pairs):
        self.pairs = tuple(pairs)
        self.qlens = sorted({q for q, _ in self.pairs})
        self.tlens = sorted({t for _, t in self.pairs})
        self.qps = [query_profile(n) for n in self.qlens]
        self.tps = [template_profile(n) for n in self.tlens]
        self.q_idx = [self.qlens.index(q) for q, _ in self.pairs]
        self.t_idx = [self.tlens.index(t) for _, t in self.pairs]

    def reversed(self):
        return Ragged(self.pairs[::-1])

    def strings(self):
        return ["A" * n for n in self.qlens], ["A" * n for n in self.tlens]

    def pools(self):
        return pool(self.qps), pool(self.tps)

    def profiles(self, p):
        return self.qps[self.q_idx[p]], self.tps[self.t_idx[p]]

    def key(self, p):
        return ("shape",) + self.pairs[p]


def shape_batch():
    return Ragged(SHAPE_PAIRS)


# --- the oracle's answers ----------------------------------------------------------------------------------------------------
def sim_reference(key, qp, tp, alpha, zero_shift):
    """-> S (read-only); zero_shift None: the raw plane (normalize = False)"""
    def make():
        S = orc.hmap2_sim(qp, tp, alpha, zero_shift)
        S.setflags(write=False)
        return S
    return _memo(("S", key, float(alpha), None if zero_shift is None else float(zero_shift)), make)


def gap_reference(key, tp, gi, ge, beta):
    def make():
        tgi, tge = orc.hmap2_precalc(tp, gi, ge, beta)
        tgi.setflags(write=False)
        tge.setflags(write=False)
        return tgi, tge
    return _memo(("G", key, float(gi), float(ge), float(beta)), make)


def reference(key, qp, tp, mode, params=None, normalize=True):
    """-> dict S, tgi, tge, D, PQ, PT, score, pairs of the oracle (computed once per key, mode and parameters; read-only).  `key`
    names the (qp, tp) pair."""
    pr = DEFAULTS if params is None else params
    zs = pr["zero_shift"] if normalize else None
    S = sim_reference(key, qp, tp, pr["alpha"], zs)
    tgi, tge = gap_reference(key, tp, pr["gi"], pr["ge"], pr["beta"])

    def make():
        rc, D, PQ, PT = orc.dp_build(S, orc.Gap(mode, tgi=tgi, tge=tge))
        assert rc == 0
        rc2, sc, pl = orc.optimal(D, PQ, PT, mode == orc.LOCAL)
        for a in (D, PQ, PT, pl):
            a.setflags(write=False)
        return dict(S=S, tgi=tgi, tge=tge, D=D, PQ=PQ, PT=PT, status=rc2, score=sc, pairs=pl)
    return _memo(("R", key, mode, tuple(sorted(pr.items())), bool(normalize)), make)


# --- the exp sweep ---------------------------------------------------------------------------------------------------------
EXP_ALPHA = 105.0
# glibc's expf (sysdeps/ieee754/flt-32/e_expf.c): the table path between -0x1.9fe368p6 (-103.972) and 0x1.62e42ep6 (88.7228),
# +0 below, +inf above; its results are denormal below -87.34.  The device's restatement left the table path at |x| >= 88.
EXP_BANDS = (
    ("underflow", -np.inf, -103.98),          # x < -103.98
    ("denormal_far", -103.98, -88.0),         # [-103.98, -88]
    ("denormal_table", -88.0, -87.34),        # (-88, -87.34)
    ("normal", -87.34, 87.0),                 # (-87.34, 87)
    ("large", 88.0, 88.7228),                 # [88, 88.7228]
    ("overflow", 88.7228, np.inf),            # x > 88.7228
)
_SAME = np.array([0.9, 0.05, 0.05], np.float32)          # pearson with itself: +1
_ANTI = np.array([0.05, 0.475, 0.475], np.float32)       # pearson with _SAME: -1
_EXP_INTERIOR = 38


def exp_sweep():
    """-> (qp, tp), a 40 x 40 pair for normalize = False and alpha = EXP_ALPHA.  Every query row carries the triple (0.9, 0.05,
    0.05); the template's odd columns carry the same triple (pearson +1), its even columns (0.05, 0.475, 0.475) (pearson -1).
    The query's confidences are the magnitudes wanted, divided by alpha: six in each of (87.45, 87.9), (88.1, 88.7), (88.8,
    89.6), (90, 103.5) and (104.2, 105), eight below 86; the template's confidences step down from 1 by 3e-5 per column (a
    factor of 0.99946 at most), which keeps a row's products inside its band.  114 cells per band and sign, before rounding.
    Every template column and every odd query row put their whole weight on the first residue type: the dot product is exactly
    1 on the odd rows, so that S is exp()'s own bits there, and a small fraction on the even rows."""
    def make():
        n = _EXP_INTERIOR
        qp, tp = random_profile(83001, n), random_profile(83002, n)
        mags = np.concatenate([np.linspace(87.45, 87.9, 6), np.linspace(88.1, 88.7, 6), np.linspace(88.8, 89.6, 6),
                               np.linspace(90.0, 103.5, 6), np.linspace(104.2, 105.0, 6), np.linspace(0.0, 86.0, 8)])
        assert len(mags) == n
        # dot products of exactly 1 on the odd query rows (S is exp() itself there), of the query's first entry on the even ones
        tp["aa"][:] = 0.0
        tp["aa"][:, 0] = 1.0
        qp["aa"][1::2] = tp["aa"][0]
        qp["sse"][:] = _SAME
        qp["conf"][1:-1] = (mags / EXP_ALPHA).astype(np.float32)
        for j in range(1, n + 1):
            tp["sse"][j] = _SAME if j % 2 else _ANTI
            tp["conf"][j] = np.float32(1.0 - 3e-5 * ((j - 1) // 2))
        return _freeze(qp), _freeze(tp)
    return _memo("exp_sweep", make)


def exp_arguments(qp, tp, alpha):
    """-> float32 [Q, T]: alpha * pearson * conf * conf of every interior cell, evaluated in float32 and in the oracle's order
    (orc_sim_hmap2: ((alpha * pc) * cq) * ct); NaN on the sentinel rows and columns"""
    Q, T = len(qp["conf"]), len(tp["conf"])
    arg = np.full((Q, T), np.nan, np.float32)
    L = orc.lib()
    a = np.float32(alpha)
    for i in range(1, Q - 1):
        sa = np.ascontiguousarray(qp["sse"][i])
        for j in range(1, T - 1):
            sb = np.ascontiguousarray(tp["sse"][j])
            pc = np.float32(L.orc_pearson(orc._fp(sa), orc._fp(sb), 3))
            arg[i, j] = np.float32(np.float32(np.float32(a * pc) * qp["conf"][i]) * tp["conf"][j])
    return arg


def exp_band_masks(arg):
    """-> {band: bool mask}; a band's closed ends are those of the list above"""
    m = {}
    for name, lo, hi in EXP_BANDS:
        if name in ("denormal_far", "large"):
            m[name] = (arg >= lo) & (arg <= hi)
        else:
            m[name] = (arg > lo) & (arg < hi)
    return m


# --- degenerate profiles -------------------------------------------------------------------------------------------------------
def _profile(seed, n):
    return random_profile(seed, n)


def degenerate_cases():
    """-> list of dict name, qp, tp, alpha, nan_raw, nan_norm: how many cells of the oracle's raw and normalised planes are NaN
    (asserted by the CPU test).  Interiors in the names.

      flat_third   10 x 13 (a 12 x 15 plane): the triple (1/3, 1/3, 1/3 as float32) at three query and two template positions.
                   Its fp32 sum rounds to 1 and its mean back to the element, so every deviation is an exact 0 — and its fp32
                   variance comes out just ABOVE 0 (sum of squares / 3 rounds up), so 0 / sd is 0, the Pearson term 0 and the
                   plane finite: the flat triple that does not poison a plane
      flat_half    the same pair with the triple (0.5, 0.5, 0.5): mean and squares are exact, the variance is exactly 0, the
                   Pearson term 0/0: 3 x 13 + 2 x 10 - 6 = 53 raw cells, and the statistics spread them over the whole
                   normalised interior
      one_cell     1 x 1: a finite raw cell, variance 0, a NaN after normalisation (N = 1 of the statistics chain)
      one_row      1 x 9, one_column 9 x 1: finite
      no_query     0 x 5, no_template 5 x 0: no interior, so norm_elements takes the whole zero matrix (hmath.h:65-66): every cell
                   0/0 after normalisation, all zero before
      conf0_alpha0 6 x 7 with every confidence 0 and alpha 0: exp(0) = 1, the plane is the dot products, finite
    """
    def make():
        third = np.float32(1.0) / np.float32(3.0)
        cases = []
        for name, flat, nan_raw, nan_norm in (("flat_third", third, 0, 0), ("flat_half", np.float32(0.5), 53, 130)):
            qp, tp = _profile(84001, 10), _profile(84002, 13)
            for i in (1, 5, 10):
                qp["sse"][i] = flat
            for j in (2, 13):
                tp["sse"][j] = flat
            cases.append(dict(name=name, qp=qp, tp=tp, alpha=0.5, nan_raw=nan_raw, nan_norm=nan_norm))
        cases.append(dict(name="one_cell", qp=_profile(84003, 1), tp=_profile(84004, 1), alpha=0.5, nan_raw=0, nan_norm=1))
        cases.append(dict(name="one_row", qp=_profile(84005, 1), tp=_profile(84006, 9), alpha=0.5, nan_raw=0, nan_norm=0))
        cases.append(dict(name="one_column", qp=_profile(84007, 9), tp=_profile(84008, 1), alpha=0.5, nan_raw=0, nan_norm=0))
        cases.append(dict(name="no_query", qp=_profile(84009, 0), tp=_profile(84010, 5), alpha=0.5, nan_raw=0, nan_norm=14))
        cases.append(dict(name="no_template", qp=_profile(84011, 5), tp=_profile(84012, 0), alpha=0.5, nan_raw=0, nan_norm=14))
        qp, tp = _profile(84013, 6), _profile(84014, 7)
        qp["conf"][:] = 0.0
        tp["conf"][:] = 0.0
        cases.append(dict(name="conf0_alpha0", qp=qp, tp=tp, alpha=0.0, nan_raw=0, nan_norm=0))
        for c in cases:
            _freeze(c["qp"])
            _freeze(c["tp"])
        return cases
    return _memo("degenerate", make)


def degenerate(name):
    return next(c for c in degenerate_cases() if c["name"] == name)


def own_pools(items):
    """items: (qp, tp) per pair, every pair with pool entries of its own -> (query strings, template strings, qpool, tpool)"""
    qs = ["A" * (len(qp["conf"]) - 2) for qp, _ in items]
    ts = ["A" * (len(tp["conf"]) - 2) for _, tp in items]
    return qs, ts, pool([qp for qp, _ in items]), pool([tp for _, tp in items])
