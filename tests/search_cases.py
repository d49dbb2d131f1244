"""Shared by tests/test_search_reference.py (CPU) and tests/test_gpu_search_ranges.py (GPU): what aln_search_topk,
aln_hits_zscores and aln_hits_align must report, restated on the int64 planes of range_cases.affine_reference, and the scoring
systems and sequence sets that feed those kernels the values their value-dependent code exists for.  Python integers and int64
only; neither aln_amd's library nor torch is imported, so no reference value can share a sweep, an integer width or a "minus
infinity" with a kernel.

  dense_reference    the score matrix of a set (and find_max's end cell of every pair, local)
  topk_reference     the header's selection: score >= min_score, score descending, ties by template index, one zero
  zstats_reference   sum and sum of squares over the shuffles of a query (aln_amd.shuffle_query, pure Python), Python ints
  z_restated         the header's z formula
  nonlocal_reference the oracle's build and traceback (orc.dp_build + orc.optimal), as nonlocal_cases.oracle_pair
"""
import collections
import math

import numpy as np

import lean_cases as lc
import nonlocal_cases as nc
import range_cases as rc

ALPHA, BLOSUM = rc.load_blosum62()
TABLES = dict(rc.table_families(ALPHA, BLOSUM))
TABLES["blosum62x888"] = rc.scaled(BLOSUM, 888)
W = "W"                                                              # BLOSUM62's best residue ...
WORST = rc.worst_partner(ALPHA, BLOSUM, W)                           # ... and its worst partner; every case uses these two letters

Case = collections.namedtuple("Case", "name table gi ge n m")        # table: a key of TABLES; n, m: residues of query, template

CASES = collections.OrderedDict((c.name, c) for c in [
    Case("score32_in", "blosum62x888", 4000, 4096, 300, 300),        # lhs_score32 = 8 387 624 < 2^23, by under 1 %
    Case("score32_out", "blosum62x888", 5000, 4096, 300, 300),       # 8 388 624: every entry goes through full builds
    Case("packed_in", "blosum62x9", 11, 0, 300, 300),                # packed left side 29 997 < 30 000: the 16-bit kernel at its limit
    Case("constant+3", "constant+3", 0, 0, 130, 257),                # ties everywhere
    Case("all_zero", "all_zero", 0, 0, 130, 257),                    # every score of every plane equal
    Case("all_negative", "all_negative", 0, 1, 130, 257),            # every local score is 0
    Case("blosum62x-1", "blosum62x-1", 1, 5, 130, 257),              # -0.0 entries, ge > gi
    Case("identity5", "identity5", 40, 0, 130, 257),                 # large gi with ge 0
    Case("blosum62", "blosum62", 11, 1, 130, 257),                   # control
])
BIG = ("score32_in", "score32_out", "packed_in")                     # the 300 x 300 cases
N_TEMPLATES = 10
KS = (4, N_TEMPLATES)                                                # the K of the GPU tests
WIDE_SYSTEMS = [("identity5", 40, 0), ("blosum62x-1", 1, 5)]
WIDE_MODES = (rc.LOCAL, rc.GLOBAL, rc.SEMI_LOCAL)


def sequences(case):
    """-> (6 queries, 10 templates).  Templates 6 and 7 repeat templates 2 and 0: equal scores at different indices in every
    row; templates 8 and 9 (254 and 255 residues = 256 and 257 columns) straddle the boundary between length classes 1 and 2."""
    n, m = case.n, case.m
    r = rc.random_seq(ALPHA, 77, min(n, m))
    qs = [W * n, WORST * n, r, rc.random_seq(ALPHA, 78, n), "", W]
    ts = [W * m, WORST * m, r, rc.random_seq(ALPHA, 79, m), "", W + WORST, r, W * m, rc.random_seq(ALPHA, 80, 254),
          rc.random_seq(ALPHA, 81, 255)]
    assert len(ts) == N_TEMPLATES
    return qs, ts


def wide_sequences():
    """-> (2 queries of 40 residues, 5 templates of 1400 .. 2046 residues: length classes 6, 7, 7, 8, 8).  A noisy copy of the
    random query sits near the end of every template, so that the best local cells lie in the last column groups."""
    q = rc.random_seq(ALPHA, 90, 40)
    qs = [q, W * 40]
    ts = []
    for k, ln in enumerate((1400, 1535, 1536, 2045, 2046)):
        body = rc.random_seq(ALPHA, 91 + k, ln)
        at = ln - 45 - 3 * k
        ts.append(body[:at] + lc.mutated(ALPHA, q, 96 + k, every=7) + body[at + 40:])
        assert len(ts[-1]) == ln
    assert [(len(t) + 2 + 255) // 256 for t in ts] == [6, 7, 7, 8, 8]
    return qs, ts


# ---- scores and end cells ---------------------------------------------------------------------------------------------------

_PAIR = {}


def pair_reference(q, t, table, mode, gi, ge):
    """-> (score Optimal reports, find_max's end cell for local builds else (Q-1, T-1)); table is a key of TABLES.  Computed once
    per input and never modified."""
    key = (q, t, table, mode, gi, ge)
    if key not in _PAIR:
        H = rc.affine_reference(rc.sim_int(q, t, ALPHA, TABLES[table]), mode, gi, ge)[0]
        end = lc.find_max_cell(H) if mode == rc.LOCAL else (H.shape[0] - 1, H.shape[1] - 1)
        _PAIR[key] = (rc.reference_score(H, mode), (int(end[0]), int(end[1])))
    return _PAIR[key]


def plane(q, t, table, mode, gi, ge):
    """-> (S, H) int64, for the walks of the alignment tests (not cached: a few pairs per test need it)"""
    S = rc.sim_int(q, t, ALPHA, TABLES[table])
    return S, rc.affine_reference(S, mode, gi, ge)[0]


def dense_reference(qs, ts, table, mode, gi, ge):
    """-> (int64 score matrix [len(qs), len(ts)], int64 end cells [len(qs), len(ts), 2]: find_max's cell under local mode,
    (Q-1, T-1) otherwise)"""
    scores = np.zeros((len(qs), len(ts)), np.int64)
    ends = np.zeros((len(qs), len(ts), 2), np.int64)
    for i, q in enumerate(qs):
        for j, t in enumerate(ts):
            scores[i, j], ends[i, j] = pair_reference(q, t, table, mode, gi, ge)
    scores.setflags(write=False)
    ends.setflags(write=False)
    return scores, ends


# ---- selection ----------------------------------------------------------------------------------------------------------------

def topk_reference(scores_row, K, min_score=-math.inf):
    """include/aln_hip.h, aln_search_topk: the templates with score >= min_score, score descending, ties by template index
    ascending, at most K of them.  -0.0 and +0.0 are one score.  -> list of template indices"""
    cand = [t for t, s in enumerate(scores_row) if s >= min_score]
    cand.sort(key=lambda t: (0 if scores_row[t] == 0 else -scores_row[t], t))
    return cand[:K]


def has_tie(scores_row, order):
    s = [scores_row[t] for t in order]
    return len(set(s)) < len(s)


# ---- z-scores -----------------------------------------------------------------------------------------------------------------

def z_restated(n, score, s, ss):
    if n < 2:
        return np.float32(0.0)
    D = n * ss - s * s
    if D == 0:
        return np.float32(0.0)
    N = n * int(score) - s
    return np.float32(float(N) * math.sqrt(float(n - 1) / (float(n) * float(D))))


def zstats_reference(seed, q_index, q, t, table, mode, gi, ge, n, shuffle=None):
    """-> (sum, sumsq, the n scores) as Python ints: shuffle s = 0 .. n-1 of query q (pool index q_index) against template t"""
    if shuffle is None:
        from aln_amd import shuffle_query as shuffle                 # pure Python; imported late so that this module stands alone
    col = [int(pair_reference(shuffle(seed, q_index, s, q), t, table, mode, gi, ge)[0]) for s in range(n)]
    return sum(col), sum(v * v for v in col), col


# ---- non-local alignments -----------------------------------------------------------------------------------------------------

def nonlocal_reference(q, t, table, mode, gi, ge):
    """-> (score, pair list) of the oracle's build and traceback"""
    D, sc, pl = nc.oracle_pair(q, t, ALPHA, TABLES[table], mode, gi, ge)
    return sc, pl
