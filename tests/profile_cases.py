"""Shared by tests/test_profile_reference.py (CPU) and tests/test_gpu_qprofile_search.py (GPU): position-specific queries
(profiles: one row of per-letter scores for every query position) for aln_score_profiles_vs_all / aln_search_topk_profiles, and
what those entries must report, restated on the int64 planes of range_cases.affine_reference.  A profile adds no arithmetic to
the recurrence, only another similarity plane, S[i][j] = profile[i][letter of t[j]], so the reference is the existing one fed
with that plane.  numpy, range_cases, lean_cases and search_cases only; neither aln_amd's library nor torch is imported.

A profile is an (L x n) int64 array over search_cases.ALPHA WITHOUT the two sentinel rows (aln_amd.QueryProfiles adds them).

  plane             the (L+2) x (T+2) similarity plane of a profile and a template: a gather of rows by letters, zero sentinels
  dense_reference   scores and end cells of a set of profiles against a set of templates
  derived           the profiles that score like residue strings under a table
  perturbed         derived + a seeded per-entry offset in [-6, 6]: rows that no table row equals
  length_set        the profile set of the GPU test's part 2
"""
import numpy as np

import lean_cases as lc
import range_cases as rc
import search_cases as sc

ALPHA = sc.ALPHA
N = len(ALPHA)
_IDX = {ch: k for k, ch in enumerate(ALPHA)}

# Interior rows of the length set: none, one, and one below / at / one above every boundary of the kernels' staging — rows are
# brought into LDS 8 at a time (sentinel row included: row i of the profile is interior row i), into a ring of 32 — and 130,
# four ring revolutions.
INTERIOR_ROWS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130)


def codes(t):
    return np.array([_IDX[ch] for ch in t], np.int64)


def plane(profile, t):
    """-> S int64, (L+2) x (T+2): S[i][j] = profile[i-1][letter of t[j-1]] inside, 0 on the sentinel rows and columns"""
    prof = np.asarray(profile, np.int64).reshape(-1, N)
    S = np.zeros((len(prof) + 2, len(t) + 2), np.int64)
    if len(prof) and len(t):
        S[1:-1, 1:-1] = prof[:, codes(t)]
    return S


def derived(seqs, table):
    """row i of profile s is the table row of residue i of seqs[s]"""
    tab = np.asarray(table)
    ti = tab.astype(np.int64)
    assert np.array_equal(ti.astype(tab.dtype), tab), "integral tables only"
    return [ti[codes(s)].reshape(len(s), N) for s in seqs]


def perturbed(seqs, table, seed, span=6):
    rng = np.random.RandomState(seed)
    return [p + rng.randint(-span, span + 1, size=p.shape) for p in derived(seqs, table)]


def peaked(rows, at, low, high):
    """`low` (negative) everywhere except row `at`, which holds `high` for every letter"""
    p = np.full((rows, N), low, np.int64)
    p[at] = high
    return p


def pair_reference(profile, t, mode, gi, ge):
    """-> (the score Optimal reports, find_max's cell for local builds else (Q-1, T-1))"""
    H = rc.affine_reference(plane(profile, t), mode, gi, ge)[0]
    end = lc.find_max_cell(H) if mode == rc.LOCAL else (H.shape[0] - 1, H.shape[1] - 1)
    return rc.reference_score(H, mode), (int(end[0]), int(end[1]))


_DENSE = {}


def dense_reference(key, profiles, ts, mode, gi, ge):
    """-> (int64 scores [len(profiles), len(ts)], int64 end cells [.., .., 2]); computed once per (key, mode, gi, ge) — the key
    names the (profiles, templates) set — and read-only"""
    k = (key, mode, gi, ge)
    if k not in _DENSE:
        scores = np.zeros((len(profiles), len(ts)), np.int64)
        ends = np.zeros((len(profiles), len(ts), 2), np.int64)
        for i, p in enumerate(profiles):
            for j, t in enumerate(ts):
                scores[i, j], ends[i, j] = pair_reference(p, t, mode, gi, ge)
        scores.setflags(write=False)
        ends.setflags(write=False)
        _DENSE[k] = (scores, ends)
    return _DENSE[k]


LENGTH_SYSTEM = ("blosum62", 11, 1)


def length_set():
    """-> (profiles, templates) of part 2: perturbed profiles of INTERIOR_ROWS rows derived from random sequences, one profile
    that is negative everywhere except a single row of the table's maximum (11, W-W), one all-zero profile; the templates of
    search_cases.sequences (empty, two residues, duplicates, 254 / 255 residues across the class boundary)."""
    table = sc.TABLES[LENGTH_SYSTEM[0]]
    seqs = [rc.random_seq(ALPHA, 300 + n, n) for n in INTERIOR_ROWS]
    profiles = perturbed(seqs, table, 7)
    top = int(np.asarray(table).max())
    profiles.append(peaked(40, 23, -3, top))
    profiles.append(np.zeros((33, N), np.int64))
    _, ts = sc.sequences(sc.CASES["blosum62"])
    return profiles, ts


def wide_set(table):
    """-> (profiles, templates): search_cases.wide_sequences()'s templates (length classes 6, 7, 8), its two 40-residue queries
    as perturbed profiles and one perturbed profile of 300 rows (nine ring revolutions at the highest register pressure) that
    carries the 40-residue query in its middle"""
    qs, ts = sc.wide_sequences()
    long_q = rc.random_seq(ALPHA, 411, 130) + qs[0] + rc.random_seq(ALPHA, 412, 130)
    return perturbed(qs + [long_q], table, 11), ts


def mixed_set():
    """-> (profiles, templates): one template of 2100 residues (beyond the register-resident kernels) among short ones, two
    perturbed 40-row profiles; the long template ends in a noisy copy of the first query, so its column holds top scores"""
    q = rc.random_seq(ALPHA, 500, 40)
    long_t = rc.random_seq(ALPHA, 501, 2055) + lc.mutated(ALPHA, q, 502, every=7) + rc.random_seq(ALPHA, 503, 5)
    ts = [rc.random_seq(ALPHA, 504, 60), long_t, q, "", rc.random_seq(ALPHA, 505, 300)]
    assert len(long_t) == 2100
    return perturbed([q, rc.random_seq(ALPHA, 506, 40)], sc.TABLES["blosum62"], 13), ts
