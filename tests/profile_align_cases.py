"""Shared by tests/test_profile_align_reference.py (CPU) and tests/test_gpu_hits_align_profiles.py (GPU): the inputs and the
references of aln_hits_align_profiles.  A profile adds no rule to the traceback, only another similarity plane, so every
reference here is an existing restatement fed with the plane of profile_cases.plane: lean_cases.reference_list (the local loop
of Optimal on the int64 plane) and nonlocal_cases.walk (strip byte, final cell's pointer, walk) with nonlocal_cases.census.
numpy, the oracle and those modules only; aln_amd's library is not imported.

  plane           profile_cases.plane for any alphabet
  tie_profiles    the tie inputs of nonlocal_cases as profiles that no table row equals
  oracle_pair     orc.dp_build + orc.optimal over the float plane of a (profile, template) pair
  restated        (score, list) of a pair by the restated rules on the int64 reference plane
  local_census    what a local list went through: deletion jumps, insertion jumps, tied cells
"""
import numpy as np

import lean_cases as lc
import nonlocal_cases as nc
import orc
import profile_cases as pc
import range_cases as rc

TIE_ALPHAS = ("AC", "ACGT")
TIE_GAPS = nc.TIE_GAPS
TIE_SEED = 17

# Conditions on the INPUTS (not tolerances): what the lists of the tie profiles must go through, per align type, summed over both
# alphabets, the four gap systems and all 36 pairs.  The minima observed over the four non-local types are 79 / 22 / 109 / 38 /
# 2076 / 1403 / 1445, local 2252 / 1527 / 1492.
NONLOCAL_FLOORS = dict(final_del=40, final_ins=15, row1=50, col1=30, del_jumps=500, ins_jumps=400, ties=1000)
LOCAL_FLOORS = dict(del_jumps=500, ins_jumps=400, ties=400)


def plane(profile, t, alpha):
    """-> S int64, (L+2) x (T+2): S[i][j] = profile[i-1][letter of t[j-1]] inside, 0 on the sentinel rows and columns"""
    if alpha == pc.ALPHA:
        return pc.plane(profile, t)
    idx = {ch: k for k, ch in enumerate(alpha)}
    prof = np.asarray(profile, np.int64).reshape(-1, len(alpha))
    S = np.zeros((len(prof) + 2, len(t) + 2), np.int64)
    if len(prof) and len(t):
        S[1:-1, 1:-1] = prof[:, [idx[ch] for ch in t]]
    return S


_TIE = {}


def tie_profiles(alpha):
    """-> (profiles, queries, templates): for every tie query, in order, the rows of tie_table(alpha) for its letters plus a
    seeded offset in {-1, 0, 1} per entry; the queries themselves (a consensus) and the tie templates"""
    if alpha not in _TIE:
        table = nc.tie_table(alpha).astype(np.int64)
        qs, ts = nc.tie_sequences(alpha)
        rng = np.random.RandomState(TIE_SEED)
        profiles = []
        for q in qs:
            p = table[[alpha.index(ch) for ch in q]]
            p = p + rng.randint(-1, 2, size=p.shape)
            p.setflags(write=False)
            profiles.append(p)
        _TIE[alpha] = (profiles, qs, ts)
    return _TIE[alpha]


def table_rows(alpha, q):
    return nc.tie_table(alpha).astype(np.int64)[[alpha.index(ch) for ch in q]]


_ORACLE = {}


def oracle_pair(profile, t, alpha, mode, gi, ge):
    """-> (D, score, list) of orc.dp_build + orc.optimal over the pair's float32 plane; computed once per input, left unchanged"""
    key = (np.asarray(profile).tobytes(), t, alpha, mode, gi, ge)
    if key not in _ORACLE:
        S = plane(profile, t, alpha).astype(np.float32)
        err, D, PQ, PT = orc.dp_build(S, orc.Gap(mode, gi, ge))
        err2, score, pl = orc.optimal(D, PQ, PT, mode == orc.LOCAL)
        assert err == 0 and err2 == 0
        _ORACLE[key] = (D, score, pl)
    return _ORACLE[key]


def restated(profile, t, alpha, mode, gi, ge):
    """-> (score as int, list int32 [n, 2] in list order) by the restated rules alone, on the int64 reference plane; the list is
    None for a non-local pair without an interior, which nonlocal_cases.walk does not restate"""
    H = rc.affine_reference(plane(profile, t, alpha), mode, gi, ge)[0]
    if mode == rc.LOCAL:
        return rc.reference_score(H, mode), lc.reference_list(H, gi, ge)
    if H.shape[0] < 3 or H.shape[1] < 3:
        return rc.reference_score(H, mode), None
    free_del, free_ins = nc.free_ends(mode)
    score, pl = nc.walk(H, gi, ge, free_del, free_ins)
    assert int(score) == rc.reference_score(H, mode)
    return int(score), pl


def new_local_census():
    return dict.fromkeys(LOCAL_FLOORS, 0)


def local_census(D, pl, gi, ge, into):
    """adds what the local list pl went through to the counters of `into`"""
    pl = np.asarray(pl).reshape(-1, 2)
    path = pl[1:-1] if (pl[0] == 0).all() else pl[:-1]
    for a, b in zip(path[:-1], path[1:]):
        into["del_jumps"] += int(b[0] - a[0] == 1 and b[1] - a[1] > 1)
        into["ins_jumps"] += int(b[1] - a[1] == 1 and b[0] - a[0] > 1)
    Di = np.asarray(D).astype(np.int64)
    for c in path:
        if c[0] >= 2 and c[1] >= 2:
            into["ties"] += int(nc.top_two_equal(Di, int(c[0]), int(c[1]), gi, ge))


def meets(census, floors):
    return all(census[k] >= v for k, v in floors.items())
