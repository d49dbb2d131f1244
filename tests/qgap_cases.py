"""Shared by tests/test_qgap_reference.py (CPU) and tests/test_gpu_qgap_search.py (GPU): position-specific GAP PENALTIES
(aln_qgaps) for aln_score_profiles_gaps_vs_all / aln_search_topk_profiles_gaps, restated in int64 straight from the definition
in include/aln_hip.h — plain maxima over every source k of every cell, O(QT(Q+T)), no collapsed keys, no running maxima —
and the case sets.  numpy, range_cases, lean_cases, profile_cases and search_cases only; aln_amd is not imported.

A profile is an (L x n) int64 array WITHOUT the sentinel rows (profile_cases); its gap rows are four sequences of L + 1
values, rows 0 .. L = Q-2 (what aln_amd.QueryGaps takes).  The reference reads an entry with int() at the moment the
definition reads it, so an entry that is never read may hold anything, a NaN included.

  del(i, L)   = del_init[i] + del_extn[i] (L-1)                      L template residues skipped between rows i and i+1
  ins(a, b)   = ins_init[a] + sum_{p=a+1..b} ins_extn[p]             profile positions a..b skipped
"""
import numpy as np

import lean_cases as lc
import profile_cases as pc
import range_cases as rc
import search_cases as sc

ALPHA = pc.ALPHA
N = pc.N
NAN = float("nan")


def ins_table(ins_init, ins_extn, Q):
    """INS[a][b] = ins(a, b) for 1 <= a <= b <= Q-2, by the definition: every skipped position pays its own price"""
    INS = np.zeros((Q, Q), np.int64)
    for a in range(1, Q - 1):
        c = int(ins_init[a])
        INS[a][a] = c
        for b in range(a + 1, Q - 1):
            c += int(ins_extn[b])
            INS[a][b] = c
    return INS


def qgap_planes(S, mode, del_init, del_extn, ins_init, ins_extn):
    """-> H int64, every cell of the Q x T plane (range_cases.affine_reference's layout: the final cell at (Q-1, T-1))"""
    S = np.asarray(S, np.int64)
    Q, T = S.shape
    local = mode == rc.LOCAL
    fdel, fins = rc.free_ends(mode)
    H = np.zeros((Q, T), np.int64)

    def dele(i, L):                                            # L: an int or an int64 array, >= 1
        return int(del_init[i]) + int(del_extn[i]) * (L - 1)

    if Q == 2:
        H[1, T - 1] = 0 if (fdel or T - 2 < 1) else -dele(0, T - 2)
        return H
    INS = ins_table(ins_init, ins_extn, Q)
    if T == 2:
        H[Q - 1, 1] = 0 if fins else -INS[1][Q - 2]
        return H
    clip = (lambda v: max(v, 0)) if local else (lambda v: v)
    for i in range(1, Q - 1):
        for j in range(1, T - 1):
            if i == 1 and j == 1:
                best = 0
            elif i == 1:                                       # the head deletion, priced by row 0
                best = 0 if fdel else -dele(0, j - 1)
            elif j == 1:                                       # the head insertion
                best = 0 if fins else -int(INS[1][i - 1])
            else:
                best = int(H[i - 1, j - 1])
                if j > 2:                                      # deletions: sources (i-1, k), 1 <= k < j-1, priced by row i-1
                    ks = np.arange(1, j - 1, dtype=np.int64)
                    best = max(best, int((H[i - 1, 1:j - 1] - dele(i - 1, j - 1 - ks)).max()))
                if i > 2:                                      # insertions: sources (k, j-1), 1 <= k < i-1
                    ks = np.arange(1, i - 1, dtype=np.int64)
                    best = max(best, int((H[1:i - 1, j - 1] - INS[ks + 1, i - 1]).max()))
            H[i, j] = clip(int(S[i, j]) + best)
    best = int(H[Q - 2, T - 2])
    if T > 3:
        ks = np.arange(1, T - 2, dtype=np.int64)
        cost = 0 if fdel else dele(Q - 2, T - 2 - ks)
        best = max(best, int((H[Q - 2, 1:T - 2] - cost).max()))
    if Q > 3:
        ks = np.arange(1, Q - 2, dtype=np.int64)
        cost = 0 if fins else INS[ks + 1, Q - 2]
        best = max(best, int((H[1:Q - 2, T - 2] - cost).max()))
    H[Q - 1, T - 1] = clip(best)
    assert int(np.abs(H).max()) < rc.EXACT_LIMIT
    return H


def with_tail(v):
    """L + 1 gap values (rows 0 .. Q-2) -> Q values, the '$' row's never read"""
    return list(v) + [NAN]


def pair_reference(profile, t, mode, gaps):
    """gaps: four sequences of L + 1 values -> (score, find_max's cell for local builds else (Q-1, T-1))"""
    H = qgap_planes(pc.plane(profile, t), mode, *[with_tail(g) for g in gaps])
    end = lc.find_max_cell(H) if mode == rc.LOCAL else (H.shape[0] - 1, H.shape[1] - 1)
    return rc.reference_score(H, mode), (int(end[0]), int(end[1]))


_DENSE = {}


def dense_reference(key, profiles, gaps, ts, mode):
    """gaps[s]: the four sequences of profile s -> (int64 scores [profiles, ts], int64 end cells [.., .., 2]); computed once
    per (key, mode) — the key names the (profiles, gaps, templates) set — and read-only"""
    k = (key, mode)
    if k not in _DENSE:
        scores = np.zeros((len(profiles), len(ts)), np.int64)
        ends = np.zeros((len(profiles), len(ts), 2), np.int64)
        for i, p in enumerate(profiles):
            for j, t in enumerate(ts):
                scores[i, j], ends[i, j] = pair_reference(p, t, mode, gaps[i])
        scores.setflags(write=False)
        ends.setflags(write=False)
        _DENSE[k] = (scores, ends)
    return _DENSE[k]


# ---- gap rows --------------------------------------------------------------------------------------------------------------------
def constant(L, gi, ge):
    return [[gi] * (L + 1), [ge] * (L + 1), [gi] * (L + 1), [ge] * (L + 1)]


def random_rows(L, seed, lo=0, hi=12):
    """all four arrays random in lo..hi, differing row by row"""
    rng = np.random.RandomState(seed)
    return [rng.randint(lo, hi + 1, L + 1).tolist() for _ in range(4)]


def one_varied(L, which, seed, gi=11, ge=1):
    """array `which` (0 del_init, 1 del_extn, 2 ins_init, 3 ins_extn) random in 0..12, the others constant"""
    g = constant(L, gi, ge)
    g[which] = np.random.RandomState(seed).randint(0, 13, L + 1).tolist()
    return g


# ---- sequences ---------------------------------------------------------------------------------------------------------------------
def with_indels(s, seed, every=9):
    """s with a residue dropped or a short random run inserted every `every` residues: alignments to s need gaps of both kinds"""
    rng = np.random.RandomState(seed)
    out = []
    for k, ch in enumerate(s):
        if k % every == every - 1:
            if rng.randint(2):
                continue
            out.append(rc.random_seq(ALPHA, seed + k, int(rng.randint(1, 4))))
        out.append(ch)
    return "".join(out)


def homolog_set(rows, t_residues, seed):
    """-> (profiles, templates): perturbed profiles of `rows` interior rows from random sequences; templates of exactly
    `t_residues` residues each, cut from (or padded around) indel copies of those sequences in turn, so that every template has
    a profile it aligns to with gaps"""
    seqs = [rc.random_seq(ALPHA, seed + 10 * k, n) for k, n in enumerate(rows)]
    profiles = pc.perturbed(seqs, sc.TABLES["blosum62"], seed)
    ts = []
    for k, n in enumerate(t_residues):
        body = with_indels(seqs[k % len(seqs)], seed + 100 + k)
        pad = rc.random_seq(ALPHA, seed + 200 + k, max(n - len(body), 0))
        half = len(pad) // 2
        ts.append((pad[:half] + body + pad[half:])[:n])
        assert len(ts[-1]) == n
    return profiles, ts


# The variation set: small shapes, one (profiles, templates) set under seven kinds of gap rows
def small_set():
    return homolog_set((6, 9, 33), (1, 20, 37), 900)


def small_gaps(kind, profiles):
    """kind: 'del_init' | 'del_extn' | 'ins_init' | 'ins_extn' (that array varied alone), 'random' (all four, 0..12),
    'free_loop' (constant 11/1, one row with del_init = del_extn = 0), 'wall' (constant 4/1, one row whose four prices are 500)"""
    names = ("del_init", "del_extn", "ins_init", "ins_extn")
    out = []
    for s, p in enumerate(profiles):
        L = len(p)
        if kind in names:
            g = one_varied(L, names.index(kind), 910 + s)
        elif kind == "random":
            g = random_rows(L, 920 + s)
        elif kind == "free_loop":
            g = constant(L, 11, 1)
            g[0][L // 2] = g[1][L // 2] = 0
        elif kind == "wall":
            g = constant(L, 4, 1)
            for a in g:
                a[L // 2] = 500
        else:
            raise KeyError(kind)
        out.append(g)
    return out


SMALL_KINDS = ("del_init", "del_extn", "ins_init", "ins_extn", "random", "free_loop", "wall")


# The shape sets: gap values that differ row by row, so that a value taken from the wrong ring slot or chunk changes a score.
#   ring   profiles of 6, 7, 8, 9, 31, 32, 33 interior rows (the 8-row chunks and the 32-row ring of the kernels' staging)
#          against templates of T = 3, 256, 257, 258 columns (the boundary between length classes 1 and 2)
#   long   a 300-row profile (nine ring revolutions) against short templates, short profiles against T = 2048 columns (class 8)
def ring_set():
    profiles, ts = homolog_set((6, 7, 8, 9, 31, 32, 33), (1, 254, 255, 256), 930)
    return profiles, [random_rows(len(p), 940 + s) for s, p in enumerate(profiles)], ts


def long_set():
    p300, t_short = homolog_set((300,), (1, 40), 950)
    p_short, t_long = homolog_set((6, 9), (2046,), 960)
    return (p300, [random_rows(300, 951)], t_short), (p_short, [random_rows(len(p), 961 + s) for s, p in enumerate(p_short)], t_long)
