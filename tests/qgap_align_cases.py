"""Shared by tests/test_qgap_align_reference.py (CPU) and tests/test_gpu_qgap_align.py (GPU): the ALIGNMENT under position-specific
gap penalties (aln_hits_align_profiles_gaps, include/aln_hip.h), restated in int64 straight from the definition over
qgap_cases.qgap_planes — the pointer of every cell as "match, deletions k ascending, insertions k ascending, a later candidate
only when strictly greater", the list of each align type —, a path scorer that shares nothing with the pointer rule, a census
of what a set of lists went through, and the case sets of the GPU test.  numpy and the existing case modules only.

Gap rows are qgap_cases': four sequences of L + 1 values (rows 0 .. L = Q-2) per profile; with_tail() appends the '$' row's.
"""
import numpy as np

import lean_cases as lc
import profile_align_cases as pac
import profile_cases as pc
import qgap_cases as qg
import range_cases as rc

ALPHA = pc.ALPHA


def dele(g, i, L):
    """del(i, L): L template residues skipped between rows i and i+1"""
    return int(g[0][i]) + int(g[1][i]) * (L - 1)


def inse(g, a, b):
    """ins(a, b): profile positions a..b skipped, every one at its own price"""
    return int(g[2][a]) + sum(int(g[3][p]) for p in range(a + 1, b + 1))


# ---- the pointer rule ------------------------------------------------------------------------------------------------------------
def candidates(H, g, i, j):
    """interior cell (i, j), i, j >= 2 -> [(value, source)] in the definition's order"""
    out = [(int(H[i - 1, j - 1]), (i - 1, j - 1))]
    out += [(int(H[i - 1, k]) - dele(g, i - 1, j - 1 - k), (i - 1, k)) for k in range(1, j - 1)]
    out += [(int(H[k, j - 1]) - inse(g, k + 1, i - 1), (k, j - 1)) for k in range(1, i - 1)]
    return out


def final_candidates(H, g, fdel, fins):
    Q, T = H.shape
    out = [(int(H[Q - 2, T - 2]), (Q - 2, T - 2))]
    out += [(int(H[Q - 2, k]) - (0 if fdel else dele(g, Q - 2, T - 2 - k)), (Q - 2, k)) for k in range(1, T - 2)]
    out += [(int(H[k, T - 2]) - (0 if fins else inse(g, k + 1, Q - 2)), (k, T - 2)) for k in range(1, Q - 2)]
    return out


def winner(cands):
    """the first candidate no later one strictly exceeds"""
    best = cands[0]
    for c in cands[1:]:
        if c[0] > best[0]:
            best = c
    return best


def pointer(H, g, i, j):
    if i == 1 or j == 1:
        return (0, 0)
    return winner(candidates(H, g, i, j))[1]


def tied(cands):
    """do the two best candidates tie?"""
    v = sorted((c[0] for c in cands), reverse=True)
    return len(v) >= 2 and v[0] == v[1]


# ---- the lists -------------------------------------------------------------------------------------------------------------------
def planes(profile, t, mode, gaps, alpha=ALPHA):
    g = [qg.with_tail(a) for a in gaps]
    return qg.qgap_planes(pac.plane(profile, t, alpha), mode, *g), g


def restated(profile, t, mode, gaps, end=None, alpha=ALPHA):
    """-> (score int, list int32 [n, 2] in list order).  ALN_LOCAL: the list from the end cell `end` (None: find_max's) and the
    score of that cell.  A pair without an interior: the list the header states for it."""
    H, g = planes(profile, t, mode, gaps, alpha)
    Q, T = H.shape
    fdel, fins = rc.free_ends(mode)
    if mode == rc.LOCAL:
        q, t_ = (int(end[0]), int(end[1])) if end is not None else lc.find_max_cell(H)
        lst = [(Q - 1, T - 1), (q, t_)]
        score = int(H[q, t_])
        while q > 0:
            if t_ <= 0:                                        # an empty template: the seed's column holds no cell
                q, t_ = -1, -1
                break
            q, t_ = pointer(H, g, q, t_)
            if H[q, t_] <= 0:
                break
            lst.append((q, t_))
        if q != 0 and t_ != 0:
            lst.append((0, 0))
        return score, np.array(lst[::-1], np.int32).reshape(-1, 2)
    score = int(H[Q - 1, T - 1])
    if Q == 2 or T == 2:
        return score, np.array([(0, 0), (Q - 1, T - 1)], np.int32)
    v, (i, j) = winner(final_candidates(H, g, fdel, fins))
    assert v == score
    lst = [(Q - 1, T - 1), (i, j)]
    while (i, j) != (0, 0):
        i, j = pointer(H, g, i, j)
        lst.append((i, j))
    return score, np.array(lst[::-1], np.int32).reshape(-1, 2)


# ---- the path scorer: from a list alone ------------------------------------------------------------------------------------------
def path_score(profile, t, mode, gaps, pl, alpha=ALPHA):
    """The score the list stands for by the definition: S over its interior entries, minus del / ins of every jump between
    consecutive entries, minus the end gaps unless free.  Shares nothing with the pointer rule.  ALN_LOCAL: the entries between
    (0,0) — where the list has it — and the final pair, no end gap charged."""
    S = pac.plane(profile, t, alpha)
    Q, T = S.shape
    g = [qg.with_tail(a) for a in gaps]
    fdel, fins = rc.free_ends(mode)
    L = [(int(a), int(b)) for a, b in np.asarray(pl).reshape(-1, 2)]
    assert L[-1] == (Q - 1, T - 1)
    inner = [c for c in L[:-1] if 1 <= c[0] <= Q - 2 and 1 <= c[1] <= T - 2]
    local = mode == rc.LOCAL
    if not local:
        assert L[0] == (0, 0) and inner == L[1:-1]
    total = sum(int(S[c]) for c in inner)

    def jump(a, b, head, tail):
        di, dj = b[0] - a[0], b[1] - a[1]
        assert di >= 1 and dj >= 1 and (di == 1 or dj == 1), (a, b)
        if dj > 1:                                             # a deletion, priced by the row it leaves
            return 0 if ((head or tail) and fdel) else dele(g, a[0], dj - 1)
        if di > 1:                                             # an insertion of positions a+1 .. b-1
            return 0 if ((head or tail) and fins) else inse(g, a[0] + 1, b[0] - 1)
        return 0

    if local:
        for a, b in zip(inner[:-1], inner[1:]):
            total -= jump(a, b, False, False)
        return total
    if not inner:                                              # no interior: one end gap
        if Q == 2:
            return 0 if (fdel or T == 2) else -dele(g, 0, T - 2)
        return 0 if fins else -inse(g, 1, Q - 2)
    total -= jump((0, 0), inner[0], True, False)
    for a, b in zip(inner[:-1], inner[1:]):
        total -= jump(a, b, False, False)
    total -= jump(inner[-1], (Q - 1, T - 1), False, True)
    return total


def check_path(profile, t, mode, gaps, pl, score, alpha=ALPHA):
    """the path scorer against a reported score; a local score of 0 goes with the lone seed cell, which is no alignment"""
    if mode == rc.LOCAL and score <= 0:
        Q, T = len(profile) + 2, len(t) + 2
        L = [tuple(c) for c in np.asarray(pl).reshape(-1, 2).tolist()]
        assert score == 0 and L[-1] == (Q - 1, T - 1) and (len(L) == 2 or (len(L) == 3 and L[0] == (0, 0))), (L, score)
        return
    got = path_score(profile, t, mode, gaps, pl, alpha)
    assert got == score, (mode, got, score, np.asarray(pl).tolist())


# ---- census ----------------------------------------------------------------------------------------------------------------------
COUNTERS = ("del_jumps", "ins_jumps", "long_jumps", "ties", "final_del", "final_ins", "local_stops")
NONLOCAL_COUNTERS = ("del_jumps", "ins_jumps", "long_jumps", "ties", "final_del", "final_ins")
LOCAL_COUNTERS = ("del_jumps", "ins_jumps", "long_jumps", "ties", "local_stops")


def new_census():
    return dict.fromkeys(COUNTERS, 0)


def census(profile, t, mode, gaps, pl, into, alpha=ALPHA):
    """adds what the list pl went through to the counters of `into`"""
    H, g = planes(profile, t, mode, gaps, alpha)
    Q, T = H.shape
    if Q < 3 or T < 3:
        return
    fdel, fins = rc.free_ends(mode)
    L = [(int(a), int(b)) for a, b in np.asarray(pl).reshape(-1, 2)]
    inner = [c for c in L[:-1] if 1 <= c[0] <= Q - 2 and 1 <= c[1] <= T - 2]
    for a, b in zip(inner[:-1], inner[1:]):
        di, dj = b[0] - a[0], b[1] - a[1]
        into["del_jumps"] += int(dj > 1)
        into["ins_jumps"] += int(di > 1)
        into["long_jumps"] += int(max(di, dj) >= 3)            # two or more skipped
    for c in inner:
        if c[0] >= 2 and c[1] >= 2:
            into["ties"] += int(tied(candidates(H, g, c[0], c[1])))
    if mode == rc.LOCAL:
        into["local_stops"] += int(L[0] == (0, 0) and inner[0][0] > 1 and inner[0][1] > 1)
    else:
        last = inner[-1]
        into["final_del"] += int(last[0] == Q - 2 and last[1] < T - 2)
        into["final_ins"] += int(last[1] == T - 2 and last[0] < Q - 2)
        into["ties"] += int(tied(final_candidates(H, g, fdel, fins)))


def applies(mode):
    return LOCAL_COUNTERS if mode == rc.LOCAL else NONLOCAL_COUNTERS


# ---- the case sets of the GPU test -------------------------------------------------------------------------------------------------
TIE_ALPHA = "ACGT"
TIE_SEEDS = (0, 1, 2)


def tie_set():
    """profile_align_cases.tie_profiles over ACGT (low-complexity sequences under a +2 / -1 table, every entry perturbed by
    -1..1) with small gap values: rows random in 0..2, so that candidates tie all the time
    -> (profiles, consensus, templates, gaps)"""
    profiles, qs, ts = pac.tie_profiles(TIE_ALPHA)
    gaps = [qg.random_rows(len(p), 980 + s, 0, 2) for s, p in enumerate(profiles)]
    return profiles, qs, ts, gaps


def all_pairs(n_q, n_t):
    """every (profile, template) pair as a hit list: hits[r][k].t = k"""
    return [(r, k) for r in range(n_q) for k in range(n_t)]


_LISTS = {}


def reference_lists(key, profiles, gaps, ts, mode, alpha=ALPHA):
    """(score, list) of every pair of a set, local lists from find_max's cell; computed once per (key, mode), read-only"""
    k = (key, mode)
    if k not in _LISTS:
        out = {}
        for r, p in enumerate(profiles):
            for c, t in enumerate(ts):
                score, pl = restated(p, t, mode, gaps[r], alpha=alpha)
                pl.setflags(write=False)
                out[r, c] = (score, pl)
        _LISTS[k] = out
    return _LISTS[k]


def final_pointer_cases():
    """Three pairs (profile, gaps, template, align type, what) whose final cell's pointer is pinned by construction; the CPU
    test checks each property on the restatement, the GPU test runs them."""
    n = len(ALPHA)

    def prof(letters, hi=5, lo=-4):
        p = np.full((len(letters), n), lo, np.int64)
        for i, ch in enumerate(letters):
            p[i, ALPHA.index(ch)] = hi
        return p

    A, C, D = ALPHA[0], ALPHA[1], ALPHA[2]
    # 1. a tail deletion priced by row Q-2 alone: the profile matches the template's head, the tail of 6 residues is skipped
    #    from row Q-2, whose prices are 1 / 0 while every other row's are 50
    p1 = prof(A + C + D + A)
    t1 = A + C + D + A + C * 6
    g1 = qg.constant(4, 50, 50)
    g1[0][4], g1[1][4] = 1, 0
    # 2. a tail insertion whose winner changes with one ins_extn[p]: the template matches the profile's head, rows 3..6 all
    #    like its last letter (row 3 best), and the price of skipping the rows below decides which of them ends the alignment
    p2 = np.vstack([prof(A + C), prof(D, hi=4), prof(D * 3, hi=3)])
    t2 = A + C + D
    g2 = qg.constant(6, 2, 1)
    g2b = [list(a) for a in g2]
    g2b[3][5] = 7                                              # skipping position 5 becomes dear
    # 3. a free-tail tie the smallest row must win: rows 2 and 4 reach column T-2 with the same score (the head insertion is
    #    free too), row Q-2 matches nothing
    p3 = np.vstack([prof(A + C + A + C), np.full((1, n), -4, np.int64)])
    t3 = A + C
    g3 = qg.constant(5, 3, 1)
    return [(p1, g1, t1, rc.GLOBAL, "del_row_Q-2"), (p2, g2, t2, rc.GLOBAL, "ins_cheap"), (p2, g2b, t2, rc.GLOBAL, "ins_dear"),
            (p3, g3, t3, rc.GLOBAL_LOCAL, "free_tail_tie")]
