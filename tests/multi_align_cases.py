"""Shared by tests/test_multi_align_reference.py (CPU) and tests/test_gpu_hits_align_multi.py (GPU): the pairs
aln_hits_align_multi is tested on, and what it must report for them, restated on the int64 planes of
range_cases.affine_reference with lean_cases' find_max and local walk.  Python integers and int64 only; aln_amd's library is
not imported, so no reference value can share a sweep, a mask layout or a walk with the kernel.

The rule (include/aln_hip.h): round 0 is Optimal's alignment; round a >= 1 is Optimal's alignment of the matrix built from the
similarity plane in which every aligned pair (1 <= i <= Q-2, 1 <= j <= T-2) of the rounds before holds -(round 0's score + 1);
a round is reported when its score is >= min_score and, after round 0, > 0; the first round that is not ends the hit.

Every case names the situations ("teeth") it was built for, and reference() asserts on the CPU that each of them really
occurs.  The teeth:
  rounds3        at least three reported rounds
  stop_diag      a round whose walk stops because the diagonal predecessor of its first cell is a forbidden cell
  stop_after_del / stop_after_ins
                 the same, and that first cell was itself reached by a deletion / insertion jump.  (A walk can not stop AT a
                 forbidden cell reached as a gap source: such a cell holds 0, a gap from it offers 0 - cost <= 0, the diagonal
                 candidate is >= 0 and comes first, and a later candidate wins only when strictly greater (dpmatrix.h:607-649).
                 test_multi_align_reference.py asserts that over every case; these two teeth are the nearest thing that exists.)
  jump_over      a deletion or insertion jump of a later round that passes over a forbidden cell of its source row / column
  row1, col1     a forbidden cell in row 1 / column 1 (column 1 is also the first interior column of lane 0 in the kernel's
                 layout, column 256 the first column of lane 0 in the second group)
  col31 col32 col255 col256 col257
                 a forbidden cell in that column: both sides of a mask word and of a column group
  tie_rounds     two consecutive rounds of equal score: find_max's first-row-major rule decides their order
  seed_zero_end  the hit ends with a round of score 0, whose end cell is the seed (Q-2, T-2), and which is not reported
  min_score_cut  min_score lies between the scores of two rounds that would otherwise both be reported
"""
import collections
import math

import numpy as np

import lean_cases as lc
import range_cases as rc

ALPHA, BLOSUM = rc.load_blosum62()
AA = ALPHA[:20]

Case = collections.namedtuple("Case", "name q t alpha table gi ge N min_score teeth")
Round = collections.namedtuple("Round", "score pairs end forbidden H")          # forbidden: the cells masked WHEN the round ran


def tie_table(alpha):
    t = np.full((len(alpha), len(alpha)), -1, np.float32)
    np.fill_diagonal(t, 2)
    return t


def interior(pairs, Q, T):
    return [(int(i), int(j)) for i, j in pairs if 1 <= i <= Q - 2 and 1 <= j <= T - 2]


def masked(S, forbidden, value, variant=None):
    Sa = np.array(S, np.int64)
    for i, j in forbidden:
        if variant == "forget_borders" and (i == 1 or j == 1):
            continue
        Sa[i, j] = value
    return Sa


def walk(H, gi, ge, through=frozenset()):
    """optimal.h:79-105 on the plane H.  `through`: cells the walk does NOT stop before although they hold 0 — the wrong variant
    "forbids, but lets the walk continue through zero cells"; empty: lean_cases.reference_list."""
    if not through:
        return lc.reference_list(H, gi, ge)
    Q, T = H.shape
    q, t = lc.find_max_cell(H)
    lst = [(Q - 1, T - 1), (q, t)]
    while q > 0:
        q, t = lc.predecessor(H, q, t, gi, ge)
        if H[q, t] <= 0 and (q, t) not in through:
            break
        lst.append((q, t))
    if q != 0 and t != 0:
        lst.append((0, 0))
    return np.array(lst[::-1], np.int32).reshape(-1, 2)


def rounds(S, gi, ge, N, min_score=-math.inf, variant=None):
    """-> (reported rounds, the round that ended the hit or None): int64 planes, Python ints.  variant: None, or one of the two
    deliberately wrong rules of the sensitivity tests ("forget_borders", "walk_through")."""
    S = np.asarray(S, np.int64)
    Q, T = S.shape
    assert Q >= 3 and T >= 3
    forb, out, value = [], [], 0
    for a in range(N):
        H = rc.affine_reference(masked(S, forb, value, variant), rc.LOCAL, gi, ge)[0]
        end = lc.find_max_cell(H)
        score = int(H[end])
        if not (score >= min_score and (a == 0 or score > 0)):
            return out, Round(score, None, end, frozenset(forb), H)
        pl = walk(H, gi, ge, frozenset(forb) if variant == "walk_through" else frozenset())
        out.append(Round(score, pl, end, frozenset(forb), H))
        if a == 0:
            value = -(score + 1)
        forb = forb + interior(pl, Q, T)
    return out, None


def census(case, reported, ender):
    """-> the set of teeth that occur in the reference's rounds of the case"""
    found = set()
    gi, ge = case.gi, case.ge
    if len(reported) >= 3:
        found.add("rounds3")
    if ender is not None and ender.score == 0 and ender.end == (ender.H.shape[0] - 2, ender.H.shape[1] - 2) and reported:
        found.add("seed_zero_end")
    for r in reported + ([ender] if ender is not None else []):     # every round that ran, the one that ended the hit included
        for i, j in r.forbidden:
            if i == 1:
                found.add("row1")
            if j in (1, 31, 32, 255, 256, 257):
                found.add("col%d" % j)
    for a, r in enumerate(reported):
        Q, T = r.H.shape
        if a > 0 and reported[a - 1].score == r.score:
            found.add("tie_rounds")
            assert reported[a - 1].end < r.end or reported[a - 1].end == (Q - 2, T - 2)     # row-major order, or the seed's privilege
        if a == 0:
            continue
        pl = [tuple(int(v) for v in p) for p in r.pairs]
        if pl[0] == (0, 0):                                          # stopped before a cell with both indices > 0
            first = pl[1]
            p = lc.predecessor(r.H, first[0], first[1], gi, ge)
            if p in r.forbidden:
                assert p == (first[0] - 1, first[1] - 1)             # never a gap source (see the module docstring)
                found.add("stop_diag")
                nxt = pl[2]
                if nxt != (Q - 1, T - 1) and nxt[0] == first[0] + 1 and nxt[1] > first[1] + 1:
                    found.add("stop_after_del")
                if nxt != (Q - 1, T - 1) and nxt[1] == first[1] + 1 and nxt[0] > first[0] + 1:
                    found.add("stop_after_ins")
        cells = [p for p in pl if p != (0, 0) and p != (Q - 1, T - 1)]
        for (i0, j0), (i1, j1) in zip(cells[:-1], cells[1:]):
            if i1 == i0 + 1 and j1 > j0 + 1 and any((i0, k) in r.forbidden for k in range(j0 + 1, j1)):
                found.add("jump_over")
            if j1 == j0 + 1 and i1 > i0 + 1 and any((k, j0) in r.forbidden for k in range(i0 + 1, i1)):
                found.add("jump_over")
    return found


def mutated(s, seed, every=7):
    return lc.mutated(ALPHA, s, seed, every=every)


def _domain_cases():
    d40 = rc.random_seq(AA, 301, 40)
    e40 = rc.random_seq(AA, 302, 40)
    f = lambda seed, n: rc.random_seq(AA, seed, n)
    three = d40 + f(303, 9) + d40 + f(304, 13) + d40
    d12 = rc.random_seq(AA, 310, 12)
    wide = d12 + f(311, 13) + d12 + f(312, 212) + d12 + f(313, 40)     # copies at columns 1-12, 26-37, 250-261
    assert wide[25:37] == d12 and wide[249:261] == d12
    unit = rc.random_seq(AA, 320, 9)
    tandem = unit * 6
    shuf_q, shuf_t = d40 + e40, mutated(e40, 330) + f(331, 20) + mutated(d40, 332)
    b = [
        Case("three_in_query", three, d40, ALPHA, BLOSUM, 11, 1, 4, -math.inf, ("rounds3", "tie_rounds", "col1", "row1")),
        Case("three_in_template", d40, three, ALPHA, BLOSUM, 11, 1, 4, -math.inf, ("rounds3", "tie_rounds", "col1", "row1", "col31", "col32")),
        Case("tandem_self", tandem, tandem, ALPHA, BLOSUM, 11, 1, 4, -math.inf, ("rounds3", "row1", "col1", "col31", "col32")),
        Case("shuffled_domains", shuf_q, shuf_t, ALPHA, BLOSUM, 11, 1, 4, -math.inf, ()),
        Case("wide_columns", d12, wide, ALPHA, BLOSUM, 11, 1, 4, -math.inf,
             ("rounds3", "row1", "col1", "col31", "col32", "col255", "col256", "col257", "tie_rounds")),
        Case("single_cell", "W", "W", ALPHA, BLOSUM, 11, 1, 4, -math.inf, ("seed_zero_end", "row1", "col1")),
        Case("all_negative", "WWWW", "CCCCC", ALPHA, BLOSUM, 11, 1, 4, -math.inf, ()),
    ]
    return b


def _tie_cases():
    """low-complexity pairs over small alphabets under the tie table and the gap families of range_cases: crossing diagonals,
    cheap gaps, equal scores"""
    out = []
    for alpha in ("AC", "ACGT"):
        for gi, ge in ((11, 1), (0, 0), (40, 0), (1, 5), (0, 1)):
            for seed in range(3):
                rs = np.random.RandomState(9000 + seed)
                q = lc_low(4100 + seed, rs.randint(20, 61), alpha)
                t = lc_low(4200 + seed, rs.randint(20, 61), alpha)
                out.append(Case("tie_%s_%d_%d_%d" % (alpha, gi, ge, seed), q, t, alpha, tie_table(alpha), gi, ge, 4, -math.inf, ()))
    for seed, tooth in ((40, "stop_after_del"), (54, "stop_after_ins")):     # found by scanning seeds 0 .. 59 on the CPU
        rs = np.random.RandomState(9000 + seed)
        q = lc_low(4100 + seed, rs.randint(20, 61), "ACGT")
        t = lc_low(4200 + seed, rs.randint(20, 61), "ACGT")
        out.append(Case("tie_ACGT_0_0_%d" % seed, q, t, "ACGT", tie_table("ACGT"), 0, 0, 4, -math.inf, ("stop_diag", tooth)))
    return out


def lc_low(seed, n, alpha):
    rs = np.random.RandomState(seed)
    if rs.randint(3) == 0:
        unit = "".join(alpha[x] for x in rs.randint(len(alpha), size=rs.randint(1, 4)))
        s = list((unit * (n // len(unit) + 1))[:n])
        for _ in range(rs.randint(0, 4)):
            s[rs.randint(n)] = alpha[rs.randint(len(alpha))]
        return "".join(s)
    return "".join(alpha[x] for x in rs.randint(len(alpha), size=n))


# teeth the tie cases must show AS A GROUP (which of them shows which is a matter of the seeds; the group is what is asserted)
TIE_GROUP_TEETH = ("stop_diag", "stop_after_del", "stop_after_ins", "jump_over", "tie_rounds", "rounds3")


def small_cases():
    """every case the oracle can build (all of them are far below 300 x 700)"""
    return _domain_cases() + _tie_cases()


SHAPE_T = {1: 200, 2: 400, 3: 700, 7: 1700}                          # residues -> columns 202, 402, 702, 1702: classes 1, 2, 3, 7
SHAPE_Q = (3, 4, 17, 130)                                            # sentinels counted


def shape_cases():
    """Q = 3, 4, 17, 130 against templates of the length classes 1, 2, 3 and 7 (the largest kept): two noisy copies of the query,
    one at the template's head and one in its last columns"""
    out = []
    for R, tn in SHAPE_T.items():
        for Q in SHAPE_Q:
            q = rc.random_seq(AA, 500 + Q, Q - 2)
            body = rc.random_seq(AA, 600 + R, tn)
            c1, c2 = mutated(q, 700 + Q + R, every=9), mutated(q, 800 + Q + R, every=11)
            if 2 * len(q) + 3 <= tn:
                t = c1 + body[len(q):tn - len(q) - 3] + c2 + body[tn - 3:]
            else:                                                    # no room for two: one copy at the head
                t = c1 + body[len(q):]
            assert len(t) == tn and (tn + 2 + 255) // 256 == R
            out.append(Case("shape_Q%d_R%d" % (Q, R), q, t, ALPHA, BLOSUM, 11, 1, 4, -math.inf, ()))
    return out


def cut_case():
    """min_score between round 0's and round 1's score of shuffled_domains"""
    base = [c for c in _domain_cases() if c.name == "shuffled_domains"][0]
    reported, _ = reference(base)
    assert len(reported) >= 2 and reported[0].score > reported[1].score > 0
    ms = (reported[0].score + reported[1].score) / 2.0
    return base._replace(name="min_score_cut", min_score=ms, teeth=("min_score_cut",))


_REF = {}


def sim(case):
    return rc.sim_int(case.q, case.t, case.alpha, case.table)


def reference(case, N=None):
    """-> (reported rounds, ender) of the case, computed once per (case, N), never modified; asserts the case's teeth"""
    N = case.N if N is None else N
    key = (case.name, N, case.min_score)
    if key not in _REF:
        reported, ender = rounds(sim(case), case.gi, case.ge, N, case.min_score)
        if N == case.N:
            found = census(case, reported, ender)
            if "min_score_cut" in case.teeth:
                free, _ = rounds(sim(case), case.gi, case.ge, N)
                assert len(free) > len(reported) >= 1 and free[len(reported)].score < case.min_score <= reported[-1].score
                found.add("min_score_cut")
            missing = set(case.teeth) - found
            assert not missing, (case.name, sorted(missing), sorted(found))
        _REF[key] = (reported, ender)
    return _REF[key]


def oracle_rounds(case, N=None):
    """the same loop on the oracle: orc.dp_build + orc.optimal on the masked float32 plane of every round"""
    import orc
    S = orc.sim_submatrix(case.q, case.t, case.alpha, case.table)
    Q, T = S.shape
    assert Q * T <= 300 * 700
    forb, out, value = [], [], 0.0
    for a in range(case.N if N is None else N):
        Sa = np.array(S, np.float32)
        for i, j in forb:
            Sa[i, j] = value
        rc_, D, PQ, PT = orc.dp_build(Sa, orc.Gap(orc.LOCAL, case.gi, case.ge))
        rc2, sc, pl = orc.optimal(D, PQ, PT, True)
        assert rc_ == 0 and rc2 == 0
        if not (sc >= case.min_score and (a == 0 or sc > 0)):
            break
        out.append((sc, pl))
        if a == 0:
            value = -(float(sc) + 1.0)
        forb += interior(pl, Q, T)
    return out
