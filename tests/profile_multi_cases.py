"""Shared by tests/test_profile_multi_reference.py (CPU) and tests/test_gpu_hits_align_multi_profiles.py (GPU): the pairs
aln_hits_align_multi_profiles is tested on and what it must report for them.  A profile adds no rule to the rounds, only another
similarity plane, so the reference is multi_align_cases.rounds fed with profile_align_cases.plane: int64 planes and Python
integers only; aln_amd's library is not imported.

  derived cases            multi_align_cases' small, shape and cut cases as profiles of their queries (row i = the table row of
                           residue i), consensus = the query: the reference must equal the residue reference
  position-specific cases  integer rows that differ at EVERY position from the table row of the consensus letter, so that the
                           residue kernel over the consensus cannot pass: the builder asserts that the residue reference over
                           the consensus reports other lists.  Query sizes (sentinels counted) 3, 4, 9, 10, 17, 33, 34, 67, 130:
                           the staged 8-row chunk edges at rows 8 and 16, the 32-row ring's first wrap and its second at 64;
                           templates of the length classes 1, 2, 3 and 7 (multi_align_cases.SHAPE_T) and one of 2040 columns
  stale-ring case          Q = 67 against three copies: rounds 1 and 2 start in rows below 8 after a round that ended above row 40

Every case names the situations ("teeth") it was built for and reference() asserts that each of them occurs:
  rounds3      at least three reported rounds
  row1, col1, row7, row8, row9, row31, row32, row33, row64, col31, col32, col255, col256, col257
               a forbidden cell in that row / column while a later round runs
  stale_ring   rounds 1 and 2 are reported, each has an aligned pair in a row below 8, and the round before each ended in a row
               above 40
"""
import collections
import math

import numpy as np

import multi_align_cases as mac
import profile_align_cases as pac
import range_cases as rc

ALPHA, BLOSUM, AA = mac.ALPHA, mac.BLOSUM, mac.AA

PCase = collections.namedtuple("PCase", "name profile consensus t alpha gi ge N min_score teeth residue")

ROW_TEETH = (1, 7, 8, 9, 31, 32, 33, 64)
COL_TEETH = (1, 31, 32, 255, 256, 257)
QUERY_SIZES = (3, 4, 9, 10, 17, 33, 34, 67, 130)                   # sentinels counted
LONG_T = 2038                                                      # residues -> 2040 columns, class 8


def table_rows(alpha, table, q):
    tab = np.asarray(table)
    ti = tab.astype(np.int64)
    assert np.array_equal(ti.astype(tab.dtype), tab)
    return ti[[alpha.index(ch) for ch in q]].reshape(len(q), len(alpha))


def derived(case):
    """a multi_align_cases.Case as a profile of its query; `residue` keeps the case the reference must equal"""
    p = table_rows(case.alpha, case.table, case.q)
    p.setflags(write=False)
    return PCase(case.name, p, case.q, case.t, case.alpha, case.gi, case.ge, case.N, case.min_score, (), case)


_DERIVED = {}


def derived_small():
    if "small" not in _DERIVED:
        _DERIVED["small"] = [derived(c) for c in mac.small_cases() + [mac.cut_case()]]
    return _DERIVED["small"]


def derived_shapes():
    if "shape" not in _DERIVED:
        _DERIVED["shape"] = [derived(c) for c in mac.shape_cases()]
    return _DERIVED["shape"]


def _specific(name, L, tn, starts, seed, teeth):
    """A profile of L rows made from a hidden sequence p — the table rows of p's letters plus a seeded offset in {-1, 0, 1} per
    entry — with a consensus that is p with every second letter, the first included, replaced; a template of tn residues
    holding a noisy copy of p at each column of `starts` (column j is residue j - 1).  Three copies and N = 4: the cells of all three are forbidden while
    round 3 runs."""
    tab = BLOSUM.astype(np.int64)
    rng = np.random.RandomState(seed)
    p = rc.random_seq(AA, seed + 1, L)
    rows = table_rows(ALPHA, BLOSUM, p) + rng.randint(-1, 2, size=(L, len(ALPHA)))
    noise = rc.random_seq(AA, seed + 2, L)
    cons = "".join(noise[i] if i % 2 == 0 else p[i] for i in range(L))
    for i in range(L):                                             # differ from the consensus letter's table row at every position
        if np.array_equal(rows[i], tab[ALPHA.index(cons[i])]):
            rows[i, ALPHA.index(cons[i])] += 1
        assert not np.array_equal(rows[i], tab[ALPHA.index(cons[i])])
    rows.setflags(write=False)
    body = list(rc.random_seq(AA, seed + 3, tn))
    for k, s in enumerate(starts):
        copy = mac.mutated(p, seed + 10 + k, every=9 + 2 * k) if L >= 8 else p
        assert s >= 1 and s - 1 + L <= tn
        body[s - 1:s - 1 + L] = copy
    return PCase(name, rows, cons, "".join(body), ALPHA, 11, 1, 4, -math.inf, ("rounds3",) + tuple(teeth), None)


def specific_cases():
    if "specific" not in _DERIVED:
        T = mac.SHAPE_T
        row = lambda *r: tuple("row%d" % k for k in r)
        col = lambda *c: tuple("col%d" % k for k in c)
        out = [
            _specific("ps_Q3_R1", 1, T[1], (1, 31, 32), 7103, row(1) + col(1)),
            _specific("ps_Q4_R2", 2, T[2], (1, 31, 255), 7104, row(1) + col(1)),
            _specific("ps_Q9_R3", 7, T[3], (1, 28, 252), 7109, row(1, 7) + col(1, 31, 32, 255, 256, 257)),
            _specific("ps_Q10_R7", 8, T[7], (1, 26, 251), 7110, row(1, 7, 8) + col(1, 31, 32, 255, 256, 257)),
            _specific("ps_Q17_R1", 15, T[1], (1, 24, 100), 7117, row(1, 7, 8, 9) + col(1, 31, 32)),
            _specific("ps_Q33_R2", 31, T[2], (1, 60, 240), 7133, row(1, 7, 8, 9, 31) + col(1, 31, 255, 256, 257)),
            _specific("ps_Q34_R3", 32, T[3], (1, 120, 240), 7134, row(1, 8, 31, 32) + col(1, 255, 256, 257)),
            _specific("ps_Q67_R7", 65, T[7], (1, 200, 800), 7167, row(1, 7, 8, 9, 31, 32, 33, 64) + col(1, 31, 32, 255, 256, 257)),
            _specific("ps_Q130_R3", 128, T[3], (1, 200, 500), 7230, row(1, 7, 8, 9, 31, 32, 33, 64) + col(1, 31, 32, 255, 256, 257)),
        ]
        assert tuple(len(c.profile) + 2 for c in out) == QUERY_SIZES
        assert sorted({(len(c.t) + 2 + 255) // 256 for c in out}) == [1, 2, 3, 7]
        _DERIVED["specific"] = out
    return _DERIVED["specific"]


def long_case():
    """Q = 130 against 2040 columns (class 8): whatever route it takes"""
    if "long" not in _DERIVED:
        c = _specific("ps_Q130_T2040", 128, LONG_T, (1, 200, 1900), 7300, row_col_long())
        assert len(c.t) + 2 == 2040
        _DERIVED["long"] = c
    return _DERIVED["long"]


def row_col_long():
    return ("row1", "row64", "col1", "col255", "col256", "col257")


def stale_ring_case():
    """Q = 67, three copies: every round runs from a row below 8 to a row above 40, so rounds 1 and 2 read rows 1 .. 7 of the ring
    after a round whose last copies went into its other slots"""
    if "stale" not in _DERIVED:
        c = _specific("ps_stale_ring", 65, mac.SHAPE_T[2], (3, 120, 300), 7400, ("stale_ring", "row64"))
        _DERIVED["stale"] = c
    return _DERIVED["stale"]


def plane(case):
    return pac.plane(case.profile, case.t, case.alpha)


_REF = {}


def census(case, reported, ender):
    found = set()
    if len(reported) >= 3:
        found.add("rounds3")
    for r in reported + ([ender] if ender is not None else []):
        for i, j in r.forbidden:
            if i in ROW_TEETH:
                found.add("row%d" % i)
            if j in COL_TEETH:
                found.add("col%d" % j)
    Q, T = len(case.profile) + 2, len(case.t) + 2
    if len(reported) >= 3 and all(min(i for i, j in mac.interior(reported[a].pairs, Q, T)) < 8 and reported[a - 1].end[0] > 40
                                  for a in (1, 2)):
        found.add("stale_ring")
    return found


def reference(case, N=None):
    """-> (reported rounds, ender): multi_align_cases.rounds on the profile's int64 plane, computed once per (case, N), never
    modified.  Asserts the case's teeth; for a position-specific case also that the residue reference over the consensus reports
    other lists; for a derived case that it reports the same."""
    N = case.N if N is None else N
    key = (case.name, N)
    if key not in _REF:
        reported, ender = mac.rounds(plane(case), case.gi, case.ge, N, case.min_score)
        if N == case.N:
            missing = set(case.teeth) - census(case, reported, ender)
            assert not missing, (case.name, sorted(missing))
            if case.residue is None:
                other, _ = mac.rounds(rc.sim_int(case.consensus, case.t, ALPHA, BLOSUM), case.gi, case.ge, N, case.min_score)
                assert [r.pairs.tolist() for r in other] != [r.pairs.tolist() for r in reported], case.name
        _REF[key] = (reported, ender)
    return _REF[key]


def same_rounds(a, b):
    return len(a) == len(b) and all(x.score == y.score and np.array_equal(x.pairs, y.pairs) for x, y in zip(a, b))


def oracle_rounds(case, N=None):
    """the same loop on the oracle: orc.dp_build + orc.optimal on the masked float32 profile plane of every round"""
    import orc
    S = plane(case).astype(np.float32)
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
        forb += mac.interior(pl, Q, T)
    return out
