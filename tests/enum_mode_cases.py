"""Shared by tests/test_enum_mode_reference.py (CPU), tests/test_gpu_enumerate_modes.py (GPU) and oracle/gen_golden.py: the
pairs, gap families and search parameters on which near-optimal enumeration is tested in the two ONE-SIDED align types
(GLOBAL_LOCAL 0 frees query end gaps only, LOCAL_GLOBAL 2 template end gaps only), under the position-dependent gap models,
and past the first 1024-candidate trip of the one-wave constant-gap scan.  Oracle and numpy only: the HIP library is never
loaded here.

A pair is a mutated homolog core (aln_amd.synth.homolog_pair) with random flanks on ONE of the two sequences, so that one
align type frees the overhang and its mirror image does not.  Every case names the situations ("teeth") it was built for, and
check() asserts on the oracle that each of them really occurs:

  end_rule     the oracle's search on the SAME planes with the mirrored align type (2 - mode: free deletions and free insertions
               swapped, the planes still built under `mode`) returns a different set.  Asserted for modes 0 and 2, every gap
               family but constant 0/0 (all gap costs are 0 there, so the end rule cannot change a cost or a set; that family
               sits on the gi >= 0 && ge >= 0 guard of the pruned scans instead), every kind.
  far_block    some alignment leaves the final cell (Q-1, T-1) by a jump longer than 128 cells: it passes two whole 64-cell
               blocks of the pruned scans
  head_jump    some alignment's first aligned pair lies more than 128 columns (rows) from the origin
  second_trip  some alignment leaves the final cell — always a branch node of cw — by a candidate whose scan index
               (match 0, deletions 1 .. ndel, insertions after them: 1 + ndel + (q0 - 2 - q)) is at least 1024
  resume       the set holds alignments the search created from candidates of the final cell on BOTH sides of index 1024: the
               scan of that node was left with an accepted candidate and resumed from its cursor into the second trip.
               (trip2 alone cannot show a scan that stops after its first trip: at delta 0.002 nothing but the optimal path passes,
               and a node where nothing passes falls back to the stored pointers, which name the same cell.  trip2_resume is the
               same pair at delta 0.03, where indices 1021 .. 1039 are accepted.)
far_block, head_jump and second_trip are asserted in the align type that frees the case's overhang (2 for t_*, 0 for q_* and
trip2), again under every gap family but constant 0/0: where no gap costs anything the best alignments collect scattered
matches all over the flank instead of jumping over it.  second_trip counts only alignments the search itself created (uid
not -1: the caller's seed alignment, Optimal's, is in the set too).  Besides the teeth: every search returns status 0, takes less than 5 s and yields at least 2 alignments.

A case that misses a tooth gets another seed, never a weaker tooth; the seeds below were found by scanning on the CPU.
"""
import collections
import time

import numpy as np

import gap_tables
import orc
import range_cases as rc
from aln_amd.synth import homolog_pair

ALPHA, BLOSUM = rc.load_blosum62()

Case = collections.namedtuple("Case", "name q t free_mode teeth")
Found = collections.namedtuple("Found", "status seconds alis")

MODES_ONE_SIDED = (0, 2)
MODES_ALL = (0, 1, 2, 3, 4)
KINDS = ("cw", "ucw", "kscw", "crcw")
CONST = collections.OrderedDict((("g11_1", (11, 1)), ("g4.73_0.34", (4.73, 0.34)), ("g0_0", (0, 0))))
GOLDEN_FAMILIES = ("g11_1", "g4.73_0.34")                     # pinned to the real reference in tests/golden/enum_modes.json
POSITION = ("tpos", "gn2", "tables")
K_LIMIT, SORT_LIMIT, MAX_OVERLAP = 4, 10, 0.3
TIME_LIMIT_S = 5.0
REFERENCE_UCW_LIMIT = 100000                                  # ucw.h:72

# name -> (seed of the core, flanked sequence, residues at the head, at the tail, teeth).  Seeds: the first of 7000, 7001, ...
# with which every search of the case meets every condition above (scanned on the CPU).
_SMALL = collections.OrderedDict((
    ("t_over8", (7000, "t", 8, 8, ("end_rule",))),
    ("q_over8", (7000, "q", 8, 8, ("end_rule",))),
    ("t_tail140", (7000, "t", 8, 140, ("end_rule", "far_block"))),
    ("q_tail140", (7000, "q", 8, 140, ("end_rule", "far_block"))),
    ("t_head140", (7001, "t", 140, 8, ("end_rule", "head_jump"))),
    ("q_head140", (7001, "q", 140, 8, ("end_rule", "head_jump"))),
))
_TRIP2_SEED = 7100


def _flanked(name, seed, side, head, tail, teeth, core=30):
    q, t = homolog_pair(seed, core, sub_rate=0.25, indel=2)
    fh, ft = rc.random_seq(ALPHA, 2 * seed + 1, head), rc.random_seq(ALPHA, 2 * seed + 2, tail)
    if side == "t":
        return Case(name, q, fh + t + ft, 2, teeth)
    return Case(name, fh + q + ft, t, 0, teeth)


def small_cases():
    """the six small pairs: about 32 x 48 and 32 x 180 cells with the sentinels"""
    return [_flanked(name, *spec) for name, spec in _SMALL.items()]


def over8_cases():
    return [c for c in small_cases() if c.name.endswith("_over8")]


def trip2_case():
    """1042 x 902 cells: a 900-residue core plus a 140-residue query tail; mode 0, constant 11/1, cw only"""
    return _flanked("trip2", _TRIP2_SEED, "q", 0, 140, ("second_trip",), core=900)


def trip2_resume_case():
    """the pair (and so the planes) of trip2, searched with a wider threshold"""
    return trip2_case()._replace(name="trip2_resume", teeth=("second_trip", "resume"))


def case(name):
    return [c for c in small_cases() + [trip2_case(), trip2_resume_case()] if c.name == name][0]


def dims(c):
    return len(c.q) + 2, len(c.t) + 2


def kinds(fam):
    return ("cw", "kscw") if fam == "g0_0" else KINDS


def params(c, fam, kind):
    """-> dict(nsub, delta, regions, user_limit): user_limit is explicit everywhere (unbounded ucw runs for minutes)"""
    if c.name.startswith("trip2"):
        return dict(nsub=20, delta=0.002 if c.name == "trip2" else 0.03, regions=2, user_limit=300)
    return dict(nsub=20, delta=0.05 if kind == "ucw" else 0.3, regions=3, user_limit=40 if fam == "g0_0" else 300)


def flags(c, fam="g11_1", kind="cw"):
    return orc.make_subopt_regions(dims(c)[1], params(c, fam, kind)["regions"])


def _stable(name):
    return sum((k + 1) * ord(ch) for k, ch in enumerate(name))


_ARRAYS = {}


def gap_arrays(c, fam):
    """The seeded per-template arrays of a position-dependent family (independent of the align type)."""
    key = (c.name, fam)
    if key not in _ARRAYS:
        T = dims(c)[1]
        rs = np.random.RandomState(40000 + _stable(c.name))
        if fam == "tpos":
            a = {"tgi": rs.uniform(6, 12, T).astype(np.float32), "tge": rs.uniform(0.5, 1.5, T).astype(np.float32)}
        elif fam == "gn2":
            a = gap_tables.gn2_tables(rs, T)
        elif fam == "tables":
            a = {"tgi": rs.uniform(2.0, 6.0, T).astype(np.float32), "tge": rs.uniform(0.1, 0.6, T).astype(np.float32)}
        else:
            raise KeyError(fam)
        _ARRAYS[key] = a
    return _ARRAYS[key]


def oracle_gap(c, fam, align_type):
    if fam in CONST:
        return orc.Gap(align_type, *CONST[fam])
    a = gap_arrays(c, fam)
    if fam == "gn2":
        return orc.Gap(align_type, gn2=a)
    return orc.Gap(align_type, tgi=a["tgi"], tge=a["tge"])      # "tables" tabulates these functions for the device


def device_gap(cs, fam, mode):
    """Keyword arguments of Batch.dp_submatrix (constant, tpos) / Batch.dp_simmatrix (gn2, tables) for a batch of the cases
    `cs`, one template per pair: pooled per-position arrays, one deletion table per template, insertion planes per pair."""
    if fam in CONST:
        return dict(gi=CONST[fam][0], ge=CONST[fam][1])
    arrs = [gap_arrays(c, fam) for c in cs]
    if fam == "tpos":
        return dict(gi=0, ge=0, tgi=np.concatenate([a["tgi"] for a in arrs]), tge=np.concatenate([a["tge"] for a in arrs]))
    if fam == "gn2":
        return dict(gi=0, ge=0, tgi=np.concatenate([a["v_gi"] for a in arrs]), tge=np.concatenate([a["v_ge"] for a in arrs]),
                    tcn=np.concatenate([a["v_cn"] for a in arrs]),
                    del_tables=[gap_tables.gn2_deletion_table(a, dims(c)[1], mode) for a, c in zip(arrs, cs)])
    tabs = [gap_tables.tabulate_gaps(oracle_gap(c, fam, mode), *dims(c)) for c in cs]
    return dict(gi=0, ge=0, del_tables=[t[0] for t in tabs], ins_tables=[t[1] for t in tabs])


def pruned_scan_precondition(c, fam):
    """what make_blockmax asks before the pruned candidate scans are used: constant model, gi, ge >= 0, both lengths <= 4096"""
    return fam in CONST and CONST[fam][0] >= 0 and CONST[fam][1] >= 0 and max(dims(c)) <= 4096


_PLANES = {}
_FOUND = {}


def planes(c, mode, fam):
    """-> S, D, PQ, PT, score and pair list of Optimal, on the oracle, built under `mode`; computed once"""
    key = (c.q, c.t, mode, fam if fam in CONST else (fam, c.name))
    if key not in _PLANES:
        S = orc.sim_submatrix(c.q, c.t, ALPHA, BLOSUM)
        status, D, PQ, PT = orc.dp_build(S, oracle_gap(c, fam, mode))
        assert status == 0, (c.name, mode, fam)
        status, sc, pl = orc.optimal(D, PQ, PT, mode == orc.LOCAL)
        assert status == 0, (c.name, mode, fam)
        for a in (S, D, PQ, PT, pl):
            a.setflags(write=False)
        _PLANES[key] = (S, D, PQ, PT, sc, pl)
    return _PLANES[key]


def search(c, mode, fam, kind, search_type=None, user_limit=None):
    """The oracle's set of (case, mode, family, kind); search_type: the align type handed to the SEARCH alone (the planes stay
    those of `mode`), for the mirrored-rule tooth; user_limit: another brake than params() names.  Computed once per key, never
    modified."""
    st = mode if search_type is None else search_type
    key = (c.name, mode, fam, kind, st, user_limit)
    if key not in _FOUND:
        S, D, PQ, PT, sc, pl = planes(c, mode, fam)
        gap = oracle_gap(c, fam, st)
        pr = dict(params(c, fam, kind))
        if user_limit is not None:
            pr["user_limit"] = user_limit
        fl = orc.make_subopt_regions(D.shape[1], pr["regions"])
        s = orc.AliSet()
        s.push(pl, sc)
        t0 = time.perf_counter()
        if kind in ("cw", "ucw"):
            status = orc.enumerate_noa(kind, D, PQ, PT, S, gap, fl, pr["nsub"], pr["delta"], s, user_limit=pr["user_limit"])
        elif kind == "kscw":
            status = orc.enumerate_ks(D, PQ, PT, S, gap, fl, pr["nsub"], pr["delta"], K_LIMIT, s, user_limit=pr["user_limit"])
        else:
            status, _ = orc.enumerate_cr(D, PQ, PT, S, gap, fl, pr["nsub"], pr["delta"], K_LIMIT, s, sort_limit=SORT_LIMIT,
                                         user_limit=pr["user_limit"], max_overlap=MAX_OVERLAP)
        seconds = time.perf_counter() - t0
        s.identity(c.q, c.t)
        _FOUND[key] = Found(status, seconds, [s.get(k) for k in range(len(s))])
    return _FOUND[key]


def same_sets(a, b):
    return len(a) == len(b) and all(x["score"].view(np.uint32) == y["score"].view(np.uint32) and x["uid"] == y["uid"]
                                    and np.array_equal(x["pairs"], y["pairs"]) for x, y in zip(a, b))


def scan_index(q0, t0, q, t):
    """place of the predecessor (q, t) among the candidates of the branch node (q0, t0): cw.h:151-194"""
    if q == q0 - 1 and t == t0 - 1:
        return 0
    if q == q0 - 1:
        return t0 - 1 - t
    assert t == t0 - 1
    return 1 + (t0 - 2) + (q0 - 2 - q)


def census(c, alis):
    """-> the teeth (end_rule apart) that occur in a set"""
    Q, T = dims(c)
    found = set()
    sides = set()
    for a in alis:
        pl = [tuple(int(v) for v in p) for p in a["pairs"]]
        if len(pl) < 3 or pl[-1] != (Q - 1, T - 1):
            continue
        q, t = pl[-2]
        if max(Q - 1 - q, T - 1 - t) - 1 > 128:
            found.add("far_block")
        if a["uid"] != -1 and q >= 1 and t >= 1 and scan_index(Q - 1, T - 1, q, t) >= 1024:
            found.add("second_trip")
        if a["uid"] != -1 and q >= 1 and t >= 1:
            sides.add(scan_index(Q - 1, T - 1, q, t) >= 1024)
        first = pl[1] if pl[0] == (0, 0) else pl[0]
        if max(first) > 128:
            found.add("head_jump")
    if len(sides) == 2:
        found.add("resume")
    return found


def check(c, mode, fam, kind):
    """the conditions and the teeth of one search the GPU tests run -> its Found"""
    what = (c.name, mode, fam, kind)
    f = search(c, mode, fam, kind)
    assert f.status == 0, what
    assert f.seconds < TIME_LIMIT_S, what + (f.seconds,)
    assert len(f.alis) >= 2, what + (len(f.alis),)
    if kind == "ucw" and mode in MODES_ONE_SIDED and fam in GOLDEN_FAMILIES:
        # the reference's ucw.h has its own brake (100000) wired in: the golden set can be compared only where the brake of
        # these tests never acts
        u = search(c, mode, fam, kind, user_limit=REFERENCE_UCW_LIMIT)
        assert u.seconds < TIME_LIMIT_S and same_sets(f.alis, u.alis), what + ("user_limit acts",)
    if "end_rule" in c.teeth and mode in MODES_ONE_SIDED and fam != "g0_0":
        m = search(c, mode, fam, kind, search_type=2 - mode)
        assert m.seconds < TIME_LIMIT_S, what + (m.seconds,)
        assert not same_sets(f.alis, m.alis), what + ("the mirrored end-gap rule gives the same set",)
    if mode == c.free_mode and fam != "g0_0":
        missing = set(c.teeth) - {"end_rule"} - census(c, f.alis)
        assert not missing, what + (sorted(missing),)
    return f


def distinct(alis):
    return len({a["pairs"].tobytes() for a in alis})


def check_distinct(c):
    """A set of 2 may hold Optimal's alignment and the search's rediscovery of it (under 11/1 most sets here do).  So for every
    small case, one-sided mode and kind, at least one of the two non-zero constant families yields two DIFFERENT alignments.
    (crcw apart: its overlap filter, max_overlap 0.3, exists to drop the neighbours of an alignment already in the set.)"""
    for mode in MODES_ONE_SIDED:
        for kind in ("cw", "ucw", "kscw"):
            assert max(distinct(search(c, mode, fam, kind).alis) for fam in GOLDEN_FAMILIES) >= 2, (c.name, mode, kind)


def constant_runs():
    """(case, mode, family, kind) of test_one_sided_modes_constant_gaps"""
    return [(c, mode, fam, kind) for mode in MODES_ONE_SIDED for fam in CONST for c in small_cases() for kind in kinds(fam)]


def position_runs():
    """(case, mode, family, kind) of test_one_sided_modes_position_gaps"""
    return [(c, mode, fam, kind) for mode in MODES_ALL for fam in POSITION for c in (small_cases() if fam == "tpos" else over8_cases())
            for kind in KINDS]


def trip2_runs():
    return [(trip2_case(), 0, "g11_1", "cw"), (trip2_resume_case(), 0, "g11_1", "cw")]


def golden_name(c, mode, fam):
    return "%s_m%d_%s" % (c.name, mode, fam)


def golden_runs():
    """(case, mode, family) pinned to the real reference: the constant-gap small cases in modes 0 and 2 at 11/1 and 4.73/0.34"""
    return [(c, mode, fam) for c in small_cases() for mode in MODES_ONE_SIDED for fam in GOLDEN_FAMILIES]
