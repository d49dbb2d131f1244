"""Shared by tests/test_enum_pool_reference.py (CPU) and tests/test_gpu_enumerate_pools.py (GPU): the pairs, parameters and
oracle sets on which the machinery AROUND the near-optimal searches is tested — sets the caller already holds
(aln_noa.n_existing >= 0), pool growth and retries of aln_batch_enumerate_all, the several-wave kernel's chunked node pool and
task ring, kept pools, the launch order, and the output contract.  Oracle and numpy only: the HIP library is never loaded here.

The comparator is always the oracle with a pre-filled orc.AliSet: orc.enumerate_* append to whatever the set holds, as the
reference's enumerate() does (cw.h:82, kscw.h:120, crcw.h:146).  An entry the caller holds is pushed as a MARKER: the pair list
(0,0), (1,1) .. (k+1,k+1) for old index k, uid -1 — no search reads the lists of the entries that are already there, and no
created alignment looks like one (every created list ends in the final cell), so after sortSet the marker tells which old entry
stands where.  search() returns them as dict(score, existing=k).

Every group of cases names what it was built to reach; tests/test_enum_pool_reference.py asserts on the oracle that it does, so
that no GPU test passes vacuously.  A case that stops biting gets other parameters, never a weaker condition.
"""
import collections
import time

import numpy as np

import orc
import range_cases as rc
from aln_amd.synth import homolog_pair

ALPHA, BLOSUM = rc.load_blosum62()

KINDS = ("cw", "ucw", "kscw", "crcw")
PAR_KINDS = ("cw", "ucw", "kscw")                 # the kinds the several-wave kernel searches
LOCAL, GLOBAL = orc.LOCAL, orc.GLOBAL
K_LIMIT, SORT_LIMIT, MAX_OVERLAP = 4, 10, 0.75
TIME_LIMIT_S = 1.0
NO_BRAKE = 100000                                 # a user_limit no search of this file reaches

Pair = collections.namedtuple("Pair", "name q t")
Found = collections.namedtuple("Found", "status seconds alis")


def dims(p):
    return len(p.q) + 2, len(p.t) + 2


def pair(name, seed, n, sub_rate=0.25, indel=3):
    return Pair(name, *homolog_pair(seed, n, sub_rate=sub_rate, indel=indel))


def flags(p, regions):
    return orc.make_subopt_regions(dims(p)[1], regions)


def flag_rows(ps, regions):
    """[n, max T] rows as aln_batch_enumerate_all takes them; regions: one count or one per pair"""
    regs = [regions] * len(ps) if np.isscalar(regions) else list(regions)
    rows = np.zeros((len(ps), max(dims(p)[1] for p in ps)), dtype=np.uint8)
    for k, (p, r) in enumerate(zip(ps, regs)):
        rows[k, :dims(p)[1]] = flags(p, r)
    return rows


_PLANES = {}
_FOUND = {}


def planes(p, mode, gap):
    """-> S, D, PQ, PT, score and pair list of Optimal on the oracle; computed once"""
    key = (p.q, p.t, mode, gap)
    if key not in _PLANES:
        S = orc.sim_submatrix(p.q, p.t, ALPHA, BLOSUM)
        status, D, PQ, PT = orc.dp_build(S, orc.Gap(mode, *gap))
        assert status == 0, (p.name, mode, gap)
        status, sc, pl = orc.optimal(D, PQ, PT, mode == LOCAL)
        assert status == 0, (p.name, mode, gap)
        for a in (S, D, PQ, PT, pl):
            a.setflags(write=False)
        _PLANES[key] = (S, D, PQ, PT, sc, pl)
    return _PLANES[key]


def marker(k):
    return np.array([(i, i) for i in range(k + 2)], dtype=np.int32)


def _marker_index(a):
    pl = a["pairs"]
    if a["uid"] == -1 and len(pl) >= 2 and tuple(pl[-1]) == (len(pl) - 1, len(pl) - 1) and np.array_equal(pl, marker(len(pl) - 2)):
        return len(pl) - 2
    return None


def search(p, mode, gap, kind, nsub, delta, regions, user_limit, existing=None, k_limit=K_LIMIT):
    """The oracle's set.  existing None: seeded with Optimal's alignment like aln_noa.n_existing = -1; a tuple of float32 scores
    (possibly empty): the set the caller holds.  Computed once per key, never modified."""
    ex = None if existing is None else tuple(np.float32(x).view(np.uint32).item() for x in existing)
    key = (p.q, p.t, mode, gap, kind, nsub, float(np.float32(delta)), regions, user_limit, ex, k_limit)
    if key not in _FOUND:
        S, D, PQ, PT, sc, pl = planes(p, mode, gap)
        g = orc.Gap(mode, *gap)
        fl = flags(p, regions)
        s = orc.AliSet()
        if existing is None:
            s.push(pl, sc)
        else:
            assert len(existing) + 2 < min(dims(p)) - 1                       # markers stay inside the matrix and off the final cell
            for k, x in enumerate(existing):
                s.push(marker(k), np.float32(x))
        t0 = time.perf_counter()
        if kind in ("cw", "ucw"):
            status = orc.enumerate_noa(kind, D, PQ, PT, S, g, fl, nsub, delta, s, user_limit=user_limit)
        elif kind == "kscw":
            status = orc.enumerate_ks(D, PQ, PT, S, g, fl, nsub, delta, k_limit, s, user_limit=user_limit)
        else:
            status, _ = orc.enumerate_cr(D, PQ, PT, S, g, fl, nsub, delta, k_limit, s, sort_limit=SORT_LIMIT, user_limit=user_limit,
                                         max_overlap=MAX_OVERLAP)
        seconds = time.perf_counter() - t0
        s.identity(p.q, p.t)
        alis = []
        Q, T = dims(p)
        for k in range(len(s)):
            a = s.get(k)
            m = _marker_index(a) if existing is not None else None
            if m is not None:
                assert m < len(existing) and a["score"].view(np.uint32) == np.float32(existing[m]).view(np.uint32), (p.name, kind, k)
                alis.append(dict(score=a["score"], existing=m))
            else:
                assert tuple(a["pairs"][-1]) == (Q - 1, T - 1), (p.name, kind, k)
                a["existing"] = None
                alis.append(a)
        _FOUND[key] = Found(status, seconds, alis)
    return _FOUND[key]


def search_kw(kind):
    """the kind's own keyword arguments of Batch.enumerate / Batch.enumerate_all"""
    kw = {}
    if kind in ("kscw", "crcw"):
        kw.update(k_limit=K_LIMIT)
    if kind == "crcw":
        kw.update(sort_limit=SORT_LIMIT, max_overlap=MAX_OVERLAP)
    return kw


def created(alis):
    return [a for a in alis if a["existing"] is None]


def same_created(a, b, uids=True):
    """two sets' created entries, in set order: scores, pair lists and (kscw and crcw number them by their place in the WHOLE
    set, so not behind different numbers of held entries) uids"""
    a, b = created(a), created(b)
    return len(a) == len(b) and all(x["score"].view(np.uint32) == y["score"].view(np.uint32) and (x["uid"] == y["uid"] or not uids)
                                    and np.array_equal(x["pairs"], y["pairs"]) for x, y in zip(a, b))


# ---- 1. sets the caller already holds (aln_noa.n_existing >= 0, through aln_batch_enumerate) ------------------------------------
HELD_PAIRS = (pair("h60", 71000, 60), pair("h95", 71001, 95), pair("h130", 71002, 130))
HELD_BATCHES = collections.OrderedDict((("local_g11_1", (LOCAL, (11, 1))), ("global_g4.73_0.34", (GLOBAL, (4.73, 0.34)))))
HELD = {"cw": (0.15, 3), "ucw": (0.02, 3), "kscw": (0.3, 6), "crcw": (0.3, 6)}    # kind -> delta_ratio, flag regions
HELD_LIMIT = 5000                                  # user_limit of these searches: no set of them comes near it
N_EXISTING = (0, 1, 2, 5)
CUTS = ("all", "tail", "half", "keep")             # number_suboptimal: >= the set, set - 1, set / 2, 0


def held_base(p, batch, kind):
    """the oracle's set of an EMPTY caller-held set, everything kept: the scores the caller's entries are chosen against"""
    mode, gap = HELD_BATCHES[batch]
    delta, regions = HELD[kind]
    return search(p, mode, gap, kind, 0, delta, regions, HELD_LIMIT, ())


def held_scores(p, batch, kind, n_ex):
    """Scores of the n_ex entries the caller holds, relative to the oracle's own set: top = its best score (the enumerator's
    seed ends with it), mid = the score of a created alignment in the middle of the set, low = its worst.
      1: (top)                                        ties with the seed
      2: (top + 7.5, mid)                             above everything; equal to a created alignment
      5: (low - 3, top, mid, mid, top + 7.5)          below everything, the tie with the seed, two equal to each other"""
    sc = sorted((a["score"] for a in held_base(p, batch, kind).alis), reverse=True)      # (number_suboptimal 0 sorts nothing)
    top, mid, low = sc[0], sc[len(sc) // 2], sc[-1]
    f = np.float32
    return {0: (), 1: (top,), 2: (f(top + f(7.5)), mid), 5: (f(low - f(3)), top, mid, mid, f(top + f(7.5)))}[n_ex]


def held_nsub(p, batch, kind, n_ex, cut):
    mode, gap = HELD_BATCHES[batch]
    delta, regions = HELD[kind]
    n = len(search(p, mode, gap, kind, 0, delta, regions, HELD_LIMIT, held_scores(p, batch, kind, n_ex)).alis)
    return {"all": n + 3, "tail": max(n - 1, 1), "half": max(n // 2, 1), "keep": 0}[cut]


def held_search(p, batch, kind, n_ex, cut):
    """-> (existing scores, number_suboptimal, the oracle's Found)"""
    mode, gap = HELD_BATCHES[batch]
    delta, regions = HELD[kind]
    ex = held_scores(p, batch, kind, n_ex)
    nsub = held_nsub(p, batch, kind, n_ex, cut)
    return ex, nsub, search(p, mode, gap, kind, nsub, delta, regions, HELD_LIMIT, ex)


def held_runs():
    return [(p, batch, kind, n_ex, cut) for batch in HELD_BATCHES for p in HELD_PAIRS for kind in KINDS for n_ex in N_EXISTING
            for cut in CUTS]


# the brake counts the whole set: kind -> (pair, batch, delta_ratio, regions).  L = the size of the un-braked set found from an
# EMPTY caller-held set; with user_limit = L that search never brakes, and the same search behind 5 held entries does.
BRAKE = {"cw": ("h95", "local_g11_1", 0.15, 3), "ucw": ("h60", "global_g4.73_0.34", 0.02, 3),
         "kscw": ("h60", "local_g11_1", 0.3, 6), "crcw": ("h60", "global_g4.73_0.34", 0.3, 6)}
BRAKE_HELD = tuple(np.float32(x) for x in (1.0, 2.0, 3.0, 4.0, 5.0))


def brake_case(kind):
    """-> pair, mode, gap, delta, regions, L, Found with no entry held, Found behind BRAKE_HELD (both with user_limit L, all kept)"""
    name, batch, delta, regions = BRAKE[kind]
    p, = [x for x in HELD_PAIRS if x.name == name]
    mode, gap = HELD_BATCHES[batch]
    L = len(search(p, mode, gap, kind, 0, delta, regions, NO_BRAKE, ()).alis)
    return (p, mode, gap, delta, regions, L, search(p, mode, gap, kind, 0, delta, regions, L, ()),
            search(p, mode, gap, kind, 0, delta, regions, L, BRAKE_HELD))


# ---- 2. - 4. one ragged batch, LOCAL 11/1, per-pair flag rows ---------------------------------------------------------------------
_LENS = (90, 30, 170, 64, 200, 47, 130, 185, 115, 150)
_RATES = (0.2, 0.25, 0.3, 0.15, 0.3, 0.25, 0.2, 0.35, 0.15, 0.25)
POOL_PAIRS = tuple(pair("r%d" % n, 72000 + n, ln, sub_rate=r) for n, (ln, r) in enumerate(zip(_LENS, _RATES)))
POOL_MODE, POOL_GAP = LOCAL, (11, 1)

Run = collections.namedtuple("Run", "kind nsub delta regions user_limit k_limit")
# the small searches: node-pool growth of the one-wave kernels, the output contract, the small ucw of the kept-pools sequence
SMALL = {"cw": Run("cw", 20, 0.15, 4, HELD_LIMIT, 0), "ucw": Run("ucw", 20, 0.02, 3, HELD_LIMIT, 0),
         "kscw": Run("kscw", 20, 0.3, 6, HELD_LIMIT, 8), "crcw": Run("crcw", 20, 0.3, 6, HELD_LIMIT, 4)}
# alignment pools of 4 slots: the brake (user_limit 40) cuts these sets, and the pool has to grow to what it bounds
BRAKED = {"kscw": SMALL["kscw"]._replace(nsub=NO_BRAKE, user_limit=40), "crcw": SMALL["crcw"]._replace(nsub=NO_BRAKE, user_limit=40)}
# the large searches: 10 - 18 thousand alignments created by the long pairs, 50 kept: more than one 65536-node chunk per pair
_LARGE_CW_REGIONS = (8, 6, 3, 10, 4, 8, 6, 5, 7, 5)
LARGE = {"cw": Run("cw", 50, 0.2, _LARGE_CW_REGIONS, NO_BRAKE, 0), "kscw": Run("kscw", 50, 0.3, 6, NO_BRAKE, 16)}


def run_regions(r):
    return [r.regions] * len(POOL_PAIRS) if np.isscalar(r.regions) else list(r.regions)


def run_flags(r):
    return flag_rows(POOL_PAIRS, run_regions(r))


def run_kw(r):
    kw = dict(user_limit=r.user_limit)
    if r.kind in ("kscw", "crcw"):
        kw.update(k_limit=r.k_limit)
    if r.kind == "crcw":
        kw.update(sort_limit=SORT_LIMIT, max_overlap=MAX_OVERLAP)
    return kw


def run_search(r, k, nsub=None, user_limit=None):
    """the oracle's set of pair k of the ragged batch under the run r (seeded with Optimal's alignment)"""
    return search(POOL_PAIRS[k], POOL_MODE, POOL_GAP, r.kind, r.nsub if nsub is None else nsub, r.delta, run_regions(r)[k],
                  r.user_limit if user_limit is None else user_limit, None, r.k_limit or K_LIMIT)


def created_counts(r):
    """alignments every pair's search creates before sortSet (the reference's as.size()): what last_enum_usage reports"""
    return [len(run_search(r, k, nsub=0).alis) for k in range(len(POOL_PAIRS))]


def optimal_scores():
    return [planes(p, POOL_MODE, POOL_GAP)[4] for p in POOL_PAIRS]


def score_order():
    """the launch order of a first call under enum_heavy_first: Optimal's score, descending, stable"""
    sc = optimal_scores()
    return sorted(range(len(sc)), key=lambda k: -float(sc[k]))


def usage_order(nodes):
    """the launch order of a later call: the previous call's nodes, descending, stable"""
    return sorted(range(len(nodes)), key=lambda k: -int(nodes[k]))


# The user_limit boundary: kind -> (pair of the ragged batch, delta_ratio, regions, k_limit): an un-braked set of 30 <= n <= 80
# (Optimal's entry included).  The brake is `as.size() > user_limit` at a branch node (cw.h:127): with user_limit >= n - 1 the
# set reaches n only with its last alignment and nothing is cut (no scan of 10 pairs x 7 thresholds x 6 region counts found a
# pair where n - 1 changes the set); with n - 2 the search is braked while its last but one alignment still branches.  The pairs
# below are those where that loses an alignment, so the two sides of the boundary are n - 2 | n - 1, n, n + 1.
BOUNDARY = {"cw": (3, 0.12, 5, 0), "ucw": (6, 0.03, 3, 0), "kscw": (5, 0.3, 6, 4), "crcw": (8, 0.3, 6, 4)}


def boundary_case(kind):
    """-> pair index, Run (all kept), n = size of the un-braked set, {user_limit: Found} for n - 2 .. n + 1"""
    k, delta, regions, kl = BOUNDARY[kind]
    r = Run(kind, NO_BRAKE, delta, regions, NO_BRAKE, kl)
    n = len(run_search(r, k).alis)
    return k, r, n, {ul: run_search(r, k, user_limit=ul) for ul in (n - 2, n - 1, n, n + 1)}


# ---- enumerations chained on ONE set, pinned to the real reference (tests/golden/enum_chain.json) ---------------------------------
# The second call sees what the first left: n_existing > 1 without inventing alignments.  A step is (kind, number_suboptimal,
# delta_ratio, flag regions); user_limit is the reference's own (cw.h:76, ucw.h:72).  "empty_cw" starts from a cleared set.
CHAIN_PAIRS = (pair("c20", 73000, 20), pair("c30", 73001, 30), pair("c40", 73002, 40))
CHAIN_MODES = collections.OrderedDict(((LOCAL, (11, 1)), (GLOBAL, (4.73, 0.34))))
CHAINS = collections.OrderedDict((("cw_ucw", (("cw", 6, 0.3, 3), ("ucw", 10, 0.05, 1))),
                                  ("ucw_cw", (("ucw", 5, 0.05, 1), ("cw", 10, 0.3, 3))),
                                  ("cw_cw", (("cw", 4, 0.2, 3), ("cw", 8, 0.4, 2)))))
CHAIN_EMPTY = ("empty_cw", (("cw", 8, 0.3, 3),))
REFERENCE_LIMIT = {"cw": 1000000, "ucw": 100000}

Chain = collections.namedtuple("Chain", "name pair mode gap empty steps")


def chain_runs():
    runs = [Chain("%s_m%d_%s" % (p.name, mode, cname), p, mode, gap, False, steps)
            for p in CHAIN_PAIRS for mode, gap in CHAIN_MODES.items() for cname, steps in CHAINS.items()]
    p = CHAIN_PAIRS[-1]
    return runs + [Chain("%s_m%d_%s" % (p.name, LOCAL, CHAIN_EMPTY[0]), p, LOCAL, CHAIN_MODES[LOCAL], True, CHAIN_EMPTY[1])]


_CHAINS = {}


def chain_oracle(c):
    """-> the oracle's set after every step (lists of dicts: score, identity, uid, pairs)"""
    if c.name not in _CHAINS:
        S, D, PQ, PT, sc, pl = planes(c.pair, c.mode, c.gap)
        g = orc.Gap(c.mode, *c.gap)
        s = orc.AliSet()
        if not c.empty:
            s.push(pl, sc)
        sets = []
        for kind, nsub, delta, regions in c.steps:
            assert orc.enumerate_noa(kind, D, PQ, PT, S, g, flags(c.pair, regions), nsub, delta, s, user_limit=REFERENCE_LIMIT[kind]) == 0
            s.identity(c.pair.q, c.pair.t)
            sets.append([s.get(k) for k in range(len(s))])
        _CHAINS[c.name] = sets
    return _CHAINS[c.name]
