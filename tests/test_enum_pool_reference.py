"""CPU only.  The cases of enum_pool_cases.py bite: every group of searches tests/test_gpu_enumerate_pools.py runs reaches what it
was built for, on the oracle — the caller's entries land above, inside and below the created ones and the cuts drop both
kinds, five held entries trip a brake an empty set does not, the 4-slot alignment pools are braked, the user_limit boundary
changes the set, the launch orders differ.  And the oracle's chained enumerations (a pre-filled set) equal the real
reference's, tests/golden/enum_chain.json, bit for bit: scores, uids, pair lists, identities, gapped strings, annotations."""
import numpy as np
import pytest

import enum_pool_cases as ep
import goldens
import orc


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def test_golden_chain_file_holds_the_builder_cases():
    gold = goldens.enum_chain_cases()
    runs = ep.chain_runs()
    assert sorted(gold) == sorted(c.name for c in runs) and len(runs) == 19
    for c in runs:
        g = gold[c.name]
        assert (g["q"], g["t"], g["mode"], g["empty"]) == (c.pair.q, c.pair.t, c.mode, c.empty)
        assert (np.float32(g["gi"]), np.float32(g["ge"])) == tuple(np.float32(x) for x in c.gap)
        assert max(len(c.pair.q), len(c.pair.t)) <= 60 and len(g["steps"]) == len(c.steps)
        for st, (kind, nsub, delta, regions) in zip(g["steps"], c.steps):
            assert (st["kind"], st["nsub"], st["delta"]) == (kind, nsub, delta) and nsub <= 12
            assert st["flags"] == "".join(str(int(x)) for x in ep.flags(c.pair, regions))


def test_oracle_chains_equal_the_reference():
    """orc.enumerate_noa appends to a pre-filled AliSet as the reference's enumerate() appends to its AlignmentSet; the second
    step of a chain starts from 2 .. 6 entries, the "empty" chain from none."""
    gold = goldens.enum_chain_cases()
    second_starts = set()
    for c in ep.chain_runs():
        sets = ep.chain_oracle(c)
        for k, alis in enumerate(sets):
            s = orc.AliSet()
            for a in alis:
                s.push(a["pairs"], a["score"], a["uid"])
            tl, qls = s.strings(c.pair.q, c.pair.t)
            goldens.check_set(gold[c.name], "CHAIN%d" % (k + 1), alis, tl, qls, [orc.annot(a["score"], a["identity"]) for a in alis])
        if len(sets) == 2:
            second_starts.add(len(sets[0]))
            assert len(sets[1]) > 2
    assert min(second_starts) >= 2 and max(second_starts) >= 5, second_starts


@pytest.mark.parametrize("batch", list(ep.HELD_BATCHES))
def test_held_sets_bite(batch):
    """For every pair and kind: status 0, under 1 s; the held scores are what held_scores() says of them (a tie with the set's
    best, a tie with a created alignment, two equal, above, below); every held entry comes back exactly once when all are kept;
    over the batch, some cut drops created entries only, some cut drops held ones."""
    only_created = held_dropped = 0
    for p in ep.HELD_PAIRS:
        for kind in ep.KINDS:
            base = ep.held_base(p, batch, kind)
            assert base.status == 0 and len(base.alis) >= 1
            for n_ex in ep.N_EXISTING:
                ex = ep.held_scores(p, batch, kind, n_ex)
                assert len(ex) == n_ex
                full = ep.held_search(p, batch, kind, n_ex, "keep")[2]
                cr = [_bits(a["score"]) for a in ep.created(full.alis)]
                assert ep.same_created(base.alis, full.alis, uids=False)                # HELD_LIMIT never brakes: the search is the same
                top, low = max(a["score"] for a in base.alis), min(a["score"] for a in base.alis)
                if n_ex == 1:
                    assert _bits(ex[0]) == _bits(top)
                if n_ex == 2:
                    assert ex[0] > top and _bits(ex[1]) in cr
                if n_ex == 5:
                    assert ex[0] < low and ex[4] > top
                    assert _bits(ex[1]) == _bits(top) and _bits(ex[2]) == _bits(ex[3]) and _bits(ex[2]) in cr
                for cut in ep.CUTS:
                    _, nsub, f = ep.held_search(p, batch, kind, n_ex, cut)
                    what = (p.name, batch, kind, n_ex, cut)
                    assert f.status == 0 and f.seconds < ep.TIME_LIMIT_S, what
                    held = sorted(a["existing"] for a in f.alis if a["existing"] is not None)
                    if cut in ("all", "keep"):
                        assert held == list(range(n_ex)) and len(f.alis) == len(full.alis), what
                        assert nsub == 0 or nsub >= len(f.alis)
                    else:
                        assert len(f.alis) == nsub < len(full.alis) or len(full.alis) == 1, what
                        if len(held) == n_ex and n_ex:
                            only_created += 1
                        if len(held) < n_ex:
                            held_dropped += 1
    assert only_created >= 8 and held_dropped >= 8, (only_created, held_dropped)


@pytest.mark.parametrize("kind", ep.KINDS)
def test_brake_counts_the_held_entries(kind):
    p, mode, gap, delta, regions, L, free, held = ep.brake_case(kind)
    assert free.status == 0 and held.status == 0
    assert len(free.alis) == L >= 15                                           # user_limit = L: never `size > L`, nothing is cut
    assert ep.same_created(free.alis, ep.search(p, mode, gap, kind, 0, delta, regions, ep.NO_BRAKE, ()).alis)
    assert len(held.alis) > L and len(ep.created(held.alis)) < L               # behind 5 held entries the same search is braked
    assert not ep.same_created(free.alis, held.alis, uids=False)


def test_ragged_batch_and_its_searches():
    ps = ep.POOL_PAIRS
    assert 8 <= len(ps) <= 12 and all(30 <= len(p.q) <= 200 and len(p.t) <= 250 for p in ps)
    slowest = 0.0
    for runs in (ep.SMALL, ep.BRAKED, ep.LARGE):
        for r in runs.values():
            for k in range(len(ps)):
                f = ep.run_search(r, k)
                assert f.status == 0 and f.seconds < ep.TIME_LIMIT_S, (r, k, f.seconds)
                slowest = max(slowest, f.seconds)
    print("slowest search %.3f s" % slowest)
    for kind, r in ep.SMALL.items():                                           # never braked; more sets than K = nsub in the batch
        n = ep.created_counts(r)
        assert max(n) < r.user_limit and max(n) > r.nsub + 2 and min(n) < r.nsub, (kind, n)
    for kind, r in ep.LARGE.items():                                           # 10 - 30 thousand created by the long pairs
        n = ep.created_counts(r)
        assert sum(10000 <= x <= 30000 for x in n) >= 4 and max(n) <= 30000 and max(n) < r.user_limit, (kind, n)


@pytest.mark.parametrize("kind", list(ep.BRAKED))
def test_four_slot_pools_are_braked(kind):
    """user_limit 40 acts: some pair's set is larger than it, and smaller and other than the un-braked one"""
    r = ep.BRAKED[kind]
    cut = 0
    for k in range(len(ep.POOL_PAIRS)):
        f, free = ep.run_search(r, k), ep.run_search(r, k, user_limit=ep.NO_BRAKE)
        assert len(f.alis) <= len(free.alis)
        if len(f.alis) > r.user_limit:
            assert len(f.alis) < len(free.alis) and not ep.same_created(f.alis, free.alis)
            cut += 1
    assert cut >= 3, cut


@pytest.mark.parametrize("kind", ep.KINDS)
def test_user_limit_boundary_changes_the_set(kind):
    k, r, n, found = ep.boundary_case(kind)
    assert 30 <= n <= 80
    assert all(f.status == 0 for f in found.values())
    assert ep.same_created(found[n].alis, found[n + 1].alis) and ep.same_created(found[n].alis, found[n - 1].alis)
    assert len(found[n].alis) == n
    assert not ep.same_created(found[n - 2].alis, found[n - 1].alis)


def test_launch_orders_differ():
    """enum_heavy_first orders a first call by Optimal's score: another permutation than the index order (the GPU test shows
    that the usage order of a second call is a third one)"""
    order = ep.score_order()
    assert order != list(range(len(ep.POOL_PAIRS))) and sorted(order) == list(range(len(ep.POOL_PAIRS)))
    assert order[0] != 0 and order[-1] != len(order) - 1
