"""-m gpu tests of the machinery AROUND the near-optimal searches: sets the caller already holds (aln_noa.n_existing >= 0),
pool growth and retries of aln_batch_enumerate_all in all four kinds, the several-wave kernel's chunked node pool and task
ring, kept pools, the launch order, and the output contract.  Cases, parameters and the oracle's sets come from
enum_pool_cases.py; tests/test_enum_pool_reference.py proves on the CPU that every case bites and pins the oracle's chained
enumerations to the real reference.  Every comparison is bit for bit: set size and order, float32 score bit patterns, uids,
pair lists, identities."""
import ctypes as C
import re

import numpy as np
import pytest

import aln_amd
import enum_pool_cases as ep
import goldens
import gpu_util
import orc

pytestmark = pytest.mark.gpu

CHUNK = 65536                                      # kChunkNodes: the several-wave kernel's node pool is handed out in such chunks
SENTINEL = -77


@pytest.fixture(params=[1, 0, 3], ids=["one_wave", "waves_auto", "waves3"])
def enum_waves(request):
    """cw / ucw / kscw in the one-wave kernels, with the default number of waves (16) and with 3; crcw has one kernel"""
    with gpu_util.ctx().hints(enum_waves=request.param):
        yield request.param


@pytest.fixture(params=[0, 3], ids=["waves_auto", "waves3"])
def par_waves(request):
    with gpu_util.ctx().hints(enum_waves=request.param):
        yield request.param


def _batch(ps, mode, gap):
    b = aln_amd.Batch(gpu_util.ctx(), [p.q for p in ps], [p.t for p in ps])
    b.dp_submatrix(ep.ALPHA, ep.BLOSUM, mode, gap[0], gap[1])
    return b


def _pool_batch():
    return _batch(ep.POOL_PAIRS, ep.POOL_MODE, ep.POOL_GAP)


@pytest.fixture(scope="module")
def held_batches():
    made = {name: _batch(ep.HELD_PAIRS, mode, gap) for name, (mode, gap) in ep.HELD_BATCHES.items()}
    yield made
    for b in made.values():
        b.close()


@pytest.fixture(scope="module")
def pool_batch():
    b = _pool_batch()
    yield b
    b.close()


def _bits(x):
    return int(np.float32(x).view(np.uint32))


# ---- aln_batch_enumerate through the ABI itself: the records as the library wrote them -------------------------------------------
def _raw_enumerate(b, p, kind, nsub, delta, fl, user_limit, max_alignments, n_existing=-1, existing=None, pairs_capacity=None, **kw):
    """-> rc, n_out, records (score, identity, uid, n_pairs, pair_off), pairs; everything sentinel-filled before the call.
    pairs_capacity: what the library is told of the pairs array (default: all of it)"""
    Q, T = b.dims(p)
    ex = None if existing is None else np.ascontiguousarray(existing, dtype=np.float32)
    noa = aln_amd.AlnNoa(aln_amd._ENUM[kind], int(nsub), float(np.float32(delta)), int(user_limit), int(n_existing),
                         ex.ctypes.data_as(C.POINTER(C.c_float)) if ex is not None and len(ex) else None,
                         int(kw.get("k_limit", 0)), int(kw.get("sort_limit", 0)), float(np.float32(kw.get("max_overlap", 0.3))))
    out = (aln_amd.AlnAlignment * max(max_alignments, 1))()
    C.memset(out, 0x5A, C.sizeof(out))
    pairs = np.full((max(max_alignments, 1) * (min(Q, T) + 3), 2), SENTINEL, dtype=np.int32)
    n = C.c_int32(SENTINEL)
    flp = np.ascontiguousarray(fl, dtype=np.uint8)
    rc = aln_amd.lib().aln_batch_enumerate(b.h, p, C.byref(noa), flp.ctypes.data_as(C.POINTER(C.c_uint8)), out, max_alignments,
                                           pairs.ctypes.data_as(C.POINTER(C.c_int32)), len(pairs) if pairs_capacity is None else pairs_capacity,
                                           C.byref(n))
    recs = [(np.float32(a.score), np.float32(a.identity), a.uid, a.n_pairs, a.pair_off) for a in out]
    return rc, n.value, recs, pairs


def _untouched(recs, pairs):
    sentinel = np.frombuffer(b"\x5a" * 4, dtype=np.float32)[0]
    return all(_bits(r[0]) == _bits(sentinel) and r[2] == 0x5A5A5A5A and r[3] == 0x5A5A5A5A for r in recs) and (pairs == SENTINEL).all()


def _check_records(rc, n, recs, pairs, want, existing, what):
    """want: the oracle's set (enum_pool_cases.search); an entry the caller holds shows n_pairs -1, pair_off = its old index,
    uid -1, identity 0 and the caller's score bits; a created one equals the oracle's entry at the same place"""
    assert rc == 0 and n == len(want), what + (rc, n, len(want))
    for k, w in enumerate(want):
        score, identity, uid, n_pairs, pair_off = recs[k]
        if w["existing"] is not None:
            assert (n_pairs, pair_off, uid) == (-1, w["existing"], -1) and _bits(identity) == 0, what + (k, n_pairs, pair_off, uid, identity)
            assert _bits(score) == _bits(existing[w["existing"]]), what + (k,)
        else:
            assert _bits(score) == _bits(w["score"]), what + (k, score, w["score"])
            assert uid == w["uid"], what + (k, uid, w["uid"])
            assert n_pairs == len(w["pairs"]) and np.array_equal(pairs[pair_off:pair_off + n_pairs], w["pairs"]), what + (k,)
            assert _bits(identity) == _bits(w["identity"]), what + (k,)


def _check_binding(got, want, existing, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        if w["existing"] is not None:
            assert sorted(g) == ["existing", "score"] and g["existing"] == w["existing"] and _bits(g["score"]) == _bits(existing[w["existing"]]), what + (k,)
        else:
            assert _bits(g["score"]) == _bits(w["score"]) and g["uid"] == w["uid"] and np.array_equal(g["pairs"], w["pairs"]), what + (k,)
            assert _bits(g["identity"]) == _bits(w["identity"]), what + (k,)


KINDS_WAVES = [(k, w, "%s-%s" % (k, n)) for k in ep.PAR_KINDS for w, n in ((1, "one_wave"), (0, "waves_auto"), (3, "waves3"))] + [("crcw", None, "crcw")]


@pytest.fixture(params=KINDS_WAVES, ids=[x[2] for x in KINDS_WAVES])
def kind(request):
    """the enumerator, run in its one-wave kernel, with the default number of waves and with 3 (crcw has one kernel).  The
    one-pair entry point allocates its node pool anew in every call, 48 Mi nodes by default (0.4 GB: tens of milliseconds, at
    times seconds); no one-pair search of this file needs more than 0.3 Mi, so the tests that make hundreds of calls ask for 1 Mi."""
    k, waves, _ = request.param
    hints = dict(enum_node_cap=1 << 20)
    if waves is not None:
        hints.update(enum_waves=waves)
    with gpu_util.ctx().hints(**hints):
        yield k


# ---- 1. caller-held sets -----------------------------------------------------------------------------------------------------------
def test_caller_held_sets(kind, held_batches):
    """n_existing 0, 1, 2 and 5 with scores above, equal to and below the created ones, number_suboptimal at least the set
    (std::sort), one and half the set short (std::partial_sort) and 0 (everything, unsorted): first_slot, the uid rule of the
    several-wave kscw path, slot_order behind the caller's entries, the n_pairs = -1 records, ali_cap."""
    n_runs = 0
    for p, batch, knd, n_ex, cut in ep.held_runs():
        if knd != kind:
            continue
        b = held_batches[batch]
        ex, nsub, f = ep.held_search(p, batch, kind, n_ex, cut)
        delta, regions = ep.HELD[kind]
        pi = ep.HELD_PAIRS.index(p)
        what = (kind, batch, p.name, n_ex, cut)
        rc, n, recs, pairs = _raw_enumerate(b, pi, kind, nsub, delta, ep.flags(p, regions), ep.HELD_LIMIT, len(f.alis) + 2, n_ex, ex,
                                            **ep.search_kw(kind))
        _check_records(rc, n, recs, pairs, f.alis, ex, what)
        if cut in ("all", "half"):
            got = b.enumerate(pi, kind, nsub, delta, ep.flags(p, regions), user_limit=ep.HELD_LIMIT, max_alignments=len(f.alis) + 2,
                              existing_scores=list(ex), **ep.search_kw(kind))
            _check_binding(got, f.alis, ex, what)
        n_runs += 1
    assert n_runs == len(ep.HELD_BATCHES) * len(ep.HELD_PAIRS) * len(ep.N_EXISTING) * len(ep.CUTS)


def test_brake_counts_the_held_entries(kind, held_batches):
    """user_limit = L, the size of the un-braked set: from an empty caller-held set nothing is cut, behind 5 held entries the
    reference's `as.size() > user_limit` (cw.h:127) brakes the same search — in the one-wave kernels by their own count, in the
    several-wave kernel by handing the pair back (kParSerial)."""
    p, mode, gap, delta, regions, L, free, held = ep.brake_case(kind)
    batch, = [name for name, mg in ep.HELD_BATCHES.items() if mg == (mode, gap)]
    b, pi = held_batches[batch], ep.HELD_PAIRS.index(p)
    for ex, want in (((), free.alis), (ep.BRAKE_HELD, held.alis)):
        rc, n, recs, pairs = _raw_enumerate(b, pi, kind, 0, delta, ep.flags(p, regions), L, len(want) + 2, len(ex), ex, **ep.search_kw(kind))
        _check_records(rc, n, recs, pairs, want, ex, (kind, "brake", len(ex)))


def test_caller_held_set_errors(kind, held_batches):
    """n_existing > 0 without scores is ALN_E_ARG and writes nothing; too few records are ALN_E_OVERFLOW with *n_out = the
    number needed (hostcpp/cw.h:45 retries with it), and the retry succeeds."""
    batch, p, n_ex = "local_g11_1", ep.HELD_PAIRS[0], 5
    b = held_batches[batch]
    ex, nsub, f = ep.held_search(p, batch, kind, n_ex, "all")
    delta, regions = ep.HELD[kind]
    args = (b, 0, kind, nsub, delta, ep.flags(p, regions), ep.HELD_LIMIT)
    rc, n, recs, pairs = _raw_enumerate(*args, len(f.alis) + 2, 2, None, **ep.search_kw(kind))
    assert rc == aln_amd.E_ARG and n == SENTINEL and _untouched(recs, pairs)
    assert len(f.alis) >= 3
    rc, n, recs, pairs = _raw_enumerate(*args, len(f.alis) - 1, n_ex, ex, **ep.search_kw(kind))
    assert rc == aln_amd.E_OVERFLOW and n == len(f.alis)
    rc, n2, recs, pairs = _raw_enumerate(*args, n, n_ex, ex, **ep.search_kw(kind))
    _check_records(rc, n2, recs, pairs, f.alis, ex, (kind, "retry"))


def test_chained_enumerations_equal_the_reference(enum_waves):
    """Two enumerations in a row on one set, as the real reference ran them (tests/golden/enum_chain.json): every call gets the
    scores of the set so far as existing_scores, and the result is merged by the `existing` indices — scores, uids, pair lists,
    identities, gapped strings and annotations of the set after every step."""
    gold = goldens.enum_chain_cases()
    batches = {mode: _batch(ep.CHAIN_PAIRS, mode, gap) for mode, gap in ep.CHAIN_MODES.items()}
    n_existing_seen = set()
    for c in ep.chain_runs():
        b, pi = batches[c.mode], ep.CHAIN_PAIRS.index(c.pair)
        held = []
        if not c.empty:
            scores, lists, status = b.optimal()
            assert status[pi] == 0
            held = [dict(score=scores[pi], uid=-1, pairs=lists[pi], identity=gpu_util.identity_for(c.pair.q, c.pair.t, lists[pi]))]
        for k, (knd, nsub, delta, regions) in enumerate(c.steps):
            n_existing_seen.add(len(held))
            got = b.enumerate(pi, knd, nsub, delta, ep.flags(c.pair, regions), max_alignments=nsub + len(held) + 2,
                              existing_scores=[h["score"] for h in held])
            for g in got:
                if "existing" in g:
                    assert _bits(g["score"]) == _bits(held[g["existing"]]["score"])
            held = [held[g["existing"]] if "existing" in g else g for g in got]
            tl, qls, idn = gpu_util.strings_for(c.pair.q, c.pair.t, [h["pairs"] for h in held])
            goldens.check_set(gold[c.name], "CHAIN%d" % (k + 1), held, tl, qls, [orc.annot(h["score"], h["identity"]) for h in held])
    for b in batches.values():
        b.close()
    assert {0, 1} <= n_existing_seen and max(n_existing_seen) >= 5


# ---- aln_batch_enumerate_all through the ABI itself ----------------------------------------------------------------------------------
def _stride(b):
    return max(min(max(b.dims(p)[0] for p in range(b.n)), max(b.dims(p)[1] for p in range(b.n))) + 3, 4)


def _raw_all(b, r, K=None, node_cap=1 << 20, ali_cap=1 << 17, flags="rows", want_pairs=True, pair_stride=None):
    """-> dict(rc, n_out, scores, lengths, pairs, status), every output sentinel-filled before the call.  flags: "rows" = the
    run's per-pair rows, or an array (1-D: one shared row, flags_stride 0)."""
    K = r.nsub + 2 if K is None else K
    kw = ep.run_kw(r)
    noa = aln_amd.AlnNoa(aln_amd._ENUM[r.kind], int(r.nsub), float(np.float32(r.delta)), int(kw["user_limit"]), -1, None,
                         int(kw.get("k_limit", 0)), int(kw.get("sort_limit", 0)), float(np.float32(kw.get("max_overlap", 0.3))))
    fl = np.ascontiguousarray(ep.run_flags(r) if isinstance(flags, str) else flags, dtype=np.uint8)
    stride = _stride(b) if pair_stride is None else pair_stride
    Kc = max(K, 1)
    o = dict(n_out=np.full(b.n, SENTINEL, np.int32), scores=np.full((b.n, Kc), SENTINEL, np.float32), lengths=np.full((b.n, Kc), SENTINEL, np.int32),
             status=np.full(b.n, SENTINEL, np.int32), pairs=np.full((b.n, Kc, max(stride, 1), 2), SENTINEL, np.int32) if want_pairs else None)
    ip = C.POINTER(C.c_int32)
    o["rc"] = aln_amd.lib().aln_batch_enumerate_all(
        b.h, C.byref(noa), fl.ctypes.data_as(C.POINTER(C.c_uint8)), fl.shape[1] if fl.ndim == 2 else 0, int(node_cap), int(ali_cap), K,
        o["n_out"].ctypes.data_as(ip), o["scores"].ctypes.data_as(C.POINTER(C.c_float)), o["lengths"].ctypes.data_as(ip),
        o["pairs"].ctypes.data_as(ip) if want_pairs else None, stride, o["status"].ctypes.data_as(ip))
    return o


def _all_untouched(o):
    return all((o[k] == SENTINEL).all() for k in ("n_out", "scores", "lengths", "status")) and (o["pairs"] is None or (o["pairs"] == SENTINEL).all())


def _valid(o, p):
    """what the call defines of pair p's outputs: n_out, status, and the first n_out scores, lengths and lists"""
    n = int(o["n_out"][p])
    lists = None if o["pairs"] is None else [o["pairs"][p, k, :o["lengths"][p, k]].tobytes() for k in range(n)]
    return n, int(o["status"][p]), o["scores"][p, :n].tobytes(), o["lengths"][p, :n].tobytes(), lists


def _same_outputs(a, b, pairs=None):
    return a["rc"] == b["rc"] and all(_valid(a, p) == _valid(b, p) for p in (range(len(a["n_out"])) if pairs is None else pairs))


def _check_pair(o, r, p, want=None, first=None):
    """pair p of the outputs against the oracle's set of the run (its first `first` entries when K cut it)"""
    want = ep.run_search(r, p).alis if want is None else want
    want = want if first is None else want[:first]
    what = (r.kind, p)
    assert o["n_out"][p] == len(want), what + (o["n_out"][p], len(want))
    for k, w in enumerate(want):
        assert _bits(o["scores"][p, k]) == _bits(w["score"]), what + (k, o["scores"][p, k], w["score"])
        assert o["lengths"][p, k] == len(w["pairs"]), what + (k,)
        if o["pairs"] is not None:
            assert np.array_equal(o["pairs"][p, k, :len(w["pairs"])], w["pairs"]), what + (k,)


def _check_all(o, r):
    assert o["rc"] == 0 and (o["status"] == 0).all(), (r.kind, o["rc"], o["status"])
    for p in range(len(ep.POOL_PAIRS)):
        _check_pair(o, r, p)


# ---- 2. pool growth and retry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knd", ep.KINDS)
def test_node_pool_grows_in_the_one_wave_kernels(knd, pool_batch):
    """A node_cap between the smallest and the largest need of the batch: with the default two retries every pair comes back
    complete (the host's rule `nodes >= node_cap - 64`, then 4 x and 16 x the pool); without retries exactly the pairs above
    the cap report ALN_E_OVERFLOW and the others are complete.  (ali_cap is the size user_limit bounds, so that no round is
    added for the alignment pool.)"""
    b, r, ctx = pool_batch, ep.SMALL[knd], gpu_util.ctx()
    with ctx.hints(enum_waves=1):
        generous = _raw_all(b, r)
        _check_all(generous, r)
        created, nodes = b.last_enum_usage()
        assert created.tolist() == ep.created_counts(r)
        assert (b.last_enum_tasks() == 0).all()
        cap = int(nodes.max()) // 8 + 64
        below, above = [p for p in range(b.n) if nodes[p] <= cap], [p for p in range(b.n) if nodes[p] > cap]
        print(knd, "nodes", nodes.tolist(), "node_cap", cap)
        assert nodes.min() <= cap < nodes.max() and len(below) >= 2 and len(above) >= 2
        assert 16 * cap >= int(nodes.max()) + 64
        grown = _raw_all(b, r, node_cap=cap)
        _check_all(grown, r)
        assert _same_outputs(grown, generous)
        assert b.last_enum_usage()[1].max() > cap and b.last_enum_usage()[1].tolist() == nodes.tolist()
        with ctx.hints(enum_pool_retries=0):
            tight = _raw_all(b, r, node_cap=cap)
        assert tight["rc"] == aln_amd.E_OVERFLOW
        assert [p for p in range(b.n) if tight["status"][p] == aln_amd.E_OVERFLOW] == above and (tight["status"][below] == 0).all()
        assert _same_outputs(dict(tight, rc=0), generous, pairs=below)
        assert (tight["n_out"][above] == 0).all()


KS_CR = [("kscw", 1, "kscw-one_wave"), ("kscw", 0, "kscw-waves_auto"), ("kscw", 3, "kscw-waves3"), ("crcw", 1, "crcw")]


@pytest.mark.parametrize("knd,waves", [x[:2] for x in KS_CR], ids=[x[2] for x in KS_CR])
def test_alignment_pool_grows_to_user_limit_kscw_crcw(knd, waves, pool_batch):
    """Alignment pools of 4 slots and no pool retries left: a pair whose set outgrows its slots is searched again until the
    pool has the size user_limit bounds, and comes back with the set the reference's brake defines — the rule
    test_batched_enumeration_grows_to_user_limit holds cw and ucw to."""
    r = ep.BRAKED[knd]
    wants = [ep.run_search(r, p).alis for p in range(pool_batch.n)]
    assert max(len(w) for w in wants) > r.user_limit
    with gpu_util.ctx().hints(enum_waves=waves, enum_pool_retries=0):
        o = _raw_all(pool_batch, r, K=max(len(w) for w in wants) + 2, node_cap=1 << 14, ali_cap=4)
    assert o["rc"] == 0 and (o["status"] == 0).all(), o["status"]
    for p, w in enumerate(wants):
        _check_pair(o, r, p, want=w)


@pytest.fixture(scope="module")
def large_one_pair(pool_batch):
    """the large searches through the one-pair entry point, once per kind (default waves)"""
    made = {}

    def get(knd):
        if knd not in made:
            r = ep.LARGE[knd]
            made[knd] = [pool_batch.enumerate(p, knd, r.nsub, r.delta, ep.flags(ep.POOL_PAIRS[p], ep.run_regions(r)[p]), max_alignments=r.nsub + 2,
                                              **ep.run_kw(r)) for p in range(pool_batch.n)]
        return made[knd]
    return get


@pytest.mark.parametrize("knd", list(ep.LARGE))
def test_chunked_node_pool(knd, par_waves, pool_batch, large_one_pair):
    """The several-wave kernel's node pool: node_cap = one 65536-node chunk per pair, so the first launch has as many chunks as
    pairs, four pairs need a second one (fetched under the LDS lock) and find the launch's chunks used up (n_chunks), and the
    4 x retry gives them room.  (A node_cap of 1 cannot do this: the pool of a launch is n_pairs x node_cap nodes rounded to
    chunks, which stays ONE chunk for the whole launch through both retries — test_one_chunk_for_a_whole_launch.)"""
    b, r, ctx = pool_batch, ep.LARGE[knd], gpu_util.ctx()
    generous = _raw_all(b, r, node_cap=1 << 20, ali_cap=1 << 16)
    _check_all(generous, r)
    created, nodes = b.last_enum_usage()
    tasks = b.last_enum_tasks()
    print(knd, par_waves, "created", created.tolist(), "nodes", nodes.tolist(), "tasks", tasks.tolist())
    assert created.tolist() == ep.created_counts(r)
    assert nodes.sum() > CHUNK and (nodes % 512 == 0).all()                    # (counted in the waves' reserves of 512)
    big = [p for p in range(b.n) if nodes[p] > CHUNK]
    assert len(big) >= 2 and len(big) <= b.n - 2                               # pairs that cross a chunk boundary by themselves
    assert all(abs(int(x) - CHUNK) > 8 * 512 for x in nodes)                   # ... and none so close that a few reserves decide it
    assert (tasks > created).all()
    o = _raw_all(b, r, node_cap=CHUNK, ali_cap=1 << 16)
    _check_all(o, r)
    assert _same_outputs(o, generous)
    for p, one in enumerate(large_one_pair(knd)):
        assert len(one) == o["n_out"][p]
        for k, g in enumerate(one):
            assert _bits(g["score"]) == _bits(o["scores"][p, k]) and np.array_equal(g["pairs"], o["pairs"][p, k, :o["lengths"][p, k]]), (knd, p, k)
    with ctx.hints(enum_pool_retries=0):
        tight = _raw_all(b, r, node_cap=CHUNK, ali_cap=1 << 18)                # (ali_cap: the size user_limit bounds — round 0 is the last)
    assert tight["rc"] == aln_amd.E_OVERFLOW
    assert [p for p in range(b.n) if tight["status"][p] == aln_amd.E_OVERFLOW] == big
    assert _same_outputs(dict(tight, rc=0), generous, pairs=[p for p in range(b.n) if p not in big])


def test_one_chunk_for_a_whole_launch(par_waves, pool_batch):
    """node_cap = 1: one chunk for the ten pairs of the launch, in the first launch and in both retries (4 and 16 nodes per
    pair still round to one chunk).  Whoever asks first gets it; every pair that reports 0 is right, the others report
    ALN_E_OVERFLOW, and so does the call."""
    b, r = pool_batch, ep.LARGE["kscw"]
    o = _raw_all(b, r, node_cap=1, ali_cap=1 << 16)
    assert o["rc"] == aln_amd.E_OVERFLOW and set(o["status"].tolist()) <= {0, aln_amd.E_OVERFLOW}
    done = [p for p in range(b.n) if o["status"][p] == 0]
    assert len(done) <= 3                                                      # at most one pair per launch can get the chunk ...
    nodes = b.last_enum_usage()[1]
    assert all(nodes[p] <= CHUNK for p in done)                                # ... and finish only if it fits
    for p in done:
        _check_pair(o, r, p)
    assert (o["n_out"][[p for p in range(b.n) if p not in done]] == 0).all()


@pytest.mark.parametrize("knd", list(ep.LARGE))
def test_task_ring_wraps(knd, par_waves, pool_batch, capfd):
    """ali_cap = the largest number of alignments a pair creates + 2200.  The task ring has ali_cap records and is indexed
    ticket % ali_cap; its overwrite guard asks for pending + min(ali_cap / 4, 2048) <= ali_cap, and every pending task owns a
    slot of its own, so pending <= created and the guard never trips.  Tickets go to every accepted candidate, the one that
    continues in its parent's slot included, so there are more tickets than slots: the ring wraps (tasks > ali_cap), with no
    retry (one group in the enum_debug report), and the sets are the oracle's."""
    b, r = pool_batch, ep.LARGE[knd]
    created = ep.created_counts(r)
    ali_cap = max(created) + 2200
    capfd.readouterr()
    with gpu_util.ctx().hints(enum_debug=1):
        o = _raw_all(b, r, node_cap=1 << 20, ali_cap=ali_cap)
    groups = re.findall(r"group of (\d+) pairs, \d+ waves/pair, node_cap \d+ ali_cap (\d+)", capfd.readouterr().err)
    assert groups == [(str(b.n), str(ali_cap))], groups
    _check_all(o, r)
    tasks = b.last_enum_tasks()
    print(knd, par_waves, "ali_cap", ali_cap, "tasks", tasks.tolist())
    assert b.last_enum_usage()[0].tolist() == created
    assert (tasks > ali_cap).sum() >= 2, (tasks.tolist(), ali_cap)


# ---- 2b. the one-pair entry point's overflow exits ------------------------------------------------------------------------------
def _one_pair(b, r, p, node_cap, **kw):
    """pair p of the ragged batch under the run r through aln_batch_enumerate, with enum_node_cap = node_cap"""
    rkw = ep.run_kw(r)
    with gpu_util.ctx().hints(enum_node_cap=node_cap):
        return _raw_enumerate(b, p, r.kind, r.nsub, r.delta, ep.flags(ep.POOL_PAIRS[p], ep.run_regions(r)[p]), rkw.pop("user_limit"),
                              r.nsub + 2, **dict(rkw, **kw))


@pytest.mark.parametrize("knd", list(ep.LARGE))
def test_one_pair_node_pool_overflows_several_waves(knd, pool_batch, large_one_pair):
    """aln_batch_enumerate has no retries: a pair that needs a second chunk of the several-wave kernel's node pool (taken from
    the usage a batched call records) reports ALN_E_OVERFLOW under enum_node_cap = one chunk and writes nothing; the same call on
    the same batch with 16 chunks returns the set the fixture's call with the default pool returned."""
    b, r = pool_batch, ep.LARGE[knd]
    want = large_one_pair(knd)
    _check_all(_raw_all(b, r, node_cap=1 << 20, ali_cap=1 << 16), r)
    nodes = b.last_enum_usage()[1]
    p = [p for p in range(b.n) if nodes[p] > CHUNK][0]
    print(knd, "pair", p, "nodes", int(nodes[p]))
    rc, n, recs, pairs = _one_pair(b, r, p, CHUNK)
    assert rc == aln_amd.E_OVERFLOW and n == SENTINEL and _untouched(recs, pairs), (knd, p, rc, n)
    rc, n, recs, pairs = _one_pair(b, r, p, 1 << 20)
    assert rc == 0 and n == len(want[p]), (knd, p, rc, n, len(want[p]))
    for k, w in enumerate(want[p]):
        score, identity, uid, n_pairs, pair_off = recs[k]
        assert _bits(score) == _bits(w["score"]) and _bits(identity) == _bits(w["identity"]) and uid == w["uid"], (knd, p, k)
        assert n_pairs == len(w["pairs"]) and np.array_equal(pairs[pair_off:pair_off + n_pairs], w["pairs"]), (knd, p, k)


@pytest.mark.parametrize("knd", ep.KINDS)
def test_one_pair_node_pool_overflows_one_wave(knd, pool_batch):
    """The one-wave kernels, enum_node_cap between the smallest and the largest need of the batch (from the recorded usage, as
    in test_node_pool_grows_in_the_one_wave_kernels): a pair above the cap reports ALN_E_OVERFLOW and writes nothing, a pair
    below it is complete, and the overflowed pair is complete under a larger cap — the error exit leaves the batch usable."""
    b, r = pool_batch, ep.SMALL[knd]
    with gpu_util.ctx().hints(enum_waves=1):
        _check_all(_raw_all(b, r), r)
        nodes = b.last_enum_usage()[1]
        cap = int(nodes.max()) // 8 + 64
        below, above = [p for p in range(b.n) if nodes[p] <= cap][0], [p for p in range(b.n) if nodes[p] > cap][0]
        print(knd, "nodes", nodes.tolist(), "node_cap", cap, "below", below, "above", above)
        rc, n, recs, pairs = _one_pair(b, r, above, cap)
        assert rc == aln_amd.E_OVERFLOW and n == SENTINEL and _untouched(recs, pairs), (knd, above, rc, n)
        _check_records(*_one_pair(b, r, below, cap), ep.run_search(r, below).alis, (), (knd, "below", below))
        _check_records(*_one_pair(b, r, above, 1 << 20), ep.run_search(r, above).alis, (), (knd, "above", above))


def test_one_pair_pairs_capacity_one_short(pool_batch):
    """Records enough, pairs_capacity one pair short of the kept lists: ALN_E_OVERFLOW from the host's assembly, behind the
    release of the device pools; the same call with the full capacity gives the oracle's set."""
    b, r, p = pool_batch, ep.SMALL["cw"], 0
    want = ep.run_search(r, p).alis
    total = sum(len(w["pairs"]) for w in want)
    rc, n, recs, pairs = _one_pair(b, r, p, 1 << 20, pairs_capacity=total - 1)
    assert rc == aln_amd.E_OVERFLOW and n == len(want), (rc, n, len(want))
    _check_records(*_one_pair(b, r, p, 1 << 20, pairs_capacity=total), want, (), ("cw", "capacity", total))


# ---- 3. kept pools and launch order ------------------------------------------------------------------------------------------------
def test_kept_pools_change_nothing():
    """One resident batch with enum_keep_pools = 1 through: the large several-wave cw search (with its chunk retries), the
    large kscw, crcw, a small one-wave ucw, the first cw again — pools larger than the request, ready words, node lengths and
    uids of the search before.  Each call equals the same call on a fresh batch that keeps nothing."""
    ctx = gpu_util.ctx()
    seq = [(ep.LARGE["cw"], 0, CHUNK, 1 << 16), (ep.LARGE["kscw"], 0, CHUNK, 1 << 16), (ep.SMALL["crcw"], 0, 1 << 20, 1 << 17),
           (ep.SMALL["ucw"], 1, 1 << 12, 1 << 10), (ep.LARGE["cw"], 0, CHUNK, 1 << 16)]
    kept = _pool_batch()
    for step, (r, waves, node_cap, ali_cap) in enumerate(seq):
        with ctx.hints(enum_keep_pools=1, enum_waves=waves):
            a = _raw_all(kept, r, node_cap=node_cap, ali_cap=ali_cap)
        fresh = _pool_batch()
        with ctx.hints(enum_keep_pools=0, enum_waves=waves):
            f = _raw_all(fresh, r, node_cap=node_cap, ali_cap=ali_cap)
        fresh.close()
        _check_all(f, r)
        assert _same_outputs(a, f), (step, r.kind)
    kept.close()


def test_launch_order_changes_nothing(enum_waves):
    """Index order (enum_heavy_first = 0), score order (a first call under enum_heavy_first = 1) and usage order (a second
    call): three different permutations of the batch, the same outputs."""
    ctx, r = gpu_util.ctx(), ep.LARGE["cw"]
    plain, heavy = _pool_batch(), _pool_batch()
    with ctx.hints(enum_heavy_first=0):
        a = _raw_all(plain, r, ali_cap=1 << 16)
    with ctx.hints(enum_heavy_first=1):
        first = _raw_all(heavy, r, ali_cap=1 << 16)
        nodes = heavy.last_enum_usage()[1]
        second = _raw_all(heavy, r, ali_cap=1 << 16)
    _check_all(a, r)
    assert _same_outputs(first, a) and _same_outputs(second, a)
    index, score, usage = list(range(plain.n)), ep.score_order(), ep.usage_order(nodes)
    print("score order", score, "usage order", usage, "nodes", nodes.tolist())
    assert usage != score and usage != index and score != index
    plain.close()
    heavy.close()


# ---- 4. output contract --------------------------------------------------------------------------------------------------------------
def test_k_below_the_kept_set(kind, pool_batch):
    """K = 8 slots for sets of up to number_suboptimal = 20: such a pair alone reports ALN_E_OVERFLOW, with n_out = K and its
    first K entries; the others are complete."""
    r, K = ep.SMALL[kind], 8
    o = _raw_all(pool_batch, r, K=K)
    wants = [ep.run_search(r, p).alis for p in range(pool_batch.n)]
    cut = [p for p, w in enumerate(wants) if len(w) > K]
    assert 3 <= len(cut) <= pool_batch.n - 1
    assert o["rc"] == aln_amd.E_OVERFLOW
    for p, w in enumerate(wants):
        assert o["status"][p] == (aln_amd.E_OVERFLOW if p in cut else 0), (kind, p)
        _check_pair(o, r, p, want=w, first=K)


def test_pairs_not_wanted(kind, pool_batch):
    r = ep.SMALL[kind]
    with_pairs, without = _raw_all(pool_batch, r), _raw_all(pool_batch, r, want_pairs=False)
    _check_all(with_pairs, r)
    _check_all(without, r)
    for k in ("n_out", "scores", "lengths", "status"):
        assert with_pairs[k].tobytes() == without[k].tobytes(), k


def test_one_shared_flag_row(kind, pool_batch):
    """flags_stride 0: every pair reads the first T bytes of one row — the same as 2-D rows that each hold that row"""
    r = ep.SMALL[kind]
    row = orc.make_subopt_regions(max(ep.dims(p)[1] for p in ep.POOL_PAIRS), 5)
    shared = _raw_all(pool_batch, r, flags=row)
    rows = _raw_all(pool_batch, r, flags=np.tile(row, (pool_batch.n, 1)))
    assert shared["rc"] == 0 and (shared["status"] == 0).all() and (shared["n_out"] >= 1).all()
    assert _same_outputs(shared, rows)
    assert _same_outputs(shared, _raw_all(pool_batch, r)) == (kind == "ucw")    # the run's own rows give other sets (ucw reads no flags)
    p = max(range(pool_batch.n), key=lambda k: ep.dims(ep.POOL_PAIRS[k])[1])    # the longest template: the row is its own, whole
    one = pool_batch.enumerate(p, kind, r.nsub, r.delta, row, max_alignments=r.nsub + 2, **ep.run_kw(r))
    assert len(one) == shared["n_out"][p]
    for k, g in enumerate(one):
        assert _bits(g["score"]) == _bits(shared["scores"][p, k]) and np.array_equal(g["pairs"], shared["pairs"][p, k, :shared["lengths"][p, k]])


def test_arguments_and_state_leave_the_outputs_alone(pool_batch):
    r = ep.SMALL["cw"]
    o = _raw_all(pool_batch, r, pair_stride=_stride(pool_batch) - 1)
    assert o["rc"] == aln_amd.E_ARG and _all_untouched(o)
    for K in (0, -3):
        o = _raw_all(pool_batch, r, K=K)
        assert o["rc"] == aln_amd.E_ARG and _all_untouched(o)
    ps = ep.POOL_PAIRS[:2]
    b = aln_amd.Batch(gpu_util.ctx(), [p.q for p in ps], [p.t for p in ps])
    r2 = r._replace(regions=3)
    fl = ep.flag_rows(ps, 3)
    b.dp_submatrix(ep.ALPHA, ep.BLOSUM, ep.POOL_MODE, 11, 1, direction=aln_amd.REV)
    o = _raw_all(b, r2, flags=fl)
    assert o["rc"] == aln_amd.E_STATE and _all_untouched(o)
    b.dp_sub_submatrix(ep.ALPHA, ep.BLOSUM, ep.POOL_MODE, 11, 1, aln_amd.FWD, [(2, 2, ep.dims(p)[0] - 3, ep.dims(p)[1] - 3) for p in ps])
    o = _raw_all(b, r2, flags=fl)
    assert o["rc"] == aln_amd.E_STATE and _all_untouched(o)
    b.dp_submatrix(ep.ALPHA, ep.BLOSUM, ep.POOL_MODE, 11, 1)                    # a forward build of the same batch: the call works again
    o = _raw_all(b, r2, flags=fl)
    assert o["rc"] == 0 and (o["status"] == 0).all() and (o["n_out"] >= 1).all()
    b.close()


def test_user_limit_boundary(kind, pool_batch):
    """user_limit = n - 2, n - 1, n, n + 1 around an un-braked set of n alignments, through both entry points: the several-wave
    kernel hands the pair back (kParSerial) exactly when the number of slots passes user_limit, and the one-wave kernel then
    brakes as the serial order does."""
    p, r, n, found = ep.boundary_case(kind)
    fl = ep.flags(ep.POOL_PAIRS[p], r.regions)
    for ul, f in sorted(found.items()):
        ru = r._replace(user_limit=ul)
        one = pool_batch.enumerate(p, kind, ru.nsub, ru.delta, fl, max_alignments=n + 4, **ep.run_kw(ru))
        _check_binding(one, f.alis, (), (kind, "boundary", ul))
        o = _raw_all(pool_batch, ru, K=n + 4, ali_cap=1 << 16)
        assert o["status"][p] == 0
        _check_pair(o, ru, p, want=f.alis)
        # the set grows to n slots: the several-wave kernel keeps the pair exactly while n <= user_limit (tasks > 0), and hands
        # it to the one-wave kernel (tasks 0) below that
        several = kind != "crcw" and gpu_util.ctx().get_hint("enum_waves") != 1
        assert (pool_batch.last_enum_tasks()[p] > 0) == (several and ul >= n), (kind, ul, n, pool_batch.last_enum_tasks()[p])
