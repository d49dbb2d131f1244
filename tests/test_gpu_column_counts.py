"""-m gpu: aln_hits_column_counts / aln_hits_column_counts_profiles — the column counts of search hits tallied on the device
(hit_local_kernel, hit_global_kernel under CountJob, csrc/search_counts.hip).  Everything is an integer and every comparison is
equality: counts and covered against the numpy tally over the oracle's pair lists (column_count_cases), the records byte for
byte against aln_hits_align called without lists and lines.

  1  every fused length class and the batch route into the same rows, a duplicated slot, weights, chunks, covered == NULL, list groups
  2  a row block with q_begin > 0
  3  a falsified local score, local pairs whose best score is 0, pairs without an interior
  4  the argument checks, in their order
  5  the profile entry: derived rows, position-specific rows at the staging boundaries, fractional rows
  6  two rounds: search, counts, pssm_from_counts, profile search"""
import ctypes as C

import numpy as np
import pytest

import aln_amd
import column_count_cases as cc
import gpu_util
import profile_align_cases as pac
import profile_cases as pc
import range_cases as rc
import search_cases as sc

pytestmark = pytest.mark.gpu

U32 = np.uint32
ALPHA = cc.ALPHA
_, GI, GE = cc.SYSTEM
K5 = 5


used_slots = cc.used_slots
hit_array = cc.hit_array


def slot_weights(weights, n_hits, K):
    return [1 if weights is None else int(weights[r, k]) for r, k in used_slots(n_hits, K)]


def check_counts(res, q_lens, ts, t_idx, n_hits, lists, weights, local, what):
    rec, counts, covered, rcode = res
    K = t_idx.shape[1]
    slots = [(r, int(t_idx[r, k])) for r, k in used_slots(n_hits, K)]
    want, want_cov = cc.tally(q_lens, ts, slots, lists, slot_weights(weights, n_hits, K), local)
    assert len(counts) == len(want)
    for r, (g, w) in enumerate(zip(counts, want)):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, r)
        print(what, "row", r, "cells that differ:", int((g != w).sum()), "sum", int(w.sum()))
        assert np.array_equal(g, w), (what, r, np.argwhere(g != w)[:6].tolist())
    if covered is not None:
        assert covered.dtype == np.int32 and np.array_equal(covered, want_cov), (what, np.argwhere(covered != want_cov)[:6].tolist())
    for (r, k), (score, pl) in zip(used_slots(n_hits, K), lists):
        assert rec["status"][r, k] == 0 and rec["n_pairs"][r, k] == len(pl), (what, r, k, rec[r, k])
        assert np.float32(rec["score"][r, k]).view(U32) == np.float32(score).view(U32), (what, r, k)
    return want, want_cov


def same_counts(a, b):
    assert a[0].tobytes() == b[0].tobytes() and a[3] == b[3]
    assert len(a[1]) == len(b[1]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))
    assert (a[2] is None) == (b[2] is None) and (a[2] is None or a[2].tobytes() == b[2].tobytes())


def class_inputs(mode):
    qs, ts = cc.class_set()
    t_idx, n_hits = cc.class_hits(K5)
    lists = [cc.pair_list(qs[r], ts[t_idx[r, k]], mode) for r, k in used_slots(n_hits, K5)]
    return qs, ts, t_idx, n_hits, lists, hit_array(t_idx, n_hits, lists, mode == rc.LOCAL)


def class_weights(n_hits):
    """0, 1 and 65535 over the used slots; the duplicate (slot 3) of every row differs from its twin (slot 0)"""
    w = np.full((len(n_hits), K5), -99, np.int32)                      # unused slots: a weight that must not be checked
    cycle = (65535, 1, 0, 1, 65535)
    for r, k in used_slots(n_hits, K5):
        w[r, k] = cycle[(r + k) % 5] if k != 3 else (0, 65535, 1)[r % 3]
    return w


# ---- 1. classes, routes, duplicates, weights, chunks ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_every_class_and_both_routes(mode):
    cc.check_sets()
    local = mode == rc.LOCAL
    qs, ts, t_idx, n_hits, lists, hits = class_inputs(mode)
    q_lens = [len(q) for q in qs]
    ctx = gpu_util.ctx()
    call = lambda **kw: aln_amd.hits_column_counts(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, align_type=mode, **kw)
    whole = call()
    fused, batched = aln_amd.hits_align_routes(ctx)
    n_used = int(n_hits.sum())
    # the LONG_T template (two slots) always goes through batches; local: so do the class-8 templates (indices 15, 16, two
    # slots each with the duplicate of row 3 ... counted from the slots themselves)
    cls = [cc.class_of(ts[t_idx[r, k]]) for r, k in used_slots(n_hits, K5)]
    want_batched = sum(c > 8 or (local and c == 8) for c in cls)
    assert (fused, batched) == (n_used - want_batched, want_batched) and want_batched >= 2 and fused >= 18
    assert sorted(set(c for c in cls if c <= (7 if local else 8))) == list(range(1, 8 if local else 9))
    want, want_cov = check_counts(whole, q_lens, ts, t_idx, n_hits, lists, None, local, ("class", mode))
    assert whole[3] == 0
    # the duplicated slot doubled what it adds: against a call without it
    n3 = np.minimum(n_hits, 3)
    lists3 = [l for (r, k), l in zip(used_slots(n_hits, K5), lists) if k < 3]
    three = aln_amd.hits_column_counts(ctx, qs, ts, hits, n3, ALPHA, cc.TABLE, GI, GE, align_type=mode)
    w3, _ = check_counts(three, q_lens, ts, t_idx, n3, lists3, None, local, ("three", mode))
    r0 = 0                                                             # row 0: slots 0 .. 3, slot 3 repeats slot 0
    only0 = cc.tally(q_lens, ts, [(r0, int(t_idx[r0, 0]))], [lists[0]], [1], local)[0][r0]
    assert only0.sum() > 0 and np.array_equal(want[r0] - w3[r0], only0)
    assert (want_cov >= np.concatenate([w.sum(axis=1) for w in want])).all()
    # the records are aln_hits_align's, byte for byte; unused slots are zero
    rec = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, align_type=mode, want_pairs=False, want_lines=False)[0]
    assert whole[0].tobytes() == rec.tobytes()
    for r in range(len(n_hits)):
        assert whole[0][r, n_hits[r]:].tobytes() == bytes(16 * (K5 - n_hits[r]))
    # weights 0, 1, 65535
    weights = class_weights(n_hits)
    heavy = call(weights=weights)
    check_counts(heavy, q_lens, ts, t_idx, n_hits, lists, weights, local, ("weights", mode))
    assert heavy[0].tobytes() == whole[0].tobytes()
    assert max(int(c.max()) for c in heavy[1]) >= 65535
    # chunks of 1 and 3 hits, covered == NULL
    for chunk in (1, 3):
        with ctx.hints(align_chunk_hits=chunk):
            same_counts(call(weights=weights), heavy)
            assert aln_amd.hits_align_routes(ctx) == (fused, batched)
    bare = call(weights=weights, want_covered=False)
    assert bare[2] is None
    same_counts((bare[0], bare[1], heavy[2], bare[3]), heavy)
    # the batch route's slots in groups (align_list_group_slots): local, its two or more slots one per group
    if local:
        with ctx.hints(align_list_group_slots=1):
            same_counts(call(weights=weights), heavy)
            assert aln_amd.hits_align_routes(ctx) == (fused, batched)
    if not local:
        with ctx.hints(align_fused_nonlocal=0):                        # every slot through batches: the route does not show
            same_counts(call(weights=weights), heavy)
            assert aln_amd.hits_align_routes(ctx) == (0, n_used)
        group = 3 if n_used % 3 else 4
        assert n_used > group and 0 < n_used % group                   # several groups, the last one shorter
        with ctx.hints(align_fused_nonlocal=0, align_list_group_slots=group):
            same_counts(call(weights=weights), heavy)
            assert aln_amd.hits_align_routes(ctx) == (0, n_used)


def test_align_list_group_slots_is_off_on_a_fresh_context_and_round_trips():
    """the hint alone, on the host: no call is made"""
    ctx = aln_amd.Context(0)
    try:
        assert ctx.get_hint("align_list_group_slots") == 0
        ctx.set_hint("align_list_group_slots", 7)
        assert ctx.get_hint("align_list_group_slots") == 7
        with ctx.hints(align_list_group_slots=2):
            assert ctx.get_hint("align_list_group_slots") == 2
        assert ctx.get_hint("align_list_group_slots") == 7
    finally:
        ctx.close()


# ---- 2. row blocks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (rc.LOCAL, rc.GLOBAL))
def test_a_row_block_indexes_its_rows_from_the_block(mode):
    qs, ts, t_idx, n_hits, lists, hits = class_inputs(mode)
    ctx = gpu_util.ctx()
    weights = class_weights(n_hits)
    whole = aln_amd.hits_column_counts(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, weights=weights, align_type=mode)
    off = np.concatenate(([0], np.cumsum([len(q) + 2 for q in qs])))
    for a, b in ((2, 5), (cc.LONG_ROW, cc.LONG_ROW + 1), (5, 6)):
        for chunk in (0, 2):
            with ctx.hints(align_chunk_hits=chunk):
                part = aln_amd.hits_column_counts(ctx, qs, ts, hits[a:b], n_hits[a:b], ALPHA, cc.TABLE, GI, GE, weights=weights[a:b],
                                                  q_begin=a, align_type=mode)
            assert part[0].tobytes() == whole[0][a:b].tobytes() and len(part[1]) == b - a
            assert all(x.tobytes() == y.tobytes() for x, y in zip(part[1], whole[1][a:b])), (mode, a, b)
            assert part[2].tobytes() == whole[2][off[a]:off[b]].tobytes(), (mode, a, b)
    empty = aln_amd.hits_column_counts(ctx, qs, ts, hits[4:4], n_hits[4:4], ALPHA, cc.TABLE, GI, GE, q_begin=4, align_type=mode)
    assert empty[0].shape == (0, K5) and empty[1] == [] and len(empty[2]) == 0 and empty[3] == 0


# ---- 3. slots that must not contribute ----------------------------------------------------------------------------------------------
def test_a_falsified_local_score_is_refused_and_adds_nothing():
    mode = rc.LOCAL
    qs, ts, t_idx, n_hits, lists, hits = class_inputs(mode)
    ctx = gpu_util.ctx()
    whole = aln_amd.hits_column_counts(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, align_type=mode)
    bad = hits.copy()
    br, bk = 1, 1                                                      # row 1 (65 residues), template 7: a fused slot
    assert cc.class_of(ts[t_idx[br, bk]]) <= 7 and lists[used_slots(n_hits, K5).index((br, bk))][0] > 0
    bad["score"][br, bk] += 1.0
    got = aln_amd.hits_column_counts(ctx, qs, ts, bad, n_hits, ALPHA, cc.TABLE, GI, GE, align_type=mode)
    assert got[3] == aln_amd.E_ARG
    want_status = np.zeros_like(whole[0]["status"])
    want_status[br, bk] = aln_amd.E_ARG
    assert np.array_equal(got[0]["status"], want_status) and got[0]["n_pairs"][br, bk] == 0
    rec = aln_amd.hits_align(ctx, qs, ts, bad, n_hits, ALPHA, cc.TABLE, GI, GE, want_pairs=False, want_lines=False)[0]
    assert got[0].tobytes() == rec.tobytes()
    weights = np.ones((len(n_hits), K5), np.int32)
    weights[br, bk] = 0                                                # the reference: the same slots without that one
    want, want_cov = cc.tally([len(q) for q in qs], ts, [(r, int(t_idx[r, k])) for r, k in used_slots(n_hits, K5)], lists,
                              slot_weights(weights, n_hits, K5), True)
    assert all(np.array_equal(g, w) for g, w in zip(got[1], want)) and np.array_equal(got[2], want_cov)
    assert not np.array_equal(got[1][br], whole[1][br])


def test_local_pairs_whose_best_score_is_zero_add_nothing():
    c = sc.CASES["all_negative"]
    qs, ts = sc.sequences(c)
    table = sc.TABLES[c.table]
    ctx = gpu_util.ctx()
    K = 4
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, ALPHA, table, c.gi, c.ge, K)
    assert (n_hits == K).all() and (hits["score"] == 0).all()
    got = aln_amd.hits_column_counts(ctx, qs, ts, hits, n_hits, ALPHA, table, c.gi, c.ge)
    fused, batched = aln_amd.hits_align_routes(ctx)
    assert fused > 0 and batched > 0 and got[3] == 0                  # the empty query and templates go through batches
    rec = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, ALPHA, table, c.gi, c.ge, want_pairs=False, want_lines=False)[0]
    assert got[0].tobytes() == rec.tobytes() and (rec["n_pairs"] > 0).any()
    assert not any(x.any() for x in got[1]) and not got[2].any()
    # the same slots under GLOBAL are alignments and do count
    glob = aln_amd.hits_column_counts(ctx, qs, ts, hits, n_hits, ALPHA, table, c.gi, c.ge, align_type=rc.GLOBAL)
    assert sum(int(x.sum()) for x in glob[1]) > 0


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_pairs_without_an_interior(mode):
    local = mode == rc.LOCAL
    qs = ["", "W", cc.homolog_set()[0][0]]                             # Q = 2, 3, 42
    ts = ["", "W", cc.homolog_set()[1][0], ""]                         # T = 2, 3, 42, 2
    t_idx = np.tile(np.arange(4, dtype=np.int32), (3, 1))
    n_hits = np.full(3, 4, np.int32)
    lists = [cc.pair_list(qs[r], ts[t_idx[r, k]], mode) for r, k in used_slots(n_hits, 4)]
    hits = hit_array(t_idx, n_hits, lists, local)
    if local:                                                          # a pair without an interior: the end cell is not checked
        for r, k in used_slots(n_hits, 4):
            if not (qs[r] and ts[k]):
                hits["q_end"][r, k], hits["t_end"][r, k] = -3, 99
    ctx = gpu_util.ctx()
    got = aln_amd.hits_column_counts(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, align_type=mode)
    assert aln_amd.hits_align_routes(ctx) == (4, 8)
    check_counts(got, [len(q) for q in qs], ts, t_idx, n_hits, lists, None, local, ("no interior", mode))
    assert not got[1][0].any() and got[1][0].shape == (2, cc.N) and got[1][2].sum() > 0
    rec = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, align_type=mode, want_pairs=False, want_lines=False)[0]
    assert got[0].tobytes() == rec.tobytes()


# ---- 4. arguments --------------------------------------------------------------------------------------------------------------------
class Raw:
    """both entries through ctypes with sentinel-filled outputs"""

    def __init__(self, qs, ts, K, table, profiles=None, mode=aln_amd.LOCAL):
        self.qp = aln_amd.SeqPool(qs)
        self.tp = aln_amd.SeqPool(ts)
        self.prof = aln_amd.QueryProfiles([np.asarray(p, np.float32) for p in profiles], ALPHA) if profiles is not None else None
        self.tab = np.ascontiguousarray(table, np.float32)
        self.sub = aln_amd.AlnSubmatrix(len(ALPHA), ALPHA.encode(), self.tab.ctypes.data_as(C.POINTER(C.c_float)))
        self.g = aln_amd.AlnGap()
        self.g.model, self.g.align_type, self.g.gap_init, self.g.gap_extn = aln_amd.GAP_AFFINE_CONST, mode, float(GI), float(GE)
        self.rows, self.K = len(qs), K
        self.n_rows = int(self.qp.offsets[-1])
        self.fill()

    def fill(self):
        self.out = np.full(self.rows * self.K * 16, 0x5A, dtype=np.uint8)
        self.counts = np.full(self.n_rows * len(ALPHA), 0x5A5A5A5A, dtype=np.int32)
        self.covered = np.full(self.n_rows, 0x5A5A5A5A, dtype=np.int32)

    def untouched(self):
        return (self.out == 0x5A).all() and (self.counts == 0x5A5A5A5A).all() and (self.covered == 0x5A5A5A5A).all()

    def call(self, hit_array_, n_array, **kw):
        ip = C.POINTER(C.c_int32)
        a = dict(q=self.qp.c, prof=self.prof.c if self.prof else None, cons=self.qp.c, templ=self.tp.c, sub=self.sub, g=self.g,
                 hits=hit_array_.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits=n_array.ctypes.data_as(ip), weights=None,
                 out=self.out.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)), counts=self.counts.ctypes.data_as(ip),
                 covered=self.covered.ctypes.data_as(ip), K=self.K, q_begin=0, q_end=self.rows)
        a.update(kw)
        if isinstance(a["weights"], np.ndarray):
            a["weights"] = a["weights"].ctypes.data_as(ip)
        ref = lambda x: None if x is None else C.byref(x)
        if self.prof is not None:
            return aln_amd.lib().aln_hits_column_counts_profiles(gpu_util.ctx().h, ref(a["prof"]), ref(a["cons"]), ref(a["templ"]),
                                                                 ref(a["g"]), a["q_begin"], a["q_end"], a["K"], a["hits"], a["n_hits"],
                                                                 a["weights"], a["out"], a["counts"], a["covered"])
        return aln_amd.lib().aln_hits_column_counts(gpu_util.ctx().h, ref(a["q"]), ref(a["templ"]), ref(a["sub"]), ref(a["g"]),
                                                    a["q_begin"], a["q_end"], a["K"], a["hits"], a["n_hits"], a["weights"], a["out"],
                                                    a["counts"], a["covered"])


gap = cc.gap


ARG_QS = ["PAWHEAE", "HEAGAWGHEE"]
ARG_TS = ["HEAGAWGHEE", "PAWHEAE", "AWHE"]


def slot_checks(raw, hits, n_hits, refused):
    """checks 3 and 4, the same for both entries: n_hits, t, the local end cell — then the weights, which come last"""
    E = aln_amd.E_ARG
    K = raw.K
    Q = [len(q) + 2 for q in ARG_QS]
    for field, r, k, value in (("n", 0, 0, -1), ("n", 1, 0, K + 1), ("t", 0, 1, -1), ("t", 1, 0, len(ARG_TS)),
                               ("q_end", 0, 0, 0), ("q_end", 1, 1, Q[1] - 1), ("t_end", 0, 1, 0),
                               ("t_end", 1, 0, len(ARG_TS[hits["t"][1, 0]]) + 1)):
        h, n = hits.copy(), n_hits.copy()
        if field == "n":
            n[r] = value
        else:
            h[field][r, k] = value
        refused(E, (field, r, k, value), h_arr=h, n_arr=n)
    ok = np.ones((2, K), np.int32)
    for r, k, value in ((0, 0, -1), (1, 1, 65536), (1, 0, 1 << 30)):
        w = ok.copy()
        w[r, k] = value
        refused(E, ("weight", r, k, value), weights=w)
    # a bad weight in a slot that is not used is not looked at; a bad end cell comes before a bad weight (the same status, so
    # the order shows only in that neither writes)
    n1 = n_hits.copy()
    n1[1] = 1
    w = ok.copy()
    w[1, 1] = -5
    raw.fill()
    assert raw.call(hits, n1, weights=w) == 0 and not raw.untouched()
    raw.fill()
    refused(0, "empty block", q_begin=1, q_end=1)


def test_argument_checks_leave_the_outputs_untouched():
    ctx = gpu_util.ctx()
    E = aln_amd.E_ARG
    K = 2
    hits, n_hits = aln_amd.search_topk(ctx, ARG_QS, ARG_TS, ALPHA, cc.TABLE, GI, GE, K)
    assert (n_hits == K).all()
    raw = Raw(ARG_QS, ARG_TS, K, cc.TABLE)
    assert raw.call(hits, n_hits) == 0 and not raw.untouched()
    assert (raw.counts >= 0).all() and raw.counts.sum() > 0 and (raw.covered >= 0).all()
    raw.fill()

    def refused(want, what, **kw):
        assert raw.call(kw.pop("h_arr", hits), kw.pop("n_arr", n_hits), **kw) == want, what
        assert raw.untouched(), what

    bad_t = aln_amd.SeqPool(["HEAGAWGHEE", "PAW?EAE", "AWHE"]).c
    # 1. NULL hits / n_hits / out / counts, K — before everything that follows
    for kw in (dict(hits=None), dict(n_hits=None), dict(out=None), dict(counts=None)):
        refused(E, kw, **kw)
    for k in (0, 1025, -1):
        refused(E, ("K", k), K=k)
    refused(E, "K before the residues", K=0, templ=bad_t)
    # 2. the checks of aln_score_all_vs_all, in its order
    for kw in (dict(q=None), dict(templ=None), dict(sub=None), dict(g=None)):
        refused(E, kw, **kw)
    refused(E, "q_begin < 0", q_begin=-1)
    refused(E, "q_end > n", q_end=3)
    refused(E, "q_begin > q_end", q_begin=1, q_end=0)
    refused(E, "gap model", g=gap(model=aln_amd.GAP_AFFINE_TPOS_MIN))
    refused(E, "align type", g=gap(align_type=5))
    refused(E, "the range comes before the residues", q_end=3, templ=bad_t)
    refused(aln_amd.E_RESIDUE, "a template letter outside the alphabet", templ=bad_t)
    refused(aln_amd.E_RESIDUE, "the residues come before n_hits", templ=bad_t, n_arr=np.array([3, 0], np.int32))
    refused(aln_amd.E_RESIDUE, "the residues come before the weights", templ=bad_t, weights=np.full((2, K), -1, np.int32))
    # 3. n_hits, t, the end cell; 4. the weights
    slot_checks(raw, hits, n_hits, refused)
    # covered may be NULL
    raw.fill()
    assert raw.call(hits, n_hits, covered=None) == 0 and (raw.covered == 0x5A5A5A5A).all() and (raw.counts != 0x5A5A5A5A).all()


def test_argument_checks_of_the_profile_entry():
    ctx = gpu_util.ctx()
    E = aln_amd.E_ARG
    K = 2
    profiles = pc.derived(ARG_QS, cc.TABLE)
    hits, n_hits = aln_amd.search_topk(ctx, ARG_QS, ARG_TS, ALPHA, cc.TABLE, GI, GE, K)
    raw = Raw(ARG_QS, ARG_TS, K, cc.TABLE, profiles=profiles)
    plain = Raw(ARG_QS, ARG_TS, K, cc.TABLE)
    assert raw.call(hits, n_hits) == 0 and plain.call(hits, n_hits) == 0
    assert raw.out.tobytes() == plain.out.tobytes() and raw.counts.tobytes() == plain.counts.tobytes()
    assert raw.covered.tobytes() == plain.covered.tobytes()
    raw.fill()

    def refused(want, what, **kw):
        assert raw.call(kw.pop("h_arr", hits), kw.pop("n_arr", n_hits), **kw) == want, what
        assert raw.untouched(), what

    def qprof(**kw):
        c = raw.prof.c
        d = dict(n_seqs=c.n_seqs, offsets=c.offsets, rows=c.rows, n=c.n, alphabet=c.alphabet)
        d.update(kw)
        return aln_amd.AlnQProfiles(d["n_seqs"], d["offsets"], d["rows"], d["n"], d["alphabet"])

    bad_t = aln_amd.SeqPool(["HEAGAWGHEE", "PAW?EAE", "AWHE"]).c
    wrong_n = aln_amd.AlnSeqs(1, raw.qp.c.offsets, raw.qp.c.residues)
    for kw in (dict(prof=None), dict(templ=None), dict(g=None), dict(hits=None), dict(n_hits=None), dict(out=None), dict(counts=None)):
        refused(E, kw, **kw)
    for k in (0, 1025):
        refused(E, ("K", k), K=k)
    refused(E, "K before the descriptor", K=0, prof=qprof(n=31), templ=bad_t)
    refused(E, "q_end > n", q_end=3)
    refused(E, "gap model", g=gap(model=aln_amd.GAP_AFFINE_TPOS_MIN))
    for kw in (dict(n=0), dict(n=31), dict(alphabet=None), dict(rows=None)):
        refused(E, kw, prof=qprof(**kw))
    refused(E, "consensus n_seqs", cons=wrong_n)
    refused(E, "the descriptor comes before the consensus", prof=qprof(n=31), cons=wrong_n, templ=bad_t)
    refused(E, "the consensus comes before the residues", cons=wrong_n, templ=bad_t)
    refused(aln_amd.E_RESIDUE, "a template letter outside the alphabet", templ=bad_t)
    refused(aln_amd.E_RESIDUE, "the residues come before n_hits", templ=bad_t, n_arr=np.array([3, 0], np.int32))
    slot_checks(raw, hits, n_hits, refused)
    raw.fill()
    assert raw.call(hits, n_hits, cons=None) == 0 and raw.counts.tobytes() == plain.counts.tobytes()


# ---- 5. the profile entry --------------------------------------------------------------------------------------------------------------
def pool(profiles):
    return aln_amd.QueryProfiles([np.asarray(p, np.float32) for p in profiles], ALPHA)


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_derived_profiles_equal_the_residue_entry(mode):
    local = mode == rc.LOCAL
    qs, ts, t_idx, n_hits, lists, hits = class_inputs(mode)
    ctx = gpu_util.ctx()
    weights = class_weights(n_hits)
    qp = aln_amd.profiles_from_sequences(qs, ALPHA, cc.TABLE)
    for w in (None, weights):
        want = aln_amd.hits_column_counts(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, weights=w, align_type=mode)
        routes_want = aln_amd.hits_align_routes(ctx)
        got = aln_amd.hits_column_counts_profiles(ctx, qp, ts, hits, n_hits, GI, GE, consensus=qs, weights=w, align_type=mode)
        routes_got = aln_amd.hits_align_routes(ctx)
        same_counts(got, want)
        # the profile side keeps class 8 of the local kernel, the residue side does not: two routes, one result
        assert sum(routes_got) == sum(routes_want) == int(n_hits.sum())
        assert routes_got[0] == routes_want[0] + (sum(cc.class_of(ts[t_idx[r, k]]) == 8 for r, k in used_slots(n_hits, K5)) if local else 0)
    rec = aln_amd.hits_align_profiles(ctx, qp, ts, hits, n_hits, GI, GE, consensus=qs, align_type=mode, want_pairs=False,
                                      want_lines=False)[0]
    assert got[0].tobytes() == rec.tobytes()
    for chunk, per_chunk in ((1, 0), (3, 1)):
        with ctx.hints(align_chunk_hits=chunk, align_rows_per_chunk=per_chunk):
            same_counts(aln_amd.hits_column_counts_profiles(ctx, qp, ts, hits, n_hits, GI, GE, consensus=qs, weights=weights,
                                                            align_type=mode), got)
    a, b = 2, 5
    off = np.concatenate(([0], np.cumsum([len(q) + 2 for q in qs])))
    for per_chunk in (0, 1):
        with ctx.hints(align_rows_per_chunk=per_chunk):
            part = aln_amd.hits_column_counts_profiles(ctx, qp, ts, hits[a:b], n_hits[a:b], GI, GE, consensus=qs, weights=weights[a:b],
                                                       q_begin=a, align_type=mode)
        assert part[0].tobytes() == got[0][a:b].tobytes() and part[2].tobytes() == got[2][off[a]:off[b]].tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(part[1], got[1][a:b]))


STAGING_ROWS = (1, 7, 8, 9, 64, 65, 130)                               # interior rows at every boundary of the staging ring


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_position_specific_rows_against_the_int64_reference(mode):
    local = mode == rc.LOCAL
    every, ts = pc.length_set()
    profiles = [p for p in every[:len(pc.INTERIOR_ROWS)] if len(p) in STAGING_ROWS]
    assert tuple(len(p) for p in profiles) == STAGING_ROWS
    _, gi, ge = pc.LENGTH_SYSTEM
    ctx = gpu_util.ctx()
    qp = pool(profiles)
    K = 4
    hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, ts, gi, ge, K, align_type=mode)
    assert (n_hits == K).all()
    hits[3, 2] = hits[3, 0]                                            # a duplicate
    slots = used_slots(n_hits, K)
    lists = []
    for r, k in slots:
        score, pl = pac.restated(profiles[r], ts[hits["t"][r, k]], ALPHA, mode, gi, ge)
        if pl is None:                                                 # a non-local pair without an interior: nothing to tally
            pl = np.zeros((0, 2), np.int32)
        lists.append((score, pl))
    weights = np.array([[1 + (3 * r + k) % 5 for k in range(K)] for r in range(len(profiles))], np.int32)
    got = aln_amd.hits_column_counts_profiles(ctx, qp, ts, hits, n_hits, gi, ge, weights=weights, align_type=mode)
    fused, batched = aln_amd.hits_align_routes(ctx)
    assert fused > 0 and fused + batched == len(slots)
    want, want_cov = cc.tally([len(p) for p in profiles], ts, [(r, int(hits["t"][r, k])) for r, k in slots], lists,
                              slot_weights(weights, n_hits, K), local)
    for r, (g, w) in enumerate(zip(got[1], want)):
        assert np.array_equal(g, w), (mode, r, np.argwhere(g != w)[:6].tolist())
    assert np.array_equal(got[2], want_cov) and sum(int(w.sum()) for w in want) > 0
    for (r, k), (score, pl) in zip(slots, lists):
        assert np.float32(got[0]["score"][r, k]).view(U32) == np.float32(score).view(U32) and got[0]["status"][r, k] == 0
    rec = aln_amd.hits_align_profiles(ctx, qp, ts, hits, n_hits, gi, ge, align_type=mode, want_pairs=False, want_lines=False)[0]
    assert got[0].tobytes() == rec.tobytes()


def tally_of_lists(q_lens, ts, hits, n_hits, res, weights, local):
    """the tally over the lists hits_align(_profiles) returned: what the entry is defined by"""
    K = hits.shape[1]
    slots = used_slots(n_hits, K)
    lists = [(res[0]["score"][r, k], res[1][r][k]) for r, k in slots]
    return cc.tally(q_lens, ts, [(r, int(hits["t"][r, k])) for r, k in slots], lists, slot_weights(weights, n_hits, K), local)


@pytest.mark.parametrize("mode", (rc.LOCAL, rc.SEMI_LOCAL))
def test_fractional_rows_go_through_batches(mode):
    profiles, ts = pc.mixed_set()
    half = [np.asarray(p, np.float32) * np.float32(0.5) for p in profiles]
    assert any((h != np.round(h)).any() for h in half)
    ctx = gpu_util.ctx()
    hp = aln_amd.QueryProfiles(half, ALPHA)
    K = 3
    hits, n_hits = aln_amd.search_topk_profiles(ctx, hp, ts, 11, 1, K, align_type=mode)
    weights = np.array([[2, 1, 65535], [1, 0, 3]], np.int32)
    got = aln_amd.hits_column_counts_profiles(ctx, hp, ts, hits, n_hits, 11, 1, weights=weights, align_type=mode)
    assert aln_amd.hits_align_routes(ctx) == (0, int(n_hits.sum()))
    res = aln_amd.hits_align_profiles(ctx, hp, ts, hits, n_hits, 11, 1, align_type=mode, want_lines=False)
    assert got[0].tobytes() == res[0].tobytes() and (res[0]["status"] == 0).all()
    want, want_cov = tally_of_lists([len(p) for p in half], ts, hits, n_hits, res, weights, mode == rc.LOCAL)
    assert all(np.array_equal(g, w) for g, w in zip(got[1], want)) and np.array_equal(got[2], want_cov)
    assert sum(int(w.sum()) for w in want) > 0


# ---- 6. two rounds ------------------------------------------------------------------------------------------------------------------------
def test_two_rounds_search_counts_profile_search():
    qs, ts = cc.homolog_set()
    assert len(qs) == 8 and len(ts) == 10
    ctx = gpu_util.ctx()
    K = 4
    mode = rc.LOCAL
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, ALPHA, cc.TABLE, GI, GE, K)                       # 1. search
    assert (n_hits == K).all()
    rec, counts, covered, rcode = aln_amd.hits_column_counts(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE)   # 2. counts
    assert rcode == 0
    lists = [cc.pair_list(qs[r], ts[hits["t"][r, k]], mode) for r, k in used_slots(n_hits, K)]
    want, want_cov = cc.tally([len(q) for q in qs], ts, [(r, int(hits["t"][r, k])) for r, k in used_slots(n_hits, K)], lists,
                              [1] * int(n_hits.sum()), True)
    assert all(np.array_equal(g, w) for g, w in zip(counts, want)) and np.array_equal(covered, want_cov)
    background = np.full(len(ALPHA), 1.0 / len(ALPHA))
    fallback = pc.derived(qs, cc.TABLE)
    rows = [aln_amd.pssm_from_counts(counts[r][1:-1], background, fallback[r]) for r in range(len(qs))]   # 3. the profile
    assert all(np.array_equal(p, np.rint(p)) for p in rows) and any((c[1:-1].sum(axis=1) > 0).all() for c in counts)
    profiles = [p.astype(np.int64) for p in rows]
    assert any(not np.array_equal(p, f) for p, f in zip(profiles, fallback))
    qp = pool(profiles)
    hits2, n2 = aln_amd.search_topk_profiles(ctx, qp, ts, GI, GE, K)                                     # 4. profile search
    scores, ends = pc.dense_reference("column_counts_two_rounds", profiles, ts, mode, GI, GE)
    for r in range(len(qs)):
        order = sc.topk_reference(scores[r], K)
        assert n2[r] == len(order) and hits2["t"][r, :len(order)].tolist() == order, (r, hits2[r].tolist(), order)
        assert np.array_equal(hits2["score"][r, :len(order)].view(U32), scores[r, order].astype(np.float32).view(U32)), r
        assert np.array_equal(hits2["q_end"][r, :len(order)], ends[r, order, 0]), r
        assert np.array_equal(hits2["t_end"][r, :len(order)], ends[r, order, 1]), r
    # and the loop closes: the second round's hits can be counted again, from the profile side
    again = aln_amd.hits_column_counts_profiles(ctx, qp, ts, hits2, n2, GI, GE, consensus=qs)
    assert again[3] == 0 and sum(int(c.sum()) for c in again[1]) > 0
