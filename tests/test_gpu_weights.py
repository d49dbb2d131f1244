"""-m gpu: aln_hits_weights / aln_hits_weights_profiles — position-based sequence weights of search hits and the column counts
under them, made on the device from letters rows that never come down (csrc/search_weights.hip).  Everything is an integer and
every comparison is equality: weights, raw, counts and covered against the integer loops of weight_cases over the oracle's pair
lists, the records byte for byte against aln_hits_align called without lists and lines.

  1  the sets under every align type and w_max: class edges, both routes into one stack, duplicates, K = 1 / 5 / 65, n_hits 0
     and below K; groups of 1 and 3 rows, chunks of 1 and 3 hits, align_fused_nonlocal = 0, list groups; a muted row
  2  raw, counts and covered each NULL in turn
  3  a row block with q_begin > 0
  4  a falsified local score
  5  the profile entry: derived rows, position-specific rows at the staging boundaries
  6  the argument checks, in their order
  7  two rounds: search, weights with counts, profile, profile search"""
import ctypes as C

import numpy as np
import pytest

import aln_amd
import column_count_cases as cc
import gpu_util
import pileup_cases as pu
import profile_cases as pc
import range_cases as rc
import search_cases as sc
import weight_cases as wc

pytestmark = pytest.mark.gpu

U32 = np.uint32
ALPHA = cc.ALPHA
_, GI, GE = cc.SYSTEM
used_slots = pu.used_slots


def same(a, b, what=None):
    """two 6-tuples of hits_weights, byte for byte"""
    assert a[5] == b[5], what
    for x, y in zip((a[0], a[1], a[2], a[4]), (b[0], b[1], b[2], b[4])):
        assert (x is None) == (y is None) and (x is None or (x.shape == y.shape and x.tobytes() == y.tobytes())), what
    assert (a[3] is None) == (b[3] is None), what
    if a[3] is not None:
        assert len(a[3]) == len(b[3]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[3], b[3])), what


def check(res, ref, n_hits, lists, what):
    """a result against weight_cases.reference"""
    rec, weights, raw, counts, covered, rcode = res
    assert rcode == 0 and weights.dtype == np.int32 and raw.dtype == np.int64 and covered.dtype == np.int32, what
    K = weights.shape[1]
    print(what, "weights that differ:", int((weights != ref["weights"]).sum()), "raw:", int((raw != ref["raw"]).sum()),
          "count rows:", sum(int((g != w).any(axis=1).sum()) for g, w in zip(counts, ref["counts"])),
          "covered:", int((covered != ref["covered"]).sum()))
    assert np.array_equal(weights, ref["weights"]), (what, weights.tolist(), ref["weights"].tolist())
    assert np.array_equal(raw, ref["raw"]), what
    assert len(counts) == len(ref["counts"]) and all(g.dtype == np.int32 and np.array_equal(g, w) for g, w in zip(counts, ref["counts"])), what
    assert np.array_equal(covered, ref["covered"]), what
    for (r, k), (score, pl) in zip(used_slots(n_hits, K), lists):
        assert rec["status"][r, k] == 0 and rec["n_pairs"][r, k] == len(pl), (what, r, k, rec[r, k])
        assert np.float32(rec["score"][r, k]).view(U32) == np.float32(score).view(U32), (what, r, k)
    for r in range(len(n_hits)):
        assert rec[r, n_hits[r]:].tobytes() == bytes(16 * (K - n_hits[r])), (what, r)


def set_inputs(name, mode):
    qs, ts, t_idx, n_hits, (table, gi, ge) = wc.sets()[name]
    lists = wc.set_lists(name, mode)
    return qs, ts, t_idx, n_hits, lists, cc.hit_array(t_idx, n_hits, lists, mode == rc.LOCAL), sc.TABLES[table], gi, ge


# ---- 1. the sets -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("class", "homolog65", "homolog1"))
@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_the_sets_against_the_reference(mode, name):
    wc.check_sets((mode,))
    local = mode == rc.LOCAL
    qs, ts, t_idx, n_hits, lists, hits, table, gi, ge = set_inputs(name, mode)
    q_lens = [len(q) for q in qs]
    ctx = gpu_util.ctx()
    call = lambda **kw: aln_amd.hits_weights(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, align_type=mode, **kw)
    for w_max in wc.W_MAXES:
        check(call(w_max=w_max), wc.reference(q_lens, ts, t_idx, n_hits, lists, local, w_max), n_hits, lists, (name, mode, w_max))
    whole = call()                                                     # w_max = 1000
    fused, batched = aln_amd.hits_align_routes(ctx)
    n_used = int(n_hits.sum())
    assert fused + batched == n_used and fused > 0
    if name == "class":                                                # row LONG_ROW: four fused slots and one through batches
        assert batched >= 1 and len(ts[t_idx[cc.LONG_ROW, 4]]) == cc.LONG_T and whole[2][cc.LONG_ROW, 4] > 0
        assert (whole[2][cc.LONG_ROW, :4] > 0).all()
    # the records are aln_hits_align's, the counts aln_hits_column_counts' under these weights: byte for byte
    rec = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, align_type=mode, want_pairs=False, want_lines=False)[0]
    assert whole[0].tobytes() == rec.tobytes()
    crec, counts, covered, crc = aln_amd.hits_column_counts(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, weights=whole[1],
                                                            align_type=mode)
    assert crc == 0 and crec.tobytes() == whole[0].tobytes() and covered.tobytes() == whole[4].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(counts, whole[3]))
    # equal slots, equal weights; unused slots 0
    for r in range(len(qs)):
        assert not whole[1][r, n_hits[r]:].any() and not whole[2][r, n_hits[r]:].any()
        for a in range(n_hits[r]):
            for b in range(a + 1, n_hits[r]):
                if t_idx[r, a] == t_idx[r, b]:
                    assert whole[1][r, a] == whole[1][r, b] and whole[2][r, a] == whole[2][r, b], (r, a, b)
    # groups of rows, chunks of hits, list groups, every slot through batches
    for rows in (1, 3):
        with ctx.hints(weights_group_rows=rows):
            same(call(), whole, ("weights_group_rows", rows))
            assert aln_amd.hits_align_routes(ctx) == (fused, batched)
    for chunk in (1, 3):
        with ctx.hints(align_chunk_hits=chunk):
            same(call(), whole, ("align_chunk_hits", chunk))
        with ctx.hints(align_chunk_hits=chunk, weights_group_rows=3):
            same(call(), whole, ("align_chunk_hits and groups", chunk))
    with ctx.hints(align_list_group_slots=1):
        same(call(), whole, "align_list_group_slots")
    if not local:
        with ctx.hints(align_fused_nonlocal=0):
            same(call(), whole, "align_fused_nonlocal")
            assert aln_amd.hits_align_routes(ctx) == (0, n_used)
        with ctx.hints(align_fused_nonlocal=0, weights_group_rows=1, align_list_group_slots=2):
            same(call(), whole, "align_fused_nonlocal in groups")


def test_every_slot_of_the_long_k_loop_through_batches():
    """K = 65 with align_fused_nonlocal = 0: the rows of a whole stack uploaded from the host"""
    mode = rc.GLOBAL_LOCAL
    qs, ts, t_idx, n_hits, lists, hits, table, gi, ge = set_inputs("homolog65", mode)
    ctx = gpu_util.ctx()
    whole = aln_amd.hits_weights(ctx, qs[:3], ts, hits[:3], n_hits[:3], ALPHA, table, gi, ge, align_type=mode)
    with ctx.hints(align_fused_nonlocal=0):
        same(aln_amd.hits_weights(ctx, qs[:3], ts, hits[:3], n_hits[:3], ALPHA, table, gi, ge, align_type=mode), whole)
        assert aln_amd.hits_align_routes(ctx) == (0, int(n_hits[:3].sum()))


def test_weights_group_rows_is_off_on_a_fresh_context_and_round_trips():
    """the hint alone, on the host: no call is made"""
    ctx = aln_amd.Context(0)
    try:
        assert ctx.get_hint("weights_group_rows") == 0
        ctx.set_hint("weights_group_rows", 7)
        assert ctx.get_hint("weights_group_rows") == 7
        with ctx.hints(weights_group_rows=2):
            assert ctx.get_hint("weights_group_rows") == 2
        assert ctx.get_hint("weights_group_rows") == 7
    finally:
        ctx.close()


def test_a_row_whose_every_slot_is_muted_weighs_nothing():
    wc.check_sets((rc.LOCAL,))
    qs, ts, t_idx, n_hits, (table, gi, ge) = wc.sets()["muted"]
    ctx = gpu_util.ctx()
    K = 3
    hits, nh = aln_amd.search_topk(ctx, qs, ts, ALPHA, sc.TABLES[table], gi, ge, K)
    assert (nh == K).all() and (hits["score"] == 0).all()
    got = aln_amd.hits_weights(ctx, qs, ts, hits, nh, ALPHA, sc.TABLES[table], gi, ge)
    assert got[5] == 0 and not got[1].any() and not got[2].any() and not got[4].any() and not any(c.any() for c in got[3])
    rec = aln_amd.hits_align(ctx, qs, ts, hits, nh, ALPHA, sc.TABLES[table], gi, ge, want_pairs=False, want_lines=False)[0]
    assert got[0].tobytes() == rec.tobytes() and (rec["n_pairs"] > 0).any()
    # the same slots under GLOBAL are alignments and do weigh
    glob = aln_amd.hits_weights(ctx, qs, ts, hits, nh, ALPHA, sc.TABLES[table], gi, ge, align_type=rc.GLOBAL)
    assert (glob[1].max(axis=1) == 1000).all() and (glob[2] > 0).all()


# ---- 2. the optional outputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (rc.LOCAL, rc.SEMI_LOCAL))
def test_raw_counts_and_covered_each_null_in_turn(mode):
    qs, ts, t_idx, n_hits, lists, hits, table, gi, ge = set_inputs("class", mode)
    ctx = gpu_util.ctx()
    call = lambda **kw: aln_amd.hits_weights(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, align_type=mode, **kw)
    whole = call()
    for drop, at in (("want_raw", 2), ("want_counts", 3), ("want_covered", 4)):
        want = list(whole)
        want[at] = None
        same(call(**{drop: False}), want, drop)
    same(call(want_raw=False, want_counts=False, want_covered=False), [whole[0], whole[1], None, None, None, whole[5]], "weights alone")
    with ctx.hints(weights_group_rows=2):
        same(call(want_counts=False), [whole[0], whole[1], whole[2], None, whole[4], whole[5]], "covered without counts, in groups")


# ---- 3. row blocks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (rc.LOCAL, rc.GLOBAL))
def test_a_row_block_with_q_begin(mode):
    qs, ts, t_idx, n_hits, lists, hits, table, gi, ge = set_inputs("class", mode)
    ctx = gpu_util.ctx()
    whole = aln_amd.hits_weights(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, align_type=mode)
    off = np.concatenate(([0], np.cumsum([len(q) + 2 for q in qs])))
    for a, b in ((2, 5), (cc.LONG_ROW, cc.LONG_ROW + 1), (5, 6)):
        for group in (0, 2):
            with ctx.hints(weights_group_rows=group):
                part = aln_amd.hits_weights(ctx, qs, ts, hits[a:b], n_hits[a:b], ALPHA, table, gi, ge, q_begin=a, align_type=mode)
            same(part, (whole[0][a:b], whole[1][a:b], whole[2][a:b], whole[3][a:b], whole[4][off[a]:off[b]], whole[5]), (mode, a, b))
    empty = aln_amd.hits_weights(ctx, qs, ts, hits[4:4], n_hits[4:4], ALPHA, table, gi, ge, q_begin=4, align_type=mode)
    assert empty[0].shape == (0, 5) and empty[1].shape == (0, 5) and empty[3] == [] and len(empty[4]) == 0 and empty[5] == 0
    # a row without hits between rows with hits
    none = n_hits.copy()
    none[2] = 0
    got = aln_amd.hits_weights(ctx, qs, ts, hits, none, ALPHA, table, gi, ge, align_type=mode)
    assert not got[1][2].any() and not got[2][2].any() and not got[3][2].any() and got[0][2].tobytes() == bytes(16 * 5)
    keep = [r for r in range(len(qs)) if r != 2]
    assert got[1][keep].tobytes() == whole[1][keep].tobytes() and got[2][keep].tobytes() == whole[2][keep].tobytes()
    assert all(got[3][r].tobytes() == whole[3][r].tobytes() for r in keep)


# ---- 4. a slot that fails -----------------------------------------------------------------------------------------------------------------
def test_a_falsified_local_score_is_refused_and_does_not_contribute():
    mode = rc.LOCAL
    qs, ts, t_idx, n_hits, lists, hits, table, gi, ge = set_inputs("class", mode)
    K = 5
    ctx = gpu_util.ctx()
    whole = aln_amd.hits_weights(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge)
    bad = hits.copy()
    br, bk = 1, 1                                                      # row 1 (65 residues), template 7: a fused slot
    assert cc.class_of(ts[t_idx[br, bk]]) <= 7 and lists[used_slots(n_hits, K).index((br, bk))][0] > 0
    bad["score"][br, bk] += 1.0
    got = aln_amd.hits_weights(ctx, qs, ts, bad, n_hits, ALPHA, table, gi, ge)
    assert got[5] == aln_amd.E_ARG
    want_status = np.zeros_like(whole[0]["status"])
    want_status[br, bk] = aln_amd.E_ARG
    assert np.array_equal(got[0]["status"], want_status) and got[0]["n_pairs"][br, bk] == 0
    rec = aln_amd.hits_align(ctx, qs, ts, bad, n_hits, ALPHA, table, gi, ge, want_pairs=False, want_lines=False)[0]
    assert got[0].tobytes() == rec.tobytes()
    # the reference: the same row without that slot (a list of score 0 is what a slot that does not contribute looks like)
    muted = list(lists)
    muted[used_slots(n_hits, K).index((br, bk))] = (0.0, lists[used_slots(n_hits, K).index((br, bk))][1])
    ref = wc.reference([len(q) for q in qs], ts, t_idx, n_hits, muted, True, 1000)
    assert np.array_equal(got[1], ref["weights"]) and np.array_equal(got[2], ref["raw"]) and np.array_equal(got[4], ref["covered"])
    assert all(np.array_equal(g, w) for g, w in zip(got[3], ref["counts"]))
    assert got[1][br, bk] == 0 and got[2][br, bk] == 0 and whole[2][br, bk] > 0 and not np.array_equal(got[2][br], whole[2][br])
    keep = [r for r in range(len(qs)) if r != br]
    assert got[1][keep].tobytes() == whole[1][keep].tobytes()


# ---- 5. the profile entry ----------------------------------------------------------------------------------------------------------------
def pool(profiles):
    return aln_amd.QueryProfiles([np.asarray(p, np.float32) for p in profiles], ALPHA)


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_derived_profiles_equal_the_residue_entry(mode):
    qs, ts, t_idx, n_hits, lists, hits, table, gi, ge = set_inputs("class", mode)
    ctx = gpu_util.ctx()
    qp = aln_amd.profiles_from_sequences(qs, ALPHA, table)
    want = aln_amd.hits_weights(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, align_type=mode)
    got = aln_amd.hits_weights_profiles(ctx, qp, ts, hits, n_hits, gi, ge, consensus=qs, align_type=mode)
    assert sum(aln_amd.hits_align_routes(ctx)) == int(n_hits.sum())
    same(got, want)
    rec = aln_amd.hits_align_profiles(ctx, qp, ts, hits, n_hits, gi, ge, consensus=qs, align_type=mode, want_pairs=False,
                                      want_lines=False)[0]
    assert got[0].tobytes() == rec.tobytes()
    for chunk, per_chunk, group in ((1, 0, 0), (3, 1, 2)):
        with ctx.hints(align_chunk_hits=chunk, align_rows_per_chunk=per_chunk, weights_group_rows=group):
            same(aln_amd.hits_weights_profiles(ctx, qp, ts, hits, n_hits, gi, ge, consensus=qs, align_type=mode), got)
    crec, counts, covered, crc = aln_amd.hits_column_counts_profiles(ctx, qp, ts, hits, n_hits, gi, ge, consensus=qs, weights=got[1],
                                                                     align_type=mode)
    assert crec.tobytes() == got[0].tobytes() and covered.tobytes() == got[4].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(counts, got[3]))
    # a given consensus and a NULL one differ only in the records' identity
    bare = aln_amd.hits_weights_profiles(ctx, qp, ts, hits, n_hits, gi, ge, align_type=mode)
    assert bare[1].tobytes() == got[1].tobytes() and bare[2].tobytes() == got[2].tobytes() and bare[4].tobytes() == got[4].tobytes()


STAGING_ROWS = (7, 64, 65)                                             # interior rows around the staging ring's boundaries


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_position_specific_rows_against_the_reference(mode):
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
    hits[1, 2] = hits[1, 0]                                            # a duplicate
    lists = [pu.profile_list(profiles[r], ts[hits["t"][r, k]], mode, gi, ge) for r, k in used_slots(n_hits, K)]
    got = aln_amd.hits_weights_profiles(ctx, qp, ts, hits, n_hits, gi, ge, align_type=mode)
    fused, batched = aln_amd.hits_align_routes(ctx)
    assert fused > 0 and fused + batched == int(n_hits.sum())
    ref = wc.reference([len(p) for p in profiles], ts, hits["t"], n_hits, lists, local, 1000)
    check(got, ref, n_hits, lists, ("rows", mode))
    assert got[1].any() and got[1][1, 2] == got[1][1, 0]
    # ... and against the numpy restatement over the library's own pileup
    letters = aln_amd.hits_pileup_profiles(ctx, qp, ts, hits, n_hits, gi, ge, align_type=mode, want_tpos=False, want_spans=False)[2]
    for r in range(len(profiles)):
        w, raw = aln_amd.weights_from_pileup(letters[r], ALPHA, 1000)
        assert np.array_equal(w, got[1][r]) and np.array_equal(raw, got[2][r]), (mode, r)
        counts, covered = aln_amd.counts_from_pileup(letters[r], ALPHA, w)
        assert np.array_equal(counts[:len(profiles[r])], got[3][r][1:-1]), (mode, r)


# ---- 6. arguments ----------------------------------------------------------------------------------------------------------------------
ARG_QS = ["PAWHEAE", "HEAGAWGHEE"]
ARG_TS = ["HEAGAWGHEE", "PAWHEAE", "AWHE"]
N_ROWS = sum(len(q) + 2 for q in ARG_QS)


class Raw:
    """both entries through ctypes with sentinel-filled outputs"""

    def __init__(self, K, profiles=None):
        self.qp = aln_amd.SeqPool(ARG_QS)
        self.tp = aln_amd.SeqPool(ARG_TS)
        self.prof = aln_amd.QueryProfiles([np.asarray(p, np.float32) for p in profiles], ALPHA) if profiles is not None else None
        self.tab = np.ascontiguousarray(cc.TABLE, np.float32)
        self.sub = aln_amd.AlnSubmatrix(len(ALPHA), ALPHA.encode(), self.tab.ctypes.data_as(C.POINTER(C.c_float)))
        self.g = cc.gap()
        self.rows, self.K = len(ARG_QS), K
        self.fill()

    def fill(self):
        n = self.rows * self.K
        self.out = np.full(n * 16, 0x5A, dtype=np.uint8)
        self.weights = np.full(n, 0x5A5A5A5A, dtype=np.int32)
        self.raw = np.full(n, 0x5A5A5A5A5A5A5A5A, dtype=np.int64)
        self.counts = np.full(N_ROWS * len(ALPHA), 0x5A5A5A5A, dtype=np.int32)
        self.covered = np.full(N_ROWS, 0x5A5A5A5A, dtype=np.int32)

    def untouched(self):
        return bool((self.out == 0x5A).all() and (self.weights == 0x5A5A5A5A).all() and (self.raw == 0x5A5A5A5A5A5A5A5A).all() and
                    (self.counts == 0x5A5A5A5A).all() and (self.covered == 0x5A5A5A5A).all())

    def call(self, hit_array_, n_array, **kw):
        ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        a = dict(q=self.qp.c, prof=self.prof.c if self.prof else None, cons=self.qp.c, templ=self.tp.c, sub=self.sub, g=self.g,
                 hits=hit_array_.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits=n_array.ctypes.data_as(ip), w_max=1000,
                 out=self.out.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)), weights=self.weights.ctypes.data_as(ip),
                 raw=self.raw.ctypes.data_as(lp), counts=self.counts.ctypes.data_as(ip), covered=self.covered.ctypes.data_as(ip),
                 K=self.K, q_begin=0, q_end=self.rows)
        a.update(kw)
        ref = lambda x: None if x is None else C.byref(x)
        tail = (a["q_begin"], a["q_end"], a["K"], a["hits"], a["n_hits"], a["w_max"], a["out"], a["weights"], a["raw"], a["counts"],
                a["covered"])
        if self.prof is not None:
            return aln_amd.lib().aln_hits_weights_profiles(gpu_util.ctx().h, ref(a["prof"]), ref(a["cons"]), ref(a["templ"]), ref(a["g"]),
                                                           *tail)
        return aln_amd.lib().aln_hits_weights(gpu_util.ctx().h, ref(a["q"]), ref(a["templ"]), ref(a["sub"]), ref(a["g"]), *tail)


def weight_and_slot_checks(raw, hits, n_hits, refused, bad_t, dotted):
    """the checks behind the scoring call's, the same for both entries: weights and w_max, then n_hits, t, the local end cell,
    and last the alphabet (dotted: keyword arguments that put a '.' into the call's alphabet)"""
    E = aln_amd.E_ARG
    K = raw.K
    Q = [len(q) + 2 for q in ARG_QS]
    refused(E, "NULL weights", weights=None)
    for w in (0, -1, 65536):
        refused(E, ("w_max", w), w_max=w)
    refused(aln_amd.E_RESIDUE, "the residues come before weights and w_max", weights=None, w_max=0, templ=bad_t)
    bad_n = n_hits.copy()
    bad_n[0] = K + 1
    refused(E, "n_hits and the alphabet", n_arr=bad_n, **dotted)
    for field, r, k, value in (("n", 0, 0, -1), ("n", 1, 0, K + 1), ("t", 0, 1, -1), ("t", 1, 0, len(ARG_TS)),
                               ("q_end", 0, 0, 0), ("q_end", 1, 1, Q[1] - 1), ("t_end", 0, 1, 0),
                               ("t_end", 1, 0, len(ARG_TS[hits["t"][1, 0]]) + 1)):
        h, n = hits.copy(), n_hits.copy()
        if field == "n":
            n[r] = value
        else:
            h[field][r, k] = value
        refused(E, (field, r, k, value), h_arr=h, n_arr=n)
    refused(E, "an alphabet with '.'", **dotted)
    refused(0, "empty block", q_begin=1, q_end=1)
    for w in (1, 65535):
        raw.fill()
        assert raw.call(hits, n_hits, w_max=w) == 0 and raw.weights.reshape(raw.rows, K).max(axis=1).tolist() == [w] * raw.rows
    for kw, kept in ((dict(raw=None), "raw"), (dict(counts=None), "counts"), (dict(covered=None), "covered"),
                     (dict(counts=None, covered=None, raw=None), "raw")):
        raw.fill()
        assert raw.call(hits, n_hits, **kw) == 0 and not (raw.weights == 0x5A5A5A5A).any()
        assert (getattr(raw, kept) == getattr(Raw(K), kept)).all(), kw   # the sentinel stands where NULL was passed
    raw.fill()


def test_argument_checks_leave_the_outputs_untouched():
    ctx = gpu_util.ctx()
    E = aln_amd.E_ARG
    K = 2
    hits, n_hits = aln_amd.search_topk(ctx, ARG_QS, ARG_TS, ALPHA, cc.TABLE, GI, GE, K)
    assert (n_hits == K).all()
    raw = Raw(K)
    assert raw.call(hits, n_hits) == 0 and not raw.untouched()
    for x in (raw.weights, raw.raw, raw.counts, raw.covered):
        assert not (x.view(np.uint8) == 0x5A).all()
    assert not (raw.weights == 0x5A5A5A5A).any() and not (raw.counts == 0x5A5A5A5A).any()
    raw.fill()

    def refused(want, what, **kw):
        assert raw.call(kw.pop("h_arr", hits), kw.pop("n_arr", n_hits), **kw) == want, what
        assert raw.untouched(), what

    bad_t = aln_amd.SeqPool(["HEAGAWGHEE", "PAW?EAE", "AWHE"]).c
    # 1. NULL hits / n_hits / out, K — before everything that follows
    for kw in (dict(hits=None), dict(n_hits=None), dict(out=None)):
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
    refused(E, "gap model", g=cc.gap(model=aln_amd.GAP_AFFINE_TPOS_MIN))
    refused(E, "align type", g=cc.gap(align_type=5))
    refused(aln_amd.E_RESIDUE, "a template letter outside the alphabet", templ=bad_t)
    refused(aln_amd.E_RESIDUE, "the residues come before n_hits", templ=bad_t, n_arr=np.array([3, 0], np.int32))
    # 3. weights, w_max; 4. n_hits, t, the end cell; 5. the alphabet: an unused letter of the table renamed '.'
    spare = [ch for ch in ALPHA if all(ch not in s for s in ARG_QS + ARG_TS)][0]
    dot_sub = aln_amd.AlnSubmatrix(len(ALPHA), ALPHA.replace(spare, ".").encode(), raw.tab.ctypes.data_as(C.POINTER(C.c_float)))
    weight_and_slot_checks(raw, hits, n_hits, refused, bad_t, dict(sub=dot_sub))
    dash_sub = aln_amd.AlnSubmatrix(len(ALPHA), ALPHA.replace(spare, "-").encode(), raw.tab.ctypes.data_as(C.POINTER(C.c_float)))
    refused(E, "an alphabet with '-'", sub=dash_sub)


def test_argument_checks_of_the_profile_entry():
    ctx = gpu_util.ctx()
    E = aln_amd.E_ARG
    K = 2
    profiles = pc.derived(ARG_QS, cc.TABLE)
    hits, n_hits = aln_amd.search_topk(ctx, ARG_QS, ARG_TS, ALPHA, cc.TABLE, GI, GE, K)
    raw = Raw(K, profiles=profiles)
    plain = Raw(K)
    assert raw.call(hits, n_hits) == 0 and plain.call(hits, n_hits) == 0
    for x, y in ((raw.out, plain.out), (raw.weights, plain.weights), (raw.raw, plain.raw), (raw.counts, plain.counts),
                 (raw.covered, plain.covered)):
        assert x.tobytes() == y.tobytes()
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
    for kw in (dict(prof=None), dict(templ=None), dict(g=None), dict(hits=None), dict(n_hits=None), dict(out=None)):
        refused(E, kw, **kw)
    for k in (0, 1025):
        refused(E, ("K", k), K=k)
    refused(E, "K before the descriptor", K=0, prof=qprof(n=31), templ=bad_t)
    refused(E, "q_end > n", q_end=3)
    refused(E, "gap model", g=cc.gap(model=aln_amd.GAP_AFFINE_TPOS_MIN))
    for kw in (dict(n=0), dict(n=31), dict(alphabet=None), dict(rows=None)):
        refused(E, kw, prof=qprof(**kw))
    refused(E, "consensus n_seqs", cons=wrong_n)
    refused(E, "the consensus comes before the residues", cons=wrong_n, templ=bad_t)
    refused(aln_amd.E_RESIDUE, "a template letter outside the alphabet", templ=bad_t)
    spare = [ch for ch in ALPHA if all(ch not in s for s in ARG_QS + ARG_TS)][0]
    weight_and_slot_checks(raw, hits, n_hits, refused, bad_t, dict(prof=qprof(alphabet=ALPHA.replace(spare, ".").encode())))
    refused(E, "an alphabet with '-'", prof=qprof(alphabet=ALPHA.replace(spare, "-").encode()))
    raw.fill()
    assert raw.call(hits, n_hits, cons=None) == 0 and raw.weights.tobytes() == plain.weights.tobytes()
    assert raw.raw.tobytes() == plain.raw.tobytes() and raw.counts.tobytes() == plain.counts.tobytes()


# ---- 7. two rounds ------------------------------------------------------------------------------------------------------------------------
def test_two_rounds_search_weights_profile_search():
    qs, ts = cc.homolog_set()
    assert len(qs) == 8 and len(ts) == 10
    ctx = gpu_util.ctx()
    K = 4
    mode = rc.LOCAL
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, ALPHA, cc.TABLE, GI, GE, K)                       # 1. search
    assert (n_hits == K).all()
    rec, weights, raw, counts, covered, rcode = aln_amd.hits_weights(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, w_max=100)   # 2.
    assert rcode == 0
    lists = [cc.pair_list(qs[r], ts[hits["t"][r, k]], mode) for r, k in used_slots(n_hits, K)]
    ref = wc.reference([len(q) for q in qs], ts, hits["t"], n_hits, lists, True, 100)
    check((rec, weights, raw, counts, covered, rcode), ref, n_hits, lists, "two rounds")
    assert (weights.max(axis=1) == 100).all() and any(len(set(w.tolist())) > 1 for w in weights)
    background = np.full(len(ALPHA), 1.0 / len(ALPHA))
    fallback = pc.derived(qs, cc.TABLE)
    rows = [aln_amd.pssm_from_counts(counts[r][1:-1], background, fallback[r]) for r in range(len(qs))]   # 3. the profile
    assert all(np.array_equal(p, np.rint(p)) for p in rows) and any((c[1:-1].sum(axis=1) > 0).all() for c in counts)
    profiles = [p.astype(np.int64) for p in rows]
    assert any(not np.array_equal(p, f) for p, f in zip(profiles, fallback))
    qp = pool(profiles)
    hits2, n2 = aln_amd.search_topk_profiles(ctx, qp, ts, GI, GE, K)                                     # 4. profile search
    scores, ends = pc.dense_reference("weights_two_rounds", profiles, ts, mode, GI, GE)
    for r in range(len(qs)):
        order = sc.topk_reference(scores[r], K)
        assert n2[r] == len(order) and hits2["t"][r, :len(order)].tolist() == order, (r, hits2[r].tolist(), order)
        assert np.array_equal(hits2["score"][r, :len(order)].view(U32), scores[r, order].astype(np.float32).view(U32)), r
        assert np.array_equal(hits2["q_end"][r, :len(order)], ends[r, order, 0]), r
        assert np.array_equal(hits2["t_end"][r, :len(order)], ends[r, order, 1]), r
    # and the loop closes: the second round's hits can be weighted again, from the profile side
    again = aln_amd.hits_weights_profiles(ctx, qp, ts, hits2, n2, GI, GE, consensus=qs)
    assert again[5] == 0 and (again[1].max(axis=1) == 1000).all() and sum(int(c.sum()) for c in again[3]) > 0
