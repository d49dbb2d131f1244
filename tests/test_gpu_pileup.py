"""-m gpu: aln_hits_pileup / aln_hits_pileup_profiles — the query-anchored rows of search hits laid out on the device
(hit_local_kernel, hit_global_kernel under PileupJob, csrc/search_pileup.hip).  Everything is an integer or a byte and every
comparison is equality: letters, tpos and spans against the numpy restatement over the oracle's pair lists (pileup_cases), the
records byte for byte against aln_hits_align called without lists and lines.

  1  every fused length class and the batch route in one row, a duplicated slot, chunks, align_fused_nonlocal = 0, list groups
  2  the outputs singly, line_stride at the longest query and beyond
  3  the pileup rebuilt from hits_align's lists; counts_from_pileup against hits_column_counts
  4  a row block with q_begin > 0
  5  a falsified local score, local pairs whose best score is 0, pairs without an interior
  6  the argument checks, in their order
  7  the profile entry: derived rows, position-specific rows at the staging boundaries, fractional rows, the consensus
  8  the homolog set as a3m rows"""
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

pytestmark = pytest.mark.gpu

U32 = np.uint32
ALPHA = cc.ALPHA
_, GI, GE = cc.SYSTEM
K5 = 5
used_slots = pu.used_slots


hit_array = cc.hit_array


def spans_array(spans):
    return np.stack([spans[f] for f in ("q_lo", "q_hi", "t_lo", "t_hi")], axis=-1)


def check_pileup(res, q_lens, ts, t_idx, n_hits, lists, local, what):
    """all five results against the reference over `lists`; unused slots are zero everywhere"""
    rec, spans, letters, tpos, rcode = res
    K = t_idx.shape[1]
    slots = used_slots(n_hits, K)
    stride = letters.shape[2]
    assert letters.dtype == np.uint8 and tpos.dtype == np.uint16 and tpos.shape == letters.shape == (len(n_hits), K, stride)
    wl, wt, ws = pu.pileup(q_lens, ts, [(r, int(t_idx[r, k])) for r, k in slots], lists, local, stride)
    sp = spans_array(spans)
    for s, (r, k) in enumerate(slots):
        print(what, "slot", r, k, "letters that differ:", int((letters[r, k] != wl[s]).sum()), "span", sp[r, k].tolist())
        assert np.array_equal(letters[r, k], wl[s]), (what, r, k, letters[r, k].tobytes(), wl[s].tobytes())
        assert np.array_equal(tpos[r, k], wt[s]), (what, r, k)
        assert np.array_equal(sp[r, k], ws[s]), (what, r, k, sp[r, k].tolist(), ws[s].tolist())
        score, pl = lists[s]
        assert rec["status"][r, k] == 0 and rec["n_pairs"][r, k] == len(pl), (what, r, k, rec[r, k])
        assert np.float32(rec["score"][r, k]).view(U32) == np.float32(score).view(U32), (what, r, k)
    for r in range(len(n_hits)):
        n = n_hits[r]
        assert not letters[r, n:].any() and not tpos[r, n:].any() and not sp[r, n:].any() and rec[r, n:].tobytes() == bytes(16 * (K - n))
    return wl, wt, ws


def same_pileup(a, b):
    assert a[4] == b[4]
    for x, y in zip(a[:4], b[:4]):
        assert (x is None) == (y is None) and (x is None or (x.shape == y.shape and x.tobytes() == y.tobytes()))


def class_inputs(mode):
    qs, ts = cc.class_set()
    t_idx, n_hits = cc.class_hits(K5)
    lists = [cc.pair_list(qs[r], ts[t_idx[r, k]], mode) for r, k in used_slots(n_hits, K5)]
    return qs, ts, t_idx, n_hits, lists, hit_array(t_idx, n_hits, lists, mode == rc.LOCAL)


# ---- 1. classes, routes, duplicates, chunks ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_every_class_and_both_routes(mode):
    pu.check_sets((mode,))
    local = mode == rc.LOCAL
    qs, ts, t_idx, n_hits, lists, hits = class_inputs(mode)
    q_lens = [len(q) for q in qs]
    ctx = gpu_util.ctx()
    call = lambda **kw: aln_amd.hits_pileup(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, align_type=mode, **kw)
    whole = call()
    fused, batched = aln_amd.hits_align_routes(ctx)
    n_used = int(n_hits.sum())
    cls = [cc.class_of(ts[t_idx[r, k]]) for r, k in used_slots(n_hits, K5)]
    want_batched = sum(c > 8 or (local and c == 8) for c in cls)
    assert (fused, batched) == (n_used - want_batched, want_batched) and want_batched >= 2 and fused >= 18
    assert sorted(set(c for c in cls if c <= (7 if local else 8))) == list(range(1, 8 if local else 9))
    assert whole[2].shape[2] == max(q_lens) and whole[4] == 0
    wl, wt, ws = check_pileup(whole, q_lens, ts, t_idx, n_hits, lists, local, ("class", mode))
    assert (wl == pu.DASH).any() and (wl == pu.DOT).any() and (wt > 0).any()
    # the records are aln_hits_align's, byte for byte
    rec = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, align_type=mode, want_pairs=False, want_lines=False)[0]
    assert whole[0].tobytes() == rec.tobytes()
    # the duplicated slot (slot 3 repeats slot 0) has the same rows
    for r in range(len(n_hits)):
        for x in whole[:4]:
            assert x[r, 3].tobytes() == x[r, 0].tobytes(), r
    # chunks of 1 and 3 hits; every slot through batches
    for chunk in (1, 3):
        with ctx.hints(align_chunk_hits=chunk):
            same_pileup(call(), whole)
            assert aln_amd.hits_align_routes(ctx) == (fused, batched)
    # the batch route's slots in groups (align_list_group_slots): local, its two or more slots one per group
    if local:
        with ctx.hints(align_list_group_slots=1):
            same_pileup(call(), whole)
            assert aln_amd.hits_align_routes(ctx) == (fused, batched)
    if not local:
        with ctx.hints(align_fused_nonlocal=0):
            same_pileup(call(), whole)
            assert aln_amd.hits_align_routes(ctx) == (0, n_used)
        group = 3 if n_used % 3 else 4
        assert n_used > group and 0 < n_used % group                   # several groups, the last one shorter
        with ctx.hints(align_fused_nonlocal=0, align_list_group_slots=group):
            same_pileup(call(), whole)
            assert aln_amd.hits_align_routes(ctx) == (0, n_used)


# ---- 2. the outputs singly, the stride -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (rc.LOCAL, rc.GLOBAL_LOCAL))
def test_outputs_singly_and_the_stride(mode):
    qs, ts, t_idx, n_hits, lists, hits = class_inputs(mode)
    ctx = gpu_util.ctx()
    call = lambda **kw: aln_amd.hits_pileup(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, align_type=mode, **kw)
    whole = call()
    no = dict(want_letters=False, want_tpos=False, want_spans=False)
    for keep, at in (("want_letters", 2), ("want_tpos", 3), ("want_spans", 1), (None, None)):
        kw = dict(no)
        if keep:
            kw[keep] = True
        got = call(**kw)
        want = [whole[0], None, None, None, whole[4]]
        if keep:
            want[at] = whole[at]
        same_pileup(got, want)
    longest = max(len(q) for q in qs)                                  # = the longest Q - 2
    same_pileup(call(line_stride=longest), whole)
    wide = call(line_stride=longest + 7)
    assert wide[2].shape[2] == longest + 7 and not wide[2][:, :, longest:].any() and not wide[3][:, :, longest:].any()
    same_pileup((wide[0], wide[1], np.ascontiguousarray(wide[2][:, :, :longest]), np.ascontiguousarray(wide[3][:, :, :longest]), wide[4]),
                whole)
    for r, q in enumerate(qs):                                         # NUL / 0 behind every query's own Q - 2
        assert not wide[2][r, :, len(q):].any() and not wide[3][r, :, len(q):].any()
        assert (wide[2][r, :n_hits[r], :len(q)] != 0).all()


# ---- 3. cross-checks that need no reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_the_pileup_of_hits_aligns_lists_and_the_column_counts(mode):
    local = mode == rc.LOCAL
    qs, ts, t_idx, n_hits, lists, hits = class_inputs(mode)
    q_lens = [len(q) for q in qs]
    ctx = gpu_util.ctx()
    whole = aln_amd.hits_pileup(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, align_type=mode)
    res = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, align_type=mode, want_lines=False)
    slots = used_slots(n_hits, K5)
    got_lists = [(res[0]["score"][r, k], res[1][r][k]) for r, k in slots]
    wl, wt, ws = pu.pileup(q_lens, ts, [(r, int(t_idx[r, k])) for r, k in slots], got_lists, local, max(q_lens))
    rebuilt = [np.zeros_like(whole[2]), np.zeros_like(whole[3]), np.zeros(whole[1].shape + (4,), np.int32)]
    for s, (r, k) in enumerate(slots):
        rebuilt[0][r, k], rebuilt[1][r, k], rebuilt[2][r, k] = wl[s], wt[s], ws[s]
    assert whole[2].tobytes() == rebuilt[0].tobytes() and whole[3].tobytes() == rebuilt[1].tobytes()
    assert spans_array(whole[1]).tobytes() == rebuilt[2].tobytes() and whole[0].tobytes() == res[0].tobytes()
    crec, counts, covered, crc = aln_amd.hits_column_counts(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, align_type=mode)
    off = np.concatenate(([0], np.cumsum([n + 2 for n in q_lens])))
    for r, L in enumerate(q_lens):
        c, cov = aln_amd.counts_from_pileup(whole[2][r], ALPHA)
        assert np.array_equal(c[:L], counts[r][1:-1]) and not c[L:].any(), (mode, r)
        assert np.array_equal(cov[:L], covered[off[r] + 1:off[r + 1] - 1]) and not cov[L:].any(), (mode, r)
    assert crec.tobytes() == whole[0].tobytes() and sum(int(c.sum()) for c in counts) > 0


# ---- 4. row blocks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (rc.LOCAL, rc.GLOBAL))
def test_a_row_block_with_q_begin(mode):
    qs, ts, t_idx, n_hits, lists, hits = class_inputs(mode)
    ctx = gpu_util.ctx()
    whole = aln_amd.hits_pileup(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, align_type=mode)
    stride = whole[2].shape[2]
    for a, b in ((2, 5), (cc.LONG_ROW, cc.LONG_ROW + 1), (5, 6)):
        for chunk in (0, 2):
            with ctx.hints(align_chunk_hits=chunk):
                part = aln_amd.hits_pileup(ctx, qs, ts, hits[a:b], n_hits[a:b], ALPHA, cc.TABLE, GI, GE, q_begin=a, align_type=mode,
                                           line_stride=stride)
            same_pileup(part, tuple(np.ascontiguousarray(x[a:b]) for x in whole[:4]) + (whole[4],))
        own = aln_amd.hits_pileup(ctx, qs, ts, hits[a:b], n_hits[a:b], ALPHA, cc.TABLE, GI, GE, q_begin=a, align_type=mode)
        w = max(len(q) for q in qs[a:b])                               # the default stride is the block's own longest query
        assert own[2].shape[2] == w and own[2].tobytes() == np.ascontiguousarray(whole[2][a:b, :, :w]).tobytes()
    empty = aln_amd.hits_pileup(ctx, qs, ts, hits[4:4], n_hits[4:4], ALPHA, cc.TABLE, GI, GE, q_begin=4, align_type=mode)
    assert empty[0].shape == (0, K5) and empty[2].shape[:2] == (0, K5) and empty[4] == 0


# ---- 5. special slots ------------------------------------------------------------------------------------------------------------------
def test_a_falsified_local_score_is_refused_and_shows_nothing():
    mode = rc.LOCAL
    qs, ts, t_idx, n_hits, lists, hits = class_inputs(mode)
    ctx = gpu_util.ctx()
    whole = aln_amd.hits_pileup(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE)
    bad = hits.copy()
    br, bk = 1, 1                                                      # row 1 (65 residues), template 7: a fused slot
    assert cc.class_of(ts[t_idx[br, bk]]) <= 7 and lists[used_slots(n_hits, K5).index((br, bk))][0] > 0
    bad["score"][br, bk] += 1.0
    got = aln_amd.hits_pileup(ctx, qs, ts, bad, n_hits, ALPHA, cc.TABLE, GI, GE)
    assert got[4] == aln_amd.E_ARG
    want_status = np.zeros_like(whole[0]["status"])
    want_status[br, bk] = aln_amd.E_ARG
    assert np.array_equal(got[0]["status"], want_status) and got[0]["n_pairs"][br, bk] == 0
    rec = aln_amd.hits_align(ctx, qs, ts, bad, n_hits, ALPHA, cc.TABLE, GI, GE, want_pairs=False, want_lines=False)[0]
    assert got[0].tobytes() == rec.tobytes()
    L = len(qs[br])
    assert got[2][br, bk].tobytes() == b"." * L + bytes(got[2].shape[2] - L) and not got[3][br, bk].any()
    assert not spans_array(got[1])[br, bk].any() and spans_array(whole[1])[br, bk].any()
    keep = np.ones(whole[0].shape, bool)
    keep[br, bk] = False
    for x, y in zip(got[1:4], whole[1:4]):                            # the others unchanged
        assert x[keep].tobytes() == y[keep].tobytes()


def test_local_pairs_whose_best_score_is_zero_show_nothing():
    c = sc.CASES["all_negative"]
    qs, ts = sc.sequences(c)
    table = sc.TABLES[c.table]
    ctx = gpu_util.ctx()
    K = 4
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, ALPHA, table, c.gi, c.ge, K)
    assert (n_hits == K).all() and (hits["score"] == 0).all()
    got = aln_amd.hits_pileup(ctx, qs, ts, hits, n_hits, ALPHA, table, c.gi, c.ge)
    fused, batched = aln_amd.hits_align_routes(ctx)
    assert fused > 0 and batched > 0 and got[4] == 0                  # the empty query and templates go through batches
    rec = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, ALPHA, table, c.gi, c.ge, want_pairs=False, want_lines=False)[0]
    assert got[0].tobytes() == rec.tobytes() and (rec["n_pairs"] > 0).any()
    assert not got[3].any() and not spans_array(got[1]).any()
    for r, q in enumerate(qs):
        assert (got[2][r, :, :len(q)] == pu.DOT).all() and not got[2][r, :, len(q):].any()
    # the same slots under GLOBAL are alignments and do show
    glob = aln_amd.hits_pileup(ctx, qs, ts, hits, n_hits, ALPHA, table, c.gi, c.ge, align_type=rc.GLOBAL)
    assert glob[3].any() and spans_array(glob[1]).any()


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
    got = aln_amd.hits_pileup(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, align_type=mode)
    assert aln_amd.hits_align_routes(ctx) == (4, 8)
    check_pileup(got, [len(q) for q in qs], ts, t_idx, n_hits, lists, local, ("no interior", mode))
    assert not got[2][0].any() and not got[3][0].any() and got[3][2].any()
    rec = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, align_type=mode, want_pairs=False, want_lines=False)[0]
    assert got[0].tobytes() == rec.tobytes()
    # a block of queries without an interior only: the stride's floor is 1, and nothing but the records is written
    lone = aln_amd.hits_pileup(ctx, qs, ts, hits[:1], n_hits[:1], ALPHA, cc.TABLE, GI, GE, align_type=mode)
    assert lone[2].shape == (1, 4, 1) and not lone[2].any() and lone[0].tobytes() == got[0][:1].tobytes()


# ---- 6. arguments ----------------------------------------------------------------------------------------------------------------------
ARG_QS = ["PAWHEAE", "HEAGAWGHEE"]
ARG_TS = ["HEAGAWGHEE", "PAWHEAE", "AWHE"]
ARG_STRIDE = 12


class Raw:
    """both entries through ctypes with sentinel-filled outputs"""

    def __init__(self, K, profiles=None):
        self.qp = aln_amd.SeqPool(ARG_QS)
        self.tp = aln_amd.SeqPool(ARG_TS)
        self.prof = aln_amd.QueryProfiles([np.asarray(p, np.float32) for p in profiles], ALPHA) if profiles is not None else None
        self.tab = np.ascontiguousarray(cc.TABLE, np.float32)
        self.sub = aln_amd.AlnSubmatrix(len(ALPHA), ALPHA.encode(), self.tab.ctypes.data_as(C.POINTER(C.c_float)))
        self.g = gap()
        self.rows, self.K = len(ARG_QS), K
        self.fill()

    def fill(self):
        n = self.rows * self.K
        self.out = np.full(n * 16, 0x5A, dtype=np.uint8)
        self.spans = np.full(n * 16, 0x5A, dtype=np.uint8)
        self.letters = np.full(n * ARG_STRIDE, 0x5A, dtype=np.uint8)
        self.tpos = np.full(n * ARG_STRIDE, 0x5A5A, dtype=np.uint16)

    def untouched(self):
        return bool((self.out == 0x5A).all() and (self.spans == 0x5A).all() and (self.letters == 0x5A).all() and
                    (self.tpos == 0x5A5A).all())

    def call(self, hit_array_, n_array, **kw):
        ip = C.POINTER(C.c_int32)
        a = dict(q=self.qp.c, prof=self.prof.c if self.prof else None, cons=self.qp.c, templ=self.tp.c, sub=self.sub, g=self.g,
                 hits=hit_array_.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits=n_array.ctypes.data_as(ip),
                 out=self.out.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)),
                 spans=self.spans.ctypes.data_as(C.POINTER(aln_amd.AlnHitSpan)),
                 letters=self.letters.ctypes.data_as(C.POINTER(C.c_uint8)), tpos=self.tpos.ctypes.data_as(C.POINTER(C.c_uint16)),
                 stride=ARG_STRIDE, K=self.K, q_begin=0, q_end=self.rows)
        a.update(kw)
        ref = lambda x: None if x is None else C.byref(x)
        tail = (a["q_begin"], a["q_end"], a["K"], a["hits"], a["n_hits"], a["out"], a["spans"], a["letters"], a["tpos"], a["stride"])
        if self.prof is not None:
            return aln_amd.lib().aln_hits_pileup_profiles(gpu_util.ctx().h, ref(a["prof"]), ref(a["cons"]), ref(a["templ"]), ref(a["g"]),
                                                          *tail)
        return aln_amd.lib().aln_hits_pileup(gpu_util.ctx().h, ref(a["q"]), ref(a["templ"]), ref(a["sub"]), ref(a["g"]), *tail)


gap = cc.gap


def stride_and_slot_checks(raw, hits, n_hits, refused, bad_t):
    """checks 3 and 4, the same for both entries: the stride against the longest query, then n_hits, t, the local end cell"""
    E = aln_amd.E_ARG
    K = raw.K
    Q = [len(q) + 2 for q in ARG_QS]
    longest = max(Q) - 2
    refused(E, "a stride one below the longest query", stride=longest - 1)
    refused(E, "... for tpos alone", stride=longest - 1, letters=None)
    refused(E, "... for letters alone", stride=longest - 1, tpos=None)
    refused(aln_amd.E_RESIDUE, "the residues come before the stride", stride=longest - 1, templ=bad_t)
    raw.fill()
    assert raw.call(hits, n_hits, stride=longest) == 0 and not raw.untouched()
    raw.fill()
    assert raw.call(hits, n_hits, stride=longest - 1, q_begin=0, q_end=1) == 0      # the block's queries only: 7 <= 9
    raw.fill()
    assert raw.call(hits, n_hits, stride=0, letters=None, tpos=None) == 0           # not read when neither is given
    assert (raw.letters == 0x5A).all() and (raw.tpos == 0x5A5A).all() and not (raw.spans == 0x5A).all()
    raw.fill()
    for field, r, k, value in (("n", 0, 0, -1), ("n", 1, 0, K + 1), ("t", 0, 1, -1), ("t", 1, 0, len(ARG_TS)),
                               ("q_end", 0, 0, 0), ("q_end", 1, 1, Q[1] - 1), ("t_end", 0, 1, 0),
                               ("t_end", 1, 0, len(ARG_TS[hits["t"][1, 0]]) + 1)):
        h, n = hits.copy(), n_hits.copy()
        if field == "n":
            n[r] = value
        else:
            h[field][r, k] = value
        refused(E, (field, r, k, value), h_arr=h, n_arr=n)
    refused(0, "empty block", q_begin=1, q_end=1)


def test_argument_checks_leave_the_outputs_untouched():
    ctx = gpu_util.ctx()
    E = aln_amd.E_ARG
    K = 2
    hits, n_hits = aln_amd.search_topk(ctx, ARG_QS, ARG_TS, ALPHA, cc.TABLE, GI, GE, K)
    assert (n_hits == K).all()
    raw = Raw(K)
    assert raw.call(hits, n_hits) == 0 and not raw.untouched()
    assert not (raw.letters == 0x5A).any() and not (raw.tpos == 0x5A5A).any() and not (raw.spans == 0x5A).all()
    raw.fill()

    def refused(want, what, **kw):
        assert raw.call(kw.pop("h_arr", hits), kw.pop("n_arr", n_hits), **kw) == want, what
        assert raw.untouched(), what

    bad_t = aln_amd.SeqPool(["HEAGAWGHEE", "PAW?EAE", "AWHE"]).c
    # 1. NULL hits / n_hits / out, K, line_stride < 1 with a line output — before everything that follows
    for kw in (dict(hits=None), dict(n_hits=None), dict(out=None)):
        refused(E, kw, **kw)
    for k in (0, 1025, -1):
        refused(E, ("K", k), K=k)
    for kw in (dict(stride=0), dict(stride=-4, tpos=None), dict(stride=0, letters=None)):
        refused(E, kw, **kw)
    refused(E, "K before the residues", K=0, templ=bad_t)
    refused(E, "the stride's sign before the residues", stride=0, templ=bad_t)
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
    # 3. the stride; 4. n_hits, t, the end cell
    stride_and_slot_checks(raw, hits, n_hits, refused, bad_t)
    # spans may be NULL
    raw.fill()
    assert raw.call(hits, n_hits, spans=None) == 0 and (raw.spans == 0x5A).all() and not (raw.letters == 0x5A).any()


def test_argument_checks_of_the_profile_entry():
    ctx = gpu_util.ctx()
    E = aln_amd.E_ARG
    K = 2
    profiles = pc.derived(ARG_QS, cc.TABLE)
    hits, n_hits = aln_amd.search_topk(ctx, ARG_QS, ARG_TS, ALPHA, cc.TABLE, GI, GE, K)
    raw = Raw(K, profiles=profiles)
    plain = Raw(K)
    assert raw.call(hits, n_hits) == 0 and plain.call(hits, n_hits) == 0
    for x, y in ((raw.out, plain.out), (raw.spans, plain.spans), (raw.letters, plain.letters), (raw.tpos, plain.tpos)):
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
    refused(E, "stride < 1", stride=0)
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
    stride_and_slot_checks(raw, hits, n_hits, refused, bad_t)
    raw.fill()
    assert raw.call(hits, n_hits, cons=None) == 0 and raw.letters.tobytes() == plain.letters.tobytes()
    assert raw.tpos.tobytes() == plain.tpos.tobytes() and raw.spans.tobytes() == plain.spans.tobytes()


# ---- 7. the profile entry ----------------------------------------------------------------------------------------------------------------
def pool(profiles):
    return aln_amd.QueryProfiles([np.asarray(p, np.float32) for p in profiles], ALPHA)


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_derived_profiles_equal_the_residue_entry(mode):
    local = mode == rc.LOCAL
    qs, ts, t_idx, n_hits, lists, hits = class_inputs(mode)
    ctx = gpu_util.ctx()
    qp = aln_amd.profiles_from_sequences(qs, ALPHA, cc.TABLE)
    want = aln_amd.hits_pileup(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, align_type=mode)
    routes_want = aln_amd.hits_align_routes(ctx)
    got = aln_amd.hits_pileup_profiles(ctx, qp, ts, hits, n_hits, GI, GE, consensus=qs, align_type=mode)
    routes_got = aln_amd.hits_align_routes(ctx)
    same_pileup(got, want)
    # the profile side keeps class 8 of the local kernel, the residue side does not: two routes, one result
    assert sum(routes_got) == sum(routes_want) == int(n_hits.sum())
    assert routes_got[0] == routes_want[0] + (sum(cc.class_of(ts[t_idx[r, k]]) == 8 for r, k in used_slots(n_hits, K5)) if local else 0)
    rec = aln_amd.hits_align_profiles(ctx, qp, ts, hits, n_hits, GI, GE, consensus=qs, align_type=mode, want_pairs=False,
                                      want_lines=False)[0]
    assert got[0].tobytes() == rec.tobytes()
    for chunk, per_chunk in ((1, 0), (3, 1)):
        with ctx.hints(align_chunk_hits=chunk, align_rows_per_chunk=per_chunk):
            same_pileup(aln_amd.hits_pileup_profiles(ctx, qp, ts, hits, n_hits, GI, GE, consensus=qs, align_type=mode), got)
    # a given consensus and a NULL one differ only in the records' identity
    bare = aln_amd.hits_pileup_profiles(ctx, qp, ts, hits, n_hits, GI, GE, align_type=mode)
    for x, y in zip(bare[1:4], got[1:4]):
        assert x.tobytes() == y.tobytes()
    for f in ("n_pairs", "status", "score"):
        assert np.array_equal(bare[0][f], got[0][f])
    assert not np.array_equal(bare[0]["identity"], got[0]["identity"])


STAGING_ROWS = (1, 7, 8, 9, 64, 65, 130)                               # interior rows at every boundary of the staging ring


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
    hits[3, 2] = hits[3, 0]                                            # a duplicate
    slots = used_slots(n_hits, K)
    lists = [pu.profile_list(profiles[r], ts[hits["t"][r, k]], mode, gi, ge) for r, k in slots]
    got = aln_amd.hits_pileup_profiles(ctx, qp, ts, hits, n_hits, gi, ge, align_type=mode)
    fused, batched = aln_amd.hits_align_routes(ctx)
    assert fused > 0 and fused + batched == len(slots) and got[4] == 0
    wl, wt, ws = check_pileup(got, [len(p) for p in profiles], ts, hits["t"], n_hits, lists, local, ("rows", mode))
    assert (wt > 0).any()
    rec = aln_amd.hits_align_profiles(ctx, qp, ts, hits, n_hits, gi, ge, align_type=mode, want_pairs=False, want_lines=False)[0]
    assert got[0].tobytes() == rec.tobytes()


@pytest.mark.parametrize("mode", (rc.LOCAL, rc.SEMI_LOCAL))
def test_fractional_rows_go_through_batches(mode):
    profiles, ts = pc.mixed_set()
    half = [np.asarray(p, np.float32) * np.float32(0.5) for p in profiles]
    assert any((h != np.round(h)).any() for h in half)
    ctx = gpu_util.ctx()
    hp = aln_amd.QueryProfiles(half, ALPHA)
    K = 3
    hits, n_hits = aln_amd.search_topk_profiles(ctx, hp, ts, 11, 1, K, align_type=mode)
    got = aln_amd.hits_pileup_profiles(ctx, hp, ts, hits, n_hits, 11, 1, align_type=mode)
    assert aln_amd.hits_align_routes(ctx) == (0, int(n_hits.sum()))
    res = aln_amd.hits_align_profiles(ctx, hp, ts, hits, n_hits, 11, 1, align_type=mode, want_lines=False)
    assert got[0].tobytes() == res[0].tobytes() and (res[0]["status"] == 0).all()
    slots = used_slots(n_hits, K)
    lists = [(res[0]["score"][r, k], res[1][r][k]) for r, k in slots]
    q_lens = [len(p) for p in half]
    wl, wt, ws = pu.pileup(q_lens, ts, [(r, int(hits["t"][r, k])) for r, k in slots], lists, mode == rc.LOCAL, max(q_lens))
    sp = spans_array(got[1])
    for s, (r, k) in enumerate(slots):
        assert np.array_equal(got[2][r, k], wl[s]) and np.array_equal(got[3][r, k], wt[s]) and np.array_equal(sp[r, k], ws[s]), (r, k)
    assert (wt > 0).any()


# ---- 8. a3m rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (rc.LOCAL, rc.SEMI_LOCAL))
def test_the_homolog_set_as_a3m_rows(mode):
    pu.check_sets((mode,))
    local = mode == rc.LOCAL
    qs, ts = cc.homolog_set()
    assert len(qs) == 8 and len(ts) == 10
    K = len(ts)
    t_idx = np.tile(np.arange(K, dtype=np.int32), (len(qs), 1))
    n_hits = np.full(len(qs), K, np.int32)
    lists = [cc.pair_list(qs[r], ts[k], mode) for r, k in used_slots(n_hits, K)]
    hits = hit_array(t_idx, n_hits, lists, local)
    ctx = gpu_util.ctx()
    got = aln_amd.hits_pileup(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, align_type=mode)
    assert aln_amd.hits_align_routes(ctx) == (len(qs) * K, 0) and got[4] == 0
    check_pileup(got, [len(q) for q in qs], ts, t_idx, n_hits, lists, local, ("homolog", mode))
    inserts = 0
    for r, k in used_slots(n_hits, K):
        L = len(qs[r])
        a3m = aln_amd.a3m_from_pileup(ts[k], got[2][r, k, :L], got[3][r, k, :L])
        assert len([c for c in a3m if not c.islower()]) == L, (r, k, a3m)
        sp = got[1][r, k]
        want = ts[k][sp["t_lo"] - 1:sp["t_hi"]] if sp["q_hi"] > 0 else ""
        assert a3m.replace("-", "").upper() == want, (r, k, a3m, want)
        inserts += sum(c.islower() for c in a3m)
    assert inserts > 0
