"""-m gpu: aln_hits_purge / aln_hits_purge_profiles — near-identical search hits purged on the device, and the weights and
weighted counts of the survivors, from letters rows that never come down (csrc/search_purge.hip).  Everything is an integer and
every comparison is equality: purge records, weights, raw, counts and covered against the integer loops of purge_cases over
the oracle's pair lists, the records byte for byte against aln_hits_align called without lists and lines.

  1  the sets under three align types and the four parameter pairs: K = 1 / 5 / 65 / 130 / 1024, n_hits of K, K-1, 64, 33, 1, 0,
     Q-2 of 1 .. 130 in one block, both routes into one stack, a muted row; 101 against hits_weights; the counts against
     hits_column_counts; the compacted hit list against hits_weights; groups, chunks, list groups, align_fused_nonlocal = 0
  2  purge only; raw, counts and covered each NULL in turn
  3  a row block with q_begin > 0, a row without hits
  4  a falsified local score
  5  the profile entry: derived rows, position-specific rows at the staging boundaries
  6  the argument checks, in their order
  7  two rounds: search, purge with counts, profile, profile search"""
import ctypes as C

import numpy as np
import pytest

import aln_amd
import column_count_cases as cc
import gpu_util
import pileup_cases as pu
import profile_cases as pc
import purge_cases as pg
import range_cases as rc
import search_cases as sc

pytestmark = pytest.mark.gpu

U32 = np.uint32
ALPHA = cc.ALPHA
_, GI, GE = cc.SYSTEM
MODES = (rc.LOCAL, rc.GLOBAL, rc.SEMI_LOCAL)
used_slots = pu.used_slots


def same(a, b, what=None):
    """two 7-tuples of hits_purge, byte for byte"""
    assert a[6] == b[6], what
    for x, y in zip((a[0], a[1], a[2], a[3], a[5]), (b[0], b[1], b[2], b[3], b[5])):
        assert (x is None) == (y is None) and (x is None or (x.shape == y.shape and x.tobytes() == y.tobytes())), what
    assert (a[4] is None) == (b[4] is None), what
    if a[4] is not None:
        assert len(a[4]) == len(b[4]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[4], b[4])), what


def records(purge):
    """the purge records as an int32 [rows, K, 4] array"""
    return np.stack([purge[f] for f in ("keeper", "same", "overlap", "letters")], axis=-1)


def check(res, ref, n_hits, lists, what):
    """a result against purge_cases.reference"""
    rec, purge, weights, raw, counts, covered, rcode = res
    assert rcode == 0 and purge.dtype == aln_amd.HIT_PURGE_DTYPE and weights.dtype == np.int32 and raw.dtype == np.int64, what
    K = weights.shape[1]
    print(what, "purge records that differ:", int((records(purge) != ref["purge"]).any(axis=-1).sum()),
          "weights:", int((weights != ref["weights"]).sum()), "raw:", int((raw != ref["raw"]).sum()),
          "count rows:", sum(int((g != w).any(axis=1).sum()) for g, w in zip(counts, ref["counts"])),
          "covered:", int((covered != ref["covered"]).sum()))
    assert np.array_equal(records(purge), ref["purge"]), what
    assert np.array_equal(weights, ref["weights"]) and np.array_equal(raw, ref["raw"]), what
    assert len(counts) == len(ref["counts"]) and all(g.dtype == np.int32 and np.array_equal(g, w) for g, w in zip(counts, ref["counts"])), what
    assert covered.dtype == np.int32 and np.array_equal(covered, ref["covered"]), what
    for (r, k), (score, pl) in zip(used_slots(n_hits, K), lists):
        assert rec["status"][r, k] == 0 and rec["n_pairs"][r, k] == len(pl), (what, r, k, rec[r, k])
        assert np.float32(rec["score"][r, k]).view(U32) == np.float32(score).view(U32), (what, r, k)
    for r in range(len(n_hits)):
        assert rec[r, n_hits[r]:].tobytes() == bytes(16 * (K - n_hits[r])), (what, r)


def set_inputs(name, mode):
    qs, ts, t_idx, n_hits, (table, gi, ge) = pg.sets()[name]
    lists = pg.set_lists(name, mode)
    return qs, ts, t_idx, n_hits, lists, cc.hit_array(t_idx, n_hits, lists, mode == rc.LOCAL), sc.TABLES[table], gi, ge


# ---- 1. the sets -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("class", "homolog65", "homolog1", "muted", "graded130", "lengths", "wide"))
@pytest.mark.parametrize("mode", MODES)
def test_the_sets_against_the_reference(mode, name):
    pg.check_sets((mode,))
    qs, ts, t_idx, n_hits, lists, hits, table, gi, ge = set_inputs(name, mode)
    K = t_idx.shape[1]
    ctx = gpu_util.ctx()
    call = lambda *par, **kw: aln_amd.hits_purge(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, *par, align_type=mode, **kw)
    got = {}
    for par in pg.PARAMS:
        got[par] = call(*par)
        check(got[par], pg.set_reference(name, mode, *par), n_hits, lists, (name, mode, par))
    whole = got[(90, 50)]
    fused, batched = aln_amd.hits_align_routes(ctx)
    n_used = int(n_hits.sum())
    assert fused + batched == n_used and fused > 0
    if name == "class":                                                # row LONG_ROW: four fused slots and one through batches
        assert batched >= 1 and len(ts[t_idx[cc.LONG_ROW, 4]]) == cc.LONG_T and whole[1]["letters"][cc.LONG_ROW, 4] > 0
    # the records are aln_hits_align's; under 101 everything is aln_hits_weights'
    rec = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, align_type=mode, want_pairs=False, want_lines=False)[0]
    assert all(g[0].tobytes() == rec.tobytes() for g in got.values())
    plain = aln_amd.hits_weights(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, align_type=mode)
    none = got[(101, 0)]
    assert (none[0].tobytes(), none[2].tobytes(), none[3].tobytes(), none[5].tobytes(), none[6]) == \
        (plain[0].tobytes(), plain[1].tobytes(), plain[2].tobytes(), plain[4].tobytes(), plain[5])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(none[4], plain[3]))
    # the counts are aln_hits_column_counts' under the returned weights: byte for byte
    crec, counts, covered, crc = aln_amd.hits_column_counts(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, weights=whole[2],
                                                            align_type=mode)
    assert crc == 0 and crec.tobytes() == whole[0].tobytes() and covered.tobytes() == whole[5].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(counts, whole[4]))
    # compaction: the hit list without the slots that are not kept weighs as the kept slots do
    keeper = whole[1]["keeper"]
    packed, packed_n = np.zeros_like(hits), np.zeros_like(n_hits)
    kept = [np.nonzero(keeper[r] == np.arange(K))[0] for r in range(len(qs))]
    for r, ks in enumerate(kept):
        packed[r, :len(ks)], packed_n[r] = hits[r, ks], len(ks)
    small = aln_amd.hits_weights(ctx, qs, ts, packed, packed_n, ALPHA, table, gi, ge, align_type=mode)
    for r, ks in enumerate(kept):
        assert np.array_equal(small[1][r, :len(ks)], whole[2][r, ks]) and np.array_equal(small[2][r, :len(ks)], whole[3][r, ks]), r
        assert not small[1][r, len(ks):].any()
    assert small[4].tobytes() == whole[5].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(small[3], whole[4]))
    # groups of rows, chunks of hits, list groups, every slot through batches
    for rows in (1, 3):
        with ctx.hints(weights_group_rows=rows):
            same(call(90, 50), whole, ("weights_group_rows", rows))
            assert aln_amd.hits_align_routes(ctx) == (fused, batched)
    for chunk in (3,) if name == "wide" else (1, 3):
        with ctx.hints(align_chunk_hits=chunk):
            same(call(90, 50), whole, ("align_chunk_hits", chunk))
        with ctx.hints(align_chunk_hits=chunk, weights_group_rows=3):
            same(call(90, 50), whole, ("align_chunk_hits and groups", chunk))
    with ctx.hints(align_list_group_slots=1):
        same(call(90, 50), whole, "align_list_group_slots")
    if mode != rc.LOCAL and name != "wide":
        with ctx.hints(align_fused_nonlocal=0):
            same(call(90, 50), whole, "align_fused_nonlocal")
            assert aln_amd.hits_align_routes(ctx) == (0, n_used)
        with ctx.hints(align_fused_nonlocal=0, weights_group_rows=1, align_list_group_slots=2):
            same(call(90, 50), whole, "align_fused_nonlocal in groups")


def test_the_wide_row_holds_kept_and_purged_slots():
    qs, ts, t_idx, n_hits, lists, hits, table, gi, ge = set_inputs("wide", rc.LOCAL)
    assert t_idx.shape == (1, 1024) and len(qs[0]) <= 40 and len(set(ts)) <= 12
    got = aln_amd.hits_purge(gpu_util.ctx(), qs, ts, hits, n_hits, ALPHA, table, gi, ge, 90, 50)
    keeper = got[1]["keeper"][0]
    n_kept = int((keeper == np.arange(1024)).sum())
    assert 2 <= n_kept <= 12 and int((keeper >= 0).sum()) - n_kept >= 1000
    assert int((got[2][0] > 0).sum()) == n_kept and got[2][0].max() == 1000


# ---- 2. the optional outputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (rc.LOCAL, rc.SEMI_LOCAL))
def test_purge_only_and_raw_counts_and_covered_each_null_in_turn(mode):
    qs, ts, t_idx, n_hits, lists, hits, table, gi, ge = set_inputs("class", mode)
    ctx = gpu_util.ctx()
    call = lambda **kw: aln_amd.hits_purge(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, 90, 50, align_type=mode, **kw)
    whole = call()
    same(call(want_weights=False), [whole[0], whole[1], None, None, None, None, whole[6]], "purge only")
    for drop, at in (("want_raw", 3), ("want_counts", 4), ("want_covered", 5)):
        want = list(whole)
        want[at] = None
        same(call(**{drop: False}), want, drop)
    same(call(want_raw=False, want_counts=False, want_covered=False), [whole[0], whole[1], whole[2], None, None, None, whole[6]],
         "weights alone")
    with ctx.hints(weights_group_rows=2):
        same(call(want_weights=False), [whole[0], whole[1], None, None, None, None, whole[6]], "purge only, in groups")
        same(call(want_counts=False), [whole[0], whole[1], whole[2], whole[3], None, whole[5], whole[6]], "covered without counts")


# ---- 3. row blocks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (rc.LOCAL, rc.GLOBAL))
def test_a_row_block_with_q_begin(mode):
    qs, ts, t_idx, n_hits, lists, hits, table, gi, ge = set_inputs("lengths", mode)
    ctx = gpu_util.ctx()
    call = lambda h, n, **kw: aln_amd.hits_purge(ctx, qs, ts, h, n, ALPHA, table, gi, ge, 90, 50, align_type=mode, **kw)
    whole = call(hits, n_hits)
    off = np.concatenate(([0], np.cumsum([len(q) + 2 for q in qs])))
    for a, b in ((2, 5), (7, 8), (4, 6)):
        for group in (0, 2):
            with ctx.hints(weights_group_rows=group):
                part = call(hits[a:b], n_hits[a:b], q_begin=a)
            same(part, (whole[0][a:b], whole[1][a:b], whole[2][a:b], whole[3][a:b], whole[4][a:b], whole[5][off[a]:off[b]], whole[6]),
                 (mode, a, b))
    empty = call(hits[4:4], n_hits[4:4], q_begin=4)
    assert empty[0].shape == (0, 5) and empty[1].shape == (0, 5) and empty[4] == [] and len(empty[5]) == 0 and empty[6] == 0
    # a row without hits between rows with hits
    none = n_hits.copy()
    none[5] = 0
    got = call(hits, none)
    assert not got[2][5].any() and not got[3][5].any() and not got[4][5].any() and got[0][5].tobytes() == bytes(16 * 5)
    assert (records(got[1])[5] == (-1, 0, 0, 0)).all()
    keep = [r for r in range(len(qs)) if r != 5]
    for at in (1, 2, 3):
        assert got[at][keep].tobytes() == whole[at][keep].tobytes()
    assert all(got[4][r].tobytes() == whole[4][r].tobytes() for r in keep)


# ---- 4. a slot that fails -----------------------------------------------------------------------------------------------------------------
def test_a_falsified_local_score_is_refused_and_does_not_contribute():
    mode = rc.LOCAL
    qs, ts, t_idx, n_hits, lists, hits, table, gi, ge = set_inputs("class", mode)
    K = 5
    ctx = gpu_util.ctx()
    whole = aln_amd.hits_purge(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, 90, 50)
    bad = hits.copy()
    br, bk = 1, 0                                                      # row 1 (65 residues), slot 0: the row's keeper
    at = used_slots(n_hits, K).index((br, bk))
    assert cc.class_of(ts[t_idx[br, bk]]) <= 7 and lists[at][0] > 0 and whole[1]["keeper"][br, bk] == bk
    assert (whole[1]["keeper"][br, 1:n_hits[br]] == bk).any()
    bad["score"][br, bk] += 1.0
    got = aln_amd.hits_purge(ctx, qs, ts, bad, n_hits, ALPHA, table, gi, ge, 90, 50)
    assert got[6] == aln_amd.E_ARG
    want_status = np.zeros_like(whole[0]["status"])
    want_status[br, bk] = aln_amd.E_ARG
    assert np.array_equal(got[0]["status"], want_status) and got[0]["n_pairs"][br, bk] == 0
    rec = aln_amd.hits_align(ctx, qs, ts, bad, n_hits, ALPHA, table, gi, ge, want_pairs=False, want_lines=False)[0]
    assert got[0].tobytes() == rec.tobytes()
    assert tuple(records(got[1])[br, bk]) == (-1, 0, 0, 0)
    # the reference: the same row without that slot (a list of score 0 is what a slot that does not contribute looks like)
    muted = list(lists)
    muted[at] = (0.0, lists[at][1])
    ref = pg.reference([len(q) for q in qs], ts, t_idx, n_hits, muted, True, 90, 50)
    assert np.array_equal(records(got[1]), ref["purge"])
    assert np.array_equal(got[2], ref["weights"]) and np.array_equal(got[3], ref["raw"]) and np.array_equal(got[5], ref["covered"])
    assert all(np.array_equal(g, w) for g, w in zip(got[4], ref["counts"]))
    assert not np.array_equal(records(got[1])[br], records(whole[1])[br])
    keep = [r for r in range(len(qs)) if r != br]
    assert got[1][keep].tobytes() == whole[1][keep].tobytes() and got[2][keep].tobytes() == whole[2][keep].tobytes()


# ---- 5. the profile entry ----------------------------------------------------------------------------------------------------------------
def pool(profiles):
    return aln_amd.QueryProfiles([np.asarray(p, np.float32) for p in profiles], ALPHA)


@pytest.mark.parametrize("name", ("class", "lengths"))
@pytest.mark.parametrize("mode", MODES)
def test_derived_profiles_equal_the_residue_entry(mode, name):
    qs, ts, t_idx, n_hits, lists, hits, table, gi, ge = set_inputs(name, mode)
    ctx = gpu_util.ctx()
    qp = aln_amd.profiles_from_sequences(qs, ALPHA, table)
    for par in ((90, 50), (100, 0)):
        want = aln_amd.hits_purge(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, *par, align_type=mode)
        got = aln_amd.hits_purge_profiles(ctx, qp, ts, hits, n_hits, gi, ge, qs, *par, align_type=mode)
        assert sum(aln_amd.hits_align_routes(ctx)) == int(n_hits.sum())
        same(got, want, par)
    rec = aln_amd.hits_align_profiles(ctx, qp, ts, hits, n_hits, gi, ge, consensus=qs, align_type=mode, want_pairs=False,
                                      want_lines=False)[0]
    assert got[0].tobytes() == rec.tobytes()
    for chunk, per_chunk, group in ((1, 0, 0), (3, 1, 2)):
        with ctx.hints(align_chunk_hits=chunk, align_rows_per_chunk=per_chunk, weights_group_rows=group):
            same(aln_amd.hits_purge_profiles(ctx, qp, ts, hits, n_hits, gi, ge, qs, 100, 0, align_type=mode), got)
    # a given consensus and a NULL one differ only in the records' identity
    bare = aln_amd.hits_purge_profiles(ctx, qp, ts, hits, n_hits, gi, ge, None, 100, 0, align_type=mode)
    assert all(bare[at].tobytes() == got[at].tobytes() for at in (1, 2, 3, 5))


STAGING_ROWS = (7, 64, 65)                                             # interior rows around the staging ring's boundaries


@pytest.mark.parametrize("mode", MODES)
def test_position_specific_rows_against_the_restatement(mode):
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
    letters = aln_amd.hits_pileup_profiles(ctx, qp, ts, hits, n_hits, gi, ge, align_type=mode, want_tpos=False, want_spans=False)[2]
    purged = 0
    for par in pg.PARAMS + ((30, 0),):
        got = aln_amd.hits_purge_profiles(ctx, qp, ts, hits, n_hits, gi, ge, None, *par, align_type=mode)
        fused, batched = aln_amd.hits_align_routes(ctx)
        assert got[6] == 0 and fused > 0 and fused + batched == int(n_hits.sum())
        for r in range(len(profiles)):
            want = np.stack(aln_amd.purge_from_pileup(letters[r], ALPHA, *par), axis=1)
            assert np.array_equal(records(got[1])[r], want), (mode, par, r)
            rows = letters[r].copy()
            rows[want[:, 0] != np.arange(K)] = ord(".")
            w, raw = aln_amd.weights_from_pileup(rows, ALPHA, 1000)
            assert np.array_equal(w, got[2][r]) and np.array_equal(raw, got[3][r]), (mode, par, r)
            counts, covered = aln_amd.counts_from_pileup(rows, ALPHA, w)
            assert np.array_equal(counts[:len(profiles[r])], got[4][r][1:-1]), (mode, par, r)
        if par[0] <= 100:
            assert got[1]["keeper"][1, 2] == 0 and got[2][1, 2] == 0 and got[1]["same"][1, 2] == got[1]["letters"][1, 2] > 0
            purged += int(((got[1]["keeper"] >= 0) & (got[1]["keeper"] != np.arange(K)[None, :])).sum())
    assert purged >= 3


# ---- 6. arguments ----------------------------------------------------------------------------------------------------------------------
ARG_QS = ["PAWHEAE", "HEAGAWGHEE"]
ARG_TS = ["HEAGAWGHEE", "PAWHEAE", "AWHE"]
N_ROWS = sum(len(q) + 2 for q in ARG_QS)
POISON = dict(out=(np.uint8, 16, 0x5A), purge=(np.uint8, 16, 0x5A), weights=(np.int32, 1, 0x5A5A5A5A),
              raw=(np.int64, 1, 0x5A5A5A5A5A5A5A5A))


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
        for name, (dtype, per_slot, value) in POISON.items():
            setattr(self, name, np.full(n * per_slot, value, dtype=dtype))
        self.counts = np.full(N_ROWS * len(ALPHA), 0x5A5A5A5A, dtype=np.int32)
        self.covered = np.full(N_ROWS, 0x5A5A5A5A, dtype=np.int32)

    def untouched(self):
        return bool(all((getattr(self, name) == value).all() for name, (_, _, value) in POISON.items()) and
                    (self.counts == 0x5A5A5A5A).all() and (self.covered == 0x5A5A5A5A).all())

    def call(self, hit_array_, n_array, **kw):
        ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        a = dict(q=self.qp.c, prof=self.prof.c if self.prof else None, cons=self.qp.c, templ=self.tp.c, sub=self.sub, g=self.g,
                 hits=hit_array_.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits=n_array.ctypes.data_as(ip), max_identity=90,
                 min_overlap=50, w_max=1000, out=self.out.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)),
                 purge=self.purge.ctypes.data_as(C.POINTER(aln_amd.AlnHitPurge)), weights=self.weights.ctypes.data_as(ip),
                 raw=self.raw.ctypes.data_as(lp), counts=self.counts.ctypes.data_as(ip), covered=self.covered.ctypes.data_as(ip),
                 K=self.K, q_begin=0, q_end=self.rows)
        a.update(kw)
        ref = lambda x: None if x is None else C.byref(x)
        tail = (a["q_begin"], a["q_end"], a["K"], a["hits"], a["n_hits"], a["max_identity"], a["min_overlap"], a["w_max"], a["out"],
                a["purge"], a["weights"], a["raw"], a["counts"], a["covered"])
        if self.prof is not None:
            return aln_amd.lib().aln_hits_purge_profiles(gpu_util.ctx().h, ref(a["prof"]), ref(a["cons"]), ref(a["templ"]), ref(a["g"]),
                                                         *tail)
        return aln_amd.lib().aln_hits_purge(gpu_util.ctx().h, ref(a["q"]), ref(a["templ"]), ref(a["sub"]), ref(a["g"]), *tail)


def purge_and_slot_checks(raw, hits, n_hits, refused, bad_t, dotted):
    """the checks behind the scoring call's, the same for both entries: purge, max_identity, min_overlap, the weights group and
    w_max, then n_hits, t, the local end cell, and last the alphabet (dotted: keyword arguments that put a '.' into the call's
    alphabet)"""
    E = aln_amd.E_ARG
    K = raw.K
    Q = [len(q) + 2 for q in ARG_QS]
    refused(E, "NULL purge", purge=None)
    for v in (0, -1, 102):
        refused(E, ("max_identity", v), max_identity=v)
    for v in (-1, 101):
        refused(E, ("min_overlap", v), min_overlap=v)
    for kw in (dict(counts=None, covered=None), dict(raw=None, covered=None), dict(raw=None, counts=None), dict()):
        refused(E, ("NULL weights with", kw), weights=None, **kw)
    for w in (0, -1, 65536):
        refused(E, ("w_max", w), w_max=w)
    refused(aln_amd.E_RESIDUE, "the residues come before purge, the bounds and w_max", purge=None, max_identity=0, min_overlap=-1, w_max=0,
            templ=bad_t)
    bad_n = n_hits.copy()
    bad_n[0] = K + 1
    refused(E, "n_hits and the alphabet", n_arr=bad_n, **dotted)
    refused(E, "w_max before n_hits", n_arr=bad_n, w_max=0)
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
    refused(E, "an alphabet with '.', purge only", weights=None, raw=None, counts=None, covered=None, **dotted)
    refused(0, "empty block", q_begin=1, q_end=1)
    # the bounds themselves are accepted; purge only reads no w_max and leaves the weight outputs alone
    for kw in (dict(max_identity=1), dict(max_identity=101), dict(min_overlap=0), dict(min_overlap=100), dict(w_max=1), dict(w_max=65535)):
        raw.fill()
        assert raw.call(hits, n_hits, **kw) == 0 and not (raw.purge == 0x5A).all(), kw
    raw.fill()
    assert raw.call(hits, n_hits, weights=None, raw=None, counts=None, covered=None, w_max=0) == 0
    assert not (raw.out == 0x5A).all() and not (raw.purge.view(np.int32) == 0x5A5A5A5A).any()
    fresh = Raw(K)
    for name in ("weights", "raw", "counts", "covered"):
        assert (getattr(raw, name) == getattr(fresh, name)).all(), name
    for kw, kept in ((dict(raw=None), "raw"), (dict(counts=None), "counts"), (dict(covered=None), "covered"),
                     (dict(counts=None, covered=None, raw=None), "raw")):
        raw.fill()
        assert raw.call(hits, n_hits, **kw) == 0 and not (raw.weights == 0x5A5A5A5A).any()
        assert (getattr(raw, kept) == getattr(fresh, kept)).all(), kw   # the sentinel stands where NULL was passed
    raw.fill()


def test_argument_checks_leave_the_outputs_untouched():
    ctx = gpu_util.ctx()
    E = aln_amd.E_ARG
    K = 2
    hits, n_hits = aln_amd.search_topk(ctx, ARG_QS, ARG_TS, ALPHA, cc.TABLE, GI, GE, K)
    assert (n_hits == K).all()
    raw = Raw(K)
    assert raw.call(hits, n_hits) == 0 and not raw.untouched()
    for x in (raw.out, raw.purge, raw.weights, raw.raw, raw.counts, raw.covered):
        assert not (x.view(np.uint8) == 0x5A).all()
    assert not (raw.weights == 0x5A5A5A5A).any() and not (raw.counts == 0x5A5A5A5A).any()
    assert not (raw.purge.view(np.int32) == 0x5A5A5A5A).any()
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
    # 3 - 7. purge, the bounds, the weights group, w_max; 8. n_hits, t, the end cell; 9. the alphabet
    spare = [ch for ch in ALPHA if all(ch not in s for s in ARG_QS + ARG_TS)][0]
    dot_sub = aln_amd.AlnSubmatrix(len(ALPHA), ALPHA.replace(spare, ".").encode(), raw.tab.ctypes.data_as(C.POINTER(C.c_float)))
    purge_and_slot_checks(raw, hits, n_hits, refused, bad_t, dict(sub=dot_sub))
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
    for name in ("out", "purge", "weights", "raw", "counts", "covered"):
        assert getattr(raw, name).tobytes() == getattr(plain, name).tobytes(), name
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
    purge_and_slot_checks(raw, hits, n_hits, refused, bad_t, dict(prof=qprof(alphabet=ALPHA.replace(spare, ".").encode())))
    refused(E, "an alphabet with '-'", prof=qprof(alphabet=ALPHA.replace(spare, "-").encode()))
    raw.fill()
    assert raw.call(hits, n_hits, cons=None) == 0
    for name in ("purge", "weights", "raw", "counts", "covered"):
        assert getattr(raw, name).tobytes() == getattr(plain, name).tobytes(), name


# ---- 7. two rounds ------------------------------------------------------------------------------------------------------------------------
def test_two_rounds_search_purge_profile_search():
    qs, ts = cc.homolog_set()
    assert len(qs) == 8 and len(ts) == 10                             # (query 3 has two relatives among them, 91 % identical)
    ctx = gpu_util.ctx()
    K = 4
    mode = rc.LOCAL
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, ALPHA, cc.TABLE, GI, GE, K)                       # 1. search
    assert (n_hits == K).all()
    rec, purge, weights, raw, counts, covered, rcode = aln_amd.hits_purge(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, 90, 50,
                                                                          w_max=100)                   # 2. purge, weights, counts
    assert rcode == 0
    lists = [cc.pair_list(qs[r], ts[hits["t"][r, k]], mode) for r, k in used_slots(n_hits, K)]
    ref = pg.reference([len(q) for q in qs], ts, hits["t"], n_hits, lists, True, 90, 50, w_max=100)
    check((rec, purge, weights, raw, counts, covered, rcode), ref, n_hits, lists, "two rounds")
    assert (weights.max(axis=1) == 100).all() and ((purge["keeper"] >= 0) & (purge["keeper"] != np.arange(K)[None, :])).any()
    background = np.full(len(ALPHA), 1.0 / len(ALPHA))
    fallback = pc.derived(qs, cc.TABLE)
    rows = [aln_amd.pssm_from_counts(counts[r][1:-1], background, fallback[r]) for r in range(len(qs))]   # 3. the profile
    assert all(np.array_equal(p, np.rint(p)) for p in rows) and any((c[1:-1].sum(axis=1) > 0).all() for c in counts)
    profiles = [p.astype(np.int64) for p in rows]
    assert any(not np.array_equal(p, f) for p, f in zip(profiles, fallback))
    qp = pool(profiles)
    hits2, n2 = aln_amd.search_topk_profiles(ctx, qp, ts, GI, GE, K)                                     # 4. profile search
    scores, ends = pc.dense_reference("purge_two_rounds", profiles, ts, mode, GI, GE)
    for r in range(len(qs)):
        order = sc.topk_reference(scores[r], K)
        assert n2[r] == len(order) and hits2["t"][r, :len(order)].tolist() == order, (r, hits2[r].tolist(), order)
        assert np.array_equal(hits2["score"][r, :len(order)].view(U32), scores[r, order].astype(np.float32).view(U32)), r
        assert np.array_equal(hits2["q_end"][r, :len(order)], ends[r, order, 0]), r
        assert np.array_equal(hits2["t_end"][r, :len(order)], ends[r, order, 1]), r
    # and the loop closes: the second round's hits can be purged again, from the profile side
    again = aln_amd.hits_purge_profiles(ctx, qp, ts, hits2, n2, GI, GE, qs)
    assert again[6] == 0 and (again[2].max(axis=1) == 1000).all() and sum(int(c.sum()) for c in again[4]) > 0
