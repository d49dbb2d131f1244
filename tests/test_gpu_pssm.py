"""-m gpu: aln_hits_pssm / aln_hits_pssm_profiles — from a search round's hits to the next round's profile rows in one call, the
log-odds made on the device by the exact integer rule of include/aln_hip.h (csrc/search_pssm.hip), and aln_amd.iterate_search
on top of them.  Every comparison is equality: the rows against aln_amd.pssm_rows_from_counts (Python integers) over the
counts of purge_cases' reference (the oracle's pair lists, not the library), every optional output byte for byte against
aln_hits_purge's.

  1  the sets under three align types: K = 5 / 65 / 1024, Q-2 of 1 .. 130 in one block, rows without hits, both routes into one
     stack, the muted rows; mix NULL and a mix that is not the background, the four scales, beta of 1, w_max and 2^26; groups,
     chunks, align_fused_nonlocal = 0
  2  every optional output NULL in turn
  3  a row block with q_begin > 0
  4  a falsified local score
  5  the profile entry: derived rows, position-specific rows that fall back to themselves
  6  alphabets of 20, 30 and 1 letters, a fractional table
  7  the argument checks, in their order
  8  iterate_search: three rounds against the chain driven by hand"""
import ctypes as C

import numpy as np
import pytest

import aln_amd
import column_count_cases as cc
import gpu_util
import profile_cases as pc
import purge_cases as pg
import range_cases as rc
import search_cases as sc

pytestmark = pytest.mark.gpu

U32 = np.uint32
ALPHA = cc.ALPHA
N = len(ALPHA)
_, GI, GE = cc.SYSTEM
MODES = (rc.LOCAL, rc.GLOBAL, rc.SEMI_LOCAL)
W_MAX = pg.W_MAX


def background(n):
    """n integer background weights in 1..1024 that are not all equal; their sum is at most 1024"""
    bg = [1 + (a * 37 + 11) % (1024 // n) for a in range(n)] if n > 1 else [777]
    assert all(1 <= b <= 1024 for b in bg) and sum(bg) <= 1024 and (n == 1 or len(set(bg)) > 1)
    return bg


def target_mix(bg):
    """a mix that is not the background: half of the background off the diagonal (at least 1), the rest of B on the diagonal"""
    n, B = len(bg), sum(bg)
    mix = [[max(bg[a] // 2, 1) for a in range(n)] for _ in range(n)]
    for b in range(n):
        mix[b][b] += B - sum(mix[b])
    assert all(min(row) >= 1 and sum(row) == B for row in mix)
    return mix


BG = background(N)
MIX = target_mix(BG)
# (mix, scale, beta): both mixes, the four scales, beta of 1, w_max and 2^26
RULES = ((None, 2, W_MAX), (MIX, 1, 1), (MIX, 4, 1 << 26), (None, 8, 1), (MIX, 8, W_MAX), (None, 1, 1 << 26), (MIX, 2, 1))


def params(mix, scale, beta, bg=BG):
    return aln_amd.AlnPssmParams.make(bg, beta, scale, mix)


def table_rows(qs, alphabet, table):
    """the fallback rows of residue queries: the table row of every residue, float32"""
    tab = np.asarray(table, np.float32).reshape(len(alphabet), len(alphabet))
    return [tab[[alphabet.index(ch) for ch in q]].reshape(len(q), len(alphabet)) for q in qs]


def expected_rows(counts, fallback, bg, beta, scale, mix):
    """per query the (Q, n) float32 rows: zero sentinel rows around pssm_rows_from_counts of the interior count rows"""
    out = []
    for c, f in zip(counts, fallback):
        n = np.asarray(f).shape[1]
        inner = aln_amd.pssm_rows_from_counts(np.asarray(c)[1:-1], bg, beta, scale, np.asarray(f, np.float32).reshape(-1, n), mix)
        out.append(np.concatenate([np.zeros((1, n), np.float32), inner.reshape(-1, n), np.zeros((1, n), np.float32)]))
    return out


def same_rows(got, want, what):
    assert len(got) == len(want), what
    for r, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and g.shape == w.shape, (what, r)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(U32) != w.view(U32))
            print(what, "row", r, "entries that differ:", len(bad), "first", bad[0], g[tuple(bad[0])], w[tuple(bad[0])])
        assert g.tobytes() == w.tobytes(), (what, r)


def same(a, b, what=None):
    """two 8-tuples of hits_pssm, byte for byte"""
    assert a[7] == b[7], what
    for at in (0, 2, 3, 4, 6):
        x, y = a[at], b[at]
        assert (x is None) == (y is None) and (x is None or (x.shape == y.shape and x.tobytes() == y.tobytes())), (what, at)
    for at in (1, 5):
        assert (a[at] is None) == (b[at] is None), (what, at)
        if a[at] is not None:
            assert len(a[at]) == len(b[at]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[at], b[at])), (what, at)


def same_as_purge(got, purge, what):
    """the optional outputs of an 8-tuple of hits_pssm against the 7-tuple of hits_purge, byte for byte"""
    assert got[7] == purge[6], what
    for mine, its in ((0, 0), (2, 1), (3, 2), (4, 3), (6, 5)):
        assert got[mine].dtype == purge[its].dtype and got[mine].tobytes() == purge[its].tobytes(), (what, mine)
    assert len(got[5]) == len(purge[4]) and all(x.tobytes() == y.tobytes() for x, y in zip(got[5], purge[4])), what


def set_inputs(name, mode):
    qs, ts, t_idx, n_hits, (table, gi, ge) = pg.sets()[name]
    lists = pg.set_lists(name, mode)
    return qs, ts, t_idx, n_hits, lists, cc.hit_array(t_idx, n_hits, lists, mode == rc.LOCAL), sc.TABLES[table], gi, ge


# ---- 1. the sets -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("class", "homolog65", "muted", "lengths", "wide"))
@pytest.mark.parametrize("mode", MODES)
def test_the_sets_against_the_reference(mode, name):
    qs, ts, t_idx, n_hits, lists, hits, table, gi, ge = set_inputs(name, mode)
    ref = pg.set_reference(name, mode, 90, 50)
    fallback = table_rows(qs, ALPHA, table)
    ctx = gpu_util.ctx()
    call = lambda par, *more, **kw: aln_amd.hits_pssm(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, par, *more, align_type=mode, **kw)
    purge = aln_amd.hits_purge(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, 90, 50, align_type=mode)
    assert all(np.array_equal(g, w) for g, w in zip(purge[4], ref["counts"]))
    n_zero = sum(int((np.asarray(c)[1:-1].sum(axis=1) == 0).sum()) for c in ref["counts"])
    n_some = sum(int((np.asarray(c)[1:-1].sum(axis=1) > 0).sum()) for c in ref["counts"])
    print(name, mode, "positions without counts:", n_zero, "with counts:", n_some)
    assert n_some >= 1 or name == "muted", (name, mode)
    assert n_zero >= 1 or name not in ("muted", "lengths", "homolog65"), (name, mode)     # (a row without hits; the muted rows)
    whole = None
    for mix, scale, beta in RULES:
        got = call(params(mix, scale, beta), 90, 50)
        same_rows(got[1], expected_rows(ref["counts"], fallback, BG, beta, scale, mix), (name, mode, scale, beta, mix is not None))
        same_as_purge(got, purge, (name, mode, scale, beta))
        whole = whole or got
    fused, batched = aln_amd.hits_align_routes(ctx)
    n_used = int(n_hits.sum())
    assert fused + batched == n_used and fused > 0
    if name == "class":                                                # row LONG_ROW: four fused slots and one through batches
        assert batched >= 1 and whole[2]["letters"][cc.LONG_ROW, 4] > 0
    # 101 purges nothing: the outputs are hits_purge's there too
    if name in ("class", "wide"):
        none = call(params(MIX, 2, W_MAX), 101, 0)
        p101 = aln_amd.hits_purge(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, 101, 0, align_type=mode)
        same_as_purge(none, p101, "101")
        same_rows(none[1], expected_rows(pg.set_reference(name, mode, 101, 0)["counts"], fallback, BG, W_MAX, 2, MIX), "101")
    # groups of rows, chunks of hits, every slot through batches
    first = params(*RULES[0])
    with ctx.hints(weights_group_rows=1):
        same(call(first, 90, 50), whole, "weights_group_rows")
        assert aln_amd.hits_align_routes(ctx) == (fused, batched)
    with ctx.hints(align_chunk_hits=3):
        same(call(first, 90, 50), whole, "align_chunk_hits")
    with ctx.hints(align_chunk_hits=1 if name != "wide" else 7, weights_group_rows=3):
        same(call(first, 90, 50), whole, "align_chunk_hits and groups")
    if mode != rc.LOCAL and name != "wide":
        with ctx.hints(align_fused_nonlocal=0):
            same(call(first, 90, 50), whole, "align_fused_nonlocal")
            assert aln_amd.hits_align_routes(ctx) == (0, n_used)


# ---- 2. the optional outputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (rc.LOCAL, rc.SEMI_LOCAL))
def test_every_optional_output_null_in_turn(mode):
    qs, ts, t_idx, n_hits, lists, hits, table, gi, ge = set_inputs("class", mode)
    ctx = gpu_util.ctx()
    par = params(MIX, 2, W_MAX)
    call = lambda **kw: aln_amd.hits_pssm(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, par, 90, 50, align_type=mode, **kw)
    whole = call()
    assert all(x is not None for x in whole)
    flags = (("want_purge", 2), ("want_weights", 3), ("want_raw", 4), ("want_counts", 5), ("want_covered", 6))
    for drop, at in flags:
        want = list(whole)
        want[at] = None
        same(call(**{drop: False}), want, drop)
    bare = [whole[0], whole[1], None, None, None, None, None, whole[7]]
    same(call(**{drop: False for drop, _ in flags}), bare, "rows alone")
    with ctx.hints(weights_group_rows=2):
        same(call(**{drop: False for drop, _ in flags}), bare, "rows alone, in groups")
        same(call(want_weights=False, want_counts=False), [whole[0], whole[1], whole[2], None, whole[4], None, whole[6], whole[7]],
             "raw and covered without weights and counts")


# ---- 3. row blocks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (rc.LOCAL, rc.GLOBAL))
def test_a_row_block_with_q_begin(mode):
    qs, ts, t_idx, n_hits, lists, hits, table, gi, ge = set_inputs("lengths", mode)
    ctx = gpu_util.ctx()
    par = params(MIX, 4, 77)
    call = lambda h, n, **kw: aln_amd.hits_pssm(ctx, qs, ts, h, n, ALPHA, table, gi, ge, par, 90, 50, align_type=mode, **kw)
    whole = call(hits, n_hits)
    off = np.concatenate(([0], np.cumsum([len(q) + 2 for q in qs])))
    for a, b in ((2, 5), (7, 8), (4, 6)):
        for group in (0, 2):
            with ctx.hints(weights_group_rows=group):
                part = call(hits[a:b], n_hits[a:b], q_begin=a)
            same(part, (whole[0][a:b], whole[1][a:b], whole[2][a:b], whole[3][a:b], whole[4][a:b], whole[5][a:b],
                        whole[6][off[a]:off[b]], whole[7]), (mode, a, b))
    empty = call(hits[4:4], n_hits[4:4], q_begin=4)
    assert empty[0].shape == (0, 5) and empty[1] == [] and empty[5] == [] and len(empty[6]) == 0 and empty[7] == 0
    # a row without hits between rows with hits: its rows are the table's
    none = n_hits.copy()
    none[5] = 0
    got = call(hits, none)
    assert got[1][5][1:-1].tobytes() == table_rows(qs, ALPHA, table)[5].tobytes() and not got[1][5][[0, -1]].any()
    assert all(got[1][r].tobytes() == whole[1][r].tobytes() for r in range(len(qs)) if r != 5)


# ---- 4. a slot that fails -----------------------------------------------------------------------------------------------------------------
def test_a_falsified_local_score_is_refused_and_does_not_contribute():
    mode = rc.LOCAL
    qs, ts, t_idx, n_hits, lists, hits, table, gi, ge = set_inputs("class", mode)
    ctx = gpu_util.ctx()
    par = params(MIX, 2, W_MAX)
    whole = aln_amd.hits_pssm(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, par, 90, 50)
    bad = hits.copy()
    br, bk = 1, 0                                                      # row 1 (65 residues), slot 0: the row's keeper
    at = cc.used_slots(n_hits, 5).index((br, bk))
    assert lists[at][0] > 0 and whole[2]["keeper"][br, bk] == bk
    bad["score"][br, bk] += 1.0
    got = aln_amd.hits_pssm(ctx, qs, ts, bad, n_hits, ALPHA, table, gi, ge, par, 90, 50)
    assert got[7] == aln_amd.E_ARG
    want_status = np.zeros_like(whole[0]["status"])
    want_status[br, bk] = aln_amd.E_ARG
    assert np.array_equal(got[0]["status"], want_status)
    same_as_purge(got, aln_amd.hits_purge(ctx, qs, ts, bad, n_hits, ALPHA, table, gi, ge, 90, 50), "falsified")
    muted = list(lists)
    muted[at] = (0.0, lists[at][1])                                    # what a slot that does not contribute looks like
    ref = pg.reference([len(q) for q in qs], ts, t_idx, n_hits, muted, True, 90, 50)
    same_rows(got[1], expected_rows(ref["counts"], table_rows(qs, ALPHA, table), BG, W_MAX, 2, MIX), "falsified")
    # (the row's other slots carry the same homolog: another slot is kept in its place, and the rows need not change)
    assert got[2][br].tobytes() != whole[2][br].tobytes() and tuple(got[2][br, bk]) == (-1, 0, 0, 0)
    assert all(got[1][r].tobytes() == whole[1][r].tobytes() for r in range(len(qs)) if r != br)


# ---- 5. the profile entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("class", "lengths"))
@pytest.mark.parametrize("mode", MODES)
def test_derived_profiles_equal_the_residue_entry(mode, name):
    qs, ts, t_idx, n_hits, lists, hits, table, gi, ge = set_inputs(name, mode)
    ctx = gpu_util.ctx()
    qp = aln_amd.profiles_from_sequences(qs, ALPHA, table)
    for rule in (RULES[0], RULES[4]):
        par = params(*rule)
        want = aln_amd.hits_pssm(ctx, qs, ts, hits, n_hits, ALPHA, table, gi, ge, par, 90, 50, align_type=mode)
        got = aln_amd.hits_pssm_profiles(ctx, qp, ts, hits, n_hits, gi, ge, par, qs, 90, 50, align_type=mode)
        assert sum(aln_amd.hits_align_routes(ctx)) == int(n_hits.sum())
        same(got, want, rule[1:])
    with ctx.hints(align_chunk_hits=3, align_rows_per_chunk=1, weights_group_rows=2):
        same(aln_amd.hits_pssm_profiles(ctx, qp, ts, hits, n_hits, gi, ge, par, qs, 90, 50, align_type=mode), got, "hints")
    # a NULL consensus changes the records' identity only
    bare = aln_amd.hits_pssm_profiles(ctx, qp, ts, hits, n_hits, gi, ge, par, None, 90, 50, align_type=mode)
    same([None] + list(bare[1:]), [None] + list(got[1:]), "NULL consensus")


STAGING_ROWS = (7, 64, 65)


@pytest.mark.parametrize("mode", MODES)
def test_position_specific_rows_fall_back_to_themselves(mode):
    every, ts = pc.length_set()
    profiles = [p for p in every[:len(pc.INTERIOR_ROWS)] if len(p) in STAGING_ROWS]
    assert tuple(len(p) for p in profiles) == STAGING_ROWS
    _, gi, ge = pc.LENGTH_SYSTEM
    ctx = gpu_util.ctx()
    qp = aln_amd.QueryProfiles([np.asarray(p, np.float32) for p in profiles], ALPHA)
    K = 4
    hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, ts, gi, ge, K, align_type=mode)
    assert (n_hits == K).all()
    n_hits[0] = 0                                                      # a profile without hits keeps all of its rows
    purge = aln_amd.hits_purge_profiles(ctx, qp, ts, hits, n_hits, gi, ge, None, 90, 50, align_type=mode)
    own = [np.asarray(p, np.float32) for p in profiles]
    for rule in (RULES[1], RULES[5]):
        got = aln_amd.hits_pssm_profiles(ctx, qp, ts, hits, n_hits, gi, ge, params(*rule), None, 90, 50, align_type=mode)
        same_as_purge(got, purge, (mode, rule[1:]))
        same_rows(got[1], expected_rows(purge[4], own, BG, rule[2], rule[1], rule[0]), (mode, rule[1:]))
    assert got[1][0][1:-1].tobytes() == own[0].tobytes()
    assert sum(int((c[1:-1].sum(axis=1) > 0).sum()) for c in purge[4]) >= 10


# ---- 6. other alphabets, a fractional table ----------------------------------------------------------------------------------------------
def extra_letters(s, letters, every):
    """s with every `every`-th residue replaced by one of `letters`"""
    return "".join(letters[(i // every) % len(letters)] if i % every == every - 1 else ch for i, ch in enumerate(s))


def alphabet_case(n):
    qs, ts = cc.homolog_set()
    assert all(ch in ALPHA[:20] for s in qs + ts for ch in s)
    if n == 20:
        return qs, ts, ALPHA[:20], np.ascontiguousarray(cc.TABLE[:20, :20]), GI, GE
    if n == 30:
        more = "JOUbjo"
        table = np.full((30, 30), -2, np.float32)
        table[:N, :N] = cc.TABLE
        table[np.arange(N, 30), np.arange(N, 30)] = 6
        return [extra_letters(q, more, 5) for q in qs], [extra_letters(t, more, 5) for t in ts], ALPHA + more, table, GI, GE
    assert n == 1
    return ["A" * 10, "AAA", "A"], ["AAAA", "AAA", "AA"], "A", np.full((1, 1), 2, np.float32), 3, 1   # 10 > 4 + 3 + 2


@pytest.mark.parametrize("n", (20, 30, 1))
def test_alphabets_of_20_30_and_1_letters(n):
    qs, ts, alphabet, table, gi, ge = alphabet_case(n)
    assert len(alphabet) == n
    ctx = gpu_util.ctx()
    K = 3
    bg = background(n)
    mix = target_mix(bg)
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, alphabet, table, gi, ge, K)
    assert (n_hits == K).all()
    purge = aln_amd.hits_purge(ctx, qs, ts, hits, n_hits, alphabet, table, gi, ge, 90, 50)
    assert purge[6] == 0 and sum(int(c.sum()) for c in purge[4]) > 0
    if n == 30:
        assert sum(int(c[:, N:].sum()) for c in purge[4]) > 0          # the letters beyond the 24th are counted
    fallback = table_rows(qs, alphabet, table)
    for m, scale, beta in ((None, 2, W_MAX), (mix, 8, 1), (mix, 1, 1 << 26), (mix, 4, 50)):
        got = aln_amd.hits_pssm(ctx, qs, ts, hits, n_hits, alphabet, table, gi, ge, aln_amd.AlnPssmParams.make(bg, beta, scale, m), 90, 50)
        same_as_purge(got, purge, (n, scale, beta))
        same_rows(got[1], expected_rows(purge[4], fallback, bg, beta, scale, m), (n, scale, beta))
    if n == 1:                                                         # one letter: every odds ratio is 1
        assert all(not g[1:-1][c[1:-1, 0] > 0].any() for g, c in zip(got[1], purge[4]))
        assert any((g[1:-1][c[1:-1, 0] == 0] == 2).all() and (c[1:-1, 0] == 0).any() for g, c in zip(got[1], purge[4]))


def test_a_fractional_table_keeps_its_rows_bit_for_bit():
    qs, ts = cc.homolog_set()
    qs, ts = qs[:3], ts[:4]
    table = (np.asarray(cc.TABLE, np.float32) * np.float32(0.5) + np.float32(0.125)).astype(np.float32)
    assert not np.array_equal(table, np.rint(table))
    ctx = gpu_util.ctx()
    K = 2
    hits, n_hits = aln_amd.search_topk(ctx, qs, ts, ALPHA, table, 5.5, 0.5, K)
    n_hits[0] = 0                                                      # a query without hits keeps the table's rows
    purge = aln_amd.hits_purge(ctx, qs, ts, hits, n_hits, ALPHA, table, 5.5, 0.5, 90, 50)
    assert purge[6] == 0 and sum(int(c.sum()) for c in purge[4]) > 0
    got = aln_amd.hits_pssm(ctx, qs, ts, hits, n_hits, ALPHA, table, 5.5, 0.5, params(MIX, 2, W_MAX), 90, 50)
    same_as_purge(got, purge, "fractional")
    fallback = table_rows(qs, ALPHA, table)
    same_rows(got[1], expected_rows(purge[4], fallback, BG, W_MAX, 2, MIX), "fractional")
    kept = sum(int((c[1:-1].sum(axis=1) == 0).sum()) for c in purge[4])
    assert kept >= 1 and any(((g[1:-1] != np.rint(g[1:-1])).any()) for g in got[1])


# ---- 7. arguments ----------------------------------------------------------------------------------------------------------------------
ARG_QS = ["PAWHEAE", "HEAGAWGHEE"]
ARG_TS = ["HEAGAWGHEE", "PAWHEAE", "AWHE"]
N_ROWS = sum(len(q) + 2 for q in ARG_QS)
POISON = dict(out=(np.uint8, 16, 0x5A), purge=(np.uint8, 16, 0x5A), weights=(np.int32, 1, 0x5A5A5A5A),
              raw=(np.int64, 1, 0x5A5A5A5A5A5A5A5A))


def pssm_params(scale=2, beta=10, bg=BG, mix=None, null_bg=False):
    p = aln_amd.AlnPssmParams.make(bg, 1, 1, mix)
    p.scale, p.beta = scale, beta                                      # (values make() would not take are set on the struct)
    if null_bg:
        p.bg = None
    return p


class Raw:
    """both entries through ctypes with sentinel-filled outputs"""

    def __init__(self, K, profiles=None):
        self.qp = aln_amd.SeqPool(ARG_QS)
        self.tp = aln_amd.SeqPool(ARG_TS)
        self.prof = aln_amd.QueryProfiles([np.asarray(p, np.float32) for p in profiles], ALPHA) if profiles is not None else None
        self.tab = np.ascontiguousarray(cc.TABLE, np.float32)
        self.sub = aln_amd.AlnSubmatrix(N, ALPHA.encode(), self.tab.ctypes.data_as(C.POINTER(C.c_float)))
        self.g = cc.gap()
        self.par = pssm_params()
        self.rows, self.K = len(ARG_QS), K
        self.fill()

    def fill(self):
        n = self.rows * self.K
        for name, (dtype, per_slot, value) in POISON.items():
            setattr(self, name, np.full(n * per_slot, value, dtype=dtype))
        self.prows = np.full(N_ROWS * N, 0x5A5A5A5A, dtype=np.uint32)
        self.counts = np.full(N_ROWS * N, 0x5A5A5A5A, dtype=np.int32)
        self.covered = np.full(N_ROWS, 0x5A5A5A5A, dtype=np.int32)

    def untouched(self):
        return bool(all((getattr(self, name) == value).all() for name, (_, _, value) in POISON.items()) and
                    (self.prows == 0x5A5A5A5A).all() and (self.counts == 0x5A5A5A5A).all() and (self.covered == 0x5A5A5A5A).all())

    def call(self, hit_array_, n_array, **kw):
        ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        a = dict(q=self.qp.c, prof=self.prof.c if self.prof else None, cons=self.qp.c, templ=self.tp.c, sub=self.sub, g=self.g,
                 hits=hit_array_.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits=n_array.ctypes.data_as(ip), max_identity=90,
                 min_overlap=50, w_max=1000, par=self.par, out=self.out.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)),
                 prows=self.prows.ctypes.data_as(C.POINTER(C.c_float)),
                 purge=self.purge.ctypes.data_as(C.POINTER(aln_amd.AlnHitPurge)), weights=self.weights.ctypes.data_as(ip),
                 raw=self.raw.ctypes.data_as(lp), counts=self.counts.ctypes.data_as(ip), covered=self.covered.ctypes.data_as(ip),
                 K=self.K, q_begin=0, q_end=self.rows)
        a.update(kw)
        ref = lambda x: None if x is None else C.byref(x)
        tail = (a["q_begin"], a["q_end"], a["K"], a["hits"], a["n_hits"], a["max_identity"], a["min_overlap"], a["w_max"], ref(a["par"]),
                a["out"], a["prows"], a["purge"], a["weights"], a["raw"], a["counts"], a["covered"])
        if self.prof is not None:
            return aln_amd.lib().aln_hits_pssm_profiles(gpu_util.ctx().h, ref(a["prof"]), ref(a["cons"]), ref(a["templ"]), ref(a["g"]),
                                                        *tail)
        return aln_amd.lib().aln_hits_pssm(gpu_util.ctx().h, ref(a["q"]), ref(a["templ"]), ref(a["sub"]), ref(a["g"]), *tail)


def rule_and_slot_checks(raw, hits, n_hits, refused, bad_t, dotted):
    """the checks behind the scoring call's, the same for both entries: max_identity, min_overlap, w_max; par and rows; scale;
    beta; bg; mix; then n_hits, t, the local end cell, and last the alphabet"""
    E = aln_amd.E_ARG
    K = raw.K
    for v in (0, -1, 102):
        refused(E, ("max_identity", v), max_identity=v)
    for v in (-1, 101):
        refused(E, ("min_overlap", v), min_overlap=v)
    for w in (0, -1, 65536):
        refused(E, ("w_max", w), w_max=w)
        refused(E, ("w_max is read without weights", w), w_max=w, weights=None, raw=None, counts=None, covered=None)
    refused(E, "NULL par", par=None)
    refused(E, "NULL rows", prows=None)
    for v in (0, 3, 5, 16, -1):
        refused(E, ("scale", v), par=pssm_params(scale=v))
    for v in (0, -1, (1 << 26) + 1):
        refused(E, ("beta", v), par=pssm_params(beta=v))
    refused(E, "NULL bg", par=pssm_params(null_bg=True))
    for at, v in ((0, 0), (N - 1, 1025), (3, -5)):
        bg = list(BG)
        bg[at] = v
        refused(E, ("bg", at, v), par=pssm_params(bg=bg))
    refused(E, "B above 1024", par=pssm_params(bg=[43] * N))
    low = [row[:] for row in MIX]
    low[2][5], low[2][6] = 0, low[2][6] + low[2][5]                   # the row still sums to B
    refused(E, "a mix entry below 1", par=pssm_params(mix=low))
    off = [row[:] for row in MIX]
    off[N - 1][0] += 1
    refused(E, "a mix row that does not sum to B", par=pssm_params(mix=off))
    refused(aln_amd.E_RESIDUE, "the residues come before the bounds, w_max, par and rows", max_identity=0, min_overlap=-1, w_max=0,
            par=None, prows=None, templ=bad_t)
    bad_n = n_hits.copy()
    bad_n[0] = K + 1
    refused(E, "n_hits and the alphabet", n_arr=bad_n, **dotted)
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
    refused(E, "an alphabet with '.'", **dotted)
    refused(0, "empty block", q_begin=1, q_end=1)
    # the bounds themselves are accepted
    full = [42] * N
    full[0] += 1024 - sum(full)
    for kw in (dict(par=pssm_params(beta=1)), dict(par=pssm_params(beta=1 << 26)), dict(par=pssm_params(scale=1)),
               dict(par=pssm_params(scale=8)), dict(par=pssm_params(bg=full)), dict(par=pssm_params(mix=MIX)), dict(w_max=1),
               dict(w_max=65535), dict(max_identity=101)):
        raw.fill()
        assert raw.call(hits, n_hits, **kw) == 0 and not (raw.prows == 0x5A5A5A5A).any(), kw
    # an optional output that is NULL leaves nothing behind; the others are written
    fresh = Raw(K)
    for name in ("purge", "weights", "raw", "counts", "covered"):
        raw.fill()
        assert raw.call(hits, n_hits, **{name: None}) == 0 and not (raw.prows == 0x5A5A5A5A).any()
        assert (getattr(raw, name) == getattr(fresh, name)).all(), name
        assert all(not (getattr(raw, other).view(np.uint8) == 0x5A).all() for other in ("out", "purge", "weights", "raw", "counts",
                                                                                       "covered") if other != name), name
    raw.fill()


def test_argument_checks_leave_the_outputs_untouched():
    ctx = gpu_util.ctx()
    E = aln_amd.E_ARG
    K = 2
    hits, n_hits = aln_amd.search_topk(ctx, ARG_QS, ARG_TS, ALPHA, cc.TABLE, GI, GE, K)
    assert (n_hits == K).all()
    raw = Raw(K)
    assert raw.call(hits, n_hits) == 0 and not raw.untouched()
    assert not (raw.prows == 0x5A5A5A5A).any() and not (raw.counts == 0x5A5A5A5A).any() and not (raw.weights == 0x5A5A5A5A).any()
    raw.fill()

    def refused(want, what, **kw):
        assert raw.call(kw.pop("h_arr", hits), kw.pop("n_arr", n_hits), **kw) == want, what
        assert raw.untouched(), what

    bad_t = aln_amd.SeqPool(["HEAGAWGHEE", "PAW?EAE", "AWHE"]).c
    for kw in (dict(hits=None), dict(n_hits=None), dict(out=None)):
        refused(E, kw, **kw)
    for k in (0, 1025, -1):
        refused(E, ("K", k), K=k)
    refused(E, "K before the residues", K=0, templ=bad_t)
    for kw in (dict(q=None), dict(templ=None), dict(sub=None), dict(g=None)):
        refused(E, kw, **kw)
    refused(E, "q_begin < 0", q_begin=-1)
    refused(E, "q_end > n", q_end=3)
    refused(E, "gap model", g=cc.gap(model=aln_amd.GAP_AFFINE_TPOS_MIN))
    refused(aln_amd.E_RESIDUE, "a template letter outside the alphabet", templ=bad_t)
    spare = [ch for ch in ALPHA if all(ch not in s for s in ARG_QS + ARG_TS)][0]
    dot_sub = aln_amd.AlnSubmatrix(N, ALPHA.replace(spare, ".").encode(), raw.tab.ctypes.data_as(C.POINTER(C.c_float)))
    rule_and_slot_checks(raw, hits, n_hits, refused, bad_t, dict(sub=dot_sub))


def test_argument_checks_of_the_profile_entry():
    ctx = gpu_util.ctx()
    E = aln_amd.E_ARG
    K = 2
    profiles = pc.derived(ARG_QS, cc.TABLE)
    hits, n_hits = aln_amd.search_topk(ctx, ARG_QS, ARG_TS, ALPHA, cc.TABLE, GI, GE, K)
    raw = Raw(K, profiles=profiles)
    plain = Raw(K)
    assert raw.call(hits, n_hits) == 0 and plain.call(hits, n_hits) == 0
    for name in ("out", "prows", "purge", "weights", "raw", "counts", "covered"):
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
    for kw in (dict(n=0), dict(n=31), dict(alphabet=None), dict(rows=None)):
        refused(E, kw, prof=qprof(**kw))
    refused(E, "consensus n_seqs", cons=wrong_n)
    refused(aln_amd.E_RESIDUE, "a template letter outside the alphabet", templ=bad_t)
    spare = [ch for ch in ALPHA if all(ch not in s for s in ARG_QS + ARG_TS)][0]
    rule_and_slot_checks(raw, hits, n_hits, refused, bad_t, dict(prof=qprof(alphabet=ALPHA.replace(spare, ".").encode())))
    raw.fill()
    assert raw.call(hits, n_hits, cons=None) == 0
    for name in ("prows", "purge", "weights", "raw", "counts", "covered"):
        assert getattr(raw, name).tobytes() == getattr(plain, name).tobytes(), name


# ---- 8. iterate_search ------------------------------------------------------------------------------------------------------------------
def test_iterate_search_equals_the_chain_driven_by_hand():
    qs, ts = cc.homolog_set()
    assert len(qs) == 8 and len(ts) == 10
    ctx = gpu_util.ctx()
    K, rounds, beta, scale = 4, 3, 300, 2
    par = params(MIX, scale, beta)
    # by hand: search, hits_purge's counts, the restatement; stop where the template lists repeat
    chain, made, previous = [], [], None
    fallback = [p.astype(np.float32) for p in pc.derived(qs, cc.TABLE)]
    qp = None
    for _ in range(rounds):
        if qp is None:
            hits, n_hits = aln_amd.search_topk(ctx, qs, ts, ALPHA, cc.TABLE, GI, GE, K)
        else:
            hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, ts, GI, GE, K)
        chain.append((hits, n_hits))
        lists = [hits["t"][r, :n_hits[r]].tolist() for r in range(len(qs))]
        if lists == previous:
            break
        previous = lists
        if qp is None:
            counts = aln_amd.hits_purge(ctx, qs, ts, hits, n_hits, ALPHA, cc.TABLE, GI, GE, 90, 50)[4]
        else:
            counts = aln_amd.hits_purge_profiles(ctx, qp, ts, hits, n_hits, GI, GE, qs, 90, 50)[4]
        fallback = [aln_amd.pssm_rows_from_counts(counts[r][1:-1], BG, beta, scale, fallback[r], MIX) for r in range(len(qs))]
        made.append(fallback)
        qp = aln_amd.QueryProfiles(fallback, ALPHA)
    assert len(chain) >= 2 and any(not np.array_equal(a, b) for a, b in zip(made[0], pc.derived(qs, cc.TABLE)))
    for n_rounds in (1, 2, 3):
        found, profiles = aln_amd.iterate_search(ctx, qs, ts, ALPHA, cc.TABLE, GI, GE, K, n_rounds, par)
        want = chain[:n_rounds]
        assert len(found) == len(want), n_rounds
        for (h, n), (wh, wn) in zip(found, want):
            assert h.tobytes() == wh.tobytes() and n.tobytes() == wn.tobytes(), n_rounds
        last = made[min(n_rounds, len(made)) - 1]
        assert len(profiles) == len(qs) and profiles.alphabet == ALPHA
        assert all(p.tobytes() == w.tobytes() for p, w in zip(profiles.profiles, last)), n_rounds
    # the second round's hits are the dense reference's on the first round's rows
    first = [p.astype(np.int64) for p in made[0]]
    assert all(np.array_equal(a, b) for a, b in zip(first, made[0]))
    scores, ends = pc.dense_reference("pssm_two_rounds", first, ts, rc.LOCAL, GI, GE)
    hits2, n2 = chain[1]
    for r in range(len(qs)):
        order = sc.topk_reference(scores[r], K)
        assert n2[r] == len(order) and hits2["t"][r, :len(order)].tolist() == order, (r, hits2[r].tolist(), order)
        assert np.array_equal(hits2["score"][r, :len(order)].view(U32), scores[r, order].astype(np.float32).view(U32)), r
        assert np.array_equal(hits2["q_end"][r, :len(order)], ends[r, order, 0]), r
        assert np.array_equal(hits2["t_end"][r, :len(order)], ends[r, order, 1]), r
