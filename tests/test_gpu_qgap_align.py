"""-m gpu: aln_hits_align_profiles_gaps and aln_hits_column_counts_profiles_gaps — the hits of a search under position-specific
gap penalties aligned and tallied under the same rows (hit_local_qgaps_kernel / hit_global_qgaps_kernel,
csrc/search_align_qgaps.h).  Every comparison is exact: lists and lengths as integers, scores and identities as uint32, lines
and count blocks byte for byte.

  1  the anchor: constant rows give aln_hits_align_profiles / aln_hits_column_counts_profiles byte for byte, five align types
  2  varying rows against the int64 restatement of the definition (qgap_align_cases): lists, scores, lines, identity, and the
     path scorer on every list; the tie set; the ring and long shapes
  3  the final cell's pointer on pairs built for it
  4  local: the search's own hits round-trip, a score off by one, a score-0 hit
  5  pairs without an interior, and the routes
  6  plumbing: row blocks, the pool's end, duplicates, chunks, strides, alphabets, a consensus pool, NaN where nothing is read
  7  counts against column_count_cases.tally over the restated lists
  8  the refusals, in their order"""
import ctypes as C

import numpy as np
import pytest

import aln_amd
import column_count_cases as cc
import gpu_util
import profile_cases as pc
import qgap_align_cases as qa
import qgap_cases as qg
import range_cases as rc
import search_cases as sc

pytestmark = pytest.mark.gpu

U32 = np.uint32
ALPHA = sc.ALPHA
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
CONST_GAPS = ((11, 1), (4, 1), (1, 0))


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(U32)


def pool(profiles, alphabet=ALPHA):
    return aln_amd.QueryProfiles([np.asarray(p, np.float32) for p in profiles], alphabet)


def gap_pool(gaps):
    return aln_amd.QueryGaps(*[[g[w] for g in gaps] for w in range(4)])


def used_slots(n_hits, K):
    return [(r, k) for r in range(len(n_hits)) for k in range(K) if k < n_hits[r]]


def same_results(a, b):
    assert a[0].tobytes() == b[0].tobytes(), (a[0].tolist(), b[0].tolist())
    assert (a[1] is None) == (b[1] is None) and (a[2] is None) == (b[2] is None)
    if a[1] is not None:
        assert all(np.array_equal(x, y) for ra, rb in zip(a[1], b[1]) for x, y in zip(ra, rb))
    if a[2] is not None:
        assert a[2] == b[2] and a[3] == b[3] and np.array_equal(a[4], b[4])
    assert a[5] == b[5]


def same_counts(a, b):
    assert a[0].tobytes() == b[0].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))
    assert (a[2] is None and b[2] is None) or a[2].tobytes() == b[2].tobytes()
    assert a[3] == b[3]


def letters_of(profiles, consensus, alpha):
    return consensus if consensus is not None else [alpha[0] * len(p) for p in profiles]


def check_restated(res, hits, n_hits, profiles, gaps, ts, mode, consensus=None, alpha=ALPHA, q_begin=0, lines=True):
    """lists, scores, lines consistent with the lists, the identity, and the path scorer on every list"""
    rec, lists, tl, ql, lengths, rcode = res
    letters = letters_of(profiles, consensus, alpha)
    for r, k in used_slots(n_hits, hits.shape[1]):
        p, t, g = profiles[q_begin + r], ts[hits["t"][r, k]], gaps[q_begin + r]
        end = (hits["q_end"][r, k], hits["t_end"][r, k]) if mode == rc.LOCAL and len(p) and len(t) else None
        score, pl = qa.restated(p, t, mode, g, end=end, alpha=alpha)
        w = (mode, r, k, lists[r][k].tolist(), pl.tolist())
        assert rec["status"][r, k] == 0 and rec["n_pairs"][r, k] == len(pl), w
        assert np.array_equal(lists[r][k], pl), w
        assert u32(rec["score"][r, k]) == u32(score), (w, rec["score"][r, k], score)
        qa.check_path(p, t, mode, g, lists[r][k], int(rec["score"][r, k]), alpha)
        if len(p) and len(t):                                  # (without an interior min(Q, T) - 2 = 0: the anchor pins the bits)
            assert rec["identity"][r, k].view(U32) == gpu_util.identity_for(letters[q_begin + r], t, pl).view(U32), w
        if lines:
            t_line, q_lines, _ = gpu_util.strings_for(letters[q_begin + r], t, [pl])
            assert (tl[r][k], ql[r][k]) == (t_line, q_lines[0]) and lengths[r, k] == len(t_line), w
    assert rcode == 0


def search(ctx, qp, gp, ts, mode, K=None, **kw):
    hits, n_hits = aln_amd.search_topk_profiles_gaps(ctx, qp, gp, ts, len(ts) if K is None else K, align_type=mode, **kw)
    return hits, n_hits


# ---- 1. the anchor -----------------------------------------------------------------------------------------------------------------
def anchor_sets():
    profiles, ts = qg.small_set()
    tp, tq, tt, _ = qa.tie_set()
    return [(profiles, None, ts, ALPHA), (tp, tq, tt, qa.TIE_ALPHA)]


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
@pytest.mark.parametrize("gi,ge", CONST_GAPS)
def test_constant_rows_equal_the_constant_gap_entries(gi, ge, mode):
    ctx = gpu_util.ctx()
    for profiles, consensus, ts, alpha in anchor_sets():
        qp = pool(profiles, alpha)
        gp = aln_amd.QueryGaps.constant(qp, gi, ge)
        hits, n_hits = aln_amd.search_topk_profiles(ctx, qp, ts, gi, ge, len(ts), align_type=mode)
        want = aln_amd.hits_align_profiles(ctx, qp, ts, hits, n_hits, gi, ge, consensus=consensus, align_type=mode)
        got = aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, consensus=consensus, align_type=mode)
        same_results(got, want)
        assert aln_amd.hits_align_routes(ctx) == (int(n_hits.sum()), 0)
        assert (got[0]["status"] == 0).all()
        want = aln_amd.hits_column_counts_profiles(ctx, qp, ts, hits, n_hits, gi, ge, consensus=consensus, align_type=mode)
        got = aln_amd.hits_column_counts_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, consensus=consensus, align_type=mode)
        same_counts(got, want)
        assert sum(int(c.sum()) for c in got[1]) > 0


# ---- 2. against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
@pytest.mark.parametrize("kind", qg.SMALL_KINDS)
def test_varied_rows(kind, mode):
    profiles, ts = qg.small_set()
    gaps = qg.small_gaps(kind, profiles)
    ctx = gpu_util.ctx()
    qp, gp = pool(profiles), gap_pool(gaps)
    hits, n_hits = search(ctx, qp, gp, ts, mode)
    res = aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, align_type=mode)
    check_restated(res, hits, n_hits, profiles, gaps, ts, mode)
    if mode == rc.LOCAL:
        assert np.array_equal(u32(res[0]["score"]), u32(hits["score"]))


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_tie_set(mode):
    profiles, qs, ts, gaps = qa.tie_set()
    ctx = gpu_util.ctx()
    qp, gp = pool(profiles, qa.TIE_ALPHA), gap_pool(gaps)
    hits, n_hits = search(ctx, qp, gp, ts, mode)
    res = aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, consensus=qs, align_type=mode)
    check_restated(res, hits, n_hits, profiles, gaps, ts, mode, consensus=qs, alpha=qa.TIE_ALPHA)


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_ring_set(mode):
    """profiles of 6, 7, 8, 9, 31, 32, 33 rows x T = 3, 256, 257, 258: the 8-row chunks, the 32-row ring, classes 1 and 2"""
    profiles, gaps, ts = qg.ring_set()
    ctx = gpu_util.ctx()
    qp, gp = pool(profiles), gap_pool(gaps)
    hits, n_hits = search(ctx, qp, gp, ts, mode)
    res = aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, align_type=mode)
    check_restated(res, hits, n_hits, profiles, gaps, ts, mode)
    assert aln_amd.hits_align_routes(ctx) == (len(profiles) * len(ts), 0)


@pytest.mark.parametrize("mode", (rc.LOCAL, rc.GLOBAL))
def test_long_set(mode):
    """300 rows (nine ring revolutions) and T = 2048 (class 8); global prices both ends by rows 0 and Q-2"""
    ctx = gpu_util.ctx()
    for profiles, gaps, ts in qg.long_set():
        qp, gp = pool(profiles), gap_pool(gaps)
        hits, n_hits = search(ctx, qp, gp, ts, mode)
        res = aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, align_type=mode)
        check_restated(res, hits, n_hits, profiles, gaps, ts, mode)
        assert aln_amd.hits_align_routes(ctx) == (len(profiles) * len(ts), 0)


# ---- 3. the final cell's pointer -----------------------------------------------------------------------------------------------------
def test_final_pointer_cases():
    """a deletion priced by row Q-2 alone, an insertion whose winner one ins_extn[p] moves, a free-tail tie the smallest row wins
    (tests/test_qgap_align_reference.py checks that the pairs are what they are built for)"""
    ctx = gpu_util.ctx()
    for p, g, t, mode, what in qa.final_pointer_cases():
        qp, gp = pool([p]), gap_pool([g])
        hits, n_hits = search(ctx, qp, gp, [t], mode)
        res = aln_amd.hits_align_profiles_gaps(ctx, qp, gp, [t], hits, n_hits, align_type=mode)
        check_restated(res, hits, n_hits, [p], [g], [t], mode)


# ---- 4. local ------------------------------------------------------------------------------------------------------------------------
def test_local_score_checks():
    profiles, ts = qg.small_set()
    gaps = qg.small_gaps("random", profiles)
    ctx = gpu_util.ctx()
    qp, gp = pool(profiles), gap_pool(gaps)
    hits, n_hits = search(ctx, qp, gp, ts, rc.LOCAL)
    good = aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, hits, n_hits)
    assert (good[0]["status"] == 0).all() and good[5] == 0          # the search's own hits round-trip: no slot is refused
    bad = hits.copy()
    bad["score"][1, 1] += 1
    res = aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, bad, n_hits)
    assert res[5] == aln_amd.E_ARG
    assert res[0][1, 1].tolist() == (0, aln_amd.E_ARG, 0.0, 0.0) and len(res[1][1][1]) == 0 and res[2][1][1] == "" and res[4][1, 1] == 0
    keep = np.ones(hits.shape, bool)
    keep[1, 1] = False
    assert res[0][keep].tobytes() == good[0][keep].tobytes() and np.array_equal(res[4][keep], good[4][keep])
    assert all(np.array_equal(res[1][r][k], good[1][r][k]) and res[2][r][k] == good[2][r][k] for r, k in zip(*np.nonzero(keep)))
    cnt = aln_amd.hits_column_counts_profiles_gaps(ctx, qp, gp, ts, bad, n_hits)
    assert cnt[3] == aln_amd.E_ARG and cnt[0].tobytes() == res[0].tobytes() == aln_amd.hits_align_profiles_gaps(
        ctx, qp, gp, ts, bad, n_hits, want_pairs=False, want_lines=False)[0].tobytes()
    # a score-0 hit: a profile that likes nothing; the seed cell's list
    zero = [np.full((7, pc.N), -3, np.int64)]
    zg = [qg.random_rows(7, 5)]
    zp, zgp = pool(zero), gap_pool(zg)
    hits, n_hits = search(ctx, zp, zgp, ts, rc.LOCAL)
    assert (hits["score"] == 0).all()
    res = aln_amd.hits_align_profiles_gaps(ctx, zp, zgp, ts, hits, n_hits)
    check_restated(res, hits, n_hits, zero, zg, ts, rc.LOCAL)
    for k in range(len(ts)):
        T = len(ts[hits["t"][0, k]]) + 2
        assert res[1][0][k][-2:].tolist() == [[7, T - 2], [8, T - 1]]
    cnt = aln_amd.hits_column_counts_profiles_gaps(ctx, zp, zgp, ts, hits, n_hits)
    assert int(cnt[1][0].sum()) == 0 and int(cnt[2].sum()) == 0      # a score-0 local list contributes nothing


# ---- 5. pairs without an interior ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_pairs_without_an_interior(mode):
    """Q = 2, T = 2 and both: the score is the definition's, the list the anchor's; the routes say who filed what"""
    rng = np.random.RandomState(77)
    profiles = [np.zeros((0, pc.N), np.int64), rng.randint(-4, 10, (5, pc.N)).astype(np.int64), rng.randint(-4, 10, (1, pc.N)).astype(np.int64)]
    ts = ["", "ACDWY", "W"]
    gaps = [qg.random_rows(len(p), 70 + s, 1, 9) for s, p in enumerate(profiles)]
    ctx = gpu_util.ctx()
    qp, gp = pool(profiles), gap_pool(gaps)
    hits, n_hits = search(ctx, qp, gp, ts, mode)
    assert (n_hits == 3).all()
    res = aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, align_type=mode)
    assert aln_amd.hits_align_routes(ctx) == (4, 5)
    check_restated(res, hits, n_hits, profiles, gaps, ts, mode)
    fdel, fins = rc.free_ends(mode)
    for r, k in used_slots(n_hits, 3):
        t = ts[hits["t"][r, k]]
        if len(profiles[r]) == 0:
            want = 0 if (fdel or not t) else -(gaps[r][0][0] + gaps[r][1][0] * (len(t) - 1))
        elif not t:
            want = 0 if fins else -(gaps[r][2][1] + sum(gaps[r][3][2:]))
        else:
            continue
        assert res[0]["score"][r, k] == want and u32(res[0]["score"][r, k]) == u32(float(want)), (mode, r, k)
    cnt = aln_amd.hits_column_counts_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, align_type=mode)
    assert aln_amd.hits_align_routes(ctx) == (4, 5)
    assert cnt[0].tobytes() == aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, align_type=mode, want_pairs=False,
                                                               want_lines=False)[0].tobytes()
    # the anchor pins the list, the lines and the record's every bit of such pairs
    for gi, ge in CONST_GAPS:
        cgp = aln_amd.QueryGaps.constant(qp, gi, ge)
        h2, n2 = aln_amd.search_topk_profiles(ctx, qp, ts, gi, ge, 3, align_type=mode)
        want = aln_amd.hits_align_profiles(ctx, qp, ts, h2, n2, gi, ge, align_type=mode)
        assert aln_amd.hits_align_routes(ctx) == (4, 5)
        same_results(aln_amd.hits_align_profiles_gaps(ctx, qp, cgp, ts, h2, n2, align_type=mode), want)
        same_counts(aln_amd.hits_column_counts_profiles_gaps(ctx, qp, cgp, ts, h2, n2, align_type=mode),
                    aln_amd.hits_column_counts_profiles(ctx, qp, ts, h2, n2, gi, ge, align_type=mode))


# ---- 6. plumbing ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (rc.LOCAL, rc.GLOBAL))
def test_plumbing(mode):
    profiles, gaps, ts = qg.ring_set()
    profiles, gaps = profiles[:5], gaps[:5]
    ts = ts[:2] + [ts[1][:40], ts[3][10:90]]
    consensus = [rc.random_seq(ALPHA, 600 + s, len(p)) for s, p in enumerate(profiles)]
    ctx = gpu_util.ctx()
    qp, gp = pool(profiles), gap_pool(gaps)
    hits, n_hits = search(ctx, qp, gp, ts, mode, K=3)
    hits[2, 2] = hits[2, 0]                                     # a duplicate slot
    n_hits[3] = 1                                               # unused slots
    whole = aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, consensus=consensus, align_type=mode)
    check_restated(whole, hits, n_hits, profiles, gaps, ts, mode, consensus=consensus)
    assert whole[0][3, 1:].tobytes() == bytes(32) and whole[2][3][1] == "" and len(whole[1][3][2]) == 0
    cwhole = aln_amd.hits_column_counts_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, consensus=consensus, align_type=mode)
    # chunks of one hit, rows per chunk, the hint that has nothing to switch to
    for hint in (dict(align_chunk_hits=1), dict(align_rows_per_chunk=1), dict(align_chunk_hits=2, align_rows_per_chunk=1),
                 dict(align_fused_nonlocal=0)):
        with ctx.hints(**hint):
            same_results(aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, consensus=consensus, align_type=mode), whole)
            assert aln_amd.hits_align_routes(ctx) == (int(n_hits.sum()), 0)
            same_counts(aln_amd.hits_column_counts_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, consensus=consensus, align_type=mode), cwhole)
    # row blocks; the last profile at the pool's end
    n = len(profiles)
    for a, b in ((1, 3), (n - 1, n), (0, 1)):
        part = aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, hits[a:b], n_hits[a:b], consensus=consensus, q_begin=a, align_type=mode)
        assert part[0].tobytes() == whole[0][a:b].tobytes() and part[2] == whole[2][a:b] and part[3] == whole[3][a:b]
        assert all(np.array_equal(x, y) for ra, rb in zip(part[1], whole[1][a:b]) for x, y in zip(ra, rb))
        cpart = aln_amd.hits_column_counts_profiles_gaps(ctx, qp, gp, ts, hits[a:b], n_hits[a:b], consensus=consensus, q_begin=a, align_type=mode)
        assert cpart[0].tobytes() == cwhole[0][a:b].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(cpart[1], cwhole[1][a:b]))
    # the output groups alone
    only = aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, consensus=consensus, align_type=mode, want_pairs=False, want_lines=False)
    assert only[0].tobytes() == whole[0].tobytes() == cwhole[0].tobytes() and only[1] is None and only[2] is None
    # a pair_stride that is too short: the first entries are written; a line_stride that is too short: empty lines
    longest = int(whole[0]["n_pairs"].max())
    short = aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, consensus=consensus, align_type=mode, pair_stride=longest - 1)
    assert short[5] == aln_amd.E_OVERFLOW
    for r, k in used_slots(n_hits, 3):
        over = whole[0]["n_pairs"][r, k] > longest - 1
        assert short[0]["status"][r, k] == (aln_amd.E_OVERFLOW if over else 0) and short[0]["n_pairs"][r, k] == whole[0]["n_pairs"][r, k]
        assert np.array_equal(short[1][r][k], whole[1][r][k][:longest - 1])
    widest = int(whole[4].max())
    short = aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, consensus=consensus, align_type=mode, line_stride=widest)
    assert short[5] == aln_amd.E_OVERFLOW
    for r, k in used_slots(n_hits, 3):
        over = whole[4][r, k] >= widest
        assert short[0]["status"][r, k] == (aln_amd.E_OVERFLOW if over else 0)
        assert (short[2][r][k], short[4][r, k]) == (("", 0) if over else (whole[2][r][k], whole[4][r, k]))
    # NaN in every entry that is never read: del_* at the '$' rows, ins_* at rows 0 and Q-1
    nan = gap_pool(gaps)
    for s in range(n):
        o, e = int(qp.offsets[s]), int(qp.offsets[s + 1]) - 1
        nan.del_init[e] = nan.del_extn[e] = nan.ins_init[e] = nan.ins_extn[e] = nan.ins_init[o] = nan.ins_extn[o] = np.nan
    same_results(aln_amd.hits_align_profiles_gaps(ctx, qp, nan, ts, hits, n_hits, consensus=consensus, align_type=mode), whole)
    same_counts(aln_amd.hits_column_counts_profiles_gaps(ctx, qp, nan, ts, hits, n_hits, consensus=consensus, align_type=mode), cwhole)
    # an empty block writes nothing
    none = aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, hits[2:2], n_hits[2:2], q_begin=2, align_type=mode)
    assert none[0].shape == (0, 3) and none[5] == 0


@pytest.mark.parametrize("n", (1, 20, 26))
def test_alphabet_sizes(n):
    alphabet = (ALPHA + "JO")[:n] if n > 1 else "A"
    rng = np.random.RandomState(1100 + n)
    profiles = [rng.randint(-4, 10, (L, n)).astype(np.int64) for L in (7, 12)]
    ts = ["".join(alphabet[k] for k in rng.randint(0, n, m)) for m in (9, 14)] + [alphabet[-1] * 8]
    gaps = [qg.random_rows(len(p), 1110 + n + s, 0, 6) for s, p in enumerate(profiles)]
    ctx = gpu_util.ctx()
    qp, gp = pool(profiles, alphabet), gap_pool(gaps)
    for mode in (rc.LOCAL, rc.GLOBAL):
        hits, n_hits = search(ctx, qp, gp, ts, mode)
        res = aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, align_type=mode)
        check_restated(res, hits, n_hits, profiles, gaps, ts, mode, alpha=alphabet)
        cnt = aln_amd.hits_column_counts_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, align_type=mode)
        assert cnt[1][0].shape == (9, n) and cnt[0].tobytes() == res[0].tobytes()
        if mode == rc.GLOBAL:                                  # the last template is the last letter alone: its column counts
            assert int(cnt[1][0][:, n - 1].sum()) > 0


# ---- 7. counts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_counts_equal_the_tally_over_the_restated_lists(mode):
    profiles, ts = qg.small_set()
    gaps = qg.small_gaps("random", profiles)
    ctx = gpu_util.ctx()
    qp, gp = pool(profiles), gap_pool(gaps)
    hits, n_hits = search(ctx, qp, gp, ts, mode)
    K = hits.shape[1]
    slots = used_slots(n_hits, K)
    lists = []
    for r, k in slots:
        end = (hits["q_end"][r, k], hits["t_end"][r, k]) if mode == rc.LOCAL else None
        lists.append(qa.restated(profiles[r], ts[hits["t"][r, k]], mode, gaps[r], end=end))
    weights = np.random.RandomState(5).randint(0, 4, hits.shape).astype(np.int32)
    weights[0, 0] = 65535
    for w in (None, weights):
        rec, counts, covered, rcode = aln_amd.hits_column_counts_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, weights=w, align_type=mode)
        assert rcode == 0
        want_counts, want_covered = cc.tally([len(p) for p in profiles], ts, [(r, int(hits["t"][r, k])) for r, k in slots], lists,
                                             [1 if w is None else int(w[r, k]) for r, k in slots], mode == rc.LOCAL)
        for r in range(len(profiles)):
            assert np.array_equal(counts[r], want_counts[r]), (mode, r)
        assert np.array_equal(covered, want_covered), mode
        assert sum(int(c.sum()) for c in counts) > 0
        with ctx.hints(align_chunk_hits=1):
            again = aln_amd.hits_column_counts_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, weights=w, align_type=mode)
        same_counts(again, (rec, counts, covered, rcode))
        no_cov = aln_amd.hits_column_counts_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, weights=w, align_type=mode, want_covered=False)
        assert no_cov[2] is None and all(x.tobytes() == y.tobytes() for x, y in zip(no_cov[1], counts))
    rec2 = aln_amd.hits_align_profiles_gaps(ctx, qp, gp, ts, hits, n_hits, align_type=mode, want_pairs=False, want_lines=False)[0]
    assert rec.tobytes() == rec2.tobytes()


# ---- 8. the refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order_leave_the_outputs_untouched():
    L = aln_amd.lib()
    ctx = gpu_util.ctx()
    E = aln_amd
    qp = pool([np.ones((3, pc.N)), np.ones((5, pc.N))])
    ok = aln_amd.QueryGaps.constant(qp, 11, 1)
    tp = aln_amd.SeqPool(["WWW", "AC"])
    good_hits = np.zeros((2, 2), dtype=aln_amd.HIT_DTYPE)
    good_hits["t"], good_hits["q_end"], good_hits["t_end"], good_hits["score"] = [[0, 1], [1, 0]], 1, 1, 1
    good_n = np.full(2, 2, np.int32)
    FILL, W = 0x5A, 0x5A5A5A5A
    NULL = object()

    def both(want, prof=None, gaps=ok, cons=None, templ=tp, mode=aln_amd.LOCAL, qb=0, qe=2, K=2, hits=good_hits, n_hits=good_n, out=True,
             pair_stride=8, lines=(True, True), line_stride=16, weights=None, what=None, only=None):
        prof = qp.c if prof is None else prof
        g = gaps.c if isinstance(gaps, aln_amd.QueryGaps) else gaps
        ref = lambda x: None if x is NULL else C.byref(x)
        rec = np.frombuffer(bytearray([FILL]) * (4 * 16), dtype=aln_amd.HIT_ALIGNMENT_DTYPE).copy()
        pairs = np.full((4, 8, 2), W, np.int32)
        tl, ql = C.create_string_buffer(bytes([FILL]) * 64, 64), C.create_string_buffer(bytes([FILL]) * 64, 64)
        lengths = np.full(4, W, np.int32)
        counts, covered = np.full((12, pc.N), W, np.int32), np.full(12, W, np.int32)
        hp = None if hits is NULL else np.ascontiguousarray(hits).ctypes.data_as(C.POINTER(aln_amd.AlnHit))
        np_ = None if n_hits is NULL else np.ascontiguousarray(n_hits, np.int32).ctypes.data_as(_ip)
        recp = rec.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)) if out else None
        lead = (ctx.h, ref(prof), ref(g), None if cons is None else C.byref(cons.c), ref(templ if templ is NULL else templ.c), mode, qb, qe, K, hp, np_)
        rcs = []
        if only != "counts":
            rcs.append(L.aln_hits_align_profiles_gaps(*lead, recp, pairs.ctypes.data_as(_ip), pair_stride, tl if lines[0] else None,
                                                      ql if lines[1] else None, line_stride, lengths.ctypes.data_as(_ip)))
        if only != "align":
            wp = None if weights is None else np.ascontiguousarray(weights, np.int32).ctypes.data_as(_ip)
            rcs.append(L.aln_hits_column_counts_profiles_gaps(*lead, wp, recp, counts.ctypes.data_as(_ip), covered.ctypes.data_as(_ip)))
        assert all(r == want for r in rcs), (what, rcs, want)
        assert rec.tobytes() == bytes([FILL]) * 64 and (pairs == W).all() and tl.raw == bytes([FILL]) * 64 and ql.raw == bytes([FILL]) * 64, what
        assert (lengths == W).all() and (counts == W).all() and (covered == W).all(), what

    def qprof(n, alphabet):
        rows = np.ones((int(qp.offsets[-1]), n), np.float32)
        d = aln_amd.AlnQProfiles(qp.c.n_seqs, qp.c.offsets, rows.ctypes.data_as(_fp), n, alphabet)
        d.keep = rows
        return d

    def varied(which, row, value):
        g = aln_amd.QueryGaps.constant(qp, 11, 1)
        getattr(g, which)[row] = value
        return g

    def slots(**kw):
        h = good_hits.copy()
        for k, v in kw.items():
            h[k][1, 1] = v
        return h

    bad_t = aln_amd.SeqPool(["WWW", "A?"])
    long_t = aln_amd.SeqPool(["WWW", "A" * 2100])
    n27 = qprof(27, (ALPHA + "JOU").encode())
    null_array = aln_amd.AlnQGaps(ok.c.del_init, ok.c.del_extn, None, ok.c.ins_extn)
    negative, fraction = varied("del_extn", 1, -1), varied("ins_init", 2, 2.5)
    frac_rows = pool([np.full((3, pc.N), 0.5), np.ones((5, pc.N))])
    bad_cons = aln_amd.SeqPool(["AAA"])                            # one sequence for two profiles
    bad_slot = slots(t=2)
    # 1. NULL pointers, K and the output groups come first: before the align type, the descriptor, everything
    both(E.E_ARG, prof=NULL, mode=5, what="NULL profiles")
    both(E.E_ARG, gaps=NULL, what="NULL gaps")
    both(E.E_ARG, templ=NULL, what="NULL templates")
    both(E.E_ARG, hits=NULL, what="NULL hits")
    both(E.E_ARG, n_hits=NULL, what="NULL n_hits")
    both(E.E_ARG, out=False, what="NULL out")
    both(E.E_ARG, K=0, templ=bad_t, what="K = 0 comes before the letters")
    both(E.E_ARG, K=1025, what="K = 1025")
    both(E.E_ARG, pair_stride=1, templ=bad_t, only="align", what="pair_stride 1")
    both(E.E_ARG, lines=(True, False), templ=long_t, only="align", what="the line group in part")
    both(E.E_ARG, line_stride=0, only="align", what="line_stride 0")
    # 2. the search entry's checks in its order, the consensus pool directly after the profile descriptor
    both(E.E_ARG, qb=1, qe=3, what="the row range")
    both(E.E_ARG, mode=5, what="align type")
    both(E.E_ARG, cons=bad_cons, templ=bad_t, what="the consensus pool comes before the letters")
    both(E.E_ARG, cons=bad_cons, gaps=fraction, what="the consensus pool comes before the gap values")
    both(E.E_ARG, prof=n27, templ=bad_t, what="n = 27 comes before the letters")
    both(E.E_ARG, gaps=null_array, templ=bad_t, what="a NULL array comes before the letters")
    both(E.E_RESIDUE, templ=bad_t, gaps=negative, hits=bad_slot, what="the letters come before the gap values and the slots")
    both(E.E_TOO_LONG, templ=long_t, gaps=negative, what="2100 residues, before the gap values")
    both(E.E_ARG, gaps=negative, prof=frac_rows.c, what="a negative gap comes before a fractional row entry")
    both(E.E_NOT_INTEGRAL, gaps=fraction, hits=bad_slot, what="a fractional gap comes before the slots")
    both(E.E_NOT_INTEGRAL, prof=frac_rows.c, hits=bad_slot, what="a fractional row entry comes before the slots")
    # 3. the slots: n_hits, t, the local end cell
    both(E.E_ARG, n_hits=np.array([2, 3], np.int32), what="n_hits above K")
    both(E.E_ARG, n_hits=np.array([-1, 2], np.int32), what="n_hits below 0")
    both(E.E_ARG, hits=bad_slot, what="t out of range")
    both(E.E_ARG, hits=slots(t=-1), what="t below 0")
    both(E.E_ARG, hits=slots(q_end=0), what="q_end 0")
    both(E.E_ARG, hits=slots(q_end=6), what="q_end Q-1")
    both(E.E_ARG, hits=slots(t_end=4), what="t_end T-1")
    both(E.E_ARG, weights=[[1, 1], [1, 65536]], only="counts", what="a weight above 65535")
    both(E.E_ARG, weights=[[1, -1], [1, 1]], only="counts", what="a negative weight")
    # a slot beyond n_hits is not read; the non-local types do not read the end cell; an empty block writes nothing
    h = slots(t=99, q_end=-5)
    res = aln_amd.hits_align_profiles_gaps(ctx, qp, ok, tp, h, np.array([2, 1], np.int32))
    assert res[5] in (0, E.E_ARG) and res[0]["n_pairs"][1, 1] == 0
    res = aln_amd.hits_align_profiles_gaps(ctx, qp, ok, tp, slots(q_end=-5, t_end=1 << 20), good_n, align_type=aln_amd.GLOBAL)
    assert res[5] == 0 and (res[0]["status"] == 0).all()
    both(0, qb=1, qe=1, what="empty block")
