"""-m gpu: aln_score_profiles_gaps_vs_all and aln_search_topk_profiles_gaps — scoring and search for profiles whose rows carry
their own gap penalties (aln_qgaps) — through ctypes, scores compared as uint32 patterns.

  1  the anchor: constant rows give aln_score_profiles_vs_all / aln_search_topk_profiles byte for byte, five align types
  2  varying rows against the int64 restatement of the definition (qgap_cases): each array alone, all four, a free loop, a
     wall of 500, the chunk and ring boundaries of the kernels' staging, T = 3, 256, 257, 258, 2048, rows 0 and Q-2
  3  an independent oracle: the transposed pair through aln_batch_dp with ALN_GAP_TABLES
  4  plumbing: row blocks, slabs, K, min_score, alphabets of 1, 20 and 26 letters
  5  the refusals, in their order"""
import ctypes as C

import numpy as np
import pytest

import aln_amd
import gpu_util
import profile_cases as pc
import qgap_cases as qg
import range_cases as rc
import search_cases as sc

pytestmark = pytest.mark.gpu

U32 = np.uint32
ALPHA = sc.ALPHA
_fp = C.POINTER(C.c_float)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(U32)


def pool(profiles, alphabet=ALPHA):
    return aln_amd.QueryProfiles([np.asarray(p, np.float32) for p in profiles], alphabet)


def gap_pool(gaps):
    """gaps[s]: the four sequences of profile s (qgap_cases) -> aln_amd.QueryGaps"""
    return aln_amd.QueryGaps(*[[g[w] for g in gaps] for w in range(4)])


def check_hits(hits, n_hits, scores, ends, K, min_score=-np.inf, what=None):
    """the header's selection (score >= min_score, score descending, ties by template index, at most K), the score's bits,
    the end cell, the padding {-1, 0, -1, -1}"""
    rows = scores.shape[0]
    assert hits.shape == (rows, K) and n_hits.shape == (rows,), what
    for r in range(rows):
        order = sc.topk_reference(scores[r], K, min_score)
        n = len(order)
        w = (what, r, K, hits[r].tolist(), order)
        assert n_hits[r] == n, w
        assert hits["t"][r, :n].tolist() == order, w
        assert np.array_equal(u32(hits["score"][r, :n]), u32(scores[r, order])), w
        assert np.array_equal(hits["q_end"][r, :n], ends[r, order, 0]) and np.array_equal(hits["t_end"][r, :n], ends[r, order, 1]), w
        pad = hits[r, n:]
        assert (pad["t"] == -1).all() and (u32(pad["score"]) == 0).all() and (pad["q_end"] == -1).all() and (pad["t_end"] == -1).all(), w


def check_set(key, profiles, gaps, ts, mode, Ks, min_scores=(-np.inf,)):
    """scores and searches of a whole set against the restatement -> (reference scores, end cells)"""
    ctx = gpu_util.ctx()
    scores, ends = qg.dense_reference(key, profiles, gaps, ts, mode)
    qp, gp = pool(profiles), gap_pool(gaps)
    got = aln_amd.score_profiles_gaps_vs_all(ctx, qp, gp, ts, align_type=mode)
    print(key, mode, "scores differ in", int((u32(got) != u32(scores)).sum()), "of", got.size)
    assert np.array_equal(u32(got), u32(scores)), (key, mode, np.argwhere(u32(got) != u32(scores))[:8].tolist())
    for K in Ks:
        for ms in min_scores:
            hits, n_hits = aln_amd.search_topk_profiles_gaps(ctx, qp, gp, ts, K, min_score=ms, align_type=mode)
            check_hits(hits, n_hits, scores, ends, K, ms, what=(key, mode, K, ms))
    return scores, ends


# ---- 1. the anchor ------------------------------------------------------------------------------------------------------------------
def check_anchor(profiles, ts, gi, ge, mode, Ks):
    ctx = gpu_util.ctx()
    qp = pool(profiles)
    gp = aln_amd.QueryGaps.constant(qp, gi, ge)
    want = aln_amd.score_profiles_vs_all(ctx, qp, ts, gi, ge, align_type=mode)
    got = aln_amd.score_profiles_gaps_vs_all(ctx, qp, gp, ts, align_type=mode)
    assert got.tobytes() == want.tobytes(), (mode, np.argwhere(u32(got) != u32(want))[:8].tolist())
    for K in Ks:
        hw, nw = aln_amd.search_topk_profiles(ctx, qp, ts, gi, ge, K, align_type=mode)
        hg, ng = aln_amd.search_topk_profiles_gaps(ctx, qp, gp, ts, K, align_type=mode)
        assert hg.tobytes() == hw.tobytes() and np.array_equal(ng, nw), (mode, K)


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_constant_rows_equal_the_constant_gap_entries(mode):
    """profile_cases.length_set: templates of 254 / 255 residues across the class boundary, empty and two-residue templates,
    duplicates for the tie order, profiles without interior rows"""
    profiles, ts = pc.length_set()
    _, gi, ge = pc.LENGTH_SYSTEM
    check_anchor(profiles, ts, gi, ge, mode, sc.KS)


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
@pytest.mark.parametrize("system", sc.WIDE_SYSTEMS, ids=lambda s: s[0])
def test_constant_rows_on_wide_templates(system, mode):
    """length classes 6, 7, 8 and the 300-row profile that goes round the ring nine times"""
    tname, gi, ge = system
    profiles, ts = pc.wide_set(sc.TABLES[tname])
    assert [len(p) for p in profiles] == [40, 40, 300]
    check_anchor(profiles, ts, gi, ge, mode, (3, len(ts)))


# ---- 2. varying rows against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
@pytest.mark.parametrize("kind", qg.SMALL_KINDS)
def test_varied_rows(kind, mode):
    profiles, ts = qg.small_set()
    gaps = qg.small_gaps(kind, profiles)
    scores, _ = check_set("small-" + kind, profiles, gaps, ts, mode, (2, len(ts)))
    if kind in ("free_loop", "wall"):
        # the special row matters: the same set under the kind's constant rows scores differently somewhere
        gi = 11 if kind == "free_loop" else 4
        plain = [qg.constant(len(p), gi, 1) for p in profiles]
        base, _ = qg.dense_reference("small-plain-%d" % gi, profiles, plain, ts, mode)
        assert (scores != base).any(), (kind, mode)
        if kind == "wall":
            assert (scores <= base).all() and (base - scores < 500).all()     # dearer, and the optimum routes around the 500


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_rows_differing_across_chunks_and_the_ring(mode):
    """6 .. 9 and 31 .. 33 interior rows (8-row chunks, 32-row ring) x T = 3, 256, 257, 258 columns (classes 1 and 2)"""
    profiles, gaps, ts = qg.ring_set()
    assert [len(p) for p in profiles] == [6, 7, 8, 9, 31, 32, 33] and [len(t) + 2 for t in ts] == [3, 256, 257, 258]
    check_set("ring", profiles, gaps, ts, mode, (len(ts),))


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_rows_of_a_long_profile_and_a_class_8_template(mode):
    (p300, g300, t_short), (p_short, g_short, t_long) = qg.long_set()
    assert len(p300[0]) == 300 and len(t_long[0]) + 2 == 2048
    check_set("long-q", p300, g300, t_short, mode, (len(t_short),))
    check_set("long-t", p_short, g_short, t_long, mode, (1,))


@pytest.mark.parametrize("mode", (rc.GLOBAL, rc.GLOBAL_LOCAL))
@pytest.mark.parametrize("row", ("first", "last"))
def test_rows_0_and_q_minus_2_price_the_end_deletions(row, mode):
    """deletions at the template's ends are priced in both align types.  The template carries the profile's sequence between
    two runs the profile scores badly, so the optimum opens with a head deletion and closes with a tail deletion; changing only
    row 0's (row Q-2's) del_* changes the score"""
    seq = rc.random_seq(ALPHA, 970, 8)
    profile = pc.derived([seq], sc.TABLES["blosum62"])[0]
    t = "W" * 5 + seq + "W" * 4
    L = len(profile)
    base = qg.constant(L, 11, 1)
    moved = [list(a) for a in base]
    at = 0 if row == "first" else L
    moved[0][at], moved[1][at] = 2, 0
    a, _ = check_set("ends-base", [profile], [base], [t], mode, (1,))
    b, _ = check_set("ends-" + row, [profile], [moved], [t], mode, (1,))
    assert a[0, 0] != b[0, 0], (row, mode, int(a[0, 0]))


# ---- 3. an independent oracle: the transposed pair under ALN_GAP_TABLES ---------------------------------------------------------------
SWAP = {rc.GLOBAL_LOCAL: rc.LOCAL_GLOBAL, rc.LOCAL_GLOBAL: rc.GLOBAL_LOCAL}


def transposed_tables(Q, T, mode, g):
    """The profile as the batch's TEMPLATE (Q positions), the sequence as its QUERY (T positions).  The batch's deletion(t1, t2)
    skips profile positions t1+1 .. t2-1 — our ins(t1+1, t2-1); its insertion between template positions t1 and t1+1 skips
    sequence residues — our del(t1, .).  End rules as the definition states them."""
    di, de, ni, ne = g
    fdel, fins = rc.free_ends(mode)
    INS = qg.ins_table(qg.with_tail(ni), qg.with_tail(ne), Q)
    D = np.zeros((Q, Q), np.float32)
    for t1 in range(Q):
        for t2 in range(t1 + 2, Q):
            end = t1 == 0 or t2 == Q - 1
            D[t1, t2] = 0 if (end and fins) else INS[t1 + 1][t2 - 1]
    dele = lambda i, L: 0 if L < 1 else di[i] + de[i] * (L - 1)
    I = np.zeros((3, Q, T), np.float32)
    for t1 in range(Q - 1):
        for d in range(1, T - 2):
            I[0, t1, d] = dele(t1, d - 1)
        for q2 in range(1, T):
            I[1, t1, q2] = 0 if fdel else dele(t1, q2 - 1)
        for q1 in range(0, T - 1):
            I[2, t1, q1] = 0 if fdel else dele(t1, T - 2 - q1)
    return D, I


def transposed_score(profile, t, mode, g):
    ctx = gpu_util.ctx()
    Q, T = len(profile) + 2, len(t) + 2
    D, I = transposed_tables(Q, T, mode, g)
    b = aln_amd.Batch(ctx, [t], [ALPHA[0] * len(profile)], [0], [0])
    try:
        b.dp_simmatrix([pc.plane(profile, t).T.astype(np.float32)], SWAP.get(mode, mode), 0, 0, del_tables=[D], ins_tables=[I])
        scores, _, status = b.optimal(want_pairs=False)
    finally:
        b.close()
    assert not status.any()
    return int(scores[0])


@pytest.mark.parametrize("mode", rc.ALIGN_TYPES)
def test_transposed_batch_under_gap_tables(mode):
    """Q, T <= 12, one pair per align type, scores only.  At constant rows the restatement is already pinned to the existing
    entries (test_qgap_reference.py), so the transposed build is checked there first; then under random rows it must give
    what the new entry gives."""
    profiles, ts = qg.homolog_set((9,), (10,), 980 + mode)
    p, t = profiles[0], ts[0]
    ctx = gpu_util.ctx()
    flat = qg.constant(len(p), 11, 1)
    assert transposed_score(p, t, mode, flat) == pc.pair_reference(p, t, mode, 11, 1)[0], "the transposed build at constant rows"
    g = qg.random_rows(len(p), 990 + mode)
    got = aln_amd.score_profiles_gaps_vs_all(ctx, pool([p]), gap_pool([g]), [t], align_type=mode)
    assert int(got[0, 0]) == transposed_score(p, t, mode, g) == qg.pair_reference(p, t, mode, g)[0]


# ---- 4. plumbing ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (rc.LOCAL, rc.SEMI_LOCAL))
def test_row_blocks_slabs_k_and_min_score(mode):
    """the ring set: its last profile (33 rows) ends at the pool's end, so its sweeps request the pad rows"""
    profiles, gaps, ts = qg.ring_set()
    ctx = gpu_util.ctx()
    scores, ends = qg.dense_reference("ring", profiles, gaps, ts, mode)
    qp, gp = pool(profiles), gap_pool(gaps)
    n = len(profiles)
    whole, n_whole = aln_amd.search_topk_profiles_gaps(ctx, qp, gp, ts, 3, align_type=mode)
    dense = aln_amd.score_profiles_gaps_vs_all(ctx, qp, gp, ts, align_type=mode)
    check_hits(whole, n_whole, scores, ends, 3, what=("whole", mode))
    with ctx.hints(search_slab_rows=1):
        hits, n_hits = aln_amd.search_topk_profiles_gaps(ctx, qp, gp, ts, 3, align_type=mode)
    assert hits.tobytes() == whole.tobytes() and np.array_equal(n_hits, n_whole)
    for a, b in ((2, 5), (n - 1, n), (0, 1)):
        hits, n_hits = aln_amd.search_topk_profiles_gaps(ctx, qp, gp, ts, 3, q_begin=a, q_end=b, align_type=mode)
        assert hits.tobytes() == whole[a:b].tobytes() and np.array_equal(n_hits, n_whole[a:b]), (mode, a, b)
        part = aln_amd.score_profiles_gaps_vs_all(ctx, qp, gp, ts, q_begin=a, q_end=b, align_type=mode)
        assert part.tobytes() == dense[a:b].tobytes(), (mode, a, b)
    for K in (1, len(ts) + 3):
        hits, n_hits = aln_amd.search_topk_profiles_gaps(ctx, qp, gp, ts, K, align_type=mode)
        check_hits(hits, n_hits, scores, ends, K, what=("K", mode, K))
    ms = float(np.median(scores))
    hits, n_hits = aln_amd.search_topk_profiles_gaps(ctx, qp, gp, ts, len(ts), min_score=ms, align_type=mode)
    check_hits(hits, n_hits, scores, ends, len(ts), ms, what=("min_score", mode))
    assert 0 < n_hits.sum() < scores.size
    hits, n_hits = aln_amd.search_topk_profiles_gaps(ctx, qp, gp, ts, 3, q_begin=2, q_end=2, align_type=mode)
    assert hits.shape == (0, 3) and n_hits.shape == (0,)
    hits, n_hits = aln_amd.search_topk_profiles_gaps(ctx, qp, gp, [], 3, align_type=mode)
    assert (n_hits == 0).all() and (hits["t"] == -1).all() and (u32(hits["score"]) == 0).all() and (hits["q_end"] == -1).all()


@pytest.mark.parametrize("n", (1, 20, 26))
def test_alphabet_sizes(n):
    """26 letters fill a device row up to the gap words; rows are random in -4 .. 9 so that the last letter's column counts"""
    alphabet = (ALPHA + "JO")[:n] if n > 1 else "A"
    assert len(set(alphabet)) == n
    rng = np.random.RandomState(1000 + n)
    profiles = [rng.randint(-4, 10, (L, n)).astype(np.int64) for L in (7, 12)]
    ts = ["".join(alphabet[k] for k in rng.randint(0, n, m)) for m in (9, 14)]
    ts.append(alphabet[-1] * 8)
    gaps = [qg.random_rows(len(p), 1010 + n + s, 0, 6) for s, p in enumerate(profiles)]
    idx = {ch: k for k, ch in enumerate(alphabet)}
    ctx = gpu_util.ctx()
    for mode in (rc.LOCAL, rc.GLOBAL):
        got = aln_amd.score_profiles_gaps_vs_all(ctx, pool(profiles, alphabet), gap_pool(gaps), ts, align_type=mode)
        for i, p in enumerate(profiles):
            for j, t in enumerate(ts):
                S = np.zeros((len(p) + 2, len(t) + 2), np.int64)
                S[1:-1, 1:-1] = p[:, [idx[ch] for ch in t]]
                H = qg.qgap_planes(S, mode, *[qg.with_tail(a) for a in gaps[i]])
                assert int(got[i, j]) == rc.reference_score(H, mode), (n, mode, i, j)


# ---- 5. the refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order_leave_the_outputs_untouched():
    L = aln_amd.lib()
    ctx = gpu_util.ctx()
    E = aln_amd
    qp = pool([np.ones((3, pc.N)), np.ones((5, pc.N))])
    ok = aln_amd.QueryGaps.constant(qp, 11, 1)
    tp = aln_amd.SeqPool(["WWW", "AC"])
    FILL = 0x5A

    def both(want, prof=None, gaps=ok, templ=tp, mode=aln_amd.LOCAL, qb=0, qe=2, K=2, what=None):
        prof = qp.c if prof is None else prof
        g = gaps.c if isinstance(gaps, aln_amd.QueryGaps) else gaps
        scores = np.full((2, 2), np.float32(-7.5))
        hits = np.frombuffer(bytearray([FILL]) * (2 * 4 * 16), dtype=aln_amd.HIT_DTYPE).reshape(2, 4).copy()
        n_hits = np.full(2, 0x5A5A5A5A, np.int32)
        rc1 = L.aln_score_profiles_gaps_vs_all(ctx.h, C.byref(prof), C.byref(g), C.byref(templ.c), mode, qb, qe, scores.ctypes.data_as(_fp))
        rc2 = L.aln_search_topk_profiles_gaps(ctx.h, C.byref(prof), C.byref(g), C.byref(templ.c), mode, qb, qe, K, -np.inf,
                                              hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits.ctypes.data_as(C.POINTER(C.c_int32)))
        assert (rc1, rc2) == (want, want), (what, rc1, rc2, want)
        assert (scores == np.float32(-7.5)).all(), what
        assert hits.tobytes() == bytes([FILL]) * (2 * 4 * 16) and (n_hits == 0x5A5A5A5A).all(), what

    def qprof(n, alphabet):
        rows = np.ones((int(qp.offsets[-1]), n), np.float32)
        d = aln_amd.AlnQProfiles(qp.c.n_seqs, qp.c.offsets, rows.ctypes.data_as(_fp), n, alphabet)
        d.keep = rows
        return d

    def varied(which, row, value):
        g = aln_amd.QueryGaps.constant(qp, 11, 1)
        getattr(g, which)[row] = value
        return g

    bad_t = aln_amd.SeqPool(["WWW", "A?"])
    long_t = aln_amd.SeqPool(["WWW", "A" * 2100])
    n27 = qprof(27, (ALPHA + "JOU").encode())
    null_array = aln_amd.AlnQGaps(ok.c.del_init, ok.c.del_extn, None, ok.c.ins_extn)
    negative, fraction, huge = varied("del_extn", 1, -1), varied("ins_init", 2, 2.5), varied("ins_extn", 7, 3e6)
    frac_rows = pool([np.full((3, pc.N), 0.5), np.ones((5, pc.N))])
    # 3. the align type; 5. n = 27 and a NULL array, before the template letters
    both(E.E_ARG, mode=5, what="align type")
    both(E.E_ARG, prof=n27, what="n = 27")
    both(E.E_ARG, prof=n27, templ=bad_t, what="n = 27 comes before the letters")
    both(E.E_ARG, gaps=null_array, what="a NULL array")
    both(E.E_ARG, gaps=null_array, templ=bad_t, what="a NULL array comes before the letters")
    # 6. letters, 7. lengths, 8. a negative gap, 9. fractional values and the bound: each before the later ones
    both(E.E_RESIDUE, templ=bad_t, gaps=negative, what="the letters come before the gap values")
    both(E.E_TOO_LONG, templ=long_t, what="2100 residues")
    both(E.E_TOO_LONG, templ=long_t, gaps=negative, what="the lengths come before the gap values")
    both(E.E_ARG, gaps=negative, what="a negative gap")
    both(E.E_ARG, gaps=negative, prof=frac_rows.c, what="a negative gap comes before a fractional row entry")
    both(E.E_NOT_INTEGRAL, gaps=fraction, what="a fractional gap")
    both(E.E_NOT_INTEGRAL, prof=frac_rows.c, what="a fractional row entry")
    both(E.E_NOT_INTEGRAL, gaps=huge, what="the bound, one large gap value")
    # entries that are never read may hold anything; an empty block writes nothing
    for which, row in (("del_init", 4), ("del_extn", 11), ("ins_init", 0), ("ins_extn", 5), ("ins_init", 4), ("ins_extn", 11)):
        g = varied(which, row, np.nan)
        want = aln_amd.score_profiles_gaps_vs_all(ctx, qp, ok, tp)
        assert aln_amd.score_profiles_gaps_vs_all(ctx, qp, g, tp).tobytes() == want.tobytes(), (which, row)
    both(0, qb=1, qe=1, what="empty block")
