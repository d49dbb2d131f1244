"""-m gpu: the 64-lane windows of strip_walk (csrc/search_align.h), the walk back all five fused hit-alignment kernels share.
The walk takes up to 64 diagonal steps per iteration and scans a gap jump's source row / column in steps of 64 cells, so what
can go wrong sits at diagonal runs and jumps of about 64 and 128.  Block-structured pairs under identity5 (match 5, mismatch
-5), gi 40, ge 0 — a gap of any length costs 8 matches, so a long jump is optimal:

    query      Kq  F1      M  Gq  F2  Sq          every block over letters of its own: nothing matches by accident,
    template   Kt  F1  Gt  M      F2  St          and no gap can slide

Optimal's alignment is F1, a deletion jump over Gt, M, an insertion jump over Gq, F2.  The walk comes from the end, so after
each jump a fresh window starts at the last pair of M / of F1:
  run n    M has n pairs: n - 1 diagonal steps from the window's first cell, then the deletion (n = 65, 66: one full window and
           0 or 1 more steps; 129, 130: two full windows)
  del g    Gt has g columns: the scan passes g - 1 set bits (g = 65: the clear bit is the first cell of the second step)
  ins g    Gq has g rows, likewise
  head n   no F1 and no Gt: the alignment STARTS with M after the junk Kq / Kt, so the local walk ends at the score bit after
           n - 1 diagonal steps (the non-local walks go on through the junk)
The builder asserts on the int64 reference (range_cases.affine_reference with lean_cases.reference_list / nonlocal_cases.walk)
that every case's list holds its run or jump under every align type the test uses.  Every case runs through all five kernels
in one call each — local and global residue, local and semi-local profile (derived from the residues), multi with N = 2 —
every slot fused, and is compared bit for bit with the int64 reference, the oracle and the batch route."""
import numpy as np
import pytest

import aln_amd
import gpu_util
import lean_cases as lc
import multi_align_cases as mc
import nonlocal_cases as nc
import range_cases as rc
import search_cases as sc
from test_gpu_hits_align_nonlocal import batch_route, check_equal, same_results
from test_gpu_hits_align_profiles import batch_comparator

pytestmark = pytest.mark.gpu

U32 = np.uint32
ALPHA, TABLE, GI, GE = sc.ALPHA, sc.TABLES["identity5"], 40, 0
NONLOCAL_RESIDUE, NONLOCAL_PROFILE = rc.GLOBAL, rc.SEMI_LOCAL
MODES = (rc.LOCAL, NONLOCAL_RESIDUE, NONLOCAL_PROFILE)
FLANK, MID, GAP_T, GAP_Q = 12, 20, 23, 21                        # block lengths where the case does not set them
SPECS = ([("run", n) for n in (63, 64, 65, 66, 129, 130)] + [("del", g) for g in (63, 64, 65, 130)] +
         [("ins", g) for g in (63, 64, 65, 130)] + [("head", n) for n in (64, 65, 66)])


def block(letters, seed, n):
    return rc.random_seq(letters, seed, n)


def build_pair(kind, n, seed):
    m = n if kind in ("run", "head") else MID
    gt = n if kind == "del" else GAP_T
    gq = n if kind == "ins" else GAP_Q
    f1, mid, f2 = block("ACDE", seed, FLANK), block("FGHI", seed + 1, m), block("LMNP", seed + 2, FLANK)
    if kind == "head":
        q, t = "KKK" + mid + "Y" * gq + f2 + "SS", "RRRRR" + mid + f2
    else:
        q, t = "KKK" + f1 + mid + "Y" * gq + f2 + "SS", "RRRRR" + f1 + "W" * gt + mid + f2
    t += "Q" * (300 - len(t))                                    # 302 columns: length class 2
    assert len(q) + 2 < 300 and (len(t) + 2 + 255) // 256 == 2
    return q, t


def cells_of(pl):
    """the aligned cells of a list in list order: without (0,0), without (Q-1, T-1)"""
    p = [tuple(int(v) for v in x) for x in pl][:-1]
    return p[1:] if p[0] == (0, 0) else p


def runs_and_jumps(cells):
    """-> (lengths in pairs of the maximal diagonal runs, column jumps of the deletions, row jumps of the insertions)"""
    runs, dels, ins, cur = [], [], [], 1
    for (i0, j0), (i1, j1) in zip(cells[:-1], cells[1:]):
        if (i1 - i0, j1 - j0) == (1, 1):
            cur += 1
            continue
        runs.append(cur)
        cur = 1
        if i1 == i0 + 1:
            dels.append(j1 - j0 - 1)
        else:
            assert j1 == j0 + 1
            ins.append(i1 - i0 - 1)
    runs.append(cur)
    return runs, dels, ins


def reference_list(q, t, mode):
    """-> (score, list, H) on the int64 plane"""
    H = rc.affine_reference(rc.sim_int(q, t, ALPHA, TABLE), mode, GI, GE)[0]
    if mode == rc.LOCAL:
        return rc.reference_score(H, mode), lc.reference_list(H, GI, GE), H
    score, pl = nc.walk(H, GI, GE, *nc.free_ends(mode))
    assert int(score) == rc.reference_score(H, mode)
    return int(score), pl, H


_CASES = []


def cases():
    """-> [(kind, n, q, t, {mode: (score, list, H)})], built once, never modified; a case that misses its situation under one
    of the align types fails here"""
    if not _CASES:
        for k, (kind, n) in enumerate(SPECS):
            q, t = build_pair(kind, n, 5000 + 10 * k)
            ref = {}
            for mode in MODES:
                ref[mode] = reference_list(q, t, mode)
                cl = cells_of(ref[mode][1])
                runs, dels, ins = runs_and_jumps(cl)
                where = (kind, n, mode, runs, dels, ins)
                if kind == "run":
                    assert n in runs and GAP_T in dels and GAP_Q in ins, where
                elif kind == "del":
                    assert n in dels and MID in runs, where
                elif kind == "ins":
                    assert n in ins and MID in runs, where
                elif mode == rc.LOCAL:                               # head: the walk stops by the score bit, inside the matrix
                    assert runs[0] == n and cl[0][0] > 1 and cl[0][1] > 1 and tuple(ref[mode][1][0]) == (0, 0), where
                else:
                    assert any(r >= n for r in runs), where
            _CASES.append((kind, n, q, t, ref))
    return _CASES


def pools():
    cs = cases()
    return [c[2] for c in cs], [c[3] for c in cs]


def diagonal_hits(mode):
    """row r -> template r; local: the reference's end cell and score, otherwise values that must not be read"""
    cs = cases()
    hits = np.zeros((len(cs), 1), dtype=aln_amd.HIT_DTYPE)
    hits["t"][:, 0] = np.arange(len(cs))
    hits["score"], hits["q_end"], hits["t_end"] = -1e30, -7, 1 << 20
    if mode == rc.LOCAL:
        for r, c in enumerate(cs):
            score, pl, H = c[4][mode]
            hits["score"][r, 0], hits["q_end"][r, 0], hits["t_end"][r, 0] = score, pl[-2][0], pl[-2][1]
    return hits, np.ones(len(cs), np.int32)


def check_reference_and_oracle(res, mode):
    rec, lists = res[0], res[1]
    for r, (kind, n, q, t, ref) in enumerate(cases()):
        score, pl, _ = ref[mode]
        assert np.array_equal(lists[r][0], pl), (kind, n, mode, lists[r][0].tolist(), pl.tolist())
        assert np.float32(rec["score"][r, 0]).view(U32) == np.float32(score).view(U32), (kind, n, mode)
        assert rec["identity"][r, 0].view(U32) == gpu_util.identity_for(q, t, pl).view(U32), (kind, n, mode)
        if mode == rc.LOCAL:
            osc, opl = mc.oracle_rounds(mc.Case("w", q, t, ALPHA, TABLE, GI, GE, 1, -np.inf, ()))[0]
        else:
            _, osc, opl = nc.oracle_pair(q, t, ALPHA, TABLE, mode, GI, GE)
        assert np.array_equal(lists[r][0], opl) and np.float32(osc).view(U32) == np.float32(score).view(U32), (kind, n, mode)


@pytest.mark.parametrize("mode", (rc.LOCAL, NONLOCAL_RESIDUE))
def test_residue_kernels(mode):
    ctx = gpu_util.ctx()
    qs, ts = pools()
    hits, n_hits = diagonal_hits(mode)
    res = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, ALPHA, TABLE, GI, GE, align_type=mode)
    assert aln_amd.hits_align_routes(ctx) == (len(qs), 0)
    assert res[5] == 0 and (res[0]["status"] == 0).all()
    check_reference_and_oracle(res, mode)
    check_equal(res, hits, n_hits, batch_route(ctx, qs, ts, hits, n_hits, ALPHA, TABLE, mode, GI, GE))
    if mode != rc.LOCAL:
        with ctx.hints(align_fused_nonlocal=0):
            batch = aln_amd.hits_align(ctx, qs, ts, hits, n_hits, ALPHA, TABLE, GI, GE, align_type=mode)
            assert aln_amd.hits_align_routes(ctx) == (0, len(qs))
        same_results(res, batch)


@pytest.mark.parametrize("mode", (rc.LOCAL, NONLOCAL_PROFILE))
def test_profile_kernels(mode):
    ctx = gpu_util.ctx()
    qs, ts = pools()
    hits, n_hits = diagonal_hits(mode)
    qp = aln_amd.profiles_from_sequences(qs, ALPHA, TABLE)
    res = aln_amd.hits_align_profiles(ctx, qp, ts, hits, n_hits, GI, GE, consensus=qs, align_type=mode)
    assert aln_amd.hits_align_routes(ctx) == (len(qs), 0)
    assert res[5] == 0 and (res[0]["status"] == 0).all()
    check_reference_and_oracle(res, mode)
    check_equal(res, hits, n_hits, batch_comparator(ctx, qp.profiles, qs, ts, hits, n_hits, mode, GI, GE))
    same_results(res, aln_amd.hits_align(ctx, qs, ts, hits, n_hits, ALPHA, TABLE, GI, GE, align_type=mode))
    if mode != rc.LOCAL:
        with ctx.hints(align_fused_nonlocal=0):
            batch = aln_amd.hits_align_profiles(ctx, qp, ts, hits, n_hits, GI, GE, consensus=qs, align_type=mode)
            assert aln_amd.hits_align_routes(ctx) == (0, len(qs))
        same_results(res, batch)


def test_multi_kernel():
    """N = 2: round 0 is the case's alignment; round 1 runs the same walk over a strip whose score bits the mask changed"""
    ctx = gpu_util.ctx()
    qs, ts = pools()
    hits, n_hits = diagonal_hits(rc.GLOBAL)                          # only .t is read
    rec, lists, tl, ql, lengths, n_found, rcode = aln_amd.hits_align_multi(ctx, qs, ts, hits, n_hits, ALPHA, TABLE, GI, GE, 2)
    assert aln_amd.hits_align_routes(ctx) == (len(qs), 0) and rcode == 0
    det = aln_amd.hits_align_multi_detour(ctx, qs, ts, [(i, i) for i in range(len(qs))], ALPHA, TABLE, GI, GE, 2)
    for r, (kind, n, q, t, ref) in enumerate(cases()):
        reported, _ = mc.rounds(rc.sim_int(q, t, ALPHA, TABLE), GI, GE, 2)
        assert np.array_equal(reported[0].pairs, ref[rc.LOCAL][1])
        assert n_found[r, 0] == len(reported) == len(det[r]), (kind, n)
        for a, rd in enumerate(reported):
            e = rec[r, 0, a]
            score, pl, ident, t_line, q_line, status = det[r][a]
            assert e["status"] == 0 and status == 0, (kind, n, a)
            assert np.array_equal(lists[r][0][a], rd.pairs) and np.array_equal(pl, rd.pairs), (kind, n, a)
            assert np.float32(e["score"]).view(U32) == np.float32(rd.score).view(U32) == np.float32(score).view(U32), (kind, n, a)
            assert np.float32(e["identity"]).view(U32) == np.float32(ident).view(U32), (kind, n, a)
            assert tl[r][0][a] == t_line and ql[r][0][a] == q_line and lengths[r, 0, a] == len(t_line), (kind, n, a)
