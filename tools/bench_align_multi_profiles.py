#!/usr/bin/env python3
"""Several non-intersecting local alignments per hit of a PROFILE search, three routes, local 11/1.

The set is bench_align_multi.py's (its docstring has the generator), the profiles are derived from the queries under BLOSUM62:
row i of profile q is the table row of residue i of query q, the consensus is the query itself.  So all three routes must
report the same bytes:
  (a) profiles  aln_hits_align_multi_profiles over the hits of aln_search_topk_profiles: one wave per hit, rows staged into LDS
  (b) residues  aln_hits_align_multi over the same hits with the queries as residue strings
  (c) detour    aln_amd.hits_align_multi_profiles_detour: per round resident batches built by dp_simmatrix from planes expanded
                from the profiles and masked on the host, optimal + optimal_strings over the consensus letters
First the outputs of (a) are asserted byte-identical to (b) on all hits and to (c) on the hits of the first CHECK_ROWS query
rows; then the three are timed in one process, alternating, as medians of 5 repetitions after a warm-up each (min and max are
printed too).  Prints one JSON line.
usage: bench_align_multi_profiles.py [n_queries] [n_templates] [K] [N]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alignment-algos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import aln_amd  # noqa: E402
from bench_align_multi import CHECK_ROWS, make_set, stat  # noqa: E402


def main():
    arg = lambda k, d: int(sys.argv[k]) if len(sys.argv) > k else d   # noqa: E731
    rows, n, K, N = arg(1, 512), arg(2, 4096), arg(3, 10), arg(4, 4)
    lines = open(os.path.join(ROOT, "tests", "golden", "BLOSUM62")).read().split("\n")
    k = 0
    while lines[k].startswith("#"):
        k += 1
    alphabet = "".join(lines[k].split())
    table = np.array([[float(x) for x in ln.split()[1:]] for ln in lines[k + 1:k + 1 + len(alphabet)]], dtype=np.float32)
    qs, ts = make_set(rows, n)
    qpool, tpool = aln_amd.SeqPool(qs), aln_amd.SeqPool(ts)
    qprof = aln_amd.profiles_from_sequences(qs, alphabet, table)
    ctx = aln_amd.Context(0)
    hits, n_hits = aln_amd.search_topk_profiles(ctx, qprof, tpool, 11, 1, K)
    used = [(r, c) for r in range(rows) for c in range(K) if c < n_hits[r]]
    pairs_qt = [(r, int(hits["t"][r, c])) for r, c in used]
    routes = {}

    def profiles():
        res = aln_amd.hits_align_multi_profiles(ctx, qprof, tpool, hits, n_hits, 11, 1, N, consensus=qpool)
        routes["a"] = aln_amd.hits_align_routes(ctx)
        return res

    def residues():
        res = aln_amd.hits_align_multi(ctx, qpool, tpool, hits, n_hits, alphabet, table, 11, 1, N)
        routes["b"] = aln_amd.hits_align_routes(ctx)
        return res

    def detour(pairs=pairs_qt):
        return aln_amd.hits_align_multi_profiles_detour(ctx, qprof, tpool, pairs, 11, 1, N, consensus=qpool)

    # ---- the outputs agree, byte for byte: with the residue entry on all hits, with the detour on the first rows -------------------
    rec, lists, tl, ql, lengths, n_found, rc = profiles()
    assert rc == 0
    rec_b, lists_b, tl_b, ql_b, lengths_b, n_found_b, rc_b = residues()
    assert rc_b == 0 and rec.tobytes() == rec_b.tobytes() and np.array_equal(n_found, n_found_b) and np.array_equal(lengths, lengths_b)
    assert tl == tl_b and ql == ql_b
    assert all(np.array_equal(x, y) for ra, rb in zip(lists, lists_b) for ka, kb in zip(ra, rb) for x, y in zip(ka, kb))
    sub = [(p, r, c) for p, (r, c) in enumerate(used) if r < CHECK_ROWS]
    det = detour([pairs_qt[p] for p, r, c in sub])
    for (p, r, c), rounds in zip(sub, det):
        assert n_found[r, c] == len(rounds), (r, c)
        for a, (score, pl, ident, t_line, q_line, status) in enumerate(rounds):
            e = rec[r, c, a]
            assert status == 0 and e["status"] == 0
            assert np.float32(e["score"]).tobytes() == np.float32(score).tobytes(), (r, c, a)
            assert np.float32(e["identity"]).tobytes() == np.float32(ident).tobytes(), (r, c, a)
            assert np.array_equal(lists[r][c][a], pl) and tl[r][c][a] == t_line and ql[r][c][a] == q_line, (r, c, a)
        for a in range(len(rounds), N):
            assert rec[r, c, a].tobytes() == bytes(16) and tl[r][c][a] == ""

    # ---- the times: alternating, medians of 5 after a warm-up each ------------------------------------------------------------
    profiles(); residues(); detour()
    t_a, t_b, t_c = [], [], []
    for _ in range(5):
        t0 = time.perf_counter(); profiles(); t_a.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); residues(); t_b.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); detour(); t_c.append(time.perf_counter() - t0)
    cells = sum((len(qs[q]) + 2) * (len(ts[t]) + 2) for q, t in pairs_qt)
    found = n_found[np.arange(K)[None, :] < n_hits[:, None]]
    med = lambda v: float(np.median(v))   # noqa: E731
    print(json.dumps({"n_queries": rows, "n_templates": n, "K": K, "N": N, "hits": len(used), "checked_hits": len(sub), "outputs_equal": True,
                      "routes_fused_batched": routes["a"], "routes_residue_entry": routes["b"], "alignments_reported": int(found.sum()),
                      "hits_by_n_found": np.bincount(found, minlength=N + 1).tolist(), "matrix_cells": cells,
                      "a_hits_align_multi_profiles": stat(t_a), "b_hits_align_multi": stat(t_b), "c_detour": stat(t_c),
                      "c_over_a": med(t_c) / med(t_a), "a_over_b": med(t_a) / med(t_b)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
