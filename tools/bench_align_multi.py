#!/usr/bin/env python3
"""Several non-intersecting local alignments per search hit, two routes, local 11/1 BLOSUM62.

The set (generator stated here, every draw from aln_amd.synth.MT19937):
  domains    64 random sequences, domain d of 60 + (draw % 61) residues, seed 7000 + d
  query q    two different domains (draws of seed 7100 + q pick them) joined by a random linker of 10 residues
  template t seed 7200 + t: 2 + (draw % 3) domain slots; slot 0 and 1 hold the two domains of query t % n_queries in SWAPPED
             order, the further slots a repeat of the first of them; every copy has 15 % of its residues redrawn; random linkers
             of 5 + (draw % 26) residues between and around the copies
so the K best templates of a query hold 2 - 4 copies of its domains in another order than the query's.

  (a) call    aln_hits_align_multi over the hits of aln_search_topk: one wave per hit, all N rounds in one launch
  (b) detour  aln_amd.hits_align_multi_detour over the same hits: per round resident batches built by dp_simmatrix from planes
              expanded and masked on the host, optimal + optimal_strings
First the outputs of (a) are asserted byte-identical to (b) on the hits of the first CHECK_ROWS query rows; then both are timed in
one process, alternating, as medians of 5 repetitions after a warm-up each (min and max are printed too).  Prints one JSON line.
usage: bench_align_multi.py [n_queries] [n_templates] [K] [N]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alignment-algos_amd"))
import aln_amd  # noqa: E402
from aln_amd.synth import AA20, MT19937, residues  # noqa: E402

CHECK_ROWS = 16


def stat(v):
    return {"median_ms": 1e3 * float(np.median(v)), "min_ms": 1e3 * float(min(v)), "max_ms": 1e3 * float(max(v)), "reps": len(v)}


def noisy(g, s):
    r = g.draw(2 * len(s))
    return "".join(AA20[int(r[2 * i + 1]) % 20] if r[2 * i] % 100 < 15 else ch for i, ch in enumerate(s))


def make_set(nq, nt):
    domains = []
    for d in range(64):
        g = MT19937(7000 + d)
        domains.append(residues(g, 60 + int(g.draw(1)[0] % 61)))
    picks, qs = [], []
    for q in range(nq):
        g = MT19937(7100 + q)
        a, b = (int(x) % 64 for x in g.draw(2))
        b = (b + 1) % 64 if b == a else b
        picks.append((a, b))
        qs.append(domains[a] + residues(g, 10) + domains[b])
    ts = []
    for t in range(nt):
        g = MT19937(7200 + t)
        a, b = picks[t % nq]
        slots = [b, a] + [b] * int(g.draw(1)[0] % 3)
        parts = [residues(g, 5 + int(g.draw(1)[0] % 26))]
        for d in slots:
            parts += [noisy(g, domains[d]), residues(g, 5 + int(g.draw(1)[0] % 26))]
        ts.append("".join(parts))
    return qs, ts


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
    ctx = aln_amd.Context(0)
    hits, n_hits = aln_amd.search_topk(ctx, qpool, tpool, alphabet, table, 11, 1, K)
    used = [(r, c) for r in range(rows) for c in range(K) if c < n_hits[r]]
    pairs_qt = [(r, int(hits["t"][r, c])) for r, c in used]
    routes = {}

    def call():
        res = aln_amd.hits_align_multi(ctx, qpool, tpool, hits, n_hits, alphabet, table, 11, 1, N)
        routes["a"] = aln_amd.hits_align_routes(ctx)
        return res

    def detour(pairs=pairs_qt):
        return aln_amd.hits_align_multi_detour(ctx, qpool, tpool, pairs, alphabet, table, 11, 1, N)

    # ---- the outputs agree, byte for byte, on the first rows ----------------------------------------------------------------
    rec, lists, tl, ql, lengths, n_found, rc = call()
    assert rc == 0
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
    call(); detour()
    t_a, t_b = [], []
    for _ in range(5):
        t0 = time.perf_counter(); call(); t_a.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); detour(); t_b.append(time.perf_counter() - t0)
    cells = sum((len(qs[q]) + 2) * (len(ts[t]) + 2) for q, t in pairs_qt)
    found = n_found[np.arange(K)[None, :] < n_hits[:, None]]
    med = lambda v: float(np.median(v))   # noqa: E731
    print(json.dumps({"n_queries": rows, "n_templates": n, "K": K, "N": N, "hits": len(used), "checked_hits": len(sub), "outputs_equal": True,
                      "routes_fused_batched": routes["a"], "alignments_reported": int(found.sum()),
                      "hits_by_n_found": np.bincount(found, minlength=N + 1).tolist(), "matrix_cells": cells,
                      "a_hits_align_multi": stat(t_a), "b_detour": stat(t_b), "b_over_a": med(t_b) / med(t_a)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
