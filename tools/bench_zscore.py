#!/usr/bin/env python3
"""Shuffle z-scores of search hits on the slice tools/bench_search.py times: the first `n_queries` of `n_templates` synthetic
proteins, length U[400,600] (seed 5000+s), against all of them, local 11/1 BLOSUM62, the K best templates of every query and
S shuffles per hit.

Two ways to the sums, each timed as the median of `reps` repetitions after a warm-up (min and max are printed too):
  (a) device  aln_search_topk + aln_hits_zscores: shuffling, scoring and the reduction on the device, 24 B per hit travel
  (b) detour  all a caller could do before: per query, S permutations made on the host (numpy), then one
              aln_score_all_vs_all of those strings against the query's hit templates, summed on the host.  It runs on the
              first `detour_rows` rows only and is SCALED to n_queries rows (the output says so).
The cell rate of the shuffle scoring is sum over scored pairs of |q| x |t| (residues) / time; next to it the rate of
aln_score_all_vs_all on the same slice with one query per wave (score_local_kernel, hint score_packed = 0) and with the packed
lanes, which is what tools/bench_c5.py times.  Prints one JSON line.
usage: bench_zscore.py [n_queries] [n_templates] [K] [S] [reps] [detour_rows]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alignment-algos_amd"))
import aln_amd  # noqa: E402
from aln_amd.synth import MT19937, residues  # noqa: E402


def stat(v):
    return {"median_ms": 1e3 * float(np.median(v)), "min_ms": 1e3 * float(min(v)), "max_ms": 1e3 * float(max(v)), "reps": len(v)}


def timed(fn, reps):
    fn()                                                        # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def main():
    arg = lambda k, d: int(sys.argv[k]) if len(sys.argv) > k else d   # noqa: E731
    rows, n, K, S, reps, drows = arg(1, 512), arg(2, 4096), arg(3, 10), arg(4, 100), arg(5, 5), arg(6, 16)
    drows = min(drows, rows)
    lines = open(os.path.join(ROOT, "tests", "golden", "BLOSUM62")).read().split("\n")
    k = 0
    while lines[k].startswith("#"):
        k += 1
    alphabet = "".join(lines[k].split())
    table = np.array([[float(x) for x in l.split()[1:]] for l in lines[k + 1:k + 1 + len(alphabet)]], dtype=np.float32)
    seqs = []
    for s in range(n):
        g = MT19937(5000 + s)
        ln = 400 + int(g.draw(1)[0] % 201)
        seqs.append(residues(g, ln))
    pool = aln_amd.SeqPool(seqs)
    ctx = aln_amd.Context(0)
    lens = np.array([len(s) for s in seqs], dtype=np.int64)

    hits, n_hits = aln_amd.search_topk(ctx, pool, pool, alphabet, table, 11, 1, K, q_end=rows)
    used = np.arange(K)[None, :] < n_hits[:, None]
    pair_cells = lens[:rows, None] * lens[np.where(used, hits["t"], 0)] * used
    cells = float(pair_cells.sum()) * S
    dcells = float(pair_cells[:drows].sum()) * S

    def search():
        return aln_amd.search_topk(ctx, pool, pool, alphabet, table, 11, 1, K, q_end=rows)

    def zscores():
        return aln_amd.hits_zscores(ctx, pool, pool, hits, n_hits, alphabet, table, 11, 1, S, seed=1)

    rng = np.random.RandomState(1)

    def detour():
        out = np.zeros((drows, K, 2), dtype=np.int64)
        for r in range(drows):
            q = np.frombuffer(seqs[r].encode(), dtype=np.uint8)
            strings = [rng.permutation(q).tobytes().decode() for _ in range(S)]
            ts = [seqs[t] for t in hits["t"][r, :n_hits[r]]]
            d = aln_amd.score_all_vs_all(ctx, strings, ts, alphabet, table, 11, 1).astype(np.int64)
            out[r, :n_hits[r], 0] = d.sum(axis=0)
            out[r, :n_hits[r], 1] = (d * d).sum(axis=0)
        return out

    def dense(packed):
        def fn():
            with ctx.hints(score_packed=packed):
                return aln_amd.score_all_vs_all(ctx, pool, pool, alphabet, table, 11, 1, 0, rows)
        return fn

    t_search, t_z, t_det = timed(search, reps), timed(zscores, reps), timed(detour, reps)
    t_c5, t_c5pk = timed(dense(0), reps), timed(dense(1), reps)
    stats = zscores()
    c5_cells = float(lens[:rows].sum()) * float(lens.sum())
    scale = rows / float(drows)
    med = lambda v: float(np.median(v))   # noqa: E731
    res = {"n_queries": rows, "n_templates": n, "K": K, "S": S, "hits": int(n_hits.sum()), "shuffle_cells": cells,
           "a_search_topk": stat(t_search), "a_hits_zscores": stat(t_z),
           "a_total_median_ms": 1e3 * (med(t_search) + med(t_z)),
           "a_shuffle_gcups": cells / med(t_z) / 1e9,
           "b_detour_rows_measured": drows, "b_detour_measured": stat(t_det),
           "b_detour_scaled_to_n_queries_median_ms": 1e3 * med(t_det) * scale,
           "b_note": "measured on %d rows, scaled x%.1f to %d rows; the search that finds the hits is not included" % (drows, scale, rows),
           "b_shuffle_gcups": dcells / med(t_det) / 1e9,
           "score_all_vs_all_one_query_per_wave": stat(t_c5), "score_local_kernel_gcups": c5_cells / med(t_c5) / 1e9,
           "score_all_vs_all_packed": stat(t_c5pk), "score_local_pk_kernel_gcups": c5_cells / med(t_c5pk) / 1e9,
           "z_median": float(np.median(stats["z"][used])), "z_max": float(stats["z"][used].max())}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
