#!/usr/bin/env python3
"""aln_hits_zscores_profiles on the slice tools/bench_zscore.py times: the first Q of N synthetic proteins, length U[400,600]
(seed 5000+s), as profiles derived from the queries (row i = the BLOSUM62 row of residue i) against all N, local 11/1, the K best
templates of every profile (aln_search_topk_profiles) and S shuffles per hit.  Derived profiles must give aln_hits_zscores'
records byte for byte: that is asserted before anything is timed.

Three ways to the sums, timed ALTERNATING (a, b, c, a, b, c, ..) after one warm-up of each; median, min and max over the
repetitions are printed:
  (a) profiles  aln_hits_zscores_profiles: one resident copy of a profile's rows read in permuted order, 2 B per row and shuffle
  (b) residues  aln_hits_zscores on the same hits: the same cell work with table rows instead of staged profile rows
  (c) detour    all a caller could do before: per profile, S row permutations made on the host (numpy), uploaded as a pool of
                S permuted copies (S x rows x 128 B on the device), one aln_score_profiles_vs_all against the profile's hit
                templates, summed on the host.  It runs on the first `detour_rows` rows only and is SCALED to Q rows.
Prints one JSON line.  usage: bench_zscore_profiles.py [Q] [N] [K] [S] [reps] [detour_rows]"""
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
        seqs.append(residues(g, 400 + int(g.draw(1)[0] % 201)))
    pool = aln_amd.SeqPool(seqs)
    qpool = aln_amd.SeqPool(seqs[:rows])
    profiles = aln_amd.profiles_from_sequences(seqs[:rows], alphabet, table)
    ctx = aln_amd.Context(0)
    lens = np.array([len(s) for s in seqs], dtype=np.int64)

    hits, n_hits = aln_amd.search_topk_profiles(ctx, profiles, pool, 11, 1, K)
    used = np.arange(K)[None, :] < n_hits[:, None]
    pair_cells = lens[:rows, None] * lens[np.where(used, hits["t"], 0)] * used
    cells = float(pair_cells.sum()) * S

    def by_profiles():
        return aln_amd.hits_zscores_profiles(ctx, profiles, pool, hits, n_hits, 11, 1, S, seed=1)

    def by_residues():
        return aln_amd.hits_zscores(ctx, qpool, pool, hits, n_hits, alphabet, table, 11, 1, S, seed=1)

    rng = np.random.RandomState(1)

    def detour():
        out = np.zeros((drows, K, 2), dtype=np.int64)
        for r in range(drows):
            p = profiles.profiles[r]
            copies = aln_amd.QueryProfiles([p[rng.permutation(len(p))] for _ in range(S)], alphabet)
            ts = [seqs[t] for t in hits["t"][r, :n_hits[r]]]
            d = aln_amd.score_profiles_vs_all(ctx, copies, ts, 11, 1).astype(np.int64)
            out[r, :n_hits[r], 0] = d.sum(axis=0)
            out[r, :n_hits[r], 1] = (d * d).sum(axis=0)
        return out

    ways = [("a_hits_zscores_profiles", by_profiles), ("b_hits_zscores", by_residues), ("c_detour", detour)]
    got = {name: fn() for name, fn in ways}                         # the warm-up of each, and the comparison
    assert got["a_hits_zscores_profiles"].tobytes() == got["b_hits_zscores"].tobytes()
    t = {name: [] for name, _ in ways}
    for _ in range(reps):
        for name, fn in ways:
            t0 = time.perf_counter()
            fn()
            t[name].append(time.perf_counter() - t0)
    med = lambda v: float(np.median(v))   # noqa: E731
    scale = rows / float(drows)
    stats = got["a_hits_zscores_profiles"]
    res = {"n_queries": rows, "n_templates": n, "K": K, "S": S, "hits": int(n_hits.sum()), "shuffle_cells": cells,
           "same_stats_as_aln_hits_zscores": True,
           "profile_rows_bytes": int(profiles.offsets[-1]) * 128,
           "materialised_bytes_the_entry_avoids": int(sum(len(p) + 2 for p in profiles.profiles)) * 128 * S,
           "a_hits_zscores_profiles": stat(t["a_hits_zscores_profiles"]), "b_hits_zscores": stat(t["b_hits_zscores"]),
           "a_over_b": med(t["a_hits_zscores_profiles"]) / med(t["b_hits_zscores"]),
           "a_shuffle_gcups": cells / med(t["a_hits_zscores_profiles"]) / 1e9,
           "b_shuffle_gcups": cells / med(t["b_hits_zscores"]) / 1e9,
           "c_detour_rows_measured": drows, "c_detour_measured": stat(t["c_detour"]),
           "c_detour_scaled_to_n_queries_median_ms": 1e3 * med(t["c_detour"]) * scale,
           "c_note": "measured on %d rows, scaled x%.1f to %d rows" % (drows, scale, rows),
           "a_over_c_scaled": med(t["a_hits_zscores_profiles"]) / (med(t["c_detour"]) * scale),
           "z_median": float(np.median(stats["z"][used])), "z_max": float(stats["z"][used].max())}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
