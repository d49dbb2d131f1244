#!/usr/bin/env python3
"""Purging of near-identical search hits, with the weights and weighted counts of the survivors, two ways on the slice
tools/bench_search.py times: the first ROWS of TEMPLATES synthetic proteins, length U[400,600] (seed 5000+s), against all of
them, 11/1 BLOSUM62, the K best templates of every query, max_identity = 90, min_overlap = 50, w_max = 1000.

  (a) device  aln_hits_purge with weights, raw, counts and covered: every hit swept once, its letters row kept on the device,
              the pair bits, the greedy pass, the purge records, the muted rows, the tally, the weights and the weighted tally
              made there; per hit two 16-byte records, the weight and raw come down, per query row one 128-byte count row
  (b) detour  aln_hits_pileup for the letters (rows x K x the longest query bytes come down), aln_amd.purge_from_pileup and
              aln_amd.weights_from_pileup over the muted rows on the host per query, then aln_hits_column_counts under those
              weights, which sweeps and walks every hit again — what a caller had to do before
  (c)         aln_hits_weights on the same hits, for scale
Records, purge records, weights, raw, counts and covered of (a) and (b) must be byte-identical (asserted first).  Then the three
alternate in one process, `reps` rounds after a warm-up; each is reported as median (min - max) in ms.  Prints one JSON line.
usage: bench_purge.py [ROWS] [TEMPLATES] [K] [align type, default local]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alignment-algos_amd"))
import aln_amd  # noqa: E402
from aln_amd.synth import MT19937, residues  # noqa: E402

ALIGN_TYPES = {"global_local": aln_amd.GLOBAL_LOCAL, "global": aln_amd.GLOBAL, "local_global": aln_amd.LOCAL_GLOBAL,
               "local": aln_amd.LOCAL, "semi_local": aln_amd.SEMI_LOCAL}
REPS = 7
W_MAX = 1000
MAX_IDENTITY, MIN_OVERLAP = 90, 50


def stat(v):
    return {"median_ms": 1e3 * float(np.median(v)), "min_ms": 1e3 * float(min(v)), "max_ms": 1e3 * float(max(v)), "reps": len(v)}


def main():
    arg = lambda k, d: int(sys.argv[k]) if len(sys.argv) > k else d   # noqa: E731
    rows, n, K = arg(1, 512), arg(2, 4096), arg(3, 10)
    name = sys.argv[4] if len(sys.argv) > 4 else "local"
    if name not in ALIGN_TYPES:
        sys.exit("align type: one of " + ", ".join(ALIGN_TYPES))
    mode = ALIGN_TYPES[name]
    lines = open(os.path.join(ROOT, "tests", "golden", "BLOSUM62")).read().split("\n")
    k = 0
    while lines[k].startswith("#"):
        k += 1
    alphabet = "".join(lines[k].split())
    table = np.array([[float(x) for x in ln.split()[1:]] for ln in lines[k + 1:k + 1 + len(alphabet)]], dtype=np.float32)
    seqs = []
    for s in range(n):
        g = MT19937(5000 + s)
        seqs.append(residues(g, 400 + int(g.draw(1)[0] % 201)))
    pool = aln_amd.SeqPool(seqs)
    ctx = aln_amd.Context(0)
    hits, n_hits = aln_amd.search_topk(ctx, pool, pool, alphabet, table, 11, 1, K, q_end=rows, align_type=mode)
    off = pool.offsets
    width = int((off[1:rows + 1] - off[:rows]).max()) - 2                       # the line stride: the longest query

    def device():
        return aln_amd.hits_purge(ctx, pool, pool, hits, n_hits, alphabet, table, 11, 1, MAX_IDENTITY, MIN_OVERLAP, w_max=W_MAX,
                                  align_type=mode)

    def detour():
        rec, _, letters, _, rc = aln_amd.hits_pileup(ctx, pool, pool, hits, n_hits, alphabet, table, 11, 1, align_type=mode,
                                                     want_tpos=False, want_spans=False, line_stride=width)
        purge = np.zeros((rows, K), aln_amd.HIT_PURGE_DTYPE)
        weights = np.zeros((rows, K), np.int32)
        raw = np.zeros((rows, K), np.int64)
        slots = np.arange(K)
        for r in range(rows):
            purge["keeper"][r], purge["same"][r], purge["overlap"][r], purge["letters"][r] = aln_amd.purge_from_pileup(
                letters[r], alphabet, MAX_IDENTITY, MIN_OVERLAP)
            muted = letters[r].copy()
            muted[purge["keeper"][r] != slots] = ord(".")
            weights[r], raw[r] = aln_amd.weights_from_pileup(muted, alphabet, W_MAX)
        crec, counts, covered, crc = aln_amd.hits_column_counts(ctx, pool, pool, hits, n_hits, alphabet, table, 11, 1, weights=weights,
                                                                align_type=mode)
        assert rc == 0 and crc == 0 and crec.tobytes() == rec.tobytes()
        return rec, purge, weights, raw, counts, covered, rc

    def weights_only():
        return aln_amd.hits_weights(ctx, pool, pool, hits, n_hits, alphabet, table, 11, 1, w_max=W_MAX, align_type=mode)

    a, b = device(), detour()
    routes = aln_amd.hits_align_routes(ctx)
    assert a[6] == 0 and a[0].tobytes() == b[0].tobytes(), "records differ"
    assert a[1].tobytes() == b[1].tobytes(), "purge records differ"
    assert a[2].tobytes() == b[2].tobytes(), "weights differ"
    assert a[3].tobytes() == b[3].tobytes(), "raw differs"
    assert len(a[4]) == len(b[4]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[4], b[4])), "counts differ"
    assert a[5].tobytes() == b[5].tobytes(), "covered differs"
    fns = (("a_hits_purge", device), ("b_pileup_host_purge_weights_column_counts", detour), ("c_hits_weights", weights_only))
    times = {key: [] for key, _ in fns}
    for _, fn in fns:
        fn()                                                        # warm-up
    for _ in range(REPS):
        for key, fn in fns:
            t0 = time.perf_counter()
            fn()
            times[key].append(time.perf_counter() - t0)
    keeper = a[1]["keeper"]
    n_used, n_rows = int(n_hits.sum()), int(off[rows] - off[0])
    out = {"align_type": name, "n_queries": rows, "n_templates": n, "K": K, "hits": n_used, "outputs_equal": True,
           "routes_fused_batched": routes, "max_identity": MAX_IDENTITY, "min_overlap": MIN_OVERLAP, "w_max": W_MAX, "line_stride": width,
           "kept": int((keeper == np.arange(K)[None, :]).sum()), "purged": int(((keeper >= 0) & (keeper != np.arange(K)[None, :])).sum()),
           "pairs": rows * K * (K - 1) // 2,
           "a_download_bytes": n_used * (32 + 4) + rows * K * (16 + 12) + n_rows * 128,    # the kernels' records, same; purge; weights, raw; count rows
           "b_download_bytes": n_used * (width + 32 + 4) + n_used * (32 + 4) + n_rows * 128}   # letters + records, then records + count rows
    for key, _ in fns:
        out[key] = stat(times[key])
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
