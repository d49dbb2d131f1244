#!/usr/bin/env python3
"""From a search round's hits to the next round's profile rows, on the slice tools/bench_search.py times: the first ROWS of
TEMPLATES synthetic proteins, length U[400,600] (seed 5000+s), against all of them, 11/1 BLOSUM62, the K best templates of
every query, max_identity = 90, min_overlap = 50, w_max = 1000, background pseudo-counts of mass beta = w_max, scale 2.

  (a) aln_hits_pssm, rows only: purge, weights, counts and the integer log-odds on the device; per query row n floats come
      down, no count row
  (b) aln_hits_purge with weights, raw, counts and covered on the same hits (what (c) starts with)
  (c) the detour (a) replaces: (b), then aln_amd.pssm_from_counts per query in float64 numpy
First the rows of (a) are asserted equal to aln_amd.pssm_rows_from_counts (Python integers) over (b)'s counts on the first
CHECK_ROWS queries, and (a)'s optional outputs, asked for once, byte-identical to (b)'s.  Then the three alternate in one
process, `reps` rounds after a warm-up; each is reported as median (min - max) in ms.  Prints one JSON line.
usage: bench_pssm.py [ROWS] [TEMPLATES] [K] [align type, default local]"""
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
SCALE, BETA = 2, W_MAX
CHECK_ROWS = 8


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
    bg = [1024 // len(alphabet)] * len(alphabet)
    par = aln_amd.AlnPssmParams.make(bg, BETA, SCALE)
    background = np.asarray(bg, np.float64) / sum(bg)
    idx = {ch: a for a, ch in enumerate(alphabet)}
    fallback = [table[[idx[ch] for ch in seqs[r]]] for r in range(rows)]

    def pssm(**kw):
        return aln_amd.hits_pssm(ctx, pool, pool, hits, n_hits, alphabet, table, 11, 1, par, MAX_IDENTITY, MIN_OVERLAP, W_MAX,
                                 align_type=mode, **kw)

    def rows_only():
        return pssm(want_purge=False, want_weights=False, want_raw=False, want_counts=False, want_covered=False)

    def purge():
        return aln_amd.hits_purge(ctx, pool, pool, hits, n_hits, alphabet, table, 11, 1, MAX_IDENTITY, MIN_OVERLAP, w_max=W_MAX,
                                  align_type=mode)

    def detour():
        res = purge()
        return res, [aln_amd.pssm_from_counts(res[4][r][1:-1], background, fallback[r], pseudo=float(BETA), scale=float(SCALE))
                     for r in range(rows)]

    a, full, b = rows_only(), pssm(), purge()
    routes = aln_amd.hits_align_routes(ctx)
    assert a[7] == 0 and b[6] == 0 and a[0].tobytes() == b[0].tobytes(), "records differ"
    for mine, its in ((0, 0), (2, 1), (3, 2), (4, 3), (6, 5)):
        assert full[mine].tobytes() == b[its].tobytes(), "optional output %d differs from hits_purge's" % mine
    assert all(x.tobytes() == y.tobytes() for x, y in zip(full[5], b[4])), "counts differ"
    assert all(x.tobytes() == y.tobytes() for x, y in zip(full[1], a[1])), "rows differ with and without the optional outputs"
    check = min(rows, CHECK_ROWS)
    for r in range(check):
        want = aln_amd.pssm_rows_from_counts(b[4][r][1:-1], bg, BETA, SCALE, fallback[r])
        assert a[1][r][1:-1].tobytes() == want.tobytes() and not a[1][r][[0, -1]].any(), "rows differ from the integer rule, query %d" % r
    host = detour()[1]
    differ = sum(int((a[1][r][1:-1] != host[r]).sum()) for r in range(rows))     # where float64 and the libm round otherwise
    fns = (("a_hits_pssm_rows_only", rows_only), ("b_hits_purge_with_counts", purge), ("c_hits_purge_then_pssm_from_counts", detour))
    times = {key: [] for key, _ in fns}
    for _, fn in fns:
        fn()                                                        # warm-up
    for _ in range(REPS):
        for key, fn in fns:
            t0 = time.perf_counter()
            fn()
            times[key].append(time.perf_counter() - t0)
    off = pool.offsets
    n_used, n_rows, n_letters = int(n_hits.sum()), int(off[rows] - off[0]), len(alphabet)
    out = {"align_type": name, "n_queries": rows, "n_templates": n, "K": K, "hits": n_used, "rows_checked_against_integers": check,
           "optional_outputs_equal_hits_purge": True, "entries_differing_from_float64_detour": differ,
           "entries": sum(int(x.size) for x in host), "routes_fused_batched": routes, "max_identity": MAX_IDENTITY,
           "min_overlap": MIN_OVERLAP, "w_max": W_MAX, "beta": BETA, "scale": SCALE,
           "a_download_bytes": n_used * (32 + 4) + rows * K * (16 + 4) + n_rows * n_letters * 4,   # records, same; purge, weights (kept by the call); rows
           "b_download_bytes": n_used * (32 + 4) + rows * K * (16 + 12) + n_rows * 128}            # records, same; purge; weights, raw; count rows
    for key, _ in fns:
        out[key] = stat(times[key])
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
