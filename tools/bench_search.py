#!/usr/bin/env python3
"""All-vs-all SEARCH on the slice tools/bench_c5.py times: `rows` queries against n synthetic proteins, length U[400,600]
(seed 5000+s), local 11/1 BLOSUM62, the K best templates of every query.

Two ways to the same hits, each timed as the median of `reps` repetitions after a warm-up:
  (1) dense  aln_score_all_vs_all + numpy.argpartition / sort on the host (all a caller could do before aln_search_topk)
  (2) search aln_search_topk: selection and end cells on the device, only rows x K hits travel
and the share of (2) the device spends scoring / selecting / in the end kernels, from the HIP events the context hint
"search_debug" makes the library report.  The two hit lists are compared before anything is printed.
usage: bench_search.py [n] [rows] [K] [reps]"""
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alignment-algos_amd"))
import aln_amd  # noqa: E402
from aln_amd.synth import MT19937, residues  # noqa: E402


def host_topk(dense, K):
    """what a caller of the dense path does: argpartition, then order the K survivors (score descending, index ascending)"""
    n_t = dense.shape[1]
    k = min(K, n_t)
    out = np.empty((dense.shape[0], k), dtype=np.int64)
    for r in range(dense.shape[0]):
        s = dense[r]
        if k < n_t:
            kth = np.partition(s, n_t - k)[n_t - k]
            cand = np.nonzero(s >= kth)[0]                     # every tie of the K-th score, so that the index rule can be applied
        else:
            cand = np.arange(n_t)
        out[r] = cand[np.lexsort((cand, -s[cand]))][:k]
    return out


def captured_stderr(fn):
    """run fn with the process's stderr (the C library's included) going to a file; -> (result, text)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            res = fn()
        finally:
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return res, tmp.read().decode(errors="replace")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    K = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
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
    cells = float(lens[:rows].sum()) * float(lens.sum())

    def dense_way():
        return host_topk(aln_amd.score_all_vs_all(ctx, pool, pool, alphabet, table, 11, 1, 0, rows), K)

    def search_way():
        return aln_amd.search_topk(ctx, pool, pool, alphabet, table, 11, 1, K, q_end=rows)

    want = dense_way()                                          # warm-up of both, and the comparison
    hits, n_hits = search_way()
    same = bool((n_hits == want.shape[1]).all() and np.array_equal(hits["t"][:, :want.shape[1]], want))
    t_dense, t_score, t_search = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        d = aln_amd.score_all_vs_all(ctx, pool, pool, alphabet, table, 11, 1, 0, rows)
        t1 = time.perf_counter()
        host_topk(d, K)
        t2 = time.perf_counter()
        t_dense.append(t2 - t0)
        t_score.append(t1 - t0)
        t0 = time.perf_counter()
        search_way()
        t_search.append(time.perf_counter() - t0)
    with ctx.hints(search_debug=1):
        _, text = captured_stderr(search_way)
    m = re.search(r"score_ms ([0-9.]+) select_ms ([0-9.]+) end_ms ([0-9.]+) \((\d+) hits\)", text)
    dev = {"score_ms": float(m.group(1)), "select_ms": float(m.group(2)), "end_ms": float(m.group(3)), "end_hits": int(m.group(4))} if m else {}
    med = lambda v: float(np.median(v))     # noqa: E731
    res = {"n": n, "rows": rows, "K": K, "reps": reps, "same_hits": same,
           "dense_plus_host_topk_s": med(t_dense), "dense_scores_only_s": med(t_score), "search_topk_s": med(t_search),
           "dense_all_s": t_dense, "search_all_s": t_search,
           "search_gcups": cells / med(t_search) / 1e9, "dense_gcups": cells / med(t_dense) / 1e9,
           "bytes_to_host_dense": rows * n * 4, "bytes_to_host_search": rows * K * 16 + rows * 4, "device": dev}
    if dev:
        tot = dev["score_ms"] + dev["select_ms"] + dev["end_ms"]
        res["share_select"] = dev["select_ms"] / tot
        res["share_end"] = dev["end_ms"] / tot
    print(json.dumps(res))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
