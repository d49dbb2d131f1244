#!/usr/bin/env python3
"""The query-anchored pileup of search hits, two ways on the slice tools/bench_search.py times: the first Q of T synthetic
proteins, length U[400,600] (seed 5000+s), against all of them, 11/1 BLOSUM62, the K best templates of every query.

  (a) device  aln_hits_pileup with all three outputs: one wave per hit sweeps, walks back through its 1 B/cell strip and stores
              the letters and template positions of its row on the device; per hit the record, the span and the two rows of
              the block's longest query come down
  (b) host    aln_hits_align with pair lists and no lines (rows x K x pair_stride x 2 int32 come down), then a vectorised
              numpy scatter into the same three arrays — what a caller had to do before
  (c)         aln_hits_align with neither lists nor lines: the records only, for scale
The outputs of (a) and (b) must be byte-identical (asserted first).  Then the three alternate in one process, `reps` rounds
after a warm-up; each is reported as median (min - max) in ms.  Prints one JSON line.
usage: bench_pileup.py [Q] [T] [K] [align type, default local]"""
import ctypes as C
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

    # what (b) reads on the host: the pool's blob, lengths and offsets
    blob = np.frombuffer(pool.blob, np.uint8)
    off = pool.offsets
    Qn = (off[1:rows + 1] - off[:rows])[:, None]                                # rows x 1
    width = int(Qn.max()) - 2                                                   # the line stride: the longest query
    used = np.arange(K)[None, :] < n_hits[:, None]
    t_of = np.where(used, hits["t"], 0)
    Tn, t0 = off[t_of + 1] - off[t_of], off[t_of]                               # rows x K
    stride = int(min(Qn.max(), (off[1:] - off[:-1]).max())) + 3
    sub = aln_amd.AlnSubmatrix(len(alphabet), alphabet.encode(), table.ctypes.data_as(C.POINTER(C.c_float)))
    gap = aln_amd._const_gap(mode, 11, 1)
    ip = C.POINTER(C.c_int32)
    col = np.arange(width)[None, None, :]

    def device():
        return aln_amd.hits_pileup(ctx, pool, pool, hits, n_hits, alphabet, table, 11, 1, align_type=mode, line_stride=width)

    def align(want_pairs):
        rec = np.zeros((rows, K), dtype=aln_amd.HIT_ALIGNMENT_DTYPE)
        pairs = np.zeros((rows, K, stride, 2), dtype=np.int32) if want_pairs else None
        rc = aln_amd.lib().aln_hits_align(ctx.h, C.byref(pool.c), C.byref(pool.c), C.byref(sub), C.byref(gap), 0, rows, K,
                                          hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits.ctypes.data_as(ip),
                                          rec.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)),
                                          pairs.ctypes.data_as(ip) if want_pairs else None, stride if want_pairs else 0, None, None, 0, None)
        assert rc == 0, rc
        return rec, pairs

    def host():
        rec, pairs = align(True)
        i, j = pairs[..., 0].astype(np.int64), pairs[..., 1].astype(np.int64)
        ok = used & (rec["status"] == 0) & ((rec["score"] > 0) if mode == aln_amd.LOCAL else True)
        m = ok[..., None] & (np.arange(stride)[None, None, :] < rec["n_pairs"][..., None])
        m &= (i >= 1) & (i <= Qn[..., None] - 2) & (j >= 1) & (j <= Tn[..., None] - 2)
        r_, k_, e_ = np.nonzero(m)
        ii, jj = i[r_, k_, e_], j[r_, k_, e_]
        tpos = np.zeros((rows, K, width), np.uint16)
        tpos[r_, k_, ii - 1] = jj
        some = m.any(axis=2)
        lo = np.where(m, i, np.iinfo(np.int64).max).min(axis=2)
        hi = np.where(m, i, -1).max(axis=2)
        letters = np.where(used[..., None] & (col < Qn[..., None] - 2), ord("."), 0).astype(np.uint8)
        letters[some[..., None] & (col >= lo[..., None] - 1) & (col <= hi[..., None] - 1)] = ord("-")
        letters[r_, k_, ii - 1] = blob[t0[r_, k_] + jj]
        spans = np.zeros((rows, K), dtype=aln_amd.HIT_SPAN_DTYPE)
        rs, ks = np.nonzero(some)
        spans["q_lo"][rs, ks], spans["q_hi"][rs, ks] = lo[rs, ks], hi[rs, ks]
        spans["t_lo"][rs, ks] = tpos[rs, ks, lo[rs, ks] - 1]
        spans["t_hi"][rs, ks] = tpos[rs, ks, hi[rs, ks] - 1]
        return rec, spans, letters, tpos

    a, b = device(), host()
    assert a[4] == 0 and a[0].tobytes() == b[0].tobytes(), "records differ"
    assert a[1].tobytes() == b[1].tobytes(), "spans differ"
    assert a[2].tobytes() == b[2].tobytes(), "letters differ"
    assert a[3].tobytes() == b[3].tobytes(), "tpos differs"
    routes = aln_amd.hits_align_routes(ctx)
    fns = (("a_pileup", device), ("b_hits_align_pairs_plus_scatter", host), ("c_hits_align_records_only", lambda: align(False)))
    times = {key: [] for key, _ in fns}
    for _, fn in fns:
        fn()                                                        # warm-up
    for _ in range(REPS):
        for key, fn in fns:
            t0_ = time.perf_counter()
            fn()
            times[key].append(time.perf_counter() - t0_)
    out = {"align_type": name, "n_queries": rows, "n_templates": n, "K": K, "hits": int(n_hits.sum()), "outputs_equal": True,
           "routes_fused_batched": routes, "aligned_pairs": int((b[3] > 0).sum()), "line_stride": width,
           "a_download_bytes": int(n_hits.sum()) * (width * 3 + 16 + 32 + 4),   # rows, span, the kernel's record, same
           "b_download_bytes": rows * K * stride * 8 + rows * K * 16}
    for key, _ in fns:
        out[key] = stat(times[key])
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
