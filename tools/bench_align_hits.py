#!/usr/bin/env python3
"""Alignments of search hits, two routes on the slice tools/bench_search.py times: the first Q of T synthetic proteins, length
U[400,600] (seed 5000+s), against all of them, local 11/1 BLOSUM62, the K best templates of every query.

  (a) fused  aln_search_topk + aln_hits_align: one wave per hit sweeps rows 1..q_end, 1 byte per cell into a transient strip,
             walks back, the gapped lines are laid out on the device
  (b) batch  aln_search_topk + aln_amd.align_hits (one resident Batch over all hits, full planes, find_max) + the gapped lines
             rendered on the host (aln_gapped_strings, one call per hit)
Each timed as the median of 5 repetitions after a warm-up (min and max are printed too).  Both routes must give the same pair
lists (checked).  Bytes written per cell: (a) 1 B over rows <= q_end of 256 ceil(T/256) columns, (b) the plane bytes
aln_batch_plane_bytes_per_cell reports over all Q x T cells.  Prints one JSON line.

With a fourth argument, an align type other than local (global_local, global, local_global, semi_local), the search and both
routes run under that type and
  (a) fused  is aln_hits_align as it stands: one wave per hit sweeps every row 1..Q-2, 1 byte per cell into a strip of Q-3 rows
  (b) batch  is the same aln_hits_align call with hint align_fused_nonlocal = 0: every hit through resident batches inside the
             call, lines included — what the call did before the non-local fused kernel existed
and the two calls' outputs must be byte-identical (checked).  aln_hits_align_last_routes is reported for both.
usage: bench_align_hits.py [Q] [T] [K] [align type, default local]"""
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


def stat(v):
    return {"median_ms": 1e3 * float(np.median(v)), "min_ms": 1e3 * float(min(v)), "max_ms": 1e3 * float(max(v)), "reps": len(v)}


def timed(fn, reps=5):
    fn()                                                        # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def host_lines(q, t, pl):
    L = aln_amd.lib()
    qs, ts = ("^" + q + "$").encode(), ("^" + t + "$").encode()
    ali = (aln_amd.AlnAlignment * 1)()
    ali[0].n_pairs, ali[0].pair_off = len(pl), 0
    a = np.ascontiguousarray(pl, dtype=np.int32)
    ip = a.ctypes.data_as(C.POINTER(C.c_int32))
    stride = L.aln_gapped_length(len(ts), ali, 1, ip) + 1
    tl, ql = C.create_string_buffer(stride), C.create_string_buffer(stride)
    rc = L.aln_gapped_strings(qs, len(qs), ts, len(ts), ali, 1, ip, tl, ql, stride)
    assert rc == 0, rc
    return tl.value.decode(), ql.value.decode()


ALIGN_TYPES = {"global_local": aln_amd.GLOBAL_LOCAL, "global": aln_amd.GLOBAL, "local_global": aln_amd.LOCAL_GLOBAL,
               "local": aln_amd.LOCAL, "semi_local": aln_amd.SEMI_LOCAL}


def nonlocal_main(ctx, pool, seqs, alphabet, table, rows, n, K, name):
    mode = ALIGN_TYPES[name]

    def search():
        return aln_amd.search_topk(ctx, pool, pool, alphabet, table, 11, 1, K, q_end=rows, align_type=mode)

    hits, n_hits = search()
    routes = {}

    def fused():
        res = aln_amd.hits_align(ctx, pool, pool, hits, n_hits, alphabet, table, 11, 1, align_type=mode)
        routes["a"] = aln_amd.hits_align_routes(ctx)
        return res

    def batch():
        with ctx.hints(align_fused_nonlocal=0):
            res = aln_amd.hits_align(ctx, pool, pool, hits, n_hits, alphabet, table, 11, 1, align_type=mode)
            routes["b"] = aln_amd.hits_align_routes(ctx)
        return res

    t_search, t_a, t_b = timed(search), timed(fused), timed(batch)
    a, b = fused(), batch()
    assert a[5] == 0 and b[5] == 0 and a[0].tobytes() == b[0].tobytes() and np.array_equal(a[4], b[4])
    assert a[2] == b[2] and a[3] == b[3]
    assert all(np.array_equal(x, y) for ra, rb in zip(a[1], b[1]) for x, y in zip(ra, rb))
    used = [(r, c) for r in range(rows) for c in range(K) if c < n_hits[r]]
    cells_all = strip = 0
    for r, c in used:
        Qn, Tn = len(seqs[r]) + 2, len(seqs[hits["t"][r, c]]) + 2
        cells_all += Qn * Tn
        strip += max(Qn - 3, 1) * 256 * ((Tn + 255) // 256)
    bt = aln_amd.Batch(ctx, pool, pool, [0], [int(hits["t"][0, 0])])
    bt.dp_submatrix(alphabet, table, mode, 11, 1)
    plane_b = bt.plane_bytes_per_cell()
    bt.close()
    med = lambda v: float(np.median(v))   # noqa: E731
    print(json.dumps({"align_type": name, "n_queries": rows, "n_templates": n, "K": K, "hits": len(used), "outputs_equal": True,
                      "a_routes_fused_batched": routes["a"], "b_routes_fused_batched": routes["b"],
                      "search_topk": stat(t_search), "a_hits_align": stat(t_a), "b_hits_align_through_batches": stat(t_b),
                      "a_total_median_ms": 1e3 * (med(t_search) + med(t_a)), "b_total_median_ms": 1e3 * (med(t_search) + med(t_b)),
                      "a_bytes_written": strip, "a_bytes_per_matrix_cell": strip / float(cells_all),
                      "b_bytes_written": plane_b * cells_all, "b_bytes_per_matrix_cell": plane_b}))
    return 0


def main():
    arg = lambda k, d: int(sys.argv[k]) if len(sys.argv) > k else d   # noqa: E731
    rows, n, K = arg(1, 512), arg(2, 4096), arg(3, 10)
    align_type = sys.argv[4] if len(sys.argv) > 4 else "local"
    if align_type not in ALIGN_TYPES:
        sys.exit("align type: one of " + ", ".join(ALIGN_TYPES))
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
    if align_type != "local":
        return nonlocal_main(ctx, pool, seqs, alphabet, table, rows, n, K, align_type)

    def search():
        return aln_amd.search_topk(ctx, pool, pool, alphabet, table, 11, 1, K, q_end=rows)

    hits, n_hits = search()

    def fused():
        return aln_amd.hits_align(ctx, pool, pool, hits, n_hits, alphabet, table, 11, 1)

    def batch():
        scores, lists = aln_amd.align_hits(ctx, pool, pool, hits, n_hits, alphabet, table, 11, 1)
        flat = hits.reshape(-1)
        used = np.nonzero((np.arange(K)[None, :] < n_hits[:, None]).reshape(-1))[0]
        return scores, lists, [host_lines(seqs[s // K], seqs[flat["t"][s]], lists[p]) for p, s in enumerate(used)]

    t_search, t_a, t_b = timed(search), timed(fused), timed(batch)
    rec, lists_a, tl, ql, lengths, rc = fused()
    scores_b, lists_b, lines_b = batch()
    used = [(r, c) for r in range(rows) for c in range(K) if c < n_hits[r]]
    assert rc == 0 and len(used) == len(lists_b)
    cells_all = strip = 0
    for p, (r, c) in enumerate(used):
        assert np.array_equal(lists_a[r][c], lists_b[p]), (r, c)
        assert (tl[r][c], ql[r][c]) == lines_b[p], (r, c)
        Qn, Tn = len(seqs[r]) + 2, len(seqs[hits["t"][r, c]]) + 2
        cells_all += Qn * Tn
        strip += max(int(hits["q_end"][r, c]) - 1, 1) * 256 * ((Tn + 255) // 256)
    b = aln_amd.Batch(ctx, pool, pool, [0], [int(hits["t"][0, 0])])
    b.dp_submatrix(alphabet, table, aln_amd.LOCAL, 11, 1)
    plane_b = b.plane_bytes_per_cell()
    b.close()
    med = lambda v: float(np.median(v))   # noqa: E731
    print(json.dumps({"n_queries": rows, "n_templates": n, "K": K, "hits": len(used), "lists_equal": True, "lines_equal": True,
                      "search_topk": stat(t_search), "a_hits_align": stat(t_a), "b_align_hits_plus_host_lines": stat(t_b),
                      "a_total_median_ms": 1e3 * (med(t_search) + med(t_a)), "b_total_median_ms": 1e3 * (med(t_search) + med(t_b)),
                      "a_bytes_written": strip, "a_bytes_per_matrix_cell": strip / float(cells_all),
                      "b_bytes_written": plane_b * cells_all, "b_bytes_per_matrix_cell": plane_b}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
