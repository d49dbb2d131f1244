#!/usr/bin/env python3
"""Alignments of the hits of a PROFILE search, three routes on the slice tools/bench_align_hits.py times: the first Q of T
synthetic proteins, length U[400,600] (seed 5000+s), against all of them, 11/1, the K best templates of every query.  The
profiles are derived from the slice's queries (row i = BLOSUM62's row of residue i) and the consensus is those queries, so the
residue entry computes the same alignments.

  (a) profiles  aln_hits_align_profiles: one wave per hit, rows staged from HBM into LDS, 1 byte per cell into a transient strip
  (b) planes    what callers did before that entry existed: one resident Batch over the hits with aln_amd.profile_planes (a
                Q x T float plane per hit expanded on the host, 4 B/cell uploaded) + optimal + optimal_strings
  (c) table     aln_hits_align on the same hits: the like-for-like table twin of (a)
a, b and c must be byte-identical — records, lists, lines, identities (checked before anything is timed).  Each is timed as the
median of 5 repetitions after a warm-up (min and max are printed too); aln_hits_align_last_routes is reported for a and c.
Prints one JSON line.
usage: bench_align_hits_profiles.py [Q] [T] [K] [align type, default local]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alignment-algos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import aln_amd  # noqa: E402
from aln_amd.synth import MT19937, residues  # noqa: E402
from bench_align_hits import ALIGN_TYPES, stat, timed  # noqa: E402


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
    tpool = aln_amd.SeqPool(seqs)
    queries = seqs[:rows]
    qpool = aln_amd.SeqPool(queries)
    profiles = aln_amd.profiles_from_sequences(queries, alphabet, table)
    ctx = aln_amd.Context(0)
    hits, n_hits = aln_amd.search_topk_profiles(ctx, profiles, tpool, 11, 1, K, align_type=mode)
    used = [(r, c) for r in range(rows) for c in range(K) if c < n_hits[r]]
    routes = {}

    def a_profiles():
        res = aln_amd.hits_align_profiles(ctx, profiles, tpool, hits, n_hits, 11, 1, consensus=qpool, align_type=mode)
        routes["a"] = aln_amd.hits_align_routes(ctx)
        return res

    def b_planes():
        b = aln_amd.Batch(ctx, qpool, tpool, [r for r, c in used], [int(hits["t"][r, c]) for r, c in used])
        try:
            b.dp_simmatrix([aln_amd.profile_planes(profiles.profiles[r], seqs[hits["t"][r, c]], alphabet) for r, c in used], mode, 11, 1)
            scores, lists, status = b.optimal()
            s2, ident, st2, tl, ql = b.optimal_strings()
        finally:
            b.close()
        return scores, lists, status, ident, tl, ql

    def c_table():
        res = aln_amd.hits_align(ctx, qpool, tpool, hits, n_hits, alphabet, table, 11, 1, align_type=mode)
        routes["c"] = aln_amd.hits_align_routes(ctx)
        return res

    a, b, c = a_profiles(), b_planes(), c_table()
    assert a[5] == 0 and c[5] == 0 and not b[2].any()
    assert a[0].tobytes() == c[0].tobytes() and np.array_equal(a[4], c[4]) and a[2] == c[2] and a[3] == c[3]
    assert all(np.array_equal(x, y) for ra, rc_ in zip(a[1], c[1]) for x, y in zip(ra, rc_))
    for p, (r, col) in enumerate(used):
        e = a[0][r, col]
        assert e["status"] == 0 and e["n_pairs"] == len(b[1][p]) and np.array_equal(a[1][r][col], b[1][p]), (r, col)
        assert np.float32(e["score"]).view(np.uint32) == b[0][p].view(np.uint32), (r, col)
        assert np.float32(e["identity"]).view(np.uint32) == b[3][p].view(np.uint32), (r, col)
        assert (a[2][r][col], a[3][r][col]) == (b[4][p], b[5][p]), (r, col)
    del a, b, c
    t_a, t_c, t_b = timed(a_profiles), timed(c_table), timed(b_planes)
    out = {"align_type": name, "n_queries": rows, "n_templates": n, "K": K, "hits": len(used), "outputs_equal": True,
           "a_routes_fused_batched": routes["a"], "c_routes_fused_batched": routes["c"],
           "a_hits_align_profiles": stat(t_a), "b_batch_over_profile_planes": stat(t_b), "c_hits_align": stat(t_c)}
    for key in ("a_hits_align_profiles", "b_batch_over_profile_planes", "c_hits_align"):
        s = out[key]
        print("%-28s %9.1f ms  (%.1f - %.1f)" % (key, s["median_ms"], s["min_ms"], s["max_ms"]))
    print("routes (fused, batched): a %s  c %s" % (routes["a"], routes["c"]))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
