#!/usr/bin/env python3
"""aln_search_topk_profiles against aln_search_topk on the slice tools/bench_search.py times: `rows` queries against n synthetic
proteins, length U[400,600] (seed 5000+s), local 11/1 BLOSUM62, the K best templates of every query.  The profiles are derived
from the same queries (row i = the BLOSUM62 row of residue i), so the hits must be byte-identical: that is asserted before
anything is timed.  Three calls, each the median of 5 after a warm-up, in one process:
  profiles        aln_search_topk_profiles (32-bit sweep, rows staged from HBM 8 at a time)
  table32         aln_search_topk with hint score_packed = 0: the like-for-like 32-bit table sweep
  table           aln_search_topk as is (packed 16-bit lanes on this slice)
and the device shares (scoring / selection / end cells) the hint "search_debug" reports for the first two.
usage: bench_search_profiles.py [n] [rows] [K]"""
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alignment-algos_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aln_amd  # noqa: E402
from aln_amd.synth import MT19937, residues  # noqa: E402
from bench_search import captured_stderr  # noqa: E402

REPS = 5


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    K = int(sys.argv[3]) if len(sys.argv) > 3 else 10
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
    profiles = aln_amd.profiles_from_sequences(seqs[:rows], alphabet, table)
    ctx = aln_amd.Context(0)
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    cells = float(lens[:rows].sum()) * float(lens.sum())

    def by_profiles():
        return aln_amd.search_topk_profiles(ctx, profiles, pool, 11, 1, K)

    def by_table():
        return aln_amd.search_topk(ctx, pool, pool, alphabet, table, 11, 1, K, q_end=rows)

    def by_table32():
        with ctx.hints(score_packed=0):
            return by_table()

    ways = [("profiles", by_profiles), ("table32", by_table32), ("table", by_table)]
    got = {name: fn() for name, fn in ways}                         # the warm-up of each, and the comparison
    for name in ("table32", "table"):
        assert got[name][0].tobytes() == got["profiles"][0].tobytes() and np.array_equal(got[name][1], got["profiles"][1]), name
    res = {"n": n, "rows": rows, "K": K, "reps": REPS, "same_hits": True, "profile_rows_bytes": int(profiles.offsets[-1]) * 128}
    for name, fn in ways:
        t = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        res[name + "_s"] = float(np.median(t))
        res[name + "_all_s"] = t
        res[name + "_gcups"] = cells / float(np.median(t)) / 1e9
    for name, fn in ways[:2]:
        with ctx.hints(search_debug=1):
            _, text = captured_stderr(fn)
        m = re.search(r"score_ms ([0-9.]+) select_ms ([0-9.]+) end_ms ([0-9.]+) \((\d+) hits\)", text)
        if m:
            sc, se, en = float(m.group(1)), float(m.group(2)), float(m.group(3))
            res[name + "_device"] = {"score_ms": sc, "select_ms": se, "end_ms": en, "end_hits": int(m.group(4)),
                                     "share_select": se / (sc + se + en), "share_end": en / (sc + se + en)}
    res["profiles_over_table32"] = res["profiles_s"] / res["table32_s"]
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
