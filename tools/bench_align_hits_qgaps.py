#!/usr/bin/env python3
"""aln_hits_align_profiles_gaps against aln_hits_align_profiles on the slice tools/bench_search_qgaps.py times: NQ profiles
derived from the first NQ of NT synthetic proteins (length U[400,600], seed 5000+s, BLOSUM62 rows), the K best templates of every
profile.  The hits come from aln_search_topk_profiles_gaps under CONSTANT gap rows (11 / 1 in every row).  First the outputs
of the new entry under those rows — records, lists, both lines, lengths — are asserted byte-identical to
aln_hits_align_profiles' under gap 11 / 1 on the same hits.  Then the two are timed alternating in one process, 7 rounds after
a warm-up: median (min - max) of each and their ratio; the yardstick is aln_hits_align_profiles on the same build and box.
Last, one call with random per-row gaps (every entry in 0..12) on the hits of a search under those rows.
usage: bench_align_hits_qgaps.py NQ NT K [align type: local | semi_local | global | global_local | local_global]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alignment-algos_amd"))
import aln_amd  # noqa: E402
from aln_amd.synth import MT19937, residues  # noqa: E402

ROUNDS = 7
MODES = {"local": aln_amd.LOCAL, "semi_local": aln_amd.SEMI_LOCAL, "global": aln_amd.GLOBAL, "global_local": aln_amd.GLOBAL_LOCAL,
         "local_global": aln_amd.LOCAL_GLOBAL}


def main():
    nq = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    nt = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    K = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    mode_name = sys.argv[4] if len(sys.argv) > 4 else "local"
    mode = MODES[mode_name]
    lines = open(os.path.join(ROOT, "tests", "golden", "BLOSUM62")).read().split("\n")
    k = 0
    while lines[k].startswith("#"):
        k += 1
    alphabet = "".join(lines[k].split())
    table = np.array([[float(x) for x in l.split()[1:]] for l in lines[k + 1:k + 1 + len(alphabet)]], dtype=np.float32)
    seqs = []
    for s in range(nt):
        g = MT19937(5000 + s)
        seqs.append(residues(g, 400 + int(g.draw(1)[0] % 201)))
    pool = aln_amd.SeqPool(seqs)
    profiles = aln_amd.profiles_from_sequences(seqs[:nq], alphabet, table)
    flat = aln_amd.QueryGaps.constant(profiles, 11, 1)
    rng = np.random.RandomState(1)
    rand = aln_amd.QueryGaps(*[[rng.randint(0, 13, len(p) + 1) for p in profiles.profiles] for _ in range(4)])
    ctx = aln_amd.Context(0)
    hits, n_hits = aln_amd.search_topk_profiles_gaps(ctx, profiles, flat, pool, K, align_type=mode)
    rhits, rn_hits = aln_amd.search_topk_profiles_gaps(ctx, profiles, rand, pool, K, align_type=mode)
    lens = np.array([len(s) + 2 for s in seqs], dtype=np.int64)
    cells = float(sum(int(lens[r]) * int(lens[hits["t"][r, k]]) for r in range(nq) for k in range(int(n_hits[r]))))

    def constant_gap():
        return aln_amd.hits_align_profiles(ctx, profiles, pool, hits, n_hits, 11, 1, consensus=seqs[:nq], align_type=mode)

    def gap_rows():
        return aln_amd.hits_align_profiles_gaps(ctx, profiles, flat, pool, hits, n_hits, consensus=seqs[:nq], align_type=mode)

    def random_rows():
        return aln_amd.hits_align_profiles_gaps(ctx, profiles, rand, pool, rhits, rn_hits, consensus=seqs[:nq], align_type=mode)

    want, got = constant_gap(), gap_rows()                         # the warm-up of each, and the comparison
    assert got[0].tobytes() == want[0].tobytes(), "records under constant gap rows differ"
    assert all(np.array_equal(x, y) for ra, rb in zip(got[1], want[1]) for x, y in zip(ra, rb)), "lists differ"
    assert got[2] == want[2] and got[3] == want[3] and np.array_equal(got[4], want[4]) and got[5] == want[5] == 0, "lines differ"
    routes = aln_amd.hits_align_routes(ctx)
    res_rand = random_rows()
    assert res_rand[5] == 0 and (res_rand[0]["status"] == 0).all(), "a slot under random rows was refused"
    t = {"constant_gap": [], "gap_rows": []}
    for _ in range(ROUNDS):
        for name, fn in (("constant_gap", constant_gap), ("gap_rows", gap_rows)):
            t0 = time.perf_counter()
            fn()
            t[name].append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    random_rows()
    t_rand = time.perf_counter() - t0
    res = {"nq": nq, "nt": nt, "K": K, "align_type": mode_name, "rounds": ROUNDS, "same_outputs": True, "slots": int(n_hits.sum()),
           "routes_gap_rows": list(routes), "swept_cells_upper_bound": cells}
    for name, v in t.items():
        res[name + "_s"] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    res["gap_rows_over_constant_gap"] = float(np.median(t["gap_rows"]) / np.median(t["constant_gap"]))
    res["random_rows_s"] = t_rand
    res["random_rows_over_constant_gap"] = float(t_rand / np.median(t["constant_gap"]))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
