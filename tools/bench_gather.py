#!/usr/bin/env python3
"""What the gather of a multi-rank step costs the launching thread, on one rank: a resident batch of small pairs runs
`reevaluate; optimal_enqueue; gather; optimal_collect` once with Comm.gather (aln_gather_scores: host round trip, blocking) and
once with Comm.gather_enqueue + gather_collect of the PREVIOUS step (aln_gather_resident_*).  Prints the median host time per
step of both loops and the median time inside gather / gather_enqueue alone.  (Comm.gather needs the scores on the host, so
its loop collects Optimal before the gather; the resident loop after it.)  A number, not a threshold.
usage: bench_gather.py [N_PAIRS] [STEPS]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alignment-algos_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import aln_amd  # noqa: E402
import orc  # noqa: E402
from aln_amd.shard import Comm, deal_units, local_units  # noqa: E402
from aln_amd.synth import random_pair  # noqa: E402

n_pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
warmup = 10
alphabet, table = orc.load_blosum(os.path.join(ROOT, "tests", "golden", "BLOSUM62"))
pairs = [random_pair(9000 + n, 40 + n % 61, 100 - n % 53) for n in range(n_pairs)]
owner, slot = deal_units([(len(q) + 2) * (len(t) + 2) for q, t in pairs], 1)
mine = local_units(owner, slot, 0)
ctx = aln_amd.Context(0)
b = aln_amd.Batch(ctx, [pairs[k][0] for k in mine], [pairs[k][1] for k in mine])
b.dp_submatrix(alphabet, table, aln_amd.LOCAL, 11, 1)
want = b.optimal(want_pairs=False)[0]
comm = Comm(ctx, 1, 0)
out = np.zeros(n_pairs, np.float32)


def host_loop():
    step, inside = [], []
    for j in range(warmup + steps):
        t0 = time.perf_counter()
        b.reevaluate()
        b.optimal_enqueue()
        scores = b.optimal_collect()[0]
        t1 = time.perf_counter()
        comm.gather(scores, mine, n_pairs, n_pairs, out=out)
        t2 = time.perf_counter()
        step.append(t2 - t0)
        inside.append(t2 - t1)
    assert np.array_equal(out[mine].view(np.uint32), want.view(np.uint32))
    return np.median(step[warmup:]) * 1e6, np.median(inside[warmup:]) * 1e6


def resident_loop():
    step, inside = [], []
    pending = False
    for j in range(warmup + steps):
        t0 = time.perf_counter()
        b.reevaluate()
        b.optimal_enqueue()
        t1 = time.perf_counter()
        comm.gather_enqueue(b, mine, n_pairs, n_pairs)
        t2 = time.perf_counter()
        if pending:
            comm.gather_collect(n_pairs, out=out)          # the previous step's
        b.optimal_collect()
        pending = True
        step.append(time.perf_counter() - t0)
        inside.append(t2 - t1)
    comm.gather_collect(n_pairs, out=out)
    assert np.array_equal(out[mine].view(np.uint32), want.view(np.uint32))
    return np.median(step[warmup:]) * 1e6, np.median(inside[warmup:]) * 1e6


ctx.synchronize()
h_step, h_in = host_loop()
ctx.synchronize()
r_step, r_in = resident_loop()
print("bench_gather: %d pairs, %d steps, 1 rank, %s" % (n_pairs, steps, b.kernel_name()))
print("  Comm.gather                    : %8.1f us per step (median), %7.1f us inside gather" % (h_step, h_in))
print("  gather_enqueue + collect(prev) : %8.1f us per step (median), %7.1f us inside gather_enqueue" % (r_step, r_in))
comm.close()
b.close()
ctx.close()
