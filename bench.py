#!/usr/bin/env python3
"""bench.py — BASELINE.json config 2 on N MI355X: batched local affine-gap DP (BLOSUM62, 11/1) over 1024 synthetic
2000 x 2000 pairs per GPU — DP build + find_max + pointer traceback — through the C ABI (libalnhip.so).

A step = one pass of the hot path over the resident batch: aln_batch_reevaluate (DP + corner kernels) +
aln_batch_optimal_enqueue/_collect (find_max + traceback, per-pair results to the host).  Sequences are resident in HBM
before the timed region.  Pairs are independent, so ranks own disjoint batches (weak scaling) and the only collective is ONE
gather of the fp32 scores per step: aln_gather_scores (RCCL all-gather over xGMI, csrc/aln_comm.hip) — never torch.

Prints ONE JSON line.  A plain run sets up, calibrates the launch pattern, warms up, times --steps steps and prints the line;
besides the contract's keys it holds:
  roofline      dominant kernel (row-sweep DP).  `achieved` uses the bytes the chosen plane layout MUST write (uint16 score +
                uint16 pointer word = 4 B per matrix cell in this configuration; `contract_bytes` keeps SURVEY 8(d)'s 8 B/cell for
                context) over the measured time; `valu` is the second roof (wave-instructions from profiles/ over the measured
                VALU issue rate); `bound` names the roof with the larger fraction.
--full adds everything that takes runs of its own or checks the result:
  parity        every resident copy of a sub-batch re-run and compared, the gathered scores against them, and the pairs the real
                reference was run on (tests/golden/full_cases.json) against its scores.
  roofline      + this box's measured fill rate (`measured_fill_GBs_this_box`, `frac_of_measured_fill`).
  kernel_only / end_to_end   SURVEY 8(d): kernel time alone, and a pass that also encodes + uploads the residues, copies every
                pair list to the host and builds the gapped strings + identities (aln_batch_optimal_strings).
  secondary     driver-timed figures of configs 3, 4 and 5 on this GPU (rank 0, N = 1).
  cpu_baseline  the reference (oracle/_ref, the real christang/alignment-algos DPMatrix) or the oracle port on this box's host
                cores: one pair alone on an idle core, then one pair per core on all cores.
--dump-outputs DIR writes what the last timed step handed its caller (rank 0): DIR/scores.npy (float32, the gathered scores of
all pairs), DIR/list_lengths.npy and DIR/status.npy (float64, rank 0's pairs).  The workload is seeded: the same arguments give
the same inputs on every run.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "alignment-algos_amd"))

import numpy as np  # noqa: E402

CAL_STEPS = 10          # steps of one calibration region (bench.py picks the launch pattern and the kernel build before the warmup)
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300-6900 GB/s is what a plain fill reaches
# gfx950 VALU issue, measured with tools/valu_rate2.hip / valu_occ.hip: ns per wave64 instruction and SIMD with >= 2 waves issuing
VALU_NS_FULL, VALU_NS_HALF = 0.92, 1.58
N_SIMD = 1024


def make_workload(rank, n_pairs, length):
    """pair p uses seed 1000+p; every second pair is a mutated homolog (long tracebacks)."""
    from aln_amd.synth import homolog_pair, random_pair
    qs, ts = [], []
    for p in range(n_pairs):
        seed = 1000 + rank * n_pairs + p
        q, t = homolog_pair(seed, length) if p % 2 else random_pair(seed, length)
        qs.append(q)
        ts.append(t)
    return qs, ts


def load_blosum():
    lines = open(os.path.join(ROOT, "tests", "golden", "BLOSUM62")).read().split("\n")
    k = 0
    while lines[k].startswith("#"):
        k += 1
    alphabet = "".join(lines[k].split())
    table = np.array([[float(x) for x in l.split()[1:]] for l in lines[k + 1:k + 1 + len(alphabet)]], dtype=np.float32)
    return alphabet, table


def cpu_baseline(qs, ts, mode, gi, ge):
    """the reference's DPMatrix constructor on this box's host cores.  (1) ONE pair on an otherwise idle core;
    (2) one pair per core on all cores the process may use (the first C pairs of rank 0's workload).  The real reference
    binary (oracle/_ref) if it travelled, else the oracle port.  Bounded: about 25 s + 50 s."""
    harness = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
    blosum = os.path.join(ROOT, "tests", "golden", "BLOSUM62")
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, len(qs), 16))      # the GPU box gives one GPU a 16-core share
    if os.path.exists(harness):
        kind = "reference"

        def start(p):
            return subprocess.Popen([harness, "aa", blosum, str(mode), str(gi), str(ge), "fwd", qs[p], ts[p], "ctime", "corner"],
                                    stdout=subprocess.PIPE, text=True)

        def finish(pr):
            out = pr.communicate()[0]
            if pr.returncode != 0:
                raise RuntimeError("reference harness failed")
            return [float(l.split()[1]) for l in out.split("\n") if l.startswith("CTIME")][0]
        t0 = time.time()
        alone = finish(start(0))
        t1 = time.time()
        per = [finish(pr) for pr in [start(p) for p in range(cores)]]
        wall = time.time() - t1
    else:
        kind = "port"
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import orc
        from concurrent.futures import ThreadPoolExecutor
        alpha, table = orc.load_blosum(blosum)

        def one(p):   # the oracle is a C library called through ctypes (releases the GIL)
            S = orc.sim_submatrix(qs[p], ts[p], alpha, table)
            t1 = time.time()
            orc.dp_build(S, orc.Gap(mode, gi, ge))
            return time.time() - t1
        alone = one(0)
        t1 = time.time()
        with ThreadPoolExecutor(cores) as ex:
            per = list(ex.map(one, range(cores)))
        wall = time.time() - t1
    cells = sum(len(qs[p]) * len(ts[p]) for p in range(cores))
    return {"value": cells / wall / 1e9, "unit": "GCUPS", "cores": cores, "kind": kind,
            "sample": "%d pairs %dx%d of the bench workload (rank 0, pairs 0..%d), one pair per core, DPMatrix build only; "
                      "single_core_value = pair 0 run alone first" % (cores, len(qs[0]), len(ts[0]), cores - 1),
            "seconds": round(wall, 3), "slowest_pair_seconds": round(max(per), 3),
            "single_core_value": len(qs[0]) * len(ts[0]) / alone / 1e9, "single_core_seconds": round(alone, 3)}


def pinned_scores(rank, n_pairs, length):
    """Optimal scores of the bench pairs the REAL reference was run on (tests/golden/full_cases.json, oracle/gen_golden_full.py)."""
    path = os.path.join(ROOT, "tests", "golden", "full_cases.json")
    if rank != 0 or length != 2000 or not os.path.exists(path):
        return {}
    with open(path) as f:
        doc = json.load(f)
    return {g["pair"]: np.array([g["opt"]["score"]], dtype=np.uint32).view(np.float32)[0] for g in doc["c2"]["pairs"] if g["pair"] < n_pairs}


def secondary_configs(aln_amd, ctx, alphabet, table, qs, ts, length):
    """Configs 3, 4, 5 on this GPU, timed here (wall clock around synchronised calls) so that they are the driver's numbers
    too.  Every figure names its workload; the parity tests of the same entry points are tests/test_gpu_full_size.py."""
    from aln_amd.synth import MT19937, make_subopt_regions, random_profile, residues
    out = {}
    n = len(qs)
    # ---- config 4: top-K=256 near-optimal alignments per pair from the resident config-2 matrices
    b = aln_amd.Batch(ctx, qs, ts)
    b.dp_submatrix(alphabet, table, aln_amd.LOCAL, 11, 1, aln_amd.FWD, aln_amd.DP_FAST)
    ctx.synchronize()
    flags = make_subopt_regions(length + 2, 10)
    best = first = None
    for rep in range(2):
        t0 = time.perf_counter()
        n_out, scores, lengths, _, status = b.enumerate_all("cw", 256, 0.01, flags, K=258, node_cap=1 << 18, ali_cap=1 << 16,
                                                            want_pairs=False, raise_on_overflow=False)
        dt = time.perf_counter() - t0
        first = dt if first is None else first
        best = dt if best is None else min(best, dt)
    sm, um = b.last_enum_ms()
    created, nodes = b.last_enum_usage()
    out["c4"] = {"workload": "config 4: %d pairs %dx%d resident from the config-2 build, ConstrainedNearOptimal NUM_SUBOPT=256, "
                             "DELTA_RATIO 0.01 (the largest of {0.05, 0.01, 0.005} the reference finishes on these homologs), "
                             "make_subopt_regions(T,10)" % (n, length, length),
                 "value": round(float(created.sum()) / best, 1), "unit": "alignments/s", "seconds": round(best, 4),
                 "value_is": "alignments the searches create (the reference's as.size() before sortSet keeps NUM_SUBOPT) / wall seconds",
                 "alignments_created": int(created.sum()), "alignments_kept": int(n_out.sum()), "trie_nodes": int(nodes.sum()),
                 "aligned_pairs_emitted": int(lengths[lengths > 0].sum()),
                 "search_kernel_ms": round(sm, 3), "unroll_kernel_ms": round(um, 3), "pairs_overflowed": int((status != 0).sum()),
                 "first_call_seconds": round(first, 4),
                 "search": "enumerate_par_kernel: 16 waves per pair take sub-searches from a per-pair ticket ring; block maxima of the score "
                           "plane prune the candidate scans; the set order is rebuilt from the slot tree on host threads; `seconds` is the "
                           "best of two calls, `first_call_seconds` the one that also allocates the node / task pools (kept with the batch)"}
    b.close()
    # ---- config 3: Hmap2Eval profile-profile, global, exact-order DP
    n_prof = 64
    qps = [random_profile(3000 + p, length) for p in range(n_prof)]
    tps = [random_profile(4000 + p, length) for p in range(n_prof)]
    qpool = {k: np.concatenate([p[k] for p in qps]) for k in ("aa", "sse", "conf")}
    tpool = {k: np.concatenate([p[k] for p in tps]) for k in ("aa", "sse", "conf")}
    q_idx = np.arange(n) % n_prof
    t_idx = (np.arange(n) * 7 + np.arange(n) // n_prof) % n_prof
    b = aln_amd.Batch(ctx, ["A" * length] * n_prof, ["A" * length] * n_prof, q_idx, t_idx)
    best = None
    for rep in range(2):
        t0 = time.perf_counter()
        b.dp_hmap2(qpool, tpool, aln_amd.GLOBAL, 4.73, 0.34, 0.5, 1.0, 0.12)
        sc, _, st = b.optimal(want_pairs=False)
        dt = time.perf_counter() - t0
        assert np.all(np.isfinite(sc)), "config 3: a profile pair without a finite score (a degenerate synthetic profile would bound the launch)"
        best = dt if best is None else min(best, dt)
    inner = n * float(length + 2) ** 2 * (2 * length + 4) / 2.0
    out["c3"] = {"workload": "config 3: %d pairs %dx%d (%d + %d distinct synthetic HMAP profiles), Hmap2Eval similarity + z-normalisation "
                             "on the device, min(t1,t2) position gaps 4.73/0.34, global, exact-order DP + Optimal; profile upload included"
                             % (n, length, length, n_prof, n_prof),
                 "value": round(n * length * length / best / 1e9, 3), "unit": "GCUPS", "seconds": round(best, 4),
                 "dp_kernel_ms": round(b.last_dp_ms(), 2), "inner_k_evals_per_s": round(inner / (b.last_dp_ms() * 1e-3), 1),
                 "kernel": b.kernel_name(), "bound": "valu"}
    b.close()
    # ---- config 5: one rank's block of the 4096 x 4096 all-vs-all (512 query rows x 4096 templates), scores only
    seqs = []
    for s in range(4096):
        g = MT19937(5000 + s)
        ln = 400 + int(g.draw(1)[0] % 201)
        seqs.append(residues(g, ln))
    pool = aln_amd.SeqPool(seqs)
    aln_amd.score_all_vs_all(ctx, pool, pool, alphabet, table, 11, 1, 0, 512)     # (same shape as the timed call: pools, code objects)
    t0 = time.perf_counter()
    aln_amd.score_all_vs_all(ctx, pool, pool, alphabet, table, 11, 1, 0, 512)
    dt = time.perf_counter() - t0
    cells = float(sum(len(s) for s in seqs[:512])) * float(sum(len(s) for s in seqs))
    out["c5"] = {"workload": "config 5, one of 8 ranks' share: 512 query rows x 4096 templates of the 4096-sequence set (400-600 aa), "
                             "local 11/1, scores only; residue upload and score download included",
                 "value": round(cells / dt / 1e9, 1), "unit": "GCUPS", "seconds": round(dt, 4), "bound": "valu"}
    # second roof of these VALU-bound kernels: wave-instructions (SQ_INSTS_VALU of the r03_sec profile set, same workloads) over the
    # kernels' time in THIS run, against the measured full-rate issue of 1024 SIMDs (one wave64 instruction per 0.92 ns and SIMD)
    pfile = os.path.join(ROOT, "profiles", "pmc_secondary.json")
    if os.path.exists(pfile) and n == 1024 and length == 2000:
        try:
            pj = json.load(open(pfile))
            peak = N_SIMD / (VALU_NS_FULL * 1e-9) / 1e12                           # T wave-instructions / s
            c3i = sum(k["valu_insts_per_call"] for k in pj["c3"])
            out["c3"]["roofline"] = {"bound": "valu", "achieved": round(c3i / (out["c3"]["dp_kernel_ms"] * 1e-3) / 1e12, 4), "peak": round(peak, 4),
                                     "unit": "T wave64 VALU instructions/s", "frac": round(c3i / (out["c3"]["dp_kernel_ms"] * 1e-3) / 1e12 / peak, 4),
                                     "valu_insts_per_call": c3i, "kernel_ms": out["c3"]["dp_kernel_ms"], "source": pj["source"]}
            c5i = sum(k["valu_insts_per_call"] for k in pj["c5"])
            out["c5"]["roofline"] = {"bound": "valu", "achieved": round(c5i / out["c5"]["seconds"] / 1e12, 4), "peak": round(peak, 4),
                                     "unit": "T wave64 VALU instructions/s", "frac": round(c5i / out["c5"]["seconds"] / 1e12 / peak, 4),
                                     "valu_insts_per_call": c5i, "seconds": out["c5"]["seconds"], "source": pj["source"],
                                     "note": "time = the whole call (uploads and the score download included)"}
            c4i = sum(k["valu_insts_per_call"] for k in pj["c4"])
            out["c4"]["roofline"] = {"bound": "latency (dependent memory round trips)", "valu_frac": round(c4i / (out["c4"]["search_kernel_ms"] * 1e-3) / 1e12 / peak, 4),
                                     "valu_insts_per_call": c4i, "source": pj["source"]}
        except Exception:
            pass
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=1024, help="pairs per GPU (config 2: 1024)")
    ap.add_argument("--length", type=int, default=2000)
    ap.add_argument("--full", action="store_true",
                    help="also the parity checks, the fill-rate roof, kernel_only, end_to_end, the config 3/4/5 figures and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's results (scores, list lengths, status) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the config 3/4/5 figures and the end-to-end pass")
    ap.add_argument("--streams", "--batches", dest="batches", type=int, default=0,
                    help="HIP streams (contexts) the launches rotate over (1 = everything on one stream; 0 = calibrate the launch pattern)")
    ap.add_argument("--alt-prio", type=int, default=-1, help="tagged kernel's row-alternating wave priority: -1 = calibrate")
    ap.add_argument("--occupancy", type=int, default=-1, help="tagged kernel's waves per SIMD (2 or 3): -1 = calibrate")
    ap.add_argument("--split", type=int, default=0,
                    help="launches a step's batch is processed in (sub-batches of pairs/split pairs; 1 = one launch per step; 0 = calibrate)")
    ap.add_argument("--lone-steps", type=int, default=10, help="with --full: lone launches (one stream, whole batch) timed after the main region for kernel_only")
    ap.add_argument("--trace-steps", action="store_true", help="add the host time stamps of every timed step to the JSON line")
    return ap.parse_args(argv)


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start N rank processes of this very script — fresh children, before this
    process has made any GPU call (it never does: no torch, no HIP here) — relay rank 0's JSON line, exit with the worst code.
    One process per GPU, rendezvous on 127.0.0.1 (the same environment torch.distributed.run would set)."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), ALN_BENCH_SPAWNED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr))
    out0 = procs[0].communicate()[0]
    worst = procs[0].returncode
    deadline = time.time() + 120
    for pr in procs[1:]:
        try:
            pr.wait(timeout=max(1.0, deadline - time.time()))
        except subprocess.TimeoutExpired:
            pr.kill()                                       # this exact child: rank 0 is gone, the others cannot finish
            pr.wait()
        worst = worst or pr.returncode
        if pr.returncode and pr.returncode < 0:
            worst = worst or 1
    for line in out0.decode().splitlines():                # stdout carries the ONE JSON line; library chatter goes to stderr
        (sys.stdout if line.startswith("{") else sys.stderr).write(line + "\n")
    sys.stdout.flush()
    return 0 if worst == 0 else (worst if worst > 0 else 1)


class RehearsalBatch:
    """ALN_BENCH_REHEARSE=cpu only: stands in for a resident batch so that the N > 1 CONTROL FLOW (spawn, rendezvous, launch
    rotation, one gather per step, agreement check, max over ranks, one JSON line) can run on a machine without a GPU.
    It computes nothing — its "scores" are the pairs' global indices — and the line it produces says so (`rehearsal`)."""

    def __init__(self, first_index, n):
        self.n = n
        self.sc = np.arange(first_index, first_index + n, dtype=np.float32)
        self.pending = 0

    def reevaluate(self):
        pass

    def optimal_enqueue(self):
        self.pending += 1

    def optimal_collect(self):
        assert self.pending > 0
        self.pending -= 1
        return self.sc.copy(), np.ones(self.n, np.int32), np.zeros(self.n, np.int32)

    def optimal(self, want_pairs=False):
        return self.sc.copy(), None, np.zeros(self.n, np.int32)

    def dp_ms_history(self, n):
        return np.zeros(0, np.float32)

    def close(self):
        pass


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))
    rank_main(args)


def rank_main(args):
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("WORLD_SIZE %d != --gpus %d" % (world, args.gpus))
    # rehearsals of the N > 1 control flow (never measurements): "cpu" = no GPU at all, gloo, stand-in batches;
    # ALN_BENCH_REHEARSE_ON_ONE_GPU=1 = the real kernels, every rank on device 0, gloo instead of RCCL
    cpu_rehearsal = os.environ.get("ALN_BENCH_REHEARSE") == "cpu"
    rehearse = cpu_rehearsal or os.environ.get("ALN_BENCH_REHEARSE_ON_ONE_GPU") == "1"
    if rehearse:
        local_rank = 0
    import torch
    import torch.distributed as dist
    dev = None
    if not cpu_rehearsal:
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearse:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    from aln_amd.shard import Comm, GlooComm
    mode, gi, ge = 3, 11, 1                                # aln_amd.LOCAL
    aln_amd, qs, ts, alphabet, table = None, None, None, None, None
    if not cpu_rehearsal:
        import aln_amd
        alphabet, table = load_blosum()
        mode = aln_amd.LOCAL
        qs, ts = make_workload(rank, args.pairs, args.length)

    # the one collective of the path: every rank's scores, gathered by the C ABI (RCCL) ONCE PER STEP; its own context/stream,
    # so that waiting for the gathered scores does not wait for compute kernels queued on the launch streams
    comm = comm_ctx = None
    n_total = args.pairs * world
    if world > 1:
        if rehearse:
            comm = GlooComm(world, rank)
        else:
            comm_ctx = aln_amd.Context(local_rank)
            comm = Comm(comm_ctx, world, rank)
        # agreement before the first collective: a rank with another batch shape must fail here, not hang in the gather
        shapes = [None] * world
        dist.all_gather_object(shapes, (args.pairs, n_total, args.split, args.batches, args.steps, args.warmup))
        if any(sh != shapes[0] for sh in shapes):
            raise SystemExit("ranks disagree on (pairs, n_total, split, streams, steps, warmup): %r" % (shapes,))
    gathered = np.zeros(n_total, dtype=np.float32)
    own_index = np.arange(rank * args.pairs, (rank + 1) * args.pairs, dtype=np.int32)
    gathers, steps_run = [0], [0]

    class Plan:
        """How a step's batch reaches the GPU.  The batch of `pairs` pairs is processed as `split` sub-batches (pairs/split pairs
        each, one launch sequence each) and consecutive launches rotate over `nb` contexts, each with its own HIP stream: launch
        j runs sub-batch j % split on stream j % nb.  Launches of different streams overlap, so there are always undispatched pairs
        to take the SIMD slots that finished pairs free, and the O(Q+T) corner kernel and the traceback run beside the next DP
        kernel.  Every step still builds, scans and traces all `pairs` pairs; every (stream, sub-batch) combination that occurs
        has its own resident planes.  nb = 1, split = 1: one lone launch per step."""

        def __init__(self, nb, split, borrow=None):
            self.nb, self.split, self.ph = nb, split, args.pairs // split
            self.units, self.ctxs, self.streams = {}, [], []
            self.borrowed = borrow is not None
            self.queue = []                                 # (batch, step id, sub-batch) enqueued, not yet collected (oldest first)
            self.count = 0
            self.open_steps = {}                            # step id -> [scores of sub-batch h or None]
            self.last = (None, None)
            self.e2e = False                                # True: every launch also encodes + uploads the residues and reads the strings back
            j = 0
            if cpu_rehearsal:
                while (j % nb, j % split) not in self.units:
                    self.units[(j % nb, j % split)] = RehearsalBatch(rank * args.pairs + (j % split) * self.ph, self.ph)
                    j += 1
                return
            if borrow is not None:                          # the same resident batches and streams as a plan with more of them
                self.ctxs = borrow.ctxs[:nb]
                self.units = {k: v for k, v in borrow.units.items() if k[0] < nb}
                return
            self.streams = [torch.cuda.Stream(dev) for _ in range(nb)]
            self.ctxs = [aln_amd.Context(local_rank, st.cuda_stream) for st in self.streams]
            while (j % nb, j % split) not in self.units:
                sidx, h = j % nb, j % split
                self.units[(sidx, h)] = aln_amd.Batch(self.ctxs[sidx], qs[h * self.ph:(h + 1) * self.ph], ts[h * self.ph:(h + 1) * self.ph])
                j += 1
            # codes + substitution table -> HBM and the first build (the DPMatrix constructors); timed steps then
            # re-run the build on the resident inputs exactly like DPMatrix::reevaluate (dpmatrix.h:213-218)
            for bt in self.units.values():
                bt.dp_submatrix(alphabet, table, mode, gi, ge, aln_amd.FWD, aln_amd.DP_FAST)

        def set_variant(self, occ, ap):
            for c in self.ctxs:
                c.set_hint("tag_occupancy", occ)
                c.set_hint("tag_alt_prio", ap)

        def collect(self):
            bt, sid, h = self.queue.pop(0)
            if self.e2e:
                sc, ident, status, _, _, lens, _ = bt.optimal_strings_collect(decode=False)
                self.last = (sc, status, ident, lens)
                kept = (ident, lens)
            else:
                sc, cnt, status = bt.optimal_collect()
                self.last = (sc, status)
                kept = (cnt, status)                        # step_result = [scores, list lengths, status] of the last step
            parts = self.open_steps.setdefault(sid, [None] * self.split)
            parts[h] = (np.array(sc, copy=True),) + tuple(np.array(x, copy=True) for x in kept)
            if all(x is not None for x in parts):           # the step is complete on this rank: its ONE gather
                mine = np.concatenate([x[0] for x in parts])
                self.step_result = [np.concatenate([x[k] for x in parts]) for k in range(len(parts[0]))]
                del self.open_steps[sid]
                steps_run[0] += 1
                if comm is not None:
                    comm.gather(mine, own_index, args.pairs, n_total, out=gathered)
                    gathers[0] += 1
                else:
                    gathered[own_index] = mine

        def launch(self):                                   # one sub-batch: build + find_max + traceback, results to the host
            j = self.count
            k = (j % self.nb, j % self.split)
            bt = self.units[k]
            self.count += 1
            while any(q[0] is bt for q in self.queue):      # its previous results must be read out before its planes are rebuilt
                self.collect()
            if self.e2e:
                bt.dp_submatrix(alphabet, table, mode, gi, ge, aln_amd.FWD, aln_amd.DP_FAST)   # encode + H2D + DP + corner
                bt.optimal_strings_enqueue()                                                     # traceback + lines + D2H
            else:
                bt.reevaluate()
                bt.optimal_enqueue()
            self.queue.append((bt, j // self.split, k[1]))
            if len(self.queue) > self.nb:
                self.collect()

        def step(self):                                     # all sub-batches of the batch
            for _ in range(self.split):
                self.launch()

        def drain(self):
            while self.queue:
                self.collect()
            self.count = 0

        def close_units(self, keep=()):                     # (Batch.close and Context.close are idempotent: shared objects may be closed twice)
            for bt in self.units.values():
                if not any(bt is k for k in keep):
                    bt.close()

        def close(self):
            self.close_units()
            for c in self.ctxs:
                c.close()
            self.units, self.ctxs = {}, []

    def fence():
        if world > 1:
            dist.barrier()
        if dev is not None:
            torch.cuda.synchronize(dev)

    def legal(nb, split):
        return nb >= 1 and split >= 1 and args.pairs % split == 0
    if args.batches > 0 or args.split > 0:                  # the caller fixed the launch pattern
        nb0, sp0 = (args.batches if args.batches > 0 else 4), (args.split if args.split > 0 else 2)
        patterns = [(nb0, sp0 if legal(nb0, sp0) else 1)]
    elif rehearse and not cpu_rehearsal:
        patterns = [(2, 1)]                                 # every rank on ONE GPU: no room for every pattern of every rank
    else:
        patterns = [p for p in ((4, 2), (2, 1), (1, 1)) if legal(*p)] or [(1, 1)]
    plans = []
    for nb_, sp_ in patterns:                               # the lone-launch plan runs on the first batch and stream of the two-stream plan
        lender = next((pl for pl in plans if pl.split == sp_ and pl.nb > nb_), None)
        plans.append(Plan(nb_, sp_, borrow=lender))

    # ---- calibration (untimed, before the warmup): the launch pattern and the build of the kernel this box prefers -----------------
    # {4 streams x 2 launches per step, 2 streams x 1, one lone launch} x {two, three waves per SIMD} x {row-alternating priority
    # off, on}: CAL_STEPS steps each after one settling step, two interleaved passes; the fastest runs the warmup and the timed region.
    # A caller that keeps batches resident would tune exactly so; boxes of the pool differ (the same build: 2.7 - 3.3 ms per step).
    calib = None
    plan = plans[0]
    if not cpu_rehearsal:
        occs = [2, 3] if args.occupancy < 0 else [args.occupancy]
        aps = [0, 1] if args.alt_prio < 0 else [args.alt_prio]
        best_of = {}
        if len(occs) * len(aps) * len(plans) > 1:
            for rep in range(2):                            # two interleaved passes: a slow moment of the box hits all variants alike
                for pi, pl in enumerate(plans):
                    for occ in occs:
                        for ap in aps:
                            pl.set_variant(occ, ap)
                            pl.step(); pl.drain(); fence()
                            t0 = time.perf_counter()
                            for _ in range(CAL_STEPS):
                                pl.step()
                            pl.drain(); fence()
                            key = (pi, occ, ap)
                            best_of[key] = min((time.perf_counter() - t0) / CAL_STEPS * 1e3, best_of.get(key, 1e9))
            if world > 1:                                   # every rank must run the same build: the slowest rank's view decides
                keys = sorted(best_of)
                tt = torch.tensor([best_of[k] for k in keys], dtype=torch.float64, device="cpu" if rehearse else dev)
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                best_of = {k: float(v) for k, v in zip(keys, tt.tolist())}
            choice = min(best_of, key=best_of.get)
            name = lambda k: "streams%d_split%d_occ%d_altprio%d" % (plans[k[0]].nb, plans[k[0]].split, k[1], k[2])   # noqa: E731
            calib = {"ms_per_step": {name(k): round(v, 3) for k, v in sorted(best_of.items())}, "chosen": name(choice),
                     "steps_each": CAL_STEPS, "passes": 2, "note": "short regions carry their own fill and drain: they rank the variants, "
                     "they are not the result"}
        else:
            choice = (0, occs[0], aps[0])
        plan = plans[choice[0]]
        plan.set_variant(choice[1], choice[2])
        # (the other plans stay resident until the timed region is over: freeing tens of GB here would idle the GPU for a few
        # hundred ms right before the warmup, and W warmup steps are too few to bring its clocks back)
    nb, split, ph = plan.nb, plan.split, plan.ph
    units = plan.units
    batches = list(units.values())
    batch = batches[0]
    calib_steps = steps_run[0]

    import gc
    gc.collect()
    gc.disable()                                            # no collector pause inside the timed region
    for _ in range(args.warmup):
        plan.step()
    plan.drain()
    fence()
    stamps = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        plan.step()
        if args.trace_steps:
            stamps.append(round((time.perf_counter() - t0) * 1e3, 3))
    plan.drain()
    fence()
    elapsed = time.perf_counter() - t0
    gc.enable()
    for pl in plans:                                        # the planes of the plans that lost; contexts live until the end
        if pl is not plan:
            pl.close_units(keep=list(plan.units.values()))
    sc, status = plan.last[:2]
    assert sc is not None and (status == 0).all()
    assert not plan.open_steps and steps_run[0] == calib_steps + args.warmup + args.steps
    # HIP events around the DP kernel of each timed launch, on the stream it was launched on
    n_launch = args.steps * split
    first = args.warmup * split                             # index of the first timed launch (plan.count restarts after a drain)
    per = {}
    for j in range(n_launch):
        k = (j % nb, j % split)
        per[k] = per.get(k, 0) + 1
    hist = [units[k].dp_ms_history(min(n, 64)) for k, n in per.items()]
    kernel_ms = np.concatenate(hist) if hist else np.zeros(0, np.float32)
    if args.dump_outputs and rank == 0:                     # what the last timed step handed its caller
        l_sc, l_cnt, l_st = plan.step_result
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "scores.npy"), np.array(gathered, dtype=np.float32))
        np.save(os.path.join(args.dump_outputs, "list_lengths.npy"), l_cnt.astype(np.float64))
        np.save(os.path.join(args.dump_outputs, "status.npy"), l_st.astype(np.float64))
    if cpu_rehearsal:
        assert np.array_equal(gathered, np.arange(n_total, dtype=np.float32)), "the gather misplaced a rank's block"
    if comm is not None:
        assert gathers[0] == steps_run[0], "not one gather per step"
    all_sc, pins = None, {}
    if args.full:
        # parity inside the bench: every resident copy of a sub-batch gives identical scores, and the pairs the REAL reference
        # was run on (tests/golden/full_cases.json) score exactly what it scored
        ref_sc = {}
        for (sidx, h), bt in units.items():
            bt.reevaluate()
            s_b, _, st_b = bt.optimal(want_pairs=False)
            assert (st_b == 0).all()
            if h not in ref_sc:
                ref_sc[h] = np.array(s_b, copy=True)
            else:
                assert np.array_equal(ref_sc[h], s_b), "resident copies of a sub-batch disagree"
        all_sc = np.concatenate([ref_sc[h] for h in range(split)])
        assert np.array_equal(gathered[rank * args.pairs:(rank + 1) * args.pairs].view(np.uint32), all_sc.view(np.uint32)), "gathered scores differ"
        pins = {} if cpu_rehearsal else pinned_scores(rank, args.pairs, args.length)
        for p, want in pins.items():
            assert np.float32(all_sc[p]).view(np.uint32) == np.float32(want).view(np.uint32), "pair %d: score %r, reference %r" % (p, all_sc[p], want)
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if rehearse else dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())

    parallelism = "pair-batch sharded, %d rank(s), one RCCL all-gather of the scores per step (aln_gather_scores)" % world
    if cpu_rehearsal:
        out = {"metric": "GCUPS (DP cell updates/s) at 1/2/4/8 MI355X; bit-exact score vs ref", "value": None, "unit": "GCUPS",
               "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": None, "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None, "dtype": "int32", "data": "synthetic",
               "rehearsal": "ALN_BENCH_REHEARSE=cpu: control flow only (spawn, rendezvous, launch rotation, one gather per step); nothing was computed or measured",
               "config": {"workload": "none (stand-in batches)", "pairs_per_gpu": args.pairs, "parallelism": parallelism,
                          "launches_per_step": split, "streams": nb, "gathers": gathers[0], "steps_run": steps_run[0]}}
        if rank == 0:
            print(json.dumps(out), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return

    # this box's plain streaming-store rate (torch fill of 8 GiB, HIP events on the same stream): what "HBM-write bound"
    # can mean on this device today; boxes of the pool differ by ~20 % on it (--full only: a run of its own)
    fill_gbs = None
    if args.full:
        try:
            buf = torch.empty(2 << 30, dtype=torch.float32, device=dev)
            buf.fill_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                buf.fill_(2.0)
            e1.record()
            torch.cuda.synchronize(dev)
            fill_gbs = 3 * buf.numel() * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9
            del buf
        except Exception:
            pass

    first_of = {}
    for (sidx, h), bt in units.items():
        first_of.setdefault(h, bt)
    cells_per_step = sum(first_of[h].cells() for h in range(split)) * world
    value = cells_per_step * args.steps / elapsed / 1e9
    ms_per_step = elapsed / args.steps * 1e3
    dp_ms = float(np.mean(kernel_ms))
    algo_bytes = batch.algorithmic_bytes()                  # of one launch (one sub-batch), with the layout the kernel chose
    contract_bytes = batch.contract_bytes()
    bench_kernel = batch.kernel_name()
    bytes_per_cell = batch.plane_bytes_per_cell()
    ctxs = plan.ctxs
    for bt in batches:
        bt.close()
    plan.units = {}
    # ---- end to end, pipelined (rank 0, one GPU): three resident batches of all the pairs take turns, one launch sequence each;
    # every launch also encodes + uploads its residues and brings the gapped lines + identities of its pairs back to the host -------
    e2e_pipe = None
    if args.full and rank == 0 and world == 1 and not args.no_secondary:
        ep = Plan(3, 1)
        ep.e2e = True
        e2e_cal = {}
        for occ, ap in ((2, 1), (3, 1), (2, 0), (3, 0)):    # the host work between launches changes how much they overlap: tune again
            ep.set_variant(occ, ap)
            ep.step(); ep.drain(); fence()
            t0 = time.perf_counter()
            for _ in range(6):
                ep.step()
            ep.drain(); fence()
            e2e_cal[(occ, ap)] = (time.perf_counter() - t0) / 6 * 1e3
        e2e_choice = min(e2e_cal, key=e2e_cal.get)
        ep.set_variant(*e2e_choice)
        ep.step(); ep.drain(); fence()
        n_pipe = 12
        t0 = time.perf_counter()
        for _ in range(n_pipe):
            ep.step()
        ep.drain(); fence()
        e2e_pipe = {"ms_per_step": (time.perf_counter() - t0) / n_pipe * 1e3, "steps": n_pipe, "result": ep.step_result,
                    "calibration": {"occ%d_altprio%d" % k: round(v, 3) for k, v in e2e_cal.items()}, "chosen": "occ%d_altprio%d" % e2e_choice}
        assert np.array_equal(ep.step_result[0].view(np.uint32), all_sc.view(np.uint32))
        ep.close()


    # ---- lone launches: the whole batch as ONE launch per step on ONE stream, nothing else on the GPU -----------------------------
    # kernel_only = the DP kernel's own duration (HIP events on its stream), the number `rocprofv3 --kernel-trace --stats` reports for
    # the same launch (profiles/r03_lone_kernel_stats.csv); lone_step = the whole step (DP + corner + find_max + traceback + results)
    lone = None
    if args.full and args.lone_steps > 0:
        c0 = ctxs[0]
        c0.set_hint("tag_occupancy", 0)                     # the library's own rule for a lone launch of this size
        c0.set_hint("tag_alt_prio", 1)
        bl = aln_amd.Batch(c0, qs, ts)
        bl.dp_submatrix(alphabet, table, mode, gi, ge, aln_amd.FWD, aln_amd.DP_FAST)
        for _ in range(3):
            bl.reevaluate(); bl.optimal_enqueue(); bl.optimal_collect()
        fence()
        t0 = time.perf_counter()
        for _ in range(args.lone_steps):
            bl.reevaluate(); bl.optimal_enqueue()
            l_sc, _, l_st = bl.optimal_collect()
        fence()
        lone_ms = (time.perf_counter() - t0) / args.lone_steps * 1e3
        assert (l_st == 0).all() and np.array_equal(l_sc.view(np.uint32), all_sc.view(np.uint32))
        lk = bl.dp_ms_history(args.lone_steps)
        lone = {"kernel_ms": float(np.mean(lk)), "kernel_ms_min": float(np.min(lk)), "step_ms": lone_ms, "kernel": bl.kernel_name(),
                "bytes": bl.algorithmic_bytes(), "cells": bl.cells(), "steps": args.lone_steps}
        bl.close()

    if nb == 1:
        achieved = algo_bytes / (dp_ms * 1e-3) / 1e9
        how = "bytes the chosen layout must write per launch / average launch duration (HIP events on the launch stream)"
    else:
        # Launches of different resident batches overlap on the GPU, so a launch's own duration (kernel_ms, what rocprofv3
        # also reports) is not the time the device spends per launch.  The kernel's aggregate rate is bounded from below by
        # all timed launches' bytes over the wall time of the timed region (which also holds the corner and traceback kernels).
        achieved = algo_bytes * args.steps * split / elapsed / 1e9
        how = ("launches of %d streams overlap: bytes the chosen layout must write, all timed launches / wall time of the timed "
               "region (lower bound; kernel_ms is one launch's own duration while it shares the GPU; kernel_only below is the lone "
               "launch rocprofv3 reproduces)" % nb)
    traffic = valu = None
    tfile = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if os.path.exists(tfile) and args.length == 2000:       # only if a PMC pass was taken on exactly this launch shape and kernel build
        try:
            doc = json.load(open(tfile))
            entries = doc["shapes"] if isinstance(doc, dict) and "shapes" in doc else [doc]
            for tj in entries:
                if tj.get("launch_pairs", 1024) != ph or tj.get("kernel") != bench_kernel:
                    continue
                traffic = tj.get("hbm_bytes_per_launch")
                if tj.get("valu_insts_per_launch"):
                    ins = float(tj["valu_insts_per_launch"]) * split          # wave-instructions per step
                    half = float(tj.get("valu_half_rate_share", 0.57))
                    ns = (1 - half) * VALU_NS_FULL + half * VALU_NS_HALF
                    floor_ms = ins / N_SIMD * ns * 1e-6
                    valu = {"insts_per_step": ins, "source": tj.get("source"), "half_rate_share": half,
                            "issue_ns_per_inst_per_simd": {"full_rate": VALU_NS_FULL, "half_rate": VALU_NS_HALF, "this_mix": round(ns, 3)},
                            "issue_floor_ms_per_step": round(floor_ms, 3), "frac": round(floor_ms / (ms_per_step / 1.0), 4)}
                break
        except Exception:
            traffic = valu = None
    hbm_frac = achieved / HBM_PEAK_GBS
    out = {
        "metric": "GCUPS (DP cell updates/s) at 1/2/4/8 MI355X; bit-exact score vs ref",
        "value": round(value, 3), "unit": "GCUPS", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "int32", "data": "synthetic",
        "config": {"workload": "config 2: %d synthetic %dx%d pairs per GPU, local SW, affine gap 11/1, BLOSUM62 submatrix evaluator, "
                               "DP build + find_max + traceback" % (args.pairs, args.length, args.length),
                   "pairs_per_gpu": args.pairs, "parallelism": parallelism,
                   "kernel": bench_kernel, "launch_pairs": ph, "launches_per_step": split, "streams": nb,
                   "launches_in_flight": nb, "timed_region": "every launch of the %d steps from first enqueue to the last result on the host "
                   "(pipeline fill and drain included); ms_per_step = that wall time / steps" % args.steps,
                   "calibration": calib,
                   "pairs_checked_against_reference_scores": sorted(pins)},
        "roofline": {"bound": "hbm" if (valu is None or hbm_frac >= valu["frac"]) else "valu",
                     "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(hbm_frac, 4), "traffic": traffic,
                     "algorithmic_bytes": algo_bytes, "bytes_per_cell": bytes_per_cell,
                     "contract_bytes": contract_bytes, "contract_note": "SURVEY 8(d) counts 8 B/cell (fp32 score + 32-bit pointer); this "
                     "kernel stores uint16 score + uint16 pointer word, so only algorithmic_bytes are written and `achieved` uses them",
                     "kernel_ms": round(dp_ms, 3), "concurrent_launches": nb, "achieved_is": how,
                     "measured_fill_GBs_this_box": round(fill_gbs, 1) if fill_gbs else None,
                     "frac_of_measured_fill": round(achieved / fill_gbs, 4) if fill_gbs else None,
                     "valu": valu},
    }
    if lone is not None:
        lone_gbs = lone["bytes"] / (lone["kernel_ms"] * 1e-3) / 1e9
        out["kernel_only"] = {"ms_per_step": round(lone["kernel_ms"], 3), "launch_ms": round(lone["kernel_ms"], 3),
                              "launch_ms_min": round(lone["kernel_ms_min"], 3),
                              "value": round(lone["cells"] / (lone["kernel_ms"] * 1e-3) / 1e9, 1), "unit": "GCUPS",
                              "achieved_GBs": round(lone_gbs, 1), "frac": round(lone_gbs / HBM_PEAK_GBS, 4),
                              "frac_of_measured_fill": round(lone_gbs / fill_gbs, 4) if fill_gbs else None,
                              "whole_step_ms": round(lone["step_ms"], 3), "steps": lone["steps"], "kernel": lone["kernel"],
                              "note": "ONE launch of all %d pairs per step on one stream, nothing overlapping: the DP kernel's own duration "
                                      "(HIP events on its stream) = what rocprofv3 --kernel-trace --stats reports for this launch; "
                                      "whole_step_ms adds corner + find_max + traceback + results to the host" % args.pairs}
    if args.trace_steps:
        out["step_stamps_ms"] = stamps
    if args.full and rank == 0 and world == 1 and not args.no_secondary:
        out["end_to_end"] = end_to_end(aln_amd, ctxs, qs, ts, alphabet, table, mode, gi, ge, all_sc, args.pairs, e2e_pipe, 3, 1)
        out["secondary"] = secondary_configs(aln_amd, ctxs[0], alphabet, table, qs, ts, args.length)
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(qs, ts, mode, gi, ge)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if comm is not None:
        comm.close()
    if comm_ctx is not None:
        comm_ctx.close()
    for pl in plans:
        for c in pl.ctxs:
            c.close()
    if world > 1:
        dist.destroy_process_group()


def end_to_end(aln_amd, ctxs, qs, ts, alphabet, table, mode, gi, ge, all_sc, n_pairs, piped, nb, split):
    """SURVEY 8(d) end to end, per step: residues encoded + uploaded (host buffers handed over), DP, find_max + traceback, the gapped
    template / query lines and identities of every pair on the host (the lines are laid out on the device, csrc/gapped_strings.hip;
    only they travel).  `piped` was measured by the caller (several resident batches taking turns: step k's copy and host work
    overlap step k+1's encoding, upload and kernels); here the same work with nothing pipelined: one batch, one stream, one call
    after the other."""
    c0 = ctxs[0]
    c0.set_hint("tag_alt_prio", 1)
    c0.set_hint("tag_occupancy", 0)
    be = aln_amd.Batch(c0, qs, ts)
    be.dp_submatrix(alphabet, table, mode, gi, ge, aln_amd.FWD, aln_amd.DP_FAST)
    be.optimal_strings(decode=False)
    n_e2e = 5
    c0.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_e2e):
        be.dp_submatrix(alphabet, table, mode, gi, ge, aln_amd.FWD, aln_amd.DP_FAST)     # encode + H2D + DP + corner
        e_sc, e_id, e_st, _, _, e_len, _ = be.optimal_strings(decode=False)               # traceback + lines + D2H
    e2e = (time.perf_counter() - t0) / n_e2e
    assert (e_st == 0).all() and (e_len > 0).all()
    assert np.array_equal(e_sc.view(np.uint32), all_sc.view(np.uint32))
    cells = be.cells()
    be.close()
    res = {"unit": "GCUPS",
           "not_pipelined": {"ms_per_step": round(e2e * 1e3, 3), "value": round(cells / e2e / 1e9, 1), "steps": n_e2e},
           "includes": "residue encoding + H2D of codes and table, DP + corner kernels, find_max + traceback, gapped template / query "
                       "lines (SequenceGaps) + identity counts of all %d pairs built on the device, D2H of the lines, identities and "
                       "the caller's line buffers filled on the host" % n_pairs}
    if piped is not None:
        p_sc, p_id, p_len = piped["result"]
        assert np.array_equal(p_id.view(np.uint32), e_id.view(np.uint32)) and np.array_equal(p_len, e_len), "pipelined and plain readout differ"
        res["ms_per_step"] = round(piped["ms_per_step"], 3)
        res["value"] = round(cells / (piped["ms_per_step"] * 1e-3) / 1e9, 1)
        res["steps"] = piped["steps"]
        res["pipelined"] = {"ms_per_step": round(piped["ms_per_step"], 3), "steps": piped["steps"],
                            "calibration_ms": piped.get("calibration"), "kernel_build": piped.get("chosen"),
                            "how": "%d resident batches of all the pairs take turns, one stream each (%d launch sequence(s) per step): "
                                   "aln_batch_dp, aln_batch_optimal_strings_enqueue, _collect of the launch %d steps back — the copy and "
                                   "the host work of one step overlap the next steps" % (nb, split, nb)}
    else:
        res["ms_per_step"] = res["not_pipelined"]["ms_per_step"]
        res["value"] = res["not_pipelined"]["value"]
        res["steps"] = n_e2e
    return res


if __name__ == "__main__":
    main()
