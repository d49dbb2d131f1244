// search_align_qgaps.h — hit alignment for profiles whose ROWS carry their own gap penalties (aln_qgaps): what
// aln_hits_align_profiles_gaps (search_align_qgaps.hip: ListJob) and aln_hits_column_counts_profiles_gaps
// (search_counts_qgaps.hip: CountJob) share.  Device: the pair of kernels hit_local_qgaps_kernel / hit_global_qgaps_kernel<R, Job>,
// siblings of search_align.h's hit_local_kernel / hit_global_kernel<R, ProfileQuery, Job> around score_sweep_qgaps.h's sweeps —
// the same strip, the same walk (strip_walk), the same jobs; a further job (pileup, weights, purge, pssm) is another
// instantiation and a thin entry.  Host: the entries' prologue (hit_entry_qgaps), the routing (route_slots_qgaps), the launch of
// the pair over a job (launch_hit_qgaps_job) and the closed-form result of a pair without an interior (NoInterior): there is no
// batch route, because no batch gap model prices a gap by the query position.
//
// The strip byte is the one defined at the head of search_align.hip, and strip_walk reads it unchanged.  Why bits 2 and 3 stay
// valid when every row has its own prices (include/aln_hip.h, aln_hits_align_profiles_gaps, has the definition):
//   bit 2   compares the deletion keys A(k) = D[i-1][k] + del_extn[i-1] k of ONE row.  A deletion from (i-1, k) into (i, j) costs
//           del_init[i-1] + del_extn[i-1] (j-2-k): for a fixed target every candidate is A(k) minus the same number, so the order
//           of the keys is the order of the candidates, whatever the row's prices are.
//   bit 3   compares the insertion keys D[k][c] - ins_init[k+1] + X[k+1] of ONE column (X: the prefix sums of ins_extn,
//           score_sweep_qgaps.h).  An insertion from (k, c) into (i, c+1) costs ins_init[k+1] + X[i-1] - X[k+1]: for a fixed target
//           every candidate is its key minus X[i-1], so the keys are comparable across rows although every row has its own prices.
//   bits 0-1 and 4 compare candidate VALUES (m, e, f) and a score with 0: nothing about them depends on how a gap is priced.
// "The smallest k wins ties" (a later candidate wins only when strictly greater) is therefore still "walk while the bit is set".
#pragma once
#include "score_sweep_qgaps.h"
#include "search_align.h"

namespace aln {

// sweep_global_qgaps' observer: the strip bytes, and what the final cell's pointer needs under per-row prices.
//   last(): of row Q-2 the match candidate D[Q-2][T-2] and the best deletion D[Q-2][k] - del(Q-2, T-2-k) with the smallest
//           column holding it; lgi / lge are row Q-2's del_init / del_extn, which the kernel reads before the sweep.
//   The insertion candidates from (k, T-2), k <= Q-3 (row Q-2 costs nothing and equals the match candidate, which comes first:
//   it never wins and is left out).  Whether one of them wins needs no value of its own: the sweep's score is the maximum of
//   the three kinds, so an insertion wins exactly when the score exceeds both the match and the best deletion.  Which row:
//     paid tail   the candidate of row k is its key D[k][T-2] - ins_init[k+1] + X[k+1] minus X[Q-2], the same number for every
//                 k — and the key is the one the sweep hands cell() for that column's slot in the loop of row k+1, whose
//                 comparison with the column's running maximum IS bit 3 of the strip byte.  So the first row holding the
//                 maximal key is found after the sweep, as strip_walk finds an insertion's source: upwards in column T-2
//                 from row Q-3 while bit 3 is set.  Nothing is tracked inside the sweep (a per-cell select of the column's
//                 key cost 15 - 29 VGPRs).
//     free tail   the candidate is D[k][T-2] itself, which no bit compares: row() keeps the first row k <= Q-3 holding the
//                 maximum, strictly greater only, as GlobalObserver does.
template <int R>
struct QGapGlobalObserver : StripObserver<false> {
  const QGapGlobalCols<R>& k;
  int free_del, free_ins, lgi, lge, lastk;      // lastk = Q - 3
  int ikey = kNegS, irow = 0;                   // free tail, owning lane only; irow == 0: no candidate
  int match = kNegS, dlv = kNegS, dlc = 0;      // after last(): wave-uniform
  __device__ __forceinline__ QGapGlobalObserver(const QGapGlobalCols<R>& k_, int free_del_, int free_ins_, int lgi_, int lge_, int lastk_)
      : k(k_), free_del(free_del_), free_ins(free_ins_), lgi(lgi_), lge(lge_), lastk(lastk_) {}
  __device__ __forceinline__ void row(int i, const int (&d)[R][4], int) {
    const int key = sweep_pick<R>(d, k.rs, k.xs, kNegS);
    const bool up = free_ins && (int)threadIdx.x == k.ls && i <= lastk && key > ikey;   // strictly greater: the smallest row wins ties
    ikey = up ? key : ikey;
    irow = up ? i : irow;
  }
  __device__ __forceinline__ void last(const int (&d)[R][4]) {
    match = __shfl(sweep_pick<R>(d, k.rs, k.xs, kNegS), k.ls);
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int c = 4 * (int)threadIdx.x + 256 * r + x;
        const int len = k.T - 2 - k.cix[r][x];
        const int cost = (len < 1 || free_del) ? 0 : lgi + __mul24(lge, len - 1);
        const int v = k.in[r][x] ? d[r][x] - cost : kNegS;
        const bool up = v > dlv;                // the lane's columns ascend
        dlv = up ? v : dlv;
        dlc = up ? c : dlc;
      }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {   // value max, column min
      const int ov = __shfl_xor(dlv, off), oc = __shfl_xor(dlc, off);
      const bool take = ov > dlv || (ov == dlv && oc < dlc);
      dlv = take ? ov : dlv;
      dlc = take ? oc : dlc;
    }
  }
  // The final cell's pointer, after the sweep and its fence (the paid tail reads strip bytes other lanes stored): match,
  // deletions from (Q-2, k) k ascending, insertions from (k, T-2) k ascending; a later candidate wins only when strictly
  // greater.  score: the sweep's, wave-uniform; (i, j): the cell the walk starts from.  Every branch is wave-uniform.
  template <int PITCH>
  __device__ __forceinline__ void final_cell(const uint8_t* strip, int score, int& i, int& j) const {
    i = lastk + 1; j = k.T - 2;
    if (dlv > match) j = dlc;
    if (score > max(match, dlv)) {              // an insertion from (k, T-2), k <= Q-3 (so Q >= 4 and the strip has row k+1)
      j = k.T - 2;
      if (free_ins) i = __shfl(irow, k.ls);
      else
        for (int k0 = lastk; k0 >= 1; k0 -= 64) {
          const int kk = k0 - (int)threadIdx.x;
          const uint32_t bb = kk >= 1 ? strip[(size_t)(kk - 1) * PITCH + j] : 0u;   // the byte of cell (kk, T-2): row kk+1 of the strip
          const unsigned long long clr = __ballot((bb & 8u) == 0u);
          if (clr) { i = k0 - __builtin_ctzll(clr); break; }                        // (row 1 always clears its bit)
        }
    }
  }
};

// hit_local_kernel<R, ProfileQuery, Job> (search_align.h) over sweep_local_qgaps.  The comment block above that kernel holds
// here word for word: the strip stores share the VM counter with the staging copies, ProfileRows::landed() drains them once per
// 8 rows, and the last copy requested is never read but is drained — the fence — before the walk and before an early return.
template <int R, class Job>
__global__ __launch_bounds__(64) void hit_local_qgaps_kernel(ScoreArgs a, typename Job::Args g, const char* __restrict__ qch,
                                                            const char* __restrict__ tch) {
  __shared__ __attribute__((aligned(16))) int lds[32 * 32];
  const int lane = threadIdx.x;
  const int hit = g.list[blockIdx.x];
  const HitDesc hd = g.desc[hit];
  const int ti = hd.t, qi = hd.q, q_end = hd.q_end, t_end = hd.t_end;
  const int4* __restrict__ qr = ProfileQuery::rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const char* __restrict__ qs = qch + a.qoff[qi];            // what the identity is counted over: characters
  const char* __restrict__ ts = tch + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);
  constexpr int kPitch = 256 * R;
  uint8_t* strip = g.strip + hd.strip_off;      // row i (2 .. q_end) at strip + (i - 2) * kPitch

  // rows 1 .. q_end (1 <= q_end <= Q - 2: the host files other pairs itself); rows below q_end are not needed
  QGapLocalCols<R> cols;
  cols.load(tc, T);
  int d[R][4];
  __builtin_assume(q_end >= 1);                 // row 1 always runs, as the host guarantees: no path around it to keep registers for
  StripObserver<true> bytes;
  bytes.strip = strip; bytes.pitch = kPitch;
  sweep_local_qgaps<R>(lds, cols, qr, q_end, d, bytes);
  __threadfence();                                           // the last copy has landed; the walk's lanes read bytes other lanes stored
  __syncthreads();
  // D[q_end][t_end]: row q_end is in d[], column t_end in slot (rs, xs) of lane ls
  const int dend = __shfl(sweep_pick<R>(d, t_end / 256, t_end & 3, 0), (t_end & 255) >> 2);
  PairResult res = {};
  res.best = (float)dend; res.corner = 0.f; res.best_q = q_end; res.best_t = t_end;
  if (!((float)dend == hd.score)) {                          // not the cell the slot's score stands in: refuse the slot
    if (lane == 0) { res.best = 0.f; res.status = ALN_E_ARG; res.n_path = 0; g.res[hit] = res; g.same[hit] = 0; }
    return;
  }

  // ---- the walk back (optimal.h:79-105), its entries handed to the job in traversal order ------------------------------------
  typename Job::template Sink<const char*> sink(g, a, hit, qi, qs, ts, tc, Q, T);
  int n = 0;
  auto emit1 = [&](int q, int t) { if (lane == 0) sink(n, q, t); ++n; };
  emit1(Q - 1, T - 1);
  emit1(q_end, t_end);
  if (strip_walk<kPitch, true>(strip, q_end, t_end, n, sink)) emit1(0, 0);
  sink.finish();
  if (lane == 0) {
    res.n_path = n;
    res.status = sink.status(n);
    g.res[hit] = res;
    g.same[hit] = sink.same;
  }
}

// The same for the four non-local align types (sweep_global_qgaps, Q >= 3 and T >= 3: the host's routing): every row 1 .. Q-2
// is swept, and the walk starts at the cell the final cell's pointer names.  Row Q-2's deletion prices, which the pointer's
// deletion candidates need while row Q-2 is still in registers, are read from the profile's device rows before the sweep (two
// scalars live across it).
template <int R, class Job>
__global__ __launch_bounds__(64) void hit_global_qgaps_kernel(ScoreArgs a, typename Job::Args g, const char* __restrict__ qch,
                                                             const char* __restrict__ tch, int free_del, int free_ins) {
  __shared__ __attribute__((aligned(16))) int lds[32 * 32];
  const int lane = threadIdx.x;
  const int hit = g.list[blockIdx.x];
  const HitDesc hd = g.desc[hit];
  const int ti = hd.t, qi = hd.q;
  const int4* __restrict__ qr = ProfileQuery::rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const char* __restrict__ qs = qch + a.qoff[qi];            // what the identity is counted over: characters
  const char* __restrict__ ts = tch + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);
  const int* __restrict__ qw = reinterpret_cast<const int*>(qr);   // row p of the profile: 32 words at qw + 32 p (Q >= 3: row Q-2 is interior)
  constexpr int kPitch = 256 * R;
  uint8_t* strip = g.strip + hd.strip_off;      // row i (2 .. Q-2) at strip + (i - 2) * kPitch

  const int lgi = __builtin_amdgcn_readfirstlane(qw[(Q - 2) * 32 + kQGapWord]);
  const int lge = __builtin_amdgcn_readfirstlane(qw[(Q - 2) * 32 + kQGapWord + 1]);
  QGapGlobalCols<R> cols;
  cols.load(tc, T);
  QGapGlobalObserver<R> ob(cols, free_del, free_ins, lgi, lge, Q - 3);
  ob.strip = strip; ob.pitch = kPitch;
  int score = sweep_global_qgaps<R>(lds, cols, qr, Q, free_del, free_ins, ob);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) score = max(score, __shfl_xor(score, off));
  __threadfence();                                           // the last copy has landed; the walk's lanes read bytes other lanes stored
  __syncthreads();

  int i, j;
  ob.template final_cell<kPitch>(strip, score, i, j);

  // ---- the walk back (optimal.h:56-74): it always runs to a cell of row 1 or column 1, which points at (0,0) -------------------
  typename Job::template Sink<const char*> sink(g, a, hit, qi, qs, ts, tc, Q, T);
  int n = 0;
  auto emit1 = [&](int q, int t) { if (lane == 0) sink(n, q, t); ++n; };
  emit1(Q - 1, T - 1);
  emit1(i, j);
  strip_walk<kPitch, false>(strip, i, j, n, sink);
  emit1(0, 0);
  sink.finish();
  if (lane == 0) {
    PairResult res = {};
    res.best = (float)score; res.corner = 0.f; res.best_q = Q - 1; res.best_t = T - 1;
    res.n_path = n;
    res.status = sink.status(n);
    g.res[hit] = res;
    g.same[hit] = sink.same;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------

// hit_entry (search_align.h) for a run with gap rows: align_routes reset; `ok`, the entry's own argument checks; the pointers
// prepare() would otherwise read; the run prepared as aln_search_topk_profiles_gaps prepares it, so that entry's descriptor and
// gap checks hold here in its order, with the consensus pool where aln_hits_align_profiles checks it.  Such a run's route is
// kFast or an error: nothing of it can reach align_through_batches or for_list_groups.
template <class Body>
int hit_entry_qgaps(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_qgaps* gaps, const aln_seqs* consensus,
                    const aln_seqs* templates, int32_t align_type, int32_t q_begin, int32_t q_end, bool ok, Body&& body) {
  if (ctx) ctx->align_routes[0] = ctx->align_routes[1] = 0;
  if (!ok || !profiles || !gaps || !templates) return ALN_E_ARG;
  ScoreRun run;
  run.consensus = consensus;
  run.qgaps = gaps; run.qgaps_align_type = align_type;
  const int rc = run.prepare(ctx, nullptr, templates, nullptr, nullptr, q_begin, q_end, profiles);
  if (rc != ALN_OK) return rc;
  return body(run, consensus ? consensus : run.queries);
}

// route_slots' checks (search_align.h) and the two routes of a run with gap rows: a pair with an interior goes to the kernels
// — every length class, every align type; prepare() has refused templates beyond 2048 columns, and hint align_fused_nonlocal has
// nothing to switch to —, a pair without one (Q = 2 or T = 2) is filed by the host (sr.bq / bt / bslot).  Writes nothing but `sr`.
inline int route_slots_qgaps(const ScoreRun& run, const aln_seqs* queries, int32_t K, const aln_hit* hits, const int32_t* n_hits,
                             SlotRoutes& sr) {
  const aln_seqs* templates = run.templates;
  for (int r = 0; r < run.rows; ++r) {
    if (n_hits[r] < 0 || n_hits[r] > K) return ALN_E_ARG;
    const int q = run.q_begin + r;
    const int64_t Q = queries->offsets[q + 1] - queries->offsets[q];
    for (int k = 0; k < n_hits[r]; ++k) {
      const size_t slot = (size_t)r * K + k;
      const aln_hit& h = hits[slot];
      if (h.t < 0 || h.t >= run.n_t) return ALN_E_ARG;
      const int64_t T = templates->offsets[h.t + 1] - templates->offsets[h.t];
      const bool interior = Q >= 3 && T >= 3;
      if (run.local && interior && (h.q_end < 1 || h.q_end > Q - 2 || h.t_end < 1 || h.t_end > T - 2)) return ALN_E_ARG;
      if (interior) {
        HitDesc d = {q, h.t, 0, 0, 0.f, (int)((T + 255) / 256), 0};   // non-local: the slot's end cell and score are ignored
        if (run.local) { d.q_end = h.q_end; d.t_end = h.t_end; d.score = h.score; }
        sr.fast.push_back(d); sr.fast_slot.push_back(slot);
      } else { sr.bq.push_back(q); sr.bt.push_back(h.t); sr.bslot.push_back(slot); }
    }
  }
  return ALN_OK;
}

// launch_hit_job (search_align.h) for the gap-row pair: per class present hit_local_qgaps_kernel or hit_global_qgaps_kernel<R, Job>
// over the class's part of the list.  A template the caller's .hip file instantiates with its own job.
template <class Job>
int launch_hit_qgaps_job(FusedRoute<HitDesc>& fr, const FusedChunk& c, typename Job::Args& g) {
  ScoreRun& run = fr.run;
  const hipStream_t stream = run.ctx->stream;
  return fr.launch(c, [&](auto, int k, int cnt, const int32_t* list, const char* qch, const char* tch) {
    const dim3 grid(cnt), block(64);
    g.list = list;
    dispatch_r<8>(k, [&](auto rc) {
      constexpr int R = decltype(rc)::value;
      if (run.local) hipLaunchKernelGGL((hit_local_qgaps_kernel<R, Job>), grid, block, 0, stream, run.a, g, qch, tch);
      else hipLaunchKernelGGL((hit_global_qgaps_kernel<R, Job>), grid, block, 0, stream, run.a, g, qch, tch, run.free_del, run.free_ins);
    });
  });
}

// A pair without an interior (Q = 2 or T = 2), in closed form.  The list is the one aln_hits_align_profiles reports for such a
// pair and does not depend on a gap price: non-local (0,0) (Q-1,T-1); local, find_max's seed (Q-2, T-2) scores 0 and lies in
// row 0 or column 0 — (0,T-2) (1,T-1) for Q = 2, and for T = 2 the seed (Q-2, 0) has no pointer, so (0,0) is prepended:
// (0,0) (Q-2,0) (Q-1,1).  The score is the definition's: Q = 2 -> -del(0, T-2), T = 2 -> -ins(1, Q-2), 0 where that end gap is
// free, where nothing is skipped and under ALN_LOCAL.
struct NoInterior {
  int32_t list[6]; int n;   // in list order
  float score;
  NoInterior(const ScoreRun& run, int32_t q, int64_t Q, int64_t T) {
    const int32_t Ql = (int32_t)Q - 1, Tl = (int32_t)T - 1;
    n = 0;
    auto add = [&](int32_t i, int32_t j) { list[2 * n] = i; list[2 * n + 1] = j; ++n; };
    int64_t cost = 0;
    if (run.local) {
      if (Q == 2) add(0, Tl - 1);
      else { add(0, 0); add(Ql - 1, 0); }
    } else {
      add(0, 0);
      const aln_qgaps* g = run.qgaps;
      const int64_t off = run.prof->offsets[q];
      if (Q == 2) {
        if (!run.free_del && T >= 3) cost = (int64_t)g->del_init[off] + (int64_t)g->del_extn[off] * (T - 3);
      } else if (!run.free_ins) {
        cost = (int64_t)g->ins_init[off + 1];
        for (int64_t p = 2; p <= Q - 2; ++p) cost += (int64_t)g->ins_extn[off + p];
      }
    }
    add(Ql, Tl);
    score = (float)(-cost);
  }
};

}  // namespace aln
