// search_counts.h — the job that counts (CountArgs, CountJob), shared by the entries that tally column counts behind a hit
// kernel pair: search_counts.hip (hit_local_kernel / hit_global_kernel, search_align.h) and search_counts_qgaps.hip
// (hit_local_qgaps_kernel / hit_global_qgaps_kernel, search_align_qgaps.h), and the driver of their chunks of fused hits
// (count_fused_hits).  The head of search_counts.hip tells what the job does and why its adds are exact.
#pragma once
#include <climits>

#include "search_align.h"

namespace aln {

constexpr int kCoveredCol = 31;                         // the alphabet has at most 30 letters: codes 0 .. 29

struct CountArgs {
  const int32_t* list;      // blockIdx.x -> hit of the chunk
  const HitDesc* desc;
  uint8_t* strip;
  const int32_t* weight;    // per hit of the chunk; 0: the record only
  int32_t* rows;            // the call's count rows, 32 int32 each; row 0 is row offsets[q_begin] of the query pool
  int64_t row0;             // offsets[q_begin]
  PairResult* res;          // best = score, n_path, status
  int32_t* same;
};

// The job that counts.  What strip_walk's entries become: the identity's count, the lane's bounds of interior query rows, one
// atomicAdd each.
struct CountJob {
  typedef CountArgs Args;
  template <class Letters>
  struct Sink {
    Letters qs, ts;                         // what the identity is counted over
    const uint8_t* tc;                      // the template's codes
    int32_t* rows;                          // the query's count rows (row i of the query at rows + 32 i)
    int Q, T, w;
    int same = 0, lo = INT_MAX, hi = -1;
    __device__ __forceinline__ Sink(const Args& g, const ScoreArgs& a, int hit, int qi, Letters qs_, Letters ts_, const uint8_t* tc_,
                                    int Q_, int T_)
        : qs(qs_), ts(ts_), tc(tc_), rows(g.rows + 32 * (a.qoff[qi] - g.row0)), Q(Q_), T(T_), w(g.weight[hit]) {}
    __device__ __forceinline__ void operator()(int, int q, int t) {
      same += (qs[q] == ts[t]) ? 1 : 0;
      if (q >= 1 && q <= Q - 2 && t >= 1 && t <= T - 2) {
        lo = min(lo, q); hi = max(hi, q);
        if (w) atomicAdd(rows + 32 * q + (int)tc[t], w);
      }
    }
    // after the walk: same summed, covered over i_lo .. i_hi (every lane calls it)
    __device__ __forceinline__ void finish() {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        same += __shfl_xor(same, off);
        lo = min(lo, __shfl_xor(lo, off));
        hi = max(hi, __shfl_xor(hi, off));
      }
      if (w && hi >= 0)                     // (a fused hit always has an interior entry: its first cell)
        for (int i = lo + (int)threadIdx.x; i <= hi; i += 64) atomicAdd(rows + 32 * i + kCoveredCol, w);
    }
    __device__ __forceinline__ int status(int) const { return 0; }
  };
};

// The chunks of fused hits of the entries that count (aln_hits_column_counts(_profiles), aln_hits_column_counts_profiles_gaps):
// no lists and no lines, so only the strips count against the budget; the count rows are zeroed once per call and come down
// once at its end, into counts (n_alpha wide) and covered (may be NULL), which the caller has zeroed; row0 / n_rows: the block's
// rows of the query pool.  weight_of(slot): the slot's weight.  launch(fr, c, g): the caller's kernel pair over CountJob.
template <class WeightOf, class Launch>
int count_fused_hits(ScoreRun& run, const aln_seqs* queries, SlotRoutes& sr, int64_t row0, size_t n_rows, int n_alpha, int32_t* counts,
                     int32_t* covered, AlignOut& ao, WeightOf&& weight_of, Launch&& launch) {
  aln_ctx* ctx = run.ctx;
  std::vector<HitDesc>& fast = sr.fast;
  const std::vector<size_t>& fast_slot = sr.fast_slot;
  FusedRoute<HitDesc> fr(run, queries, fast);
  std::vector<int32_t> fast_w(fast.size());
  for (size_t h = 0; h < fast.size(); ++h) fast_w[h] = (run.local && !(fast[h].score > 0.f)) ? 0 : weight_of(fast_slot[h]);
  fr.cut(0, false, 0, [&](const HitDesc& d) { return HitNeed{hit_strip_bytes(run, queries, d), 0, 0}; });
  int32_t *dw = nullptr, *drows = nullptr;
  HitRecords rec;
  RTRY(fr.begin());
  STRY(fr.bufs.get(dw, fr.max_n));
  RTRY(rec.alloc(fr.bufs, fr.max_n));
  STRY(fr.bufs.get(drows, std::max<size_t>(n_rows, 1) * 32));
  STRY(hipMemsetAsync(drows, 0, std::max<size_t>(n_rows, 1) * 128, ctx->stream));      // once per call, not per chunk
  if (run.prof) RTRY(fr.upload_pools());
  for (const FusedChunk& c : fr.chunks) {
    RTRY(fr.stage(c, [&]() -> int {
      STRY(hipMemcpyAsync(dw, fast_w.data() + c.h0, c.n * 4, hipMemcpyHostToDevice, ctx->stream));
      return ALN_OK;
    }));
    CountArgs g = {};
    g.desc = fr.ddesc; g.strip = fr.dstrip; g.weight = dw; g.rows = drows; g.row0 = row0; g.res = rec.dres; g.same = rec.dsame;
    RTRY(launch(fr, c, g));
    RTRY(rec.enqueue_download(ctx, c.n));
    STRY(hipStreamSynchronize(ctx->stream));                 // the records' host images are read by the copies until here
    rec.put(ao, fr, c, fast_slot, [](size_t, size_t, int64_t) {});
  }
  std::vector<int32_t> hrows(n_rows * 32);
  STRY(hipMemcpyAsync(hrows.data(), drows, n_rows * 128, hipMemcpyDeviceToHost, ctx->stream));
  STRY(hipStreamSynchronize(ctx->stream));
  for (size_t r = 0; r < n_rows; ++r) {
    memcpy(counts + r * (size_t)n_alpha, hrows.data() + r * 32, (size_t)n_alpha * 4);
    if (covered) covered[r] = hrows[r * 32 + kCoveredCol];
  }
  return ALN_OK;
}

}  // namespace aln
