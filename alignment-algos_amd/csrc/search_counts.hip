// search_counts.hip — the column counts of search hits, on the device: aln_hits_column_counts (gfx950).
//
// The step from one search round to the next needs, per query position, how often each template letter stands under it in
// the alignments of the query's hits: one small integer matrix per query, not the alignments.  So the two kernels of
// search_align.hip are repeated here with another sink behind the same walk:
//   count_local_hit_kernel<R, Side>    sweep_local + StripObserver<true> + the score check + strip_walk, as align_local_hit_kernel;
//   count_global_hit_kernel<R, Side>   sweep_global + GlobalObserver + final_cell + strip_walk, as align_global_hit_kernel.
// One wave per hit.  The sink counts `same` for the identity (the record is aln_hits_align's), keeps the lane's smallest and
// largest interior query row, and issues ONE integer atomicAdd of the slot's weight into the call's count rows — row
// (offsets[q] - offsets[q_begin] + i), 32 int32 wide as the profile side's device rows are, column = the template letter's
// code; nothing reads the old value.  Within a hit every query row occurs once, so adds collide only between hits of one
// query, and integer adds commute: the result is exact whatever the order.  After the walk the wave reduces the two bounds
// and adds the weight to the spare column 31 (`covered`) of rows i_lo .. i_hi, 64 rows per step.  There is no list, no line
// buffer and no gapped_strings_kernel; the rows are zeroed once per call and downloaded once at its end.
// A slot that must not contribute — weight 0, a local score <= 0 (the seed cell's list) — still needs its record: the host
// passes weight 0 for it and the kernel leaves the adds out.  A local slot whose sweep score differs from .score returns
// before the walk.  Everything the kernels do not take goes through align_through_batches (search_align.hip) with pair lists
// wanted, which the host tallies into the same outputs.
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "search_align.h"

namespace aln {

constexpr size_t kCountStripBudget = (size_t)1 << 30;   // bytes of strips resident at a time
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

// What strip_walk's entries become: the identity's count, the lane's bounds of interior query rows, one atomicAdd each.
template <class Letters>
struct CountSink {
  Letters qs, ts;                         // what the identity is counted over
  const uint8_t* tc;                      // the template's codes
  int32_t* rows;                          // the query's count rows (row i of the query at rows + 32 i)
  int Q, T, w;
  int same = 0, lo = INT_MAX, hi = -1;
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
};

template <int R, class Side>
__global__ __launch_bounds__(64) void count_local_hit_kernel(ScoreArgs a, CountArgs g, const char* __restrict__ qch,
                                                            const char* __restrict__ tch) {
  __shared__ __attribute__((aligned(16))) int lds[32 * 32];
  const int lane = threadIdx.x;
  Side::stage(lds, a);
  const int hit = g.list[blockIdx.x];
  const HitDesc hd = g.desc[hit];
  const int ti = hd.t, qi = hd.q, q_end = hd.q_end, t_end = hd.t_end;
  const typename Side::Rows::Src* __restrict__ qr = Side::rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const auto* __restrict__ qs = Side::letters(a.qcodes, qch) + a.qoff[qi];
  const auto* __restrict__ ts = Side::letters(a.tcodes, tch) + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);
  constexpr int kPitch = 256 * R;
  uint8_t* strip = g.strip + hd.strip_off;      // row i (2 .. q_end) at strip + (i - 2) * kPitch

  LocalCols<R> cols;
  cols.load(tc, T, a.gi, a.ge);
  int d[R][4];
  __builtin_assume(q_end >= 1);
  StripObserver<true> bytes;
  bytes.strip = strip; bytes.pitch = kPitch;
  sweep_local<R, typename Side::Rows>(lds, cols, qr, q_end, d, bytes);
  if constexpr (Side::kStaged) {
    __threadfence();                                         // the last copy has landed; the walk's lanes read bytes other lanes stored
    __syncthreads();
  }
  const int dend = __shfl(sweep_pick<R>(d, t_end / 256, t_end & 3, 0), (t_end & 255) >> 2);
  PairResult res = {};
  res.best = (float)dend; res.corner = 0.f; res.best_q = q_end; res.best_t = t_end;
  if (!((float)dend == hd.score)) {                          // not the cell the slot's score stands in: refuse the slot
    if (lane == 0) { res.best = 0.f; res.status = ALN_E_ARG; res.n_path = 0; g.res[hit] = res; g.same[hit] = 0; }
    return;
  }
  if constexpr (!Side::kStaged) {
    __threadfence();
    __syncthreads();
  }

  CountSink<decltype(Side::letters(a.tcodes, tch))> sink = {qs, ts, tc, g.rows + 32 * (a.qoff[qi] - g.row0), Q, T, g.weight[hit]};
  int n = 0;
  auto emit1 = [&](int q, int t) { if (lane == 0) sink(n, q, t); ++n; };
  emit1(Q - 1, T - 1);
  emit1(q_end, t_end);
  if (strip_walk<kPitch, true>(strip, q_end, t_end, n, sink)) emit1(0, 0);
  sink.finish();
  if (lane == 0) {
    res.n_path = n;
    res.status = 0;
    g.res[hit] = res;
    g.same[hit] = sink.same;
  }
}

template <int R, class Side>
__global__ __launch_bounds__(64) void count_global_hit_kernel(ScoreArgs a, CountArgs g, const char* __restrict__ qch,
                                                             const char* __restrict__ tch, int free_del, int free_ins) {
  __shared__ __attribute__((aligned(16))) int lds[32 * 32];
  const int lane = threadIdx.x;
  Side::stage(lds, a);
  const int hit = g.list[blockIdx.x];
  const HitDesc hd = g.desc[hit];
  const int ti = hd.t, qi = hd.q;
  const typename Side::Rows::Src* __restrict__ qr = Side::rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const auto* __restrict__ qs = Side::letters(a.qcodes, qch) + a.qoff[qi];
  const auto* __restrict__ ts = Side::letters(a.tcodes, tch) + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);   // Q >= 3, T >= 3: the host's routing
  const int gi = a.gi, ge = a.ge;
  constexpr int kPitch = 256 * R;
  uint8_t* strip = g.strip + hd.strip_off;      // row i (2 .. Q-2) at strip + (i - 2) * kPitch

  GlobalCols<R> cols;
  cols.load(tc, T, gi, ge);
  GlobalObserver<R> ob(cols, free_del, free_ins ? 0 : ge, Q - 3);
  ob.strip = strip; ob.pitch = kPitch;
  int score = sweep_global<R, typename Side::Rows>(lds, cols, qr, Q, free_del, free_ins, ob);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) score = max(score, __shfl_xor(score, off));

  int i, j;
  ob.final_cell(free_ins, i, j);
  __threadfence();                                           // (staged side: the last copy has landed;) the walk's lanes read bytes other lanes stored
  __syncthreads();

  CountSink<decltype(Side::letters(a.tcodes, tch))> sink = {qs, ts, tc, g.rows + 32 * (a.qoff[qi] - g.row0), Q, T, g.weight[hit]};
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
    res.status = 0;
    g.res[hit] = res;
    g.same[hit] = sink.same;
  }
}

// The shared body of aln_hits_column_counts and aln_hits_column_counts_profiles (run: prepared; `queries`: the pool the query
// letters and lengths are read from, as in align_block): the slot checks, the routes, the chunks of fused hits, the batches.
static int count_block(ScoreRun& run, const aln_seqs* queries, int32_t K, const aln_hit* hits, const int32_t* n_hits,
                       const int32_t* weights, aln_hit_alignment* out, int32_t* counts, int32_t* covered) {
  aln_ctx* ctx = run.ctx;
  const aln_seqs* templates = run.templates;
  const aln_qprofiles* prof = run.prof;
  const int32_t q_begin = run.q_begin;
  const int rows = run.rows, n_t = run.n_t;
  if (rows == 0) return ALN_OK;
  const int n_alpha = prof ? prof->n : run.sub->n;
  const char* alphabet = prof ? prof->alphabet : run.sub->alphabet;
  const int64_t row0 = queries->offsets[q_begin];
  const size_t n_rows = (size_t)(queries->offsets[run.q_end] - row0);

  // align_block's walk (every used slot validated and described for its route), then the weights; nothing written before
  SlotRoutes sr;
  int rc = route_slots(run, queries, K, hits, n_hits, sr);
  if (rc != ALN_OK) return rc;
  std::vector<HitDesc>& fast = sr.fast;
  const std::vector<size_t>& fast_slot = sr.fast_slot;
  const std::vector<int32_t>&bq = sr.bq, &bt = sr.bt;
  const std::vector<size_t>& bslot = sr.bslot;
  if (weights)
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < n_hits[r]; ++k)
        if (weights[(size_t)r * K + k] < 0 || weights[(size_t)r * K + k] > 65535) return ALN_E_ARG;
  auto weight_of = [&](size_t slot) { return weights ? weights[slot] : 1; };
  ctx->align_routes[0] = (int64_t)fast.size(); ctx->align_routes[1] = (int64_t)bq.size();

  memset(counts, 0, n_rows * (size_t)n_alpha * 4);
  if (covered) memset(covered, 0, n_rows * 4);
  for (int r = 0; r < rows; ++r)
    for (int k = n_hits[r]; k < K; ++k) out[(size_t)r * K + k] = aln_hit_alignment{0, 0, 0.0f, 0.0f};
  AlignOut ao = {out, nullptr, 0, nullptr, nullptr, 0, nullptr};

  // chunks of fused hits: the strips stay below the budget; the hint only asks for fewer
  struct Chunk { size_t h0, n; size_t strip; int cls_cnt[9]; };
  std::vector<Chunk> chunks;
  std::vector<int32_t> fast_w(fast.size());
  {
    const size_t forced = ctx->hints.align_chunk_hits > 0 ? (size_t)ctx->hints.align_chunk_hits : (size_t)-1;
    Chunk c = {0, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0, 0}};
    for (size_t h = 0; h < fast.size(); ++h) {
      HitDesc& d = fast[h];
      fast_w[h] = (run.local && !(d.score > 0.f)) ? 0 : weight_of(fast_slot[h]);
      const int srows = run.local ? d.q_end - 1 : (int)(queries->offsets[d.q + 1] - queries->offsets[d.q]) - 3;
      const size_t need = (size_t)std::max(srows, 1) * 256 * (size_t)d.cls;
      if (c.n > 0 && (c.n >= forced || c.strip + need > kCountStripBudget)) {
        chunks.push_back(c);
        c = {h, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0, 0}};
      }
      d.strip_off = (int64_t)c.strip;
      c.strip += need; c.n++; c.cls_cnt[d.cls]++;
    }
    if (c.n > 0) chunks.push_back(c);
  }

  if (!chunks.empty()) {
    size_t max_n = 1, max_strip = 1;
    for (const Chunk& c : chunks) { max_n = std::max(max_n, c.n); max_strip = std::max(max_strip, c.strip); }
    uint8_t* dstrip = nullptr; HitDesc* ddesc = nullptr; int32_t *dlist = nullptr, *dfill = nullptr, *dw = nullptr, *dsame = nullptr;
    int32_t* drows = nullptr; PairResult* dres = nullptr; char *dqch = nullptr, *dtch = nullptr;
    auto cleanup = [&]() {
      hipFree(dstrip); hipFree(ddesc); hipFree(dlist); hipFree(dfill); hipFree(dw); hipFree(dsame); hipFree(drows); hipFree(dres);
      hipFree(dqch); hipFree(dtch);
      run.release();
    };
#define STRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { ctx->last_error = std::string(#expr) + ": " + hipGetErrorString(e_); hipStreamSynchronize(ctx->stream); cleanup(); return ALN_E_HIP; } } while (0)
#define RTRY(expr) do { int r_ = (expr); if (r_ != ALN_OK) { hipStreamSynchronize(ctx->stream); cleanup(); return r_; } } while (0)
    if (prof)
      run.rows_per_slab = ctx->hints.align_rows_per_chunk != 0 ||
                          ((size_t)(prof->offsets[run.q_end] - prof->offsets[q_begin]) + kProfilePadRows) * 128 > kCountStripBudget;
    RTRY(run.upload());
    STRY(hipMalloc((void**)&dstrip, max_strip));
    STRY(hipMalloc((void**)&ddesc, max_n * sizeof(HitDesc)));
    STRY(hipMalloc((void**)&dlist, max_n * 4));
    STRY(hipMalloc((void**)&dfill, 9 * 4));
    STRY(hipMalloc((void**)&dw, max_n * 4));
    STRY(hipMalloc((void**)&dsame, max_n * 4));
    STRY(hipMalloc((void**)&dres, max_n * sizeof(PairResult)));
    STRY(hipMalloc((void**)&drows, std::max<size_t>(n_rows, 1) * 128));
    STRY(hipMemsetAsync(drows, 0, std::max<size_t>(n_rows, 1) * 128, ctx->stream));      // once per call, not per chunk
    std::vector<PairResult> hres(max_n);
    std::vector<int32_t> hsame(max_n);
    if (prof) {                            // the profile kernels count the identity over the characters
      const size_t nq = (size_t)queries->offsets[queries->n_seqs], nt = (size_t)templates->offsets[n_t];
      STRY(hipMalloc((void**)&dqch, std::max<size_t>(nq, 1)));
      STRY(hipMalloc((void**)&dtch, std::max<size_t>(nt, 1)));
      STRY(hipMemcpyAsync(dqch, queries->residues, nq, hipMemcpyHostToDevice, ctx->stream));
      STRY(hipMemcpyAsync(dtch, templates->residues, nt, hipMemcpyHostToDevice, ctx->stream));
    }
    for (const Chunk& c : chunks) {
      const int n = (int)c.n;
      ClassOff co = {};
      for (int k = 1; k < 9; ++k) co.off[k] = co.off[k - 1] + c.cls_cnt[k - 1];
      if (prof && run.rows_per_slab) RTRY(run.upload_profile_rows(fast[c.h0].q, fast[c.h0 + c.n - 1].q + 1));
      STRY(hipMemcpyAsync(ddesc, fast.data() + c.h0, (size_t)n * sizeof(HitDesc), hipMemcpyHostToDevice, ctx->stream));
      STRY(hipMemcpyAsync(dw, fast_w.data() + c.h0, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
      STRY(hipMemsetAsync(dfill, 0, 9 * 4, ctx->stream));
      const DescClass dc = {ddesc};
      hipLaunchKernelGGL(class_list_kernel<DescClass>, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, dc, n, co, dfill, dlist);
      STRY(hipGetLastError());
      CountArgs g = {};
      g.desc = ddesc; g.strip = dstrip; g.weight = dw; g.rows = drows; g.row0 = row0; g.res = dres; g.same = dsame;
      for (int k = 1; k <= 8; ++k) {
        if (c.cls_cnt[k] == 0) continue;
        g.list = dlist + co.off[k];
        auto launch = [&](auto side) {
          typedef decltype(side) Side;
          const dim3 grid(c.cls_cnt[k]), block(64);
          const char *qch = Side::kStaged ? dqch : nullptr, *tch = Side::kStaged ? dtch : nullptr;
          constexpr int kLocalMax = ((Side::kFusedLocal >> 8) & 1u) ? 8 : 7;   // a class the mask leaves out never gets here
          if (run.local)
            dispatch_r<kLocalMax>(k, [&](auto rc) {
              hipLaunchKernelGGL((count_local_hit_kernel<decltype(rc)::value, Side>), grid, block, 0, ctx->stream, run.a, g, qch, tch);
            });
          else
            dispatch_r<8>(k, [&](auto rc) {
              hipLaunchKernelGGL((count_global_hit_kernel<decltype(rc)::value, Side>), grid, block, 0, ctx->stream, run.a, g, qch, tch,
                                 run.free_del, run.free_ins);
            });
        };
        if (prof) launch(ProfileQuery());
        else launch(ResidueQuery());
        STRY(hipGetLastError());
      }
      STRY(hipMemcpyAsync(hres.data(), dres, (size_t)n * sizeof(PairResult), hipMemcpyDeviceToHost, ctx->stream));
      STRY(hipMemcpyAsync(hsame.data(), dsame, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
      STRY(hipStreamSynchronize(ctx->stream));                 // the host vectors above are read by the copies until here
      for (int h = 0; h < n; ++h) {
        const HitDesc& d = fast[c.h0 + h];
        const int64_t Q = queries->offsets[d.q + 1] - queries->offsets[d.q], T = templates->offsets[d.t + 1] - templates->offsets[d.t];
        put_fused(ao, fast_slot[c.h0 + h], hres[h], hsame[h], Q, T, nullptr, nullptr, nullptr, 0);
      }
    }
    std::vector<int32_t> hrows(n_rows * 32);
    STRY(hipMemcpyAsync(hrows.data(), drows, n_rows * 128, hipMemcpyDeviceToHost, ctx->stream));
    STRY(hipStreamSynchronize(ctx->stream));
    for (size_t r = 0; r < n_rows; ++r) {
      memcpy(counts + r * (size_t)n_alpha, hrows.data() + r * 32, (size_t)n_alpha * 4);
      if (covered) covered[r] = hrows[r * 32 + kCoveredCol];
    }
#undef STRY
#undef RTRY
    cleanup();
  }

  // the batch route, a group of slots at a time: records and pair lists into buffers of the group, tallied here
  if (!bq.empty()) {
    int idx[256];
    for (int i = 0; i < 256; ++i) idx[i] = -1;
    for (int i = 0; i < n_alpha; ++i) idx[(unsigned char)alphabet[i]] = i;
    constexpr size_t kGroupBytes = (size_t)256 << 20;        // of pair lists on the host at a time
    std::vector<aln_hit_alignment> grec;
    std::vector<int32_t> gpairs, gq, gt;
    std::vector<size_t> gslot;
    for (size_t b0 = 0; b0 < bq.size();) {
      size_t b1 = b0; int64_t stride = 4;
      while (b1 < bq.size()) {
        const int64_t Q = queries->offsets[bq[b1] + 1] - queries->offsets[bq[b1]];
        const int64_t T = templates->offsets[bt[b1] + 1] - templates->offsets[bt[b1]];
        const int64_t s = std::max(stride, std::min(Q, T) + 3);
        if (b1 > b0 && (b1 + 1 - b0) * (size_t)s * 8 > kGroupBytes) break;
        stride = s; ++b1;
      }
      const size_t nb = b1 - b0;
      grec.assign(nb, aln_hit_alignment{0, 0, 0.0f, 0.0f});
      gpairs.assign(nb * (size_t)stride * 2, 0);
      gq.assign(bq.begin() + b0, bq.begin() + b1); gt.assign(bt.begin() + b0, bt.begin() + b1);
      gslot.resize(nb);
      for (size_t p = 0; p < nb; ++p) gslot[p] = p;
      AlignOut go = {grec.data(), gpairs.data(), (int32_t)stride, nullptr, nullptr, 0, nullptr};
      rc = align_through_batches(ctx, queries, templates, run.sub, prof, run.gap, gq, gt, gslot, go);
      if (rc != ALN_OK) return rc;
      for (size_t p = 0; p < nb; ++p) {
        const size_t slot = bslot[b0 + p];
        const aln_hit_alignment& rec = grec[p];
        out[slot] = rec;
        ao.note(rec.status);
        const int w = weight_of(slot);
        if (rec.status != 0 || w <= 0 || (run.local && !(rec.score > 0.f))) continue;
        const int64_t qo = queries->offsets[gq[p]], Q = queries->offsets[gq[p] + 1] - qo;
        const int64_t to = templates->offsets[gt[p]], T = templates->offsets[gt[p] + 1] - to;
        const int32_t* l = gpairs.data() + p * (size_t)stride * 2;
        int64_t lo = INT64_MAX, hi = -1;
        for (int k = 0; k < rec.n_pairs; ++k) {
          const int64_t i = l[2 * k], j = l[2 * k + 1];
          if (i < 1 || i > Q - 2 || j < 1 || j > T - 2) continue;
          const int a = idx[(unsigned char)templates->residues[to + j]];
          if (a >= 0) counts[(size_t)(qo - row0 + i) * n_alpha + a] += w;
          lo = std::min(lo, i); hi = std::max(hi, i);
        }
        if (covered)
          for (int64_t i = lo; i <= hi; ++i) covered[qo - row0 + i] += w;
      }
      b0 = b1;
    }
  }
  return ao.worst;
}

}  // namespace aln

using namespace aln;

extern "C" int aln_hits_column_counts(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                                      const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K, const aln_hit* hits,
                                      const int32_t* n_hits, const int32_t* weights, aln_hit_alignment* out, int32_t* counts,
                                      int32_t* covered) {
  if (ctx) ctx->align_routes[0] = ctx->align_routes[1] = 0;
  if (!hits || !n_hits || !out || !counts || K < 1 || K > 1024) return ALN_E_ARG;
  ScoreRun run;
  int rc = run.prepare(ctx, queries, templates, sub, gap, q_begin, q_end);
  if (rc != ALN_OK) return rc;
  return count_block(run, run.queries, K, hits, n_hits, weights, out, counts, covered);
}

extern "C" int aln_hits_column_counts_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus,
                                               const aln_seqs* templates, const aln_gap* gap, int32_t q_begin, int32_t q_end,
                                               int32_t K, const aln_hit* hits, const int32_t* n_hits, const int32_t* weights,
                                               aln_hit_alignment* out, int32_t* counts, int32_t* covered) {
  if (ctx) ctx->align_routes[0] = ctx->align_routes[1] = 0;
  if (!profiles || !templates || !gap) return ALN_E_ARG;
  if (!hits || !n_hits || !out || !counts || K < 1 || K > 1024) return ALN_E_ARG;
  ScoreRun run;
  run.consensus = consensus;
  int rc = run.prepare(ctx, nullptr, templates, nullptr, gap, q_begin, q_end, profiles);
  if (rc != ALN_OK) return rc;
  return count_block(run, consensus ? consensus : run.queries, K, hits, n_hits, weights, out, counts, covered);
}
