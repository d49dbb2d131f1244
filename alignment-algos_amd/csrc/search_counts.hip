// search_counts.hip — the column counts of search hits, on the device: aln_hits_column_counts (gfx950).
//
// The step from one search round to the next needs, per query position, how often each template letter stands under it in
// the alignments of the query's hits: one small integer matrix per query, not the alignments.  So the two kernels of
// search_align.h are instantiated here with another job behind the same sweep and walk:
//   hit_local_kernel<R, Side, CountJob>    sweep_local + StripObserver<true> + the score check + strip_walk;
//   hit_global_kernel<R, Side, CountJob>   sweep_global + GlobalObserver + final_cell + strip_walk.
// One wave per hit.  The job's sink counts `same` for the identity (the record is aln_hits_align's), keeps the lane's smallest and
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

// The shared body of aln_hits_column_counts and aln_hits_column_counts_profiles (run: prepared; `queries`: the pool the query
// letters and lengths are read from, as in align_block): the slot checks, the routes, the chunks of fused hits, the batches.
static int count_block(ScoreRun& run, const aln_seqs* queries, int32_t K, const aln_hit* hits, const int32_t* n_hits,
                       const int32_t* weights, aln_hit_alignment* out, int32_t* counts, int32_t* covered) {
  aln_ctx* ctx = run.ctx;
  const aln_seqs* templates = run.templates;
  const aln_qprofiles* prof = run.prof;
  const int32_t q_begin = run.q_begin;
  const int rows = run.rows;
  if (rows == 0) return ALN_OK;
  const int n_alpha = prof ? prof->n : run.sub->n;
  const char* alphabet = prof ? prof->alphabet : run.sub->alphabet;
  const int64_t row0 = queries->offsets[q_begin];
  const size_t n_rows = (size_t)(queries->offsets[run.q_end] - row0);

  // align_block's walk (every used slot validated and described for its route), then the weights; nothing written before
  SlotRoutes sr;
  int rc = route_slots(run, queries, K, hits, n_hits, hit_kernel_classes(run), run.local, sr);
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

  // chunks of fused hits: no lists and no lines, so only the strips count against the budget
  if (!fast.empty()) {
    FusedRoute<HitDesc> fr(run, queries, fast);
    std::vector<int32_t> fast_w(fast.size());
    for (size_t h = 0; h < fast.size(); ++h) fast_w[h] = (run.local && !(fast[h].score > 0.f)) ? 0 : weight_of(fast_slot[h]);
    fr.cut(0, false, 0, [&](const HitDesc& d) {
      const int srows = run.local ? d.q_end - 1 : (int)(queries->offsets[d.q + 1] - queries->offsets[d.q]) - 3;
      return HitNeed{(size_t)std::max(srows, 1) * 256 * (size_t)d.cls, 0, 0};
    });
    const size_t max_n = fr.max_n;
    int32_t *dw = nullptr, *dsame = nullptr, *drows = nullptr; PairResult* dres = nullptr;
    RTRY(fr.begin());
    STRY(fr.bufs.get(dw, max_n));
    STRY(fr.bufs.get(dsame, max_n));
    STRY(fr.bufs.get(dres, max_n));
    STRY(fr.bufs.get(drows, std::max<size_t>(n_rows, 1) * 32));
    STRY(hipMemsetAsync(drows, 0, std::max<size_t>(n_rows, 1) * 128, ctx->stream));      // once per call, not per chunk
    std::vector<PairResult> hres(max_n);
    std::vector<int32_t> hsame(max_n);
    if (prof) RTRY(fr.upload_pools());
    for (const FusedChunk& c : fr.chunks) {
      const int n = (int)c.n;
      RTRY(fr.stage(c, [&]() -> int {
        STRY(hipMemcpyAsync(dw, fast_w.data() + c.h0, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        return ALN_OK;
      }));
      CountArgs g = {};
      g.desc = fr.ddesc; g.strip = fr.dstrip; g.weight = dw; g.rows = drows; g.row0 = row0; g.res = dres; g.same = dsame;
      RTRY(fr.launch(c, [&](auto side, int k, int cnt, const int32_t* list, const char* qch, const char* tch) {
        typedef decltype(side) Side;
        const dim3 grid(cnt), block(64);
        g.list = list;
        constexpr int kLocalMax = ((Side::kFusedLocal >> 8) & 1u) ? 8 : 7;   // a class the mask leaves out never gets here
        if (run.local)
          dispatch_r<kLocalMax>(k, [&](auto rc) {
            hipLaunchKernelGGL((hit_local_kernel<decltype(rc)::value, Side, CountJob>), grid, block, 0, ctx->stream, run.a, g, qch, tch);
          });
        else
          dispatch_r<8>(k, [&](auto rc) {
            hipLaunchKernelGGL((hit_global_kernel<decltype(rc)::value, Side, CountJob>), grid, block, 0, ctx->stream, run.a, g, qch, tch,
                               run.free_del, run.free_ins);
          });
      }));
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

#undef STRY
#undef RTRY
