// search_pssm.hip — from a search round's hits to the next round's profile rows, on the device: aln_hits_pssm (gfx950).
//
// The last step of an iterative search round that was left to the host: the weighted counts of the purged, weighted hits become
// integer log-odds rows, the aln_qprofiles rows of the next round.  include/aln_hip.h has the definition — the pseudo-count
// mix, num and den in 64-bit integers, lg16 and the rounding; pssm_rule.h is that rule for host and device — and it is exact:
// the rows depend on neither chunking, grouping, route nor launch order, nor on a libm.
// Everything up to the counts is aln_hits_purge's (purge_block, search_purge.hip, over search_stack.h's HitStack and
// StackWeights): the stack, the four purge launches, the four weight launches.  The group's weighted count rows stay on the
// device (32 int32 each, covered in column 31) and here
//   pssm_rows_kernel   one half-wave per count row, lane = letter; eight rows per block.  N by five xor-shuffles; g[a] =
//                      sum_b c[b] mix[b][a] with mix staged once per block into LDS (32 x 32 words: lane a of a half-wave reads
//                      word b * 32 + a, the 32 banks once) and c[b] broadcast across the half-wave; num, den and the score per
//                      lane; a row leaves as n consecutive floats, the rows of a block as one contiguous run.  A row without
//                      counts (N == 0) leaves as kNoCounts and the host fills it from the table row of the query's residue or
//                      from the profile's own row, and zeroes the sentinel rows.
// Only the rows come down, plus what aln_hits_purge downloads for the optional outputs that were asked for.
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "pssm_rule.h"
#include "search_stack.h"

namespace aln {

constexpr int kPssmBlockRows = 8;                       // half-waves of a block
constexpr uint32_t kNoCounts = 0x7FC00000u;             // a NaN: no score is one (every score is an integer within +-296)

// out[row * n + a] for the g_rows count rows of a group: the score of letter a, or kNoCounts in a row whose counts sum to 0.
// cnt: 32 int32 per row, the letters' weighted counts in columns 0 .. n-1.  mix: n x n (the caller's, or n rows of bg).
__global__ __launch_bounds__(32 * kPssmBlockRows) void pssm_rows_kernel(const int32_t* __restrict__ cnt, unsigned g_rows, int n, int scale,
                                                                        uint32_t beta, uint32_t B, const int32_t* __restrict__ bg,
                                                                        const int32_t* __restrict__ mix, float* __restrict__ out) {
  __shared__ uint32_t smix[32 * 32];
  for (int i = threadIdx.x; i < 32 * 32; i += 32 * kPssmBlockRows) {
    const int b = i >> 5, a = i & 31;
    smix[i] = (b < n && a < n) ? (uint32_t)mix[b * n + a] : 0u;
  }
  __syncthreads();
  const int a = threadIdx.x & 31;
  const unsigned row = blockIdx.x * kPssmBlockRows + (threadIdx.x >> 5);
  const bool mine = row < g_rows && a < n;
  const uint32_t c = mine ? (uint32_t)cnt[(size_t)row * 32 + a] : 0u;
  uint32_t N = c;                                       // below 2^26
#pragma unroll
  for (int off = 16; off >= 1; off >>= 1) N += __shfl_xor(N, off);   // (stays inside the half-wave)
  uint64_t g = 0;                                       // at most N B < 2^36
  for (int b = 0; b < n; ++b) g += (uint64_t)(uint32_t)__shfl(c, b, 32) * smix[b * 32 + a];
  if (!mine) return;
  uint32_t v = kNoCounts;
  if (N != 0) {
    const uint64_t num = (uint64_t)c * N * B + (uint64_t)beta * g;             // < 2^62 + 2^62
    const uint64_t den = (uint64_t)(N + beta) * N * (uint32_t)bg[a];           // < 2^27 2^26 2^10
    v = __float_as_uint((float)pssm_score(num, den, scale));
  }
  out[(size_t)row * n + a] = __uint_as_float(v);
}

// The shared body of aln_hits_pssm and aln_hits_pssm_profiles (run: prepared; `queries`: the pool the query letters and
// lengths are read from — hit_entry's pool, search_align.h).
static int pssm_block(ScoreRun& run, const aln_seqs* queries, int32_t K, const aln_hit* hits, const int32_t* n_hits,
                      int32_t max_identity, int32_t min_overlap, int32_t w_max, const aln_pssm_params* par, aln_hit_alignment* out,
                      float* rows, aln_hit_purge* purge, int32_t* weights, int64_t* raw, int32_t* counts, int32_t* covered) {
  aln_ctx* ctx = run.ctx;
  if (max_identity < 1 || max_identity > 101 || min_overlap < 0 || min_overlap > 100) return ALN_E_ARG;
  if (w_max < 1 || w_max > 65535) return ALN_E_ARG;
  if (!par || !rows) return ALN_E_ARG;
  if (!pssm_scale_ok(par->scale)) return ALN_E_ARG;
  if (par->beta < 1 || par->beta > (1 << 26)) return ALN_E_ARG;
  const int n = run.prof ? run.prof->n : run.sub->n;
  if (!par->bg) return ALN_E_ARG;
  int64_t B = 0;
  for (int a = 0; a < n; ++a) {
    if (par->bg[a] < 1 || par->bg[a] > 1024) return ALN_E_ARG;
    B += par->bg[a];
  }
  if (B > 1024) return ALN_E_ARG;
  std::vector<int32_t> hmix((size_t)n * n);
  for (int b = 0; b < n; ++b) {
    int64_t sum = 0;
    for (int a = 0; a < n; ++a) {
      const int32_t m = par->mix ? par->mix[b * n + a] : par->bg[a];
      if (m < 1) return ALN_E_ARG;
      hmix[(size_t)b * n + a] = m;
      sum += m;
    }
    if (sum != B) return ALN_E_ARG;
  }
  if (run.rows == 0) return ALN_OK;

  // the outputs the caller did not ask for that the purge and the weights need a place for
  const size_t n_slots = (size_t)run.rows * K;
  std::vector<aln_hit_purge> own_purge(purge ? 0 : n_slots);
  std::vector<int32_t> own_weights(weights ? 0 : n_slots);

  int32_t *dbg = nullptr, *dmix = nullptr; float* drows = nullptr;
  const StackHook after = [&](HitStack& st, StackWeights& sw, const StackGroup& g) -> int {
    if (!drows) {                                            // the first group: max_grows is known since alloc()
      STRY(st.own.get(dbg, (size_t)n));
      STRY(st.own.get(dmix, (size_t)n * n));
      STRY(st.own.get(drows, st.max_grows * n));
      STRY(hipMemcpyAsync(dbg, par->bg, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));     // (both alive until the synchronisation below)
      STRY(hipMemcpyAsync(dmix, hmix.data(), hmix.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    const unsigned blocks = (unsigned)((g.g_rows + kPssmBlockRows - 1) / kPssmBlockRows);
    hipLaunchKernelGGL(pssm_rows_kernel, dim3(blocks), dim3(32 * kPssmBlockRows), 0, ctx->stream, sw.dcnt, (unsigned)g.g_rows, n,
                       (int)par->scale, (uint32_t)par->beta, (uint32_t)B, dbg, dmix, drows);
    STRY(hipGetLastError());
    float* grows = rows + (size_t)(g.grow0 - st.row0) * n;
    STRY(hipMemcpyAsync(grows, drows, g.g_rows * (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    STRY(hipStreamSynchronize(ctx->stream));
    // the sentinel rows, and the rows without counts: the table row of the query's residue, or the profile's own row
    for (size_t r = 0; r < g.gn; ++r) {
      const int64_t o = queries->offsets[run.q_begin + g.g0 + r], Q = queries->offsets[run.q_begin + g.g0 + r + 1] - o;
      float* qrows = rows + (size_t)(o - st.row0) * n;
      memset(qrows, 0, (size_t)n * 4);
      memset(qrows + (size_t)(Q - 1) * n, 0, (size_t)n * 4);
      for (int64_t i = 1; i + 1 < Q; ++i) {
        uint32_t first;
        memcpy(&first, qrows + (size_t)i * n, 4);
        if (first != kNoCounts) continue;
        const float* from = nullptr;
        if (run.prof) from = run.prof->rows + (size_t)(o + i) * n;
        else {
          // (< 0 only under a fractional table, where the run leaves the residue check to the batches: such a row is zeros)
          const int at = st.idx[(unsigned char)queries->residues[o + i]];
          if (at >= 0) from = run.sub->table + (size_t)at * n;
        }
        if (from) memcpy(qrows + (size_t)i * n, from, (size_t)n * 4);
        else memset(qrows + (size_t)i * n, 0, (size_t)n * 4);
      }
    }
    return ALN_OK;
  };
  return purge_block(run, queries, K, hits, n_hits, max_identity, min_overlap, w_max, out, purge ? purge : own_purge.data(),
                     weights ? weights : own_weights.data(), raw, counts, covered, &after);
}

}  // namespace aln

using namespace aln;

extern "C" int32_t aln_pssm_entry(uint64_t num, uint64_t den, int32_t scale) {
  if (num == 0 || den == 0 || (num >> 63) || (den >> 63) || !pssm_scale_ok(scale)) return 0;
  return pssm_score(num, den, scale);
}

extern "C" int aln_hits_pssm(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                             const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K, const aln_hit* hits,
                             const int32_t* n_hits, int32_t max_identity, int32_t min_overlap, int32_t w_max,
                             const aln_pssm_params* par, aln_hit_alignment* out, float* rows, aln_hit_purge* purge,
                             int32_t* weights, int64_t* raw, int32_t* counts, int32_t* covered) {
  return hit_entry(ctx, false, queries, nullptr, nullptr, templates, sub, gap, q_begin, q_end, hit_list_ok(K, hits, n_hits, out),
                   [&](ScoreRun& run, const aln_seqs* pool) {
                     return pssm_block(run, pool, K, hits, n_hits, max_identity, min_overlap, w_max, par, out, rows, purge, weights,
                                       raw, counts, covered);
                   });
}

extern "C" int aln_hits_pssm_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus,
                                      const aln_seqs* templates, const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                                      const aln_hit* hits, const int32_t* n_hits, int32_t max_identity, int32_t min_overlap,
                                      int32_t w_max, const aln_pssm_params* par, aln_hit_alignment* out, float* rows,
                                      aln_hit_purge* purge, int32_t* weights, int64_t* raw, int32_t* counts, int32_t* covered) {
  return hit_entry(ctx, true, nullptr, profiles, consensus, templates, nullptr, gap, q_begin, q_end, hit_list_ok(K, hits, n_hits, out),
                   [&](ScoreRun& run, const aln_seqs* pool) {
                     return pssm_block(run, pool, K, hits, n_hits, max_identity, min_overlap, w_max, par, out, rows, purge, weights,
                                       raw, counts, covered);
                   });
}

#undef STRY
#undef RTRY
