// search_weights.hip — position-based sequence weights of search hits, on the device: aln_hits_weights (gfx950).
//
// Before the hits of a search round become the next round's profile, redundant hits are weighted down: forty near-copies of one
// homolog must not out-vote five distant ones.  Henikoff's position-based weights are read off the query-anchored pileup
// (include/aln_hip.h has the definition: exact integers, so the result depends on neither launch order, chunking nor route), and
// here the pileup never leaves the device:
//   the stack        the letters rows of a GROUP of consecutive queries, slot-major: slot (r, k) of the group at
//                    stack + (r K + k) stride, stride = the block's longest Q - 2.  Preset to '.', so unused, muted, refused
//                    and failed slots are rows of '.', which count nowhere.  A fused hit's row is written by
//                    hit_local_kernel / hit_global_kernel<R, Side, PileupJob> (search_pileup.h; the kernels are search_pileup.hip's)
//                    into the chunk's row buffer and moved to its slot by scatter_rows_kernel — hits of one query fall into
//                    different chunks, and the batch route's slots are missing from the chunks' numbering; a batch slot's row is
//                    laid out on the host (pileup_from_list) and uploaded into its slot.
//   column_tally_kernel<false>   per query and tile of 64 positions one wave, lanes along positions (a slot's row is read
//                    coalesced), a loop over the K slots; every lane owns a 32-counter histogram in LDS (stride 33 words: the
//                    lanes of a wave hit different banks).  Leaves n_p[a] and, in the spare column 31, k_p.
//   slot_raw_kernel  one wave per slot, lanes along positions: raw = sum floor(2^24 / (k_p n_p[a])), an exact 32-bit divide,
//                    the int64 sums reduced across the wave.
//   normalise_kernel one wave per query: M = max raw over the K slots, weight = max(1, floor(w_max raw / M)) in 64 bits.
//   column_tally_kernel<true>    the same tally weighted by weight[k]: the count rows aln_hits_column_counts downloads (32 int32,
//                    `covered` in column 31: the weight of every slot whose letter is neither '.' nor NUL).
// Only weights, raw, the hits' records and the count rows come down.  A block whose stack would exceed kStackBudget is cut into
// groups of consecutive queries (hint weights_group_rows asks for fewer rows); a group runs the fused route (FusedRoute), the
// batch route (for_list_groups) and the four kernels over its own queries.  The stack's construction is search_stack.h's
// HitStack, which aln_hits_purge (search_purge.hip) builds the same stack with; the kernels of this file reach it through
// launch_scatter_rows and launch_weight_kernels.
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "search_stack.h"

namespace aln {

constexpr int kHistStride = 33;                         // words between the histograms of neighbouring lanes

// a chunk's letters rows into their slots of the stack: one wave per hit
__global__ __launch_bounds__(64) void scatter_rows_kernel(const char* __restrict__ src, char* __restrict__ stack,
                                                          const int32_t* __restrict__ slot, int64_t stride) {
  const char* s = src + (size_t)blockIdx.x * stride;
  char* d = stack + (size_t)slot[blockIdx.x] * stride;
  for (int64_t i = threadIdx.x; i < stride; i += 64) d[i] = s[i];
}

// The tally of one tile: out[(row + p) * 32 + a] = sum over the slots k whose letter at p is alphabet[a] of w_k (1, or
// weight[r K + k]); column 31: the number of letters present (unweighted), the weight of the slots that span p (weighted).
// idx: character -> index in the alphabet, -1 for every other byte.
template <bool WEIGHTED>
__global__ __launch_bounds__(64) void column_tally_kernel(const char* __restrict__ stack, int64_t stride, int K,
                                                          const WeightQuery* __restrict__ qr, const int8_t* __restrict__ idx,
                                                          const int32_t* __restrict__ weight, int32_t* __restrict__ out) {
  __shared__ int hist[64 * kHistStride];
  __shared__ int8_t lidx[256];
  const int lane = threadIdx.x, r = blockIdx.y, p0 = blockIdx.x * 64;
  const WeightQuery q = qr[r];
  if (p0 >= q.len) return;                                   // block-uniform
  for (int i = lane; i < 256; i += 64) lidx[i] = idx[i];
  for (int i = lane; i < 64 * kHistStride; i += 64) hist[i] = 0;
  __syncthreads();
  const bool in = p0 + lane < q.len;
  const char* col = stack + (size_t)r * K * stride + p0 + lane;
  const int32_t* w = weight + (size_t)r * K;
  int* h = hist + lane * kHistStride;
  int cov = 0;
  for (int k = 0; k < K; ++k) {
    const unsigned char c = in ? (unsigned char)col[(size_t)k * stride] : (unsigned char)'.';
    const int wk = WEIGHTED ? w[k] : 1;
    const int a = lidx[c];
    if (a >= 0) h[a] += wk;
    if (WEIGHTED) cov += (c != '.' && c != 0) ? wk : 0;
  }
  if (WEIGHTED) h[kSpareCol] = cov;
  else {
    int kp = 0;
    for (int a = 0; a < 30; ++a) kp += h[a] > 0 ? 1 : 0;
    h[kSpareCol] = kp;
  }
  __syncthreads();
  const int n = min(64, q.len - p0);                         // the tile's rows are consecutive count rows
  int32_t* o = out + (q.row + p0) * 32;
  for (int i = lane; i < n * 32; i += 64) o[i] = hist[(i >> 5) * kHistStride + (i & 31)];
}

// raw[slot] = sum over the positions whose letter a is in the alphabet of floor(2^24 / (k_p n_p[a])); np: the unweighted tally
__global__ __launch_bounds__(64) void slot_raw_kernel(const char* __restrict__ stack, int64_t stride, int K,
                                                      const WeightQuery* __restrict__ qr, const int8_t* __restrict__ idx,
                                                      const int32_t* __restrict__ np, int64_t* __restrict__ raw) {
  __shared__ int8_t lidx[256];
  const int lane = threadIdx.x, slot = blockIdx.x;
  const WeightQuery q = qr[slot / K];
  for (int i = lane; i < 256; i += 64) lidx[i] = idx[i];
  __syncthreads();
  const char* row = stack + (size_t)slot * stride;
  const int32_t* n = np + q.row * 32;
  long long s = 0;
  for (int p = lane; p < q.len; p += 64) {
    const int a = lidx[(unsigned char)row[p]];
    if (a >= 0) {
      const unsigned d = (unsigned)n[(size_t)p * 32 + kSpareCol] * (unsigned)n[(size_t)p * 32 + a];   // >= 1: the slot itself was counted
      s += d ? (1u << 24) / d : 0u;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) raw[slot] = s;
}

// weight[r K + k] = 0 where raw is 0, else max(1, floor(w_max raw / M)), M the largest raw of the row's K slots
__global__ __launch_bounds__(64) void normalise_kernel(const int64_t* __restrict__ raw, int K, int w_max, int32_t* __restrict__ weight) {
  const int lane = threadIdx.x;
  const int64_t* x = raw + (size_t)blockIdx.x * K;
  int32_t* w = weight + (size_t)blockIdx.x * K;
  long long m = 0;
  for (int k = lane; k < K; k += 64) m = max(m, (long long)x[k]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = max(m, __shfl_xor(m, off));
  for (int k = lane; k < K; k += 64) {
    const unsigned long long v = (unsigned long long)x[k];
    w[k] = v == 0 ? 0 : (int32_t)max(1ull, (unsigned long long)w_max * v / (unsigned long long)m);
  }
}

// scatter_rows_kernel and the four launches over a complete group behind ordinary functions (search_stack.h): the kernels are
// instantiated in this file alone
int launch_scatter_rows(aln_ctx* ctx, const char* src, char* stack, const int32_t* slot, int64_t stride, size_t n) {
  hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)n), dim3(64), 0, ctx->stream, src, stack, slot, stride);
  STRY(hipGetLastError());
  return ALN_OK;
}

int launch_weight_kernels(aln_ctx* ctx, const WeightLaunch& w) {
  const dim3 tiles((unsigned)((w.stride + 63) / 64), (unsigned)w.gn), wave(64);
  hipLaunchKernelGGL(column_tally_kernel<false>, tiles, wave, 0, ctx->stream, w.stack, w.stride, w.K, w.qr, w.idx, w.wt, w.np);
  STRY(hipGetLastError());
  hipLaunchKernelGGL(slot_raw_kernel, dim3((unsigned)(w.gn * w.K)), wave, 0, ctx->stream, w.stack, w.stride, w.K, w.qr, w.idx, w.np, w.raw);
  STRY(hipGetLastError());
  hipLaunchKernelGGL(normalise_kernel, dim3((unsigned)w.gn), wave, 0, ctx->stream, w.raw, w.K, w.w_max, w.wt);
  STRY(hipGetLastError());
  if (w.cnt) {
    STRY(hipMemsetAsync(w.cnt, 0, w.g_rows * 128, ctx->stream));                          // the sentinel rows stay zero
    hipLaunchKernelGGL(column_tally_kernel<true>, tiles, wave, 0, ctx->stream, w.stack, w.stride, w.K, w.qr, w.idx, w.wt, w.cnt);
    STRY(hipGetLastError());
  }
  return ALN_OK;
}

// The shared body of aln_hits_weights and aln_hits_weights_profiles (run: prepared; `queries`: the pool the query lengths are
// read from — hit_entry's pool, search_align.h).  The stack's construction and the weights' buffers: search_stack.h.
static int weights_block(ScoreRun& run, const aln_seqs* queries, int32_t K, const aln_hit* hits, const int32_t* n_hits, int32_t w_max,
                         aln_hit_alignment* out, int32_t* weights, int64_t* raw, int32_t* counts, int32_t* covered) {
  aln_ctx* ctx = run.ctx;
  if (!weights || w_max < 1 || w_max > 65535) return ALN_E_ARG;
  if (run.rows == 0) return ALN_OK;
  HitStack st(run, queries, K, out);
  const int rc = st.route(hits, n_hits);                     // nothing written before
  if (rc != ALN_OK) return rc;
  StackWeights sw(st, w_max, weights, raw, counts, covered);
  sw.clear();
  st.ao.clear_unused(run.rows, K, n_hits);
  RTRY(st.alloc(1, 0));                                      // the stride: the block's longest Q - 2
  RTRY(sw.alloc());
  RTRY(st.build("aln_hits_weights", [&](const StackGroup& g) { return sw.group(g); }));
  return st.ao.worst;
}

}  // namespace aln

using namespace aln;

extern "C" int aln_hits_weights(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                                const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K, const aln_hit* hits,
                                const int32_t* n_hits, int32_t w_max, aln_hit_alignment* out, int32_t* weights, int64_t* raw,
                                int32_t* counts, int32_t* covered) {
  return hit_entry(ctx, false, queries, nullptr, nullptr, templates, sub, gap, q_begin, q_end, hit_list_ok(K, hits, n_hits, out),
                   [&](ScoreRun& run, const aln_seqs* pool) {
                     return weights_block(run, pool, K, hits, n_hits, w_max, out, weights, raw, counts, covered);
                   });
}

extern "C" int aln_hits_weights_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus,
                                         const aln_seqs* templates, const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                                         const aln_hit* hits, const int32_t* n_hits, int32_t w_max, aln_hit_alignment* out,
                                         int32_t* weights, int64_t* raw, int32_t* counts, int32_t* covered) {
  return hit_entry(ctx, true, nullptr, profiles, consensus, templates, nullptr, gap, q_begin, q_end, hit_list_ok(K, hits, n_hits, out),
                   [&](ScoreRun& run, const aln_seqs* pool) {
                     return weights_block(run, pool, K, hits, n_hits, w_max, out, weights, raw, counts, covered);
                   });
}

#undef STRY
#undef RTRY
