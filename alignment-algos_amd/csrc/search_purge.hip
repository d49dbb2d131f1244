// search_purge.hip — purging of near-identical search hits, on the device: aln_hits_purge (gfx950).
//
// Before the weights of a round are made, hits that are near-copies of a better hit are removed (PSI-BLAST at 94 % identity,
// hhfilter -id 90): weights damp redundancy, they do not remove it.  include/aln_hip.h has the definition — letters, overlap
// and same of two letters rows, NEAR, the greedy rule over the slots in the search's order; exact integers, so the result
// depends on neither launch order, chunking, grouping nor route.  The stack is aln_hits_weights' (search_stack.h: the letters
// rows of a group of consecutive queries, slot-major, preset to '.'), with the stride padded to a multiple of 4 so that every
// row starts on a dword and no read passes a row.  Over a complete group:
//   pair_near_kernel   the hot path.  Per query one wave per TILE: 64 slots k on the lanes x kTileJ slots j, only tiles that
//                      hold a pair j < k.  Rows are staged through LDS kChunkDw dwords of positions at a time, read coalesced
//                      and translated while staging by the 256-byte character -> index table: a letter becomes its index
//                      (< 0x80), every other byte 0xFF.  A lane reads its own row's dwords with a row stride of kChunkDw + 1
//                      dwords (odd: the 64 lanes hit different banks); the j row's dword is the same address for every lane,
//                      an LDS broadcast.  Four positions per dword:
//                        overlap += popcount(~(a | b) & 0x80808080)
//                        same    += popcount(zero-byte-mask(a ^ b) & ~(a | b) & 0x80808080)
//                      letters(k) is counted over the lane's own row on the way (the tile of j = 0 .. stores it).  The wave's 64
//                      near bits of one j leave as one 64-bit word (a ballot): word (r, j, k / 64) of the pair bits.
//   greedy_kernel      one wave per query, sequential over j = 0 .. K-1, lane w holding word w of the K-bit masks: a slot that
//                      shows a letter and is not yet purged is KEPT and purges every slot near it that is not purged yet — so
//                      a purged slot's keeper is the smallest kept slot it is near, and a purged slot purges nobody.
//   purge_record_kernel  one wave per slot: the record; for a purged slot same and overlap against its keeper are counted
//                      again (one pair per slot: the pair kernel stores no counts).
//   mute_rows_kernel   the rows of the slots that are not kept rewritten to '.'.
// Then, when weights are wanted, aln_hits_weights' four launches over the muted stack (launch_weight_kernels: they are
// search_weights.hip's, this file instantiates none of them).  Only records, purge records, weights, raw and count rows come down.
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "search_stack.h"

namespace aln {

constexpr int kTileJ = 32;                              // rows j of a tile: two accumulators per row and lane stay in registers
constexpr int kChunkDw = 32;                            // dwords of positions staged at a time (128 positions)
constexpr int kRowDw = kChunkDw + 1;                    // dwords between the staged rows of neighbouring lanes
constexpr uint32_t kHigh = 0x80808080u;

// four bytes through the table: a letter -> its index, every other byte -> 0xFF
__device__ __forceinline__ uint32_t translate4(const uint8_t* lidx, uint32_t v) {
  return (uint32_t)lidx[v & 255u] | ((uint32_t)lidx[(v >> 8) & 255u] << 8) | ((uint32_t)lidx[(v >> 16) & 255u] << 16) |
         ((uint32_t)lidx[v >> 24] << 24);
}
// per dword of two translated rows: bit 7 of every byte where both show a letter, and of those where the letters are equal
__device__ __forceinline__ uint32_t both_letters(uint32_t a, uint32_t b) { return ~(a | b) & kHigh; }
__device__ __forceinline__ uint32_t equal_letters(uint32_t a, uint32_t b, uint32_t both) {
  const uint32_t v = a ^ b;                             // where `both` is set, bit 7 of v's byte is clear: no carry crosses a byte
  return ~((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) & both;
}

// Tile x of a query: k tile kt (64 slots) has the j tiles 0 .. 2 kt + 1 (kTileJ = 32 slots each: every j < 64 kt + 64), so
// kt (kt + 1) tiles precede it.  near: word (r K + j) W + kt, bit k - 64 kt set when slot k is near slot j (j < k < K).
__global__ __launch_bounds__(64) void pair_near_kernel(const char* __restrict__ stack, int64_t stride, int K, int W,
                                                       const WeightQuery* __restrict__ qr, const int8_t* __restrict__ idx,
                                                       int max_identity, int min_overlap, unsigned long long* __restrict__ near,
                                                       int32_t* __restrict__ letters) {
  __shared__ uint32_t rowk[64 * kRowDw];
  __shared__ uint32_t rowj[kTileJ * kChunkDw];
  __shared__ uint8_t lidx[256];
  const int lane = threadIdx.x, r = blockIdx.y;
  int kt = 0;
  while ((kt + 1) * (kt + 2) <= (int)blockIdx.x) ++kt;
  const int jt = (int)blockIdx.x - kt * (kt + 1);
  const int k0 = kt * 64, j0 = jt * kTileJ;
  if (j0 >= K) return;                                  // block-uniform (the last k tile of a K that is no multiple of 64)
  for (int i = lane; i < 256; i += 64) lidx[i] = (uint8_t)idx[i];
  const int nd = (qr[r].len + 3) >> 2;                  // dwords of the query's rows (the stride is a multiple of 4)
  const uint32_t* base = reinterpret_cast<const uint32_t*>(stack + (size_t)r * K * stride);
  const size_t sd = (size_t)(stride >> 2);
  int ov[kTileJ], sm[kTileJ], let = 0;
#pragma unroll
  for (int j = 0; j < kTileJ; ++j) { ov[j] = 0; sm[j] = 0; }

  for (int c0 = 0; c0 < nd; c0 += kChunkDw) {
    __syncthreads();                                    // the table is written; the previous chunk has been read
    // two rows per step, 32 consecutive dwords of each: slots beyond K and dwords beyond the row are no letters
    for (int i = lane; i < 64 * kChunkDw; i += 64) {
      const int row = i / kChunkDw, d = i % kChunkDw;
      const bool in = k0 + row < K && c0 + d < nd;
      rowk[row * kRowDw + d] = in ? translate4(lidx, base[(size_t)(k0 + row) * sd + c0 + d]) : 0xFFFFFFFFu;
    }
    for (int i = lane; i < kTileJ * kChunkDw; i += 64) {
      const int row = i / kChunkDw, d = i % kChunkDw;
      const bool in = j0 + row < K && c0 + d < nd;
      rowj[i] = in ? translate4(lidx, base[(size_t)(j0 + row) * sd + c0 + d]) : 0xFFFFFFFFu;
    }
    __syncthreads();
    const int n = min(kChunkDw, nd - c0);
    for (int d = 0; d < n; ++d) {
      const uint32_t a = rowk[lane * kRowDw + d];
      let += __popc(~a & kHigh);
#pragma unroll
      for (int j = 0; j < kTileJ; ++j) {
        const uint32_t b = rowj[j * kChunkDw + d];      // the same address on every lane
        const uint32_t both = both_letters(a, b);
        ov[j] += __popc(both);
        sm[j] += __popc(equal_letters(a, b, both));
      }
    }
  }

  const int k = k0 + lane;
  unsigned long long mine = 0;
#pragma unroll
  for (int j = 0; j < kTileJ; ++j) {
    const bool is_near = j0 + j < k && k < K && ov[j] >= 1 && 100 * ov[j] >= min_overlap * let && 100 * sm[j] >= max_identity * ov[j];
    const unsigned long long word = __ballot(is_near);
    if (lane == j) mine = word;
  }
  if (lane < kTileJ && j0 + lane < K) near[((size_t)r * K + j0 + lane) * W + kt] = mine;
  if (jt == 0 && k < K) letters[(size_t)r * K + k] = let;
}

// keeper[r K + k]: k for a kept slot, the smallest kept slot it is near for a purged one, -1 for a slot without a letter.
// Every slot's entry is written once: by lane k / 64 at the step that keeps or purges it, or here at the start.
__global__ __launch_bounds__(64) void greedy_kernel(const unsigned long long* __restrict__ near, const int32_t* __restrict__ letters,
                                                    int K, int W, int32_t* __restrict__ keeper) {
  const int lane = threadIdx.x;
  const unsigned long long* row = near + (size_t)blockIdx.x * K * W;
  const int32_t* let = letters + (size_t)blockIdx.x * K;
  int32_t* keep = keeper + (size_t)blockIdx.x * K;
  unsigned long long has = 0, purged = 0;               // lane w: bits 64 w .. 64 w + 63 of the masks
  for (int w = 0; w < W; ++w) {
    const int k = 64 * w + lane;
    const bool shows = k < K && let[k] > 0;
    if (k < K && !shows) keep[k] = -1;
    const unsigned long long word = __ballot(shows);
    if (lane == w) has = word;
  }
  unsigned long long nxt = lane < W ? row[lane] : 0ull;   // row j is read a step ahead; words below j / 64 are never written
  for (int j = 0; j < K; ++j) {
    const unsigned long long cur = nxt;
    if (j + 1 < K) nxt = (lane >= ((j + 1) >> 6) && lane < W) ? row[(size_t)(j + 1) * W + lane] : 0ull;
    const int jw = j >> 6;
    const unsigned long long bit = 1ull << (j & 63);
    const bool kept = (__shfl(has, jw) & bit) != 0 && (__shfl(purged, jw) & bit) == 0;   // wave-uniform
    if (!kept) continue;
    if (lane == jw) keep[j] = j;
    unsigned long long now = cur & has & ~purged;       // (lanes below jw hold 0)
    purged |= now;
    while (now) {
      keep[64 * lane + __builtin_ctzll(now)] = j;
      now &= now - 1;
    }
  }
}

struct PurgeRecord { int32_t keeper, same, overlap, letters; };   // aln_hit_purge

// one wave per slot: the record; same and overlap of a purged slot against its keeper, lanes along the dwords of the rows
__global__ __launch_bounds__(64) void purge_record_kernel(const char* __restrict__ stack, int64_t stride, int K,
                                                          const WeightQuery* __restrict__ qr, const int8_t* __restrict__ idx,
                                                          const int32_t* __restrict__ keeper, const int32_t* __restrict__ letters,
                                                          PurgeRecord* __restrict__ out) {
  __shared__ uint8_t lidx[256];
  const int lane = threadIdx.x;
  const size_t slot = blockIdx.x;
  const int r = (int)(slot / K), k = (int)(slot % K), j = keeper[slot];
  if (j < 0 || j == k) {                                // block-uniform
    if (lane == 0) out[slot] = j < 0 ? PurgeRecord{-1, 0, 0, 0} : PurgeRecord{k, 0, 0, letters[slot]};
    return;
  }
  for (int i = lane; i < 256; i += 64) lidx[i] = (uint8_t)idx[i];
  __syncthreads();
  const int nd = (qr[r].len + 3) >> 2;
  const uint32_t* mine = reinterpret_cast<const uint32_t*>(stack + slot * stride);
  const uint32_t* its = reinterpret_cast<const uint32_t*>(stack + ((size_t)r * K + j) * stride);
  int ov = 0, sm = 0;
  for (int d = lane; d < nd; d += 64) {
    const uint32_t a = translate4(lidx, mine[d]), b = translate4(lidx, its[d]);
    const uint32_t both = both_letters(a, b);
    ov += __popc(both);
    sm += __popc(equal_letters(a, b, both));
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { ov += __shfl_xor(ov, off); sm += __shfl_xor(sm, off); }
  if (lane == 0) out[slot] = PurgeRecord{j, sm, ov, letters[slot]};
}

// one wave per slot: the row of a slot that is not kept shows '.' at every position
__global__ __launch_bounds__(64) void mute_rows_kernel(char* __restrict__ stack, int64_t stride, int K,
                                                       const int32_t* __restrict__ keeper) {
  const size_t slot = blockIdx.x;
  if (keeper[slot] == (int)(slot % K)) return;          // block-uniform
  uint32_t* row = reinterpret_cast<uint32_t*>(stack + slot * stride);
  for (int d = threadIdx.x; d < (int)(stride >> 2); d += 64) row[d] = 0x2E2E2E2Eu;
}

// The shared body of aln_hits_purge and aln_hits_purge_profiles (run: prepared; `queries`: the pool the query lengths are read
// from — hit_entry's pool, search_align.h).  after (search_stack.h; weights given): the weighted count rows stay on the device
// and after(st, sw, group) runs over every group once its weights have come down — aln_hits_pssm (search_pssm.hip).
int purge_block(ScoreRun& run, const aln_seqs* queries, int32_t K, const aln_hit* hits, const int32_t* n_hits,
                int32_t max_identity, int32_t min_overlap, int32_t w_max, aln_hit_alignment* out, aln_hit_purge* purge,
                int32_t* weights, int64_t* raw, int32_t* counts, int32_t* covered, const StackHook* after) {
  static_assert(sizeof(PurgeRecord) == sizeof(aln_hit_purge) && sizeof(aln_hit_purge) == 16, "aln_hit_purge is 16 bytes");
  aln_ctx* ctx = run.ctx;
  if (!purge || max_identity < 1 || max_identity > 101 || min_overlap < 0 || min_overlap > 100) return ALN_E_ARG;
  if (!weights && (raw || counts || covered)) return ALN_E_ARG;
  if (weights && (w_max < 1 || w_max > 65535)) return ALN_E_ARG;
  const int rows = run.rows;
  if (rows == 0) return ALN_OK;

  HitStack st(run, queries, K, out);
  int rc = st.route(hits, n_hits);                           // nothing written before
  if (rc != ALN_OK) return rc;
  StackWeights sw(st, w_max, weights, raw, counts, covered, after != nullptr);
  if (weights) sw.clear();
  st.ao.clear_unused(rows, K, n_hits);

  // a group keeps the stack and the pair bits below the budget each; rows start on a dword
  const size_t W = ((size_t)K + 63) / 64;
  RTRY(st.alloc(4, (size_t)K * W * 8));
  if (weights) RTRY(sw.alloc());
  unsigned long long* dnear = nullptr; int32_t *dlet = nullptr, *dkeep = nullptr; PurgeRecord* dpur = nullptr;
  STRY(st.own.get(dnear, st.group * K * W));
  STRY(st.own.get(dlet, st.group * K));
  STRY(st.own.get(dkeep, st.group * K));
  STRY(st.own.get(dpur, st.group * K));
  const unsigned KT = (unsigned)W, tiles = KT * (KT + 1);
  const int64_t dw = (int64_t)st.dw;

  rc = st.build("aln_hits_purge", [&](const StackGroup& g) -> int {
    const dim3 wave(64);
    const unsigned slots = (unsigned)(g.gn * K);
    hipLaunchKernelGGL(pair_near_kernel, dim3(tiles, (unsigned)g.gn), wave, 0, ctx->stream, st.dstack, dw, (int)K, (int)W, st.dqr, st.didx,
                       (int)max_identity, (int)min_overlap, dnear, dlet);
    STRY(hipGetLastError());
    hipLaunchKernelGGL(greedy_kernel, dim3((unsigned)g.gn), wave, 0, ctx->stream, dnear, dlet, (int)K, (int)W, dkeep);
    STRY(hipGetLastError());
    hipLaunchKernelGGL(purge_record_kernel, dim3(slots), wave, 0, ctx->stream, st.dstack, dw, (int)K, st.dqr, st.didx, dkeep, dlet, dpur);
    STRY(hipGetLastError());
    hipLaunchKernelGGL(mute_rows_kernel, dim3(slots), wave, 0, ctx->stream, st.dstack, dw, (int)K, dkeep);
    STRY(hipGetLastError());
    STRY(hipMemcpyAsync(purge + g.slot0, dpur, (size_t)slots * sizeof(PurgeRecord), hipMemcpyDeviceToHost, ctx->stream));
    if (weights) {
      RTRY(sw.group(g));
      return after ? (*after)(st, sw, g) : ALN_OK;
    }
    STRY(hipStreamSynchronize(ctx->stream));
    return ALN_OK;
  });
  RTRY(rc);
  return st.ao.worst;
}

}  // namespace aln

using namespace aln;

extern "C" int aln_hits_purge(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                              const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K, const aln_hit* hits,
                              const int32_t* n_hits, int32_t max_identity, int32_t min_overlap, int32_t w_max,
                              aln_hit_alignment* out, aln_hit_purge* purge, int32_t* weights, int64_t* raw, int32_t* counts,
                              int32_t* covered) {
  return hit_entry(ctx, false, queries, nullptr, nullptr, templates, sub, gap, q_begin, q_end, hit_list_ok(K, hits, n_hits, out),
                   [&](ScoreRun& run, const aln_seqs* pool) {
                     return purge_block(run, pool, K, hits, n_hits, max_identity, min_overlap, w_max, out, purge, weights, raw, counts,
                                        covered);
                   });
}

extern "C" int aln_hits_purge_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus,
                                       const aln_seqs* templates, const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                                       const aln_hit* hits, const int32_t* n_hits, int32_t max_identity, int32_t min_overlap,
                                       int32_t w_max, aln_hit_alignment* out, aln_hit_purge* purge, int32_t* weights, int64_t* raw,
                                       int32_t* counts, int32_t* covered) {
  return hit_entry(ctx, true, nullptr, profiles, consensus, templates, nullptr, gap, q_begin, q_end, hit_list_ok(K, hits, n_hits, out),
                   [&](ScoreRun& run, const aln_seqs* pool) {
                     return purge_block(run, pool, K, hits, n_hits, max_identity, min_overlap, w_max, out, purge, weights, raw, counts,
                                        covered);
                   });
}

#undef STRY
#undef RTRY
