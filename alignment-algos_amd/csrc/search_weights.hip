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
// batch route (for_list_groups) and the four kernels over its own queries.
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "search_pileup.h"

namespace aln {

constexpr size_t kStackBudget = (size_t)1 << 30;        // bytes of letters rows resident at a time
constexpr int kSpareCol = 31;                           // the alphabet has at most 30 letters: k_p, or covered
constexpr int kHistStride = 33;                         // words between the histograms of neighbouring lanes

struct WeightQuery {        // one query row of the group
  int64_t row;              // the count row of its position 0 (query row 1), relative to the group's first count row
  int32_t len;              // Q - 2
  int32_t pad;
};

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

// The shared body of aln_hits_weights and aln_hits_weights_profiles (run: prepared; `queries`: the pool the query lengths are
// read from — hit_entry's pool, search_align.h).
static int weights_block(ScoreRun& run, const aln_seqs* queries, int32_t K, const aln_hit* hits, const int32_t* n_hits, int32_t w_max,
                         aln_hit_alignment* out, int32_t* weights, int64_t* raw, int32_t* counts, int32_t* covered) {
  aln_ctx* ctx = run.ctx;
  const aln_seqs* templates = run.templates;
  if (!weights || w_max < 1 || w_max > 65535) return ALN_E_ARG;
  const int rows = run.rows;
  if (rows == 0) return ALN_OK;
  const int n_alpha = run.prof ? run.prof->n : run.sub->n;
  const char* alphabet = run.prof ? run.prof->alphabet : run.sub->alphabet;
  const int64_t row0 = queries->offsets[run.q_begin];
  const size_t n_rows = (size_t)(queries->offsets[run.q_end] - row0);
  int64_t maxw = 1;                                          // the stack's stride: the longest Q - 2 of the block
  for (int q = run.q_begin; q < run.q_end; ++q) maxw = std::max<int64_t>(maxw, queries->offsets[q + 1] - queries->offsets[q] - 2);

  // route_slots' walk (every used slot validated and described for its route), then the alphabet; nothing written before
  SlotRoutes sr;
  int rc = route_slots(run, queries, K, hits, n_hits, hit_kernel_classes(run), run.local, sr);
  if (rc != ALN_OK) return rc;
  int8_t idx[256];
  memset(idx, -1, sizeof idx);
  for (int i = 0; i < n_alpha; ++i) {
    if (alphabet[i] == '.' || alphabet[i] == '-') return ALN_E_ARG;      // the pileup could not show them as letters
    idx[(unsigned char)alphabet[i]] = (int8_t)i;
  }
  ctx->align_routes[0] = (int64_t)sr.fast.size(); ctx->align_routes[1] = (int64_t)sr.bq.size();

  const size_t n_slots = (size_t)rows * K;
  const bool want_counts = counts || covered;
  memset(weights, 0, n_slots * 4);
  if (raw) memset(raw, 0, n_slots * 8);
  if (counts) memset(counts, 0, n_rows * (size_t)n_alpha * 4);
  if (covered) memset(covered, 0, n_rows * 4);
  AlignOut ao = {out, nullptr, 0, nullptr, nullptr, 0, nullptr};
  ao.clear_unused(rows, K, n_hits);

  // groups of consecutive queries: as many rows as keep the stack below the budget; the hint only asks for fewer
  const size_t dw = (size_t)maxw;
  size_t group = std::max<size_t>(kStackBudget / ((size_t)K * dw), 1);
  if (ctx->hints.weights_group_rows > 0) group = std::min(group, (size_t)ctx->hints.weights_group_rows);
  group = std::min(std::min(group, (size_t)rows), (size_t)32768);   // (a group's rows are a launch's blockIdx.y)
  size_t max_grows = 1;                                      // the most count rows of a group
  for (size_t g0 = 0; g0 < (size_t)rows; g0 += group) {
    const size_t g1 = std::min(g0 + group, (size_t)rows);
    max_grows = std::max(max_grows, (size_t)(queries->offsets[run.q_begin + g1] - queries->offsets[run.q_begin + g0]));
  }

  DeviceBufs own(run);
  char* dstack = nullptr; int8_t* didx = nullptr; WeightQuery* dqr = nullptr;
  int32_t *dnp = nullptr, *dcnt = nullptr, *dwt = nullptr; int64_t* draw = nullptr;
  STRY(own.get(dstack, group * K * dw));
  STRY(own.get(didx, 256));
  STRY(own.get(dqr, group));
  STRY(own.get(dnp, max_grows * 32));
  if (want_counts) STRY(own.get(dcnt, max_grows * 32));
  STRY(own.get(dwt, group * K));
  STRY(own.get(draw, group * K));
  STRY(hipMemcpyAsync(didx, idx, sizeof idx, hipMemcpyHostToDevice, ctx->stream));        // (alive until the first synchronisation)
  std::vector<WeightQuery> hqr(group);
  std::vector<int32_t> hcnt(want_counts ? max_grows * 32 : 0);
  std::vector<char> hrow(dw);

  size_t f0 = 0, b0 = 0;                                     // the group's first fused hit and first batch slot (both row-major)
  for (size_t g0 = 0; g0 < (size_t)rows; g0 += group) {
    const size_t g1 = std::min(g0 + group, (size_t)rows), gn = g1 - g0;
    const size_t slot0 = g0 * K, slot1 = g1 * K;
    const int64_t grow0 = queries->offsets[run.q_begin + g0];
    const size_t g_rows = (size_t)(queries->offsets[run.q_begin + g1] - grow0);
    size_t f1 = f0, b1 = b0;
    while (f1 < sr.fast.size() && sr.fast_slot[f1] < slot1) ++f1;
    while (b1 < sr.bq.size() && sr.bslot[b1] < slot1) ++b1;
    for (size_t r = 0; r < gn; ++r) {
      const int64_t o = queries->offsets[run.q_begin + g0 + r];
      hqr[r] = WeightQuery{o - grow0 + 1, (int32_t)(queries->offsets[run.q_begin + g0 + r + 1] - o - 2), 0};
    }
    STRY(hipMemcpyAsync(dqr, hqr.data(), gn * sizeof(WeightQuery), hipMemcpyHostToDevice, ctx->stream));
    STRY(hipMemsetAsync(dstack, '.', gn * K * dw, ctx->stream));

    // the group's fused hits, chunk by chunk: the rows of a chunk, then their move into the stack
    if (f1 > f0) {
      std::vector<HitDesc> fast(sr.fast.begin() + f0, sr.fast.begin() + f1);
      const std::vector<size_t> fast_slot(sr.fast_slot.begin() + f0, sr.fast_slot.begin() + f1);
      FusedRoute<HitDesc> fr(run, queries, fast);
      std::vector<int32_t> fast_live(fast.size()), fast_at(fast.size());
      for (size_t h = 0; h < fast.size(); ++h) {
        fast_live[h] = (run.local && !(fast[h].score > 0.f)) ? 0 : 1;
        fast_at[h] = (int32_t)(fast_slot[h] - slot0);
      }
      fr.cut(1, true, (int)std::min<int64_t>(maxw, INT_MAX),
             [&](const HitDesc& d) { return HitNeed{hit_strip_bytes(run, queries, d), 0, 0}; });
      const size_t max_n = fr.max_n;
      int32_t *dlive = nullptr, *dat = nullptr; char* dlet = nullptr; PileupRows* drows = nullptr;
      HitRecords rec;
      RTRY(fr.begin());
      STRY(fr.bufs.get(dlive, max_n));
      STRY(fr.bufs.get(dat, max_n));
      RTRY(rec.alloc(fr.bufs, max_n));
      STRY(fr.bufs.get(dlet, max_n * dw));
      STRY(fr.bufs.get(drows, 1));
      RTRY(fr.upload_pools());                                 // the templates' characters, on both sides
      const PileupRows where = {dlive, fr.dtch, dlet, nullptr, nullptr, (int64_t)dw};   // (alive until the first chunk's synchronisation)
      STRY(hipMemcpyAsync(drows, &where, sizeof(where), hipMemcpyHostToDevice, ctx->stream));
      for (const FusedChunk& c : fr.chunks) {
        const size_t n = c.n;
        RTRY(fr.stage(c, [&]() -> int {
          STRY(hipMemcpyAsync(dlive, fast_live.data() + c.h0, n * 4, hipMemcpyHostToDevice, ctx->stream));
          STRY(hipMemcpyAsync(dat, fast_at.data() + c.h0, n * 4, hipMemcpyHostToDevice, ctx->stream));
          STRY(hipMemsetAsync(dlet, '.', n * dw, ctx->stream));
          return ALN_OK;
        }));
        PileupArgs g = {};
        g.desc = fr.ddesc; g.strip = fr.dstrip; g.rows = drows; g.res = rec.dres; g.same = rec.dsame;
        RTRY(launch_pileup_job(fr, c, g));
        hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)n), dim3(64), 0, ctx->stream, dlet, dstack, dat, (int64_t)dw);
        STRY(hipGetLastError());
        RTRY(rec.enqueue_download(ctx, n));
        STRY(hipStreamSynchronize(ctx->stream));               // the records' host images are read by the copies until here
        rec.put(ao, fr, c, fast_slot, [](size_t, size_t, int64_t) {});
      }
    }

    // the group's batch slots (for_list_groups, search_align.h): every surviving slot's row laid out here and uploaded
    if (b1 > b0) {
      SlotRoutes gs;
      gs.bq.assign(sr.bq.begin() + b0, sr.bq.begin() + b1);
      gs.bt.assign(sr.bt.begin() + b0, sr.bt.begin() + b1);
      gs.bslot.assign(sr.bslot.begin() + b0, sr.bslot.begin() + b1);
      int up = ALN_OK;
      rc = for_list_groups(run, queries, gs, ao, [&](size_t slot, int32_t q, int32_t t, const int32_t* l, int n_pairs) {
        const int64_t Q = queries->offsets[q + 1] - queries->offsets[q];
        const int64_t to = templates->offsets[t], T = templates->offsets[t + 1] - to;
        if (Q < 3 || up != ALN_OK) return;
        memset(hrow.data(), '.', (size_t)(Q - 2));
        pileup_from_list(l, n_pairs, Q, T, templates->residues + to, hrow.data(), nullptr, nullptr);
        if (hipMemcpyAsync(dstack + (slot - slot0) * dw, hrow.data(), (size_t)(Q - 2), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) {   // hrow is written again for the next slot
          ctx->last_error = "aln_hits_weights: upload of a batch slot's row failed";
          up = ALN_E_HIP;
        }
      });
      RTRY(rc);
      RTRY(up);
    }

    // the stack is complete: the tally, the slots' sums, the weights, the weighted tally
    const dim3 tiles((unsigned)((dw + 63) / 64), (unsigned)gn), wave(64);
    hipLaunchKernelGGL(column_tally_kernel<false>, tiles, wave, 0, ctx->stream, dstack, (int64_t)dw, (int)K, dqr, didx, dwt, dnp);
    STRY(hipGetLastError());
    hipLaunchKernelGGL(slot_raw_kernel, dim3((unsigned)(gn * K)), wave, 0, ctx->stream, dstack, (int64_t)dw, (int)K, dqr, didx, dnp, draw);
    STRY(hipGetLastError());
    hipLaunchKernelGGL(normalise_kernel, dim3((unsigned)gn), wave, 0, ctx->stream, draw, (int)K, (int)w_max, dwt);
    STRY(hipGetLastError());
    if (want_counts) {
      STRY(hipMemsetAsync(dcnt, 0, g_rows * 128, ctx->stream));                           // the sentinel rows stay zero
      hipLaunchKernelGGL(column_tally_kernel<true>, tiles, wave, 0, ctx->stream, dstack, (int64_t)dw, (int)K, dqr, didx, dwt, dcnt);
      STRY(hipGetLastError());
      STRY(hipMemcpyAsync(hcnt.data(), dcnt, g_rows * 128, hipMemcpyDeviceToHost, ctx->stream));
    }
    STRY(hipMemcpyAsync(weights + slot0, dwt, gn * K * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (raw) STRY(hipMemcpyAsync(raw + slot0, draw, gn * K * 8, hipMemcpyDeviceToHost, ctx->stream));
    STRY(hipStreamSynchronize(ctx->stream));
    if (want_counts) {
      const size_t base = (size_t)(grow0 - row0);
      for (size_t r = 0; r < g_rows; ++r) {
        if (counts) memcpy(counts + (base + r) * (size_t)n_alpha, hcnt.data() + r * 32, (size_t)n_alpha * 4);
        if (covered) covered[base + r] = hcnt[r * 32 + kSpareCol];
      }
    }
    f0 = f1; b0 = b1;
  }
  return ao.worst;
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
