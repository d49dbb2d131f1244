// search_zscore.hip — shuffle z-scores of search hits: the background sample of every hit scored and reduced on the device (gfx950).
//
// A raw local score is length- and composition-biased; the classic remedy places it against the scores of the SAME template
// with permutations of the query.  That is n_shuffles x (number of hits) score-only alignments — the work score_only.hip's
// register-resident row sweep was built for — and nothing but two 64-bit sums per hit has to leave the device:
//   shuffle_queries_kernel         one thread per (query row, shuffle): the permuted residue codes, sentinels in place
//   class_list_kernel              (score_common.h) the used hit slots listed by template length class R = ceil(T / 256), over
//                                  a plain array of template indices: any align type, any hit list
//   score_shuffled_kernel<R,LOCAL> one wave per (listed slot, group of shuffles): the template-side state of
//                                  score_local_kernel<R> / score_global_kernel<R> is built ONCE, then the row sweep
//                                  (score_sweep.h) runs once per shuffle of the group; score and score^2 are summed in 64 bits
//                                  and leave the wave as two atomic adds (integer addition: the result does not depend on the order)
// Query rows are handled a chunk at a time so that the shuffled strings and the accumulators stay below 1 GiB each.  Hits on
// templates beyond 2048 columns go the way they go in aln_score_all_vs_all: the host materialises the same permutations (its
// own statement of the rule) and score_through_batches scores them through full builds.
#include <cstdio>
#include <string>
#include <vector>

#include "search_zscore.h"

namespace aln {

struct ShuffleArgs {
  const uint8_t* qcodes; const int64_t* qoff;   // query pool
  const int64_t* poff;                          // nr + 1: row r's shuffles start at pool[poff[r]], |q| bytes each (no used slot: none)
  uint8_t* pool;
  int q_first, nr, S;                           // q_first: query index of the chunk's row 0
  uint32_t seed;
};

// Fisher-Yates is serial per string; the strings are independent.  The string lives in global memory: a swap is two byte
// loads and two byte stores that stay in L2, and the whole pass is a small fraction of the scoring that follows.
__global__ __launch_bounds__(256) void shuffle_queries_kernel(ShuffleArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)a.nr * a.S) return;
  const int row = (int)(e / a.S), s = (int)(e % a.S);
  const int64_t p0 = a.poff[row];
  if (a.poff[row + 1] == p0) return;
  const int q = a.q_first + row;
  const int Q = (int)(a.qoff[q + 1] - a.qoff[q]);
  const uint8_t* __restrict__ src = a.qcodes + a.qoff[q];
  uint8_t* dst = a.pool + p0 + (int64_t)s * Q;
  for (int i = 0; i < Q; ++i) dst[i] = src[i];
  const uint32_t key = fmix32(fmix32(fmix32(a.seed ^ 0x9E3779B9u) + (uint32_t)q) + (uint32_t)s);
  uint8_t* v = dst + 1;
  for (int i = Q - 3; i >= 1; --i) {
    const uint32_t r = fmix32(key + (uint32_t)i * 0x9E3779B9u);
    const int j = (int)(((uint64_t)r * (uint32_t)(i + 1)) >> 32);
    const uint8_t x = v[i]; v[i] = v[j]; v[j] = x;
  }
}

struct ZScoreArgs {
  ScoreArgs a;                                  // a.q_begin: query index of the chunk's row 0; a.qcodes is not read
  const int32_t* list;                          // blockIdx.x -> slot of the chunk
  const int32_t* slot_t;                        // slot -> template index
  const int64_t* poff; const uint8_t* pool;     // the shuffled strings (ShuffleArgs)
  unsigned long long* acc;                      // slot -> { sum, sum of squares }
  int K, S, G;                                  // G: shuffles per wave; blockIdx.y = group
  int free_del, free_ins;
};

// The template-side state of score_local_kernel<R> / score_global_kernel<R> (score_sweep.h) is built once, the sweep runs once
// per shuffle of the group.
template <int R, bool LOCAL>
__global__ __launch_bounds__(64) void score_shuffled_kernel(ZScoreArgs z) {
  __shared__ int tab[32 * 32];
  const int lane = threadIdx.x;
  for (int k = lane; k < 32 * 32; k += 64) tab[k] = z.a.table32[k];
  __syncthreads();
  const int slot = z.list[blockIdx.x];
  const int row = slot / z.K, ti = z.slot_t[slot], qi = z.a.q_begin + row;
  const int s0 = blockIdx.y * z.G, n_s = min(z.G, z.S - s0);
  const int Q = (int)(z.a.qoff[qi + 1] - z.a.qoff[qi]), T = (int)(z.a.toff[ti + 1] - z.a.toff[ti]);
  const uint8_t* __restrict__ q0 = z.pool + z.poff[row] + (int64_t)s0 * Q;
  const uint8_t* __restrict__ tc = z.a.tcodes + z.a.toff[ti];
  long long sum = 0, sumsq = 0;
  auto add = [&](int m) {                                      // one shuffle's score, reduced over the wave
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o));
    sum += m; sumsq += (long long)m * m;
  };
  if constexpr (LOCAL) {
    LocalCols<R> cols;
    cols.load(tc, T, z.a.gi, z.a.ge);
    for (int s = 0; s < n_s; ++s) {
      int d[R][4];
      add(sweep_local<R>(tab, cols, q0 + (size_t)s * Q, Q - 2, d, NoObserver()));
    }
  } else if (Q == 2 || T == 2) {
    // degenerate shortcuts of score_global_kernel: one gap from the origin, the same for every shuffle
    int cost = 0;
    if (Q == 2) { const int len = T - 2; cost = (len < 1 || z.free_del) ? 0 : z.a.gi + z.a.ge * (len - 1); }
    else { const int len = Q - 2; cost = (len < 1 || z.free_ins) ? 0 : z.a.gi + z.a.ge * (len - 1); }
    sum = -(long long)cost * n_s; sumsq = (long long)cost * cost * n_s;
  } else {
    GlobalCols<R> cols;
    cols.load(tc, T, z.a.gi, z.a.ge);
    for (int s = 0; s < n_s; ++s) add(sweep_global<R>(tab, cols, q0 + (size_t)s * Q, Q, z.free_del, z.free_ins, NoObserver()));
  }
  if (lane == 0) {
    atomicAdd(&z.acc[2 * (size_t)slot], (unsigned long long)sum);
    atomicAdd(&z.acc[2 * (size_t)slot + 1], (unsigned long long)sumsq);
  }
}

}  // namespace aln

using namespace aln;

extern "C" int aln_hits_zscores(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                                const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K, const aln_hit* hits,
                                const int32_t* n_hits, int32_t n_shuffles, uint32_t seed, aln_hit_stats* stats) {
  if (!hits || !n_hits || !stats || K < 1 || K > 1024 || n_shuffles < 1 || n_shuffles > 4096) return ALN_E_ARG;
  ScoreRun run;
  int rc = run.prepare(ctx, queries, templates, sub, gap, q_begin, q_end);
  if (rc != ALN_OK) return rc;
  const int rows = run.rows, n_t = run.n_t, S = n_shuffles;
  if (rows == 0) return ALN_OK;
  for (int r = 0; r < rows; ++r) {
    if (n_hits[r] < 0 || n_hits[r] > K) return ALN_E_ARG;
    for (int k = 0; k < n_hits[r]; ++k) {
      const int32_t t = hits[(size_t)r * K + k].t;
      if (t < 0 || t >= n_t) return ALN_E_ARG;
    }
  }
  if (run.route == ScoreRun::kAllFull) return ALN_E_NOT_INTEGRAL;
  auto write_chunk = [&](int r0, int nr, const long long* acc) {   // acc: the chunk's { sum, sumsq } per slot
    for (int r = 0; r < nr; ++r)
      for (int k = 0; k < K; ++k) {
        const size_t g = (size_t)(r0 + r) * K + k, c = (size_t)r * K + k;
        aln_hit_stats o = {0, 0, 0, 0.0f};
        if (k < n_hits[r0 + r]) {
          o.sum = acc[2 * c]; o.sumsq = acc[2 * c + 1]; o.n = S;
          o.z = z_of(S, hits[g].score, o.sum, o.sumsq);
        }
        stats[g] = o;
      }
  };
  if (run.route == ScoreRun::kNothing) {           // no template, hence no used slot
    write_chunk(0, rows, nullptr);
    return ALN_OK;
  }

  // chunks of query rows: shuffled strings (S x |q| bytes per row with a used slot) and accumulators (16 B x K per row)
  struct Chunk { int r0, nr; size_t pool; };
  std::vector<Chunk> chunks;
  {
    const int cap = (int)std::min<size_t>((size_t)0x7FFFFFFF / (size_t)K, kZBudget / ((size_t)K * 16));
    const int forced = ctx->hints.zscore_chunk_rows;
    const int max_rows = forced > 0 ? std::min(forced, cap) : cap;   // a forced size is an upper bound: the budgets still hold
    Chunk c = {0, 0, 0};
    for (int r = 0; r < rows; ++r) {
      const size_t need = n_hits[r] > 0 ? (size_t)S * (size_t)(queries->offsets[q_begin + r + 1] - queries->offsets[q_begin + r]) : 0;
      if (c.nr > 0 && (c.nr >= max_rows || c.pool + need > kZBudget)) { chunks.push_back(c); c = {r, 0, 0}; }
      c.nr++; c.pool += need;
    }
    chunks.push_back(c);
  }
  size_t max_pool = 1; int max_nr = 1;
  for (const Chunk& c : chunks) { max_pool = std::max(max_pool, c.pool); max_nr = std::max(max_nr, c.nr); }

  uint8_t* dpool = nullptr; int64_t* dpoff = nullptr; int32_t *dslot = nullptr, *dlist = nullptr, *dfill = nullptr;
  unsigned long long* dacc = nullptr;
  auto cleanup = [&]() {
    hipFree(dpool); hipFree(dpoff); hipFree(dslot); hipFree(dlist); hipFree(dfill); hipFree(dacc);
    run.release();
  };
#define STRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { ctx->last_error = std::string(#expr) + ": " + hipGetErrorString(e_); hipStreamSynchronize(ctx->stream); cleanup(); return ALN_E_HIP; } } while (0)
#define RTRY(expr) do { int r_ = (expr); if (r_ != ALN_OK) { hipStreamSynchronize(ctx->stream); cleanup(); return r_; } } while (0)
  RTRY(run.upload());
  const size_t max_slots = (size_t)max_nr * K;
  STRY(hipMalloc((void**)&dpool, max_pool));
  STRY(hipMalloc((void**)&dpoff, (size_t)(max_nr + 1) * 8));
  STRY(hipMalloc((void**)&dslot, max_slots * 4));
  STRY(hipMalloc((void**)&dlist, max_slots * 4));
  STRY(hipMalloc((void**)&dfill, 9 * 4));
  STRY(hipMalloc((void**)&dacc, max_slots * 16));
  std::vector<int64_t> poff((size_t)max_nr + 1);
  std::vector<int32_t> slot_t(max_slots);
  std::vector<long long> acc(max_slots * 2);
  std::vector<int32_t> fcol((size_t)n_t, 0), long_list;
  std::vector<float> long_sc;
  std::string shuf; std::vector<int64_t> shuf_off((size_t)S + 1);
  const int n_groups = (S + kShufGroup - 1) / kShufGroup, G = (S + n_groups - 1) / n_groups;   // groups of equal size

  for (const Chunk& c : chunks) {
    const int r0 = c.r0, nr = c.nr, n_slots = nr * K;
    int cls_cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    poff[0] = 0;
    for (int r = 0; r < nr; ++r) {
      const int64_t Q = queries->offsets[q_begin + r0 + r + 1] - queries->offsets[q_begin + r0 + r];
      poff[(size_t)r + 1] = poff[r] + (n_hits[r0 + r] > 0 ? (int64_t)S * Q : 0);
      for (int k = 0; k < K; ++k) {
        int32_t t = -1;
        if (k < n_hits[r0 + r]) {
          t = hits[(size_t)(r0 + r) * K + k].t;
          const int64_t T = templates->offsets[t + 1] - templates->offsets[t];
          cls_cnt[T > 2048 ? 0 : (int)((T + 255) / 256)]++;
        }
        slot_t[(size_t)r * K + k] = t;
      }
    }
    int n_used = 0;
    ClassOff co = {};
    for (int k = 0; k < 9; ++k) { if (k) co.off[k] = co.off[k - 1] + cls_cnt[k - 1]; n_used += cls_cnt[k]; }
    if (n_used > cls_cnt[0]) {
      STRY(hipMemcpyAsync(dpoff, poff.data(), (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
      STRY(hipMemcpyAsync(dslot, slot_t.data(), (size_t)n_slots * 4, hipMemcpyHostToDevice, ctx->stream));
      STRY(hipMemsetAsync(dfill, 0, 9 * 4, ctx->stream));
      STRY(hipMemsetAsync(dacc, 0, (size_t)n_slots * 16, ctx->stream));
      ShuffleArgs sh = {};
      sh.qcodes = run.dq; sh.qoff = run.dqo; sh.poff = dpoff; sh.pool = dpool; sh.q_first = q_begin + r0; sh.nr = nr; sh.S = S; sh.seed = seed;
      const long long n_str = (long long)nr * S;
      hipLaunchKernelGGL(shuffle_queries_kernel, dim3((unsigned)((n_str + 255) / 256)), dim3(256), 0, ctx->stream, sh);
      STRY(hipGetLastError());
      const SlotClass sc = {dslot, run.dto};
      hipLaunchKernelGGL(class_list_kernel<SlotClass>, dim3((n_slots + 255) / 256), dim3(256), 0, ctx->stream, sc, n_slots, co, dfill, dlist);
      STRY(hipGetLastError());
      ZScoreArgs z = {};
      z.a = run.a; z.a.q_begin = q_begin + r0;
      z.slot_t = dslot; z.poff = dpoff; z.pool = dpool; z.acc = dacc; z.K = K; z.S = S; z.G = G;
      z.free_del = run.free_del; z.free_ins = run.free_ins;
      for (int k = 1; k <= 8; ++k) {
        if (cls_cnt[k] == 0) continue;
        z.list = dlist + co.off[k];
        const dim3 grid(cls_cnt[k], n_groups);
        dispatch_r<8>(k, [&](auto rc) {
          constexpr int R = decltype(rc)::value;
          if (run.local) hipLaunchKernelGGL((score_shuffled_kernel<R, true>), grid, dim3(64), 0, ctx->stream, z);
          else hipLaunchKernelGGL((score_shuffled_kernel<R, false>), grid, dim3(64), 0, ctx->stream, z);
        });
        STRY(hipGetLastError());
      }
      STRY(hipMemcpyAsync(acc.data(), dacc, (size_t)n_slots * 16, hipMemcpyDeviceToHost, ctx->stream));
      STRY(hipStreamSynchronize(ctx->stream));
    } else std::fill(acc.begin(), acc.begin() + (size_t)n_slots * 2, 0LL);
    // hits on templates beyond 2048 columns: the same strings made here, scored through full builds row by row
    if (cls_cnt[0] > 0)
      for (int r = 0; r < nr; ++r) {
        long_list.clear();
        for (int k = 0; k < n_hits[r0 + r]; ++k) {
          const int32_t t = slot_t[(size_t)r * K + k];
          if (templates->offsets[t + 1] - templates->offsets[t] <= 2048) continue;
          if (std::find(long_list.begin(), long_list.end(), t) == long_list.end()) { fcol[t] = (int32_t)long_list.size(); long_list.push_back(t); }
        }
        if (long_list.empty()) continue;
        const int q = q_begin + r0 + r;
        const int64_t Q = queries->offsets[q + 1] - queries->offsets[q];
        shuf.resize((size_t)S * Q);
        for (int s = 0; s < S; ++s) {
          shuf_off[s] = (int64_t)s * Q;
          std::copy(queries->residues + queries->offsets[q], queries->residues + queries->offsets[q + 1], shuf.begin() + (size_t)s * Q);
          host_shuffle(seed, (uint32_t)q, (uint32_t)s, &shuf[(size_t)s * Q], Q);
        }
        shuf_off[S] = (int64_t)S * Q;
        aln_seqs sq = {S, shuf_off.data(), shuf.data()};
        const size_t ld = long_list.size();
        long_sc.assign((size_t)S * ld, 0.f);
        RTRY(score_through_batches(ctx, &sq, templates, sub, gap, 0, S, long_list, long_sc.data(), fcol.data(), ld));
        for (int k = 0; k < n_hits[r0 + r]; ++k) {
          const int32_t t = slot_t[(size_t)r * K + k];
          if (templates->offsets[t + 1] - templates->offsets[t] <= 2048) continue;
          long long sum = 0, sumsq = 0;
          for (int s = 0; s < S; ++s) { const long long v = (long long)long_sc[(size_t)s * ld + fcol[t]]; sum += v; sumsq += v * v; }
          acc[2 * ((size_t)r * K + k)] = sum; acc[2 * ((size_t)r * K + k) + 1] = sumsq;
        }
      }
    write_chunk(r0, nr, acc.data());
  }
#undef STRY
#undef RTRY
  cleanup();
  return ALN_OK;
}
