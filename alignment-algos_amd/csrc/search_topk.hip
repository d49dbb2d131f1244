// search_topk.hip — all-vs-all SEARCH: for every query row the K best templates with the end cell of each hit (gfx950).
//
// aln_score_all_vs_all can only hand its caller a dense rows x n_t matrix; a search wants, per query, the few best templates
// and where their alignments end.  Here the score kernels of score_only.hip leave a slab of query rows' scores in a device
// buffer (ScoreRun, score_common.h), and three kernels turn the slab into hits without the matrix ever reaching the host:
//   topk_select_kernel         one workgroup per query row: the K largest 64-bit keys (score mapped to uint32, ~template index)
//   class_list_kernel          (score_common.h) the hits of local searches, listed by template length class R = ceil(T / 256)
//   score_local_end_kernel<R>  one wave per hit: the row sweep of score_local_kernel<R> (score_sweep.h), observed for the
//                              cell Optimal::find_max returns
// Only K x 16 B per query row travel to the host.  Pairs the register-resident kernels do not take (templates beyond 2048
// columns, fractional values, the value-range test) are scored through full builds as in aln_score_all_vs_all, uploaded into
// the slab before the selection, and the end cells of such hits come from one resident batch over just those hits.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>

#include "score_common.h"

namespace aln {

constexpr int kSelThreads = 256;
constexpr int kSelKeep = 1024;                 // keys a row keeps between merges (the largest K the ABI takes)
constexpr size_t kSlabBudget = (size_t)1 << 30;   // bytes of slab scores, and of slab hits, resident at a time

// float score -> uint32 with the same order (-0.0 counts as +0.0), high word; ~t low word: one unsigned 64-bit "greater"
// is "score greater, or equal and template index smaller".  Every real key is > 0 (the high word of -inf is 0x007FFFFF).
__device__ __forceinline__ unsigned long long hit_key(float s, int t) {
  unsigned u = __float_as_uint(s == 0.f ? 0.f : s);
  u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
  return ((unsigned long long)u << 32) | (unsigned)~t;
}

struct SelectArgs {
  const float* slab;                           // nr x n_t scores
  const int64_t* qoff; const int64_t* toff;
  aln_hit* hits;                               // nr x K
  int32_t* n_hits;                             // nr
  int32_t* cls_cnt;                            // [9]: hits per template length class (0 = full-build route), local searches only
  int n_t, K, q_first;                         // q_first: query index of the slab's row 0
  float min_score;
  int local, all_full;
};

__device__ __forceinline__ int hit_class(int T, int all_full) { return (all_full || T > 2048) ? 0 : (T + 255) / 256; }

// One workgroup per query row.  LDS holds 2048 keys: [0, 1024) the best so far in descending order, [1024, 2048) candidates
// that beat the current K-th key, appended tile by tile (256 templates); when the next tile might not fit the 2048 keys are
// merged (bitonic sort of the candidates, bitonic merge with the kept half) and the K-th key becomes the new bar.  After the
// first merge few candidates of an unordered row pass the bar: such a row of n_t scores costs about n_t / 256 tiles of two
// barriers each and a handful of merges; a row whose scores rise with the template index merges about every third tile.
__global__ __launch_bounds__(kSelThreads) void topk_select_kernel(SelectArgs a) {
  __shared__ unsigned long long buf[2 * kSelKeep];
  __shared__ int cnt;
  __shared__ int ccnt[9];
  const int tid = threadIdx.x, lane = tid & 63;
  const int row = blockIdx.x;
  const float* __restrict__ sr = a.slab + (size_t)row * a.n_t;
  for (int i = tid; i < 2 * kSelKeep; i += kSelThreads) buf[i] = 0;
  if (tid == 0) cnt = 0;
  if (tid < 9) ccnt[tid] = 0;
  __syncthreads();
  unsigned long long bar = 0;
  auto merge = [&]() {                          // called by all threads; buf is quiescent on entry (a barrier precedes)
    // [0, 1024) is already descending: sort only the candidate half, ascending (55 stages over 512 pairs), which makes the
    // 2048 keys bitonic, then one descending merge (11 stages over 1024 pairs)
    for (int k = 2; k <= 2 * kSelKeep; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int p = (k <= kSelKeep ? kSelKeep / 2 : 0) + tid; p < kSelKeep; p += kSelThreads) {
          const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), o = i | j;
          const unsigned long long x = buf[i], y = buf[o];
          const bool asc = (i & k) != 0;
          if (asc ? x > y : x < y) { buf[i] = y; buf[o] = x; }
        }
        __syncthreads();
      }
    bar = buf[a.K - 1];
    __syncthreads();
    for (int i = kSelKeep + tid; i < 2 * kSelKeep; i += kSelThreads) buf[i] = 0;
    if (tid == 0) cnt = 0;
    __syncthreads();
  };
  for (int base = 0; base < a.n_t; base += kSelThreads) {
    const int c = cnt;
    __syncthreads();                            // everybody has read cnt before anybody adds to it
    if (c > kSelKeep - kSelThreads) merge();
    const int t = base + tid;
    unsigned long long key = 0;
    if (t < a.n_t) {
      const float s = sr[t];
      if (s >= a.min_score) key = hit_key(s, t);
    }
    const bool pass = key > bar;
    const unsigned long long mask = __ballot(pass);
    int wbase = 0;
    if (lane == 0 && mask) wbase = atomicAdd(&cnt, __popcll(mask));
    wbase = __shfl(wbase, 0);
    if (pass) buf[kSelKeep + wbase + __popcll(mask & ((1ull << lane) - 1))] = key;
    __syncthreads();
  }
  merge();
  for (int k = tid; k < a.K; k += kSelThreads) {
    const unsigned long long key = buf[k];
    aln_hit h;
    if (key) {
      const int t = (int)~(unsigned)key;
      const int T = (int)(a.toff[t + 1] - a.toff[t]), Q = (int)(a.qoff[a.q_first + row + 1] - a.qoff[a.q_first + row]);
      h.t = t; h.score = sr[t];
      if (a.local) { h.q_end = -1; h.t_end = -1; atomicAdd(&ccnt[hit_class(T, a.all_full)], 1); }   // the end kernels fill these in
      else { h.q_end = Q - 1; h.t_end = T - 1; }                                                   // the cell Optimal starts from
      if (buf[k + 1] == 0 || k == a.K - 1) a.n_hits[row] = k + 1;
    } else {
      h.t = -1; h.score = 0.f; h.q_end = -1; h.t_end = -1;
      if (k == 0) a.n_hits[row] = 0;
    }
    a.hits[(size_t)row * a.K + k] = h;
  }
  __syncthreads();
  if (a.local && tid < 9 && ccnt[tid]) atomicAdd(&a.cls_cnt[tid], ccnt[tid]);
}

// slot (row * K + k) -> the length class of its hit's template, -1 for a padding slot (class_list_kernel, score_common.h)
struct HitClass {
  const aln_hit* hits; const int64_t* toff; int all_full;
  __device__ int operator()(int h) const {
    const int t = hits[h].t;
    return t < 0 ? -1 : hit_class((int)(toff[t + 1] - toff[t]), all_full);
  }
};

// scores of the full-build route, computed on the host side as compact nr x n_cols, into their columns of the slab
__global__ __launch_bounds__(256) void scatter_cols_kernel(float* slab, int n_t, const float* vals, const int32_t* cols, int n_cols,
                                                           long long n) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < n) slab[(size_t)(e / n_cols) * n_t + cols[e % n_cols]] = vals[e];
}

// ---- the end cell of a local hit -------------------------------------------------------------------------------------
// sweep_local (score_sweep.h) for ONE hit slot per wave (blockIdx.x -> list -> (row, template)), observed for what
// Optimal::find_max (optimal.h:108-124) needs.  find_max seeds (Q-2, T-2) and replaces it only on a strictly greater score,
// scanning rows, then columns, ascending: the seed wins every tie it takes part in, otherwise the first maximal cell in
// row-major order does.  Per lane: the row at which the running maximum last strictly improved and — inside that rare
// branch — the smallest of the lane's columns holding it; the wave reduces by (value max, row min, column min); then the seed
// exception: D[Q-2][T-2] is in the registers when the sweep ends.  A maximum of 0 (no positive cell, or no interior) is the seed's.
// (FirstMaxObserver: score_common.h.  Side: the query side, ResidueQuery or ProfileQuery, same header.)
template <int R, class Side>
__global__ __launch_bounds__(64) void score_local_end_kernel(ScoreArgs a, const int32_t* __restrict__ list, aln_hit* hits, int K) {
  __shared__ __attribute__((aligned(16))) int lds[32 * 32];
  const int lane = threadIdx.x;
  Side::stage(lds, a);
  const int slot = list[blockIdx.x];
  const int ti = hits[slot].t, qi = a.q_begin + slot / K;
  const typename Side::Rows::Src* __restrict__ qr = Side::rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);
  LocalCols<R> cols;
  cols.load(tc, T, a.gi, a.ge);
  int d[R][4];
  FirstMaxObserver first;
  const int lmax = sweep_local<R, typename Side::Rows>(lds, cols, qr, Q - 2, d, first);
  // wave reduction: value max, then row min, then column min among the lanes that hold it
  int m = lmax;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o));
  int br = (lmax == m) ? first.lrow : 0x7FFFFFFF;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) br = min(br, __shfl_xor(br, o));
  int bc = (lmax == m && first.lrow == br) ? first.lcol : 0x7FFFFFFF;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) bc = min(bc, __shfl_xor(bc, o));
  // the seed D[Q-2][T-2]: row Q-2 is in d[] (Q >= 3), column T-2 in slot (rs, xs) of lane ls (T >= 3)
  int seed = 0;
  if (m > 0) {
    const int cl = T - 2;
    seed = __shfl(sweep_pick<R>(d, cl / 256, cl & 3, 0), (cl & 255) >> 2);
  }
  if (lane == 0) {
    const bool seed_wins = (m == 0) || (seed == m);
    hits[slot].q_end = seed_wins ? Q - 2 : br;
    hits[slot].t_end = seed_wins ? T - 2 : bc;
  }
}

// End cells of local hits whose pair went the full-build route: resident batches over just those hits, Optimal's pair list —
// enumerate_local (optimal.h:79-105) appends (Q-1, T-1) and prepends find_max's cell, so the entry before the last is that cell.
// Groups are BatchGroup's (score_common.h); prof != nullptr: as there, planes expanded on the host.
static int end_cells_through_batches(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                                     const aln_gap* gap, const std::vector<int32_t>& qi_all, const std::vector<int32_t>& ti_all,
                                     const std::vector<aln_hit*>& where, const aln_qprofiles* prof) {
  std::vector<int32_t> n, st, pairs;
  BatchGroup grp;
  while (grp.next(queries, templates, qi_all.data(), ti_all.data(), qi_all.size(), prof != nullptr)) {
    const size_t g0 = grp.g0;
    const int32_t np = (int32_t)(grp.g1 - g0), stride = (int32_t)std::max<int64_t>(std::min(grp.max_q, grp.max_t) + 3, 4);
    n.assign((size_t)np, 0); st.assign((size_t)np, 0); pairs.assign((size_t)np * stride * 2, 0);
    aln_batch* bb = nullptr;
    BatchSim bs;
    bs.set(sub, prof, templates, (size_t)np, qi_all.data() + g0, ti_all.data() + g0);
    int rc = aln_batch_create(ctx, queries, templates, np, qi_all.data() + g0, ti_all.data() + g0, 0, &bb);
    if (rc == ALN_OK) rc = aln_batch_dp(bb, &bs.sim, gap, ALN_FWD, ALN_DP_AUTO, 0);
    if (rc == ALN_OK) rc = aln_batch_optimal(bb, nullptr, n.data(), pairs.data(), stride, st.data());
    if (bb) aln_batch_destroy(bb);
    if (rc != ALN_OK) return rc;
    for (int32_t p = 0; p < np; ++p) {
      if (st[p] != 0) return st[p];
      if (n[p] < 2 || n[p] > stride) return ALN_E_OVERFLOW;
      const int32_t* e = pairs.data() + ((size_t)p * stride + (size_t)(n[p] - 2)) * 2;
      where[g0 + p]->q_end = e[0]; where[g0 + p]->t_end = e[1];
    }
  }
  return ALN_OK;
}

// The shared body of aln_search_topk and aln_search_topk_profiles (run: prepared): slabs, selection, end cells
static int search_block(ScoreRun& run, int32_t K, float min_score, aln_hit* hits, int32_t* n_hits, const char* entry) {
  aln_ctx* ctx = run.ctx;
  const aln_seqs *queries = run.queries, *templates = run.templates;
  const aln_submatrix* sub = run.sub; const aln_gap* gap = run.gap; const aln_qprofiles* prof = run.prof;
  const int32_t q_begin = run.q_begin;
  const int rows = run.rows, n_t = run.n_t;
  if (rows == 0) return ALN_OK;
  if (n_t == 0) {
    for (size_t k = 0; k < (size_t)rows * K; ++k) { hits[k].t = -1; hits[k].score = 0.f; hits[k].q_end = -1; hits[k].t_end = -1; }
    for (int r = 0; r < rows; ++r) n_hits[r] = 0;
    return ALN_OK;
  }
  const bool all_full = run.route == ScoreRun::kAllFull, local = run.local;
  const std::vector<int32_t>& full_t = all_full ? run.every_t : run.long_t;
  const int n_full = (int)full_t.size();

  // slab rows: scores (4 B x n_t per row) and hits (16 B x K per row) each stay below the budget
  int slab_rows = (int)std::min<size_t>((size_t)rows, std::max<size_t>(1, std::min(kSlabBudget / ((size_t)n_t * 4), kSlabBudget / ((size_t)K * 16))));
  if (ctx->hints.search_slab_rows > 0) slab_rows = std::min(rows, ctx->hints.search_slab_rows);
  const bool debug = ctx->hints.search_debug != 0;

  // Everything below leaves through STRY / RTRY (score_common.h): the stream is synchronised before `bufs` frees the slab,
  // the hit buffers and the run's device state, and before the debug events go.
  DeviceBufs bufs(run);
  struct Events {                                  // search_debug's four timestamps
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ~Events() { for (hipEvent_t e : ev) if (e) hipEventDestroy(e); }
  } events;
  hipEvent_t (&ev)[4] = events.ev;
  float *dslab = nullptr, *dfull = nullptr; aln_hit* dhits = nullptr; int32_t *dnh = nullptr, *dlist = nullptr, *dcnt = nullptr, *dfcols = nullptr;
  // profiles: the block's device rows (128 B each) stay below the slab budget too, else every slab brings its own
  run.rows_per_slab = prof && (size_t)(prof->offsets[run.q_end] - prof->offsets[q_begin]) * 128 > kSlabBudget;
  RTRY(all_full ? run.upload_offsets() : run.upload());
  STRY(bufs.get(dslab, (size_t)slab_rows * n_t));
  STRY(bufs.get(dhits, (size_t)slab_rows * K));
  STRY(bufs.get(dnh, (size_t)slab_rows));
  STRY(bufs.get(dcnt, 18));
  if (local) STRY(bufs.get(dlist, (size_t)slab_rows * K));
  std::vector<float> hfull;                      // the full-build route's scores of one slab: nr x n_full
  std::vector<int32_t> fcol;                     // template -> column of hfull
  std::vector<char> is_full((size_t)n_t, all_full ? 1 : 0);
  if (n_full) {
    hfull.resize((size_t)slab_rows * n_full);
    if (!all_full) {
      fcol.assign((size_t)n_t, 0);
      for (int j = 0; j < n_full; ++j) { fcol[full_t[j]] = j; is_full[full_t[j]] = 1; }
      STRY(bufs.get(dfull, hfull.size()));
      STRY(bufs.get(dfcols, (size_t)n_full));
      STRY(hipMemcpyAsync(dfcols, full_t.data(), (size_t)n_full * 4, hipMemcpyHostToDevice, ctx->stream));
    }
  }
  if (debug) for (hipEvent_t& e : ev) STRY(hipEventCreate(&e));
  float ms_score = 0, ms_select = 0, ms_end = 0; double ms_full_end = 0; int n_slabs = 0; long long n_end = 0, n_full_end = 0;

  for (int r0 = 0; r0 < rows; r0 += slab_rows, ++n_slabs) {
    const int nr = std::min(slab_rows, rows - r0);
    if (debug) STRY(hipEventRecord(ev[0], ctx->stream));
    // (a) the slab's scores
    if (!all_full) RTRY(run.launch(r0, nr, dslab));
    if (n_full) {
      RTRY(score_through_batches(ctx, queries, templates, sub, gap, q_begin + r0, q_begin + r0 + nr, full_t, hfull.data(),
                                 all_full ? nullptr : fcol.data(), (size_t)n_full, prof));
      if (all_full) STRY(hipMemcpyAsync(dslab, hfull.data(), (size_t)nr * n_t * 4, hipMemcpyHostToDevice, ctx->stream));
      else {
        const long long ne = (long long)nr * n_full;
        STRY(hipMemcpyAsync(dfull, hfull.data(), (size_t)ne * 4, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(scatter_cols_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, ctx->stream, dslab, n_t, dfull, dfcols, n_full, ne);
        STRY(hipGetLastError());
      }
    }
    if (debug) STRY(hipEventRecord(ev[1], ctx->stream));
    // (b) the K best of every row, and the local hits listed by length class
    STRY(hipMemsetAsync(dcnt, 0, 18 * 4, ctx->stream));
    SelectArgs sa = {};
    sa.slab = dslab; sa.qoff = run.dqo; sa.toff = run.dto; sa.hits = dhits; sa.n_hits = dnh; sa.cls_cnt = dcnt;
    sa.n_t = n_t; sa.K = K; sa.q_first = q_begin + r0; sa.min_score = min_score; sa.local = local; sa.all_full = all_full;
    hipLaunchKernelGGL(topk_select_kernel, dim3(nr), dim3(kSelThreads), 0, ctx->stream, sa);
    STRY(hipGetLastError());
    int cls_cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (local) {
      STRY(hipMemcpyAsync(cls_cnt, dcnt, sizeof cls_cnt, hipMemcpyDeviceToHost, ctx->stream));
      STRY(hipStreamSynchronize(ctx->stream));
      const int n_slots = nr * K;
      const HitClass hc = {dhits, run.dto, (int)all_full};
      hipLaunchKernelGGL(class_list_kernel<HitClass>, dim3((n_slots + 255) / 256), dim3(256), 0, ctx->stream, hc, n_slots, ClassOff::of(cls_cnt), dcnt + 9, dlist);
      STRY(hipGetLastError());
    }
    if (debug) STRY(hipEventRecord(ev[2], ctx->stream));
    // (c) end cells of the local hits the register-resident kernels scored
    if (local && !all_full) {
      ScoreArgs s = run.a;
      s.q_begin = q_begin + r0;
      STRY(launch_classes(prof != nullptr, cls_cnt, [&](auto side, auto rc, int cnt, int off) {
        if (run.qgaps) launch_qgaps_end(decltype(rc)::value, cnt, ctx->stream, s, dlist + off, dhits, K);
        else hipLaunchKernelGGL((score_local_end_kernel<decltype(rc)::value, decltype(side)>), dim3(cnt), dim3(64), 0, ctx->stream, s, dlist + off, dhits, K);
        n_end += cnt;
      }));
    }
    if (debug) STRY(hipEventRecord(ev[3], ctx->stream));
    aln_hit* out = hits + (size_t)r0 * K;
    STRY(hipMemcpyAsync(out, dhits, (size_t)nr * K * sizeof(aln_hit), hipMemcpyDeviceToHost, ctx->stream));
    STRY(hipMemcpyAsync(n_hits + r0, dnh, (size_t)nr * 4, hipMemcpyDeviceToHost, ctx->stream));
    STRY(hipStreamSynchronize(ctx->stream));
    if (debug) {
      float ms = 0;
      STRY(hipEventElapsedTime(&ms, ev[0], ev[1])); ms_score += ms;
      STRY(hipEventElapsedTime(&ms, ev[1], ev[2])); ms_select += ms;
      STRY(hipEventElapsedTime(&ms, ev[2], ev[3])); ms_end += ms;
    }
    // ... and of the hits that went the full-build route
    if (local && cls_cnt[0] > 0) {
      const auto t0 = std::chrono::steady_clock::now();
      std::vector<int32_t> qi, tix; std::vector<aln_hit*> where;
      for (int r = 0; r < nr; ++r)
        for (int k = 0; k < n_hits[r0 + r]; ++k) {
          aln_hit* h = &out[(size_t)r * K + k];
          if (is_full[h->t]) { qi.push_back(q_begin + r0 + r); tix.push_back(h->t); where.push_back(h); }
        }
      RTRY(end_cells_through_batches(ctx, queries, templates, sub, gap, qi, tix, where, prof));
      n_full_end += (long long)qi.size();
      ms_full_end += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
  }
  if (debug)
    fprintf(stderr, "%s: rows %d n_t %d K %d slabs %d (%d rows each) score_ms %.3f select_ms %.3f end_ms %.3f (%lld hits) "
            "full_end_ms %.3f (%lld hits)\n", entry, rows, n_t, K, n_slabs, slab_rows, ms_score, ms_select, ms_end, n_end, ms_full_end, n_full_end);
  return ALN_OK;
}

}  // namespace aln

using namespace aln;

extern "C" int aln_search_topk(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                               const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K, float min_score,
                               aln_hit* hits, int32_t* n_hits) {
  if (!hits || !n_hits || K < 1 || K > kSelKeep) return ALN_E_ARG;
  ScoreRun run;
  int rc = run.prepare(ctx, queries, templates, sub, gap, q_begin, q_end);
  if (rc != ALN_OK) return rc;
  return search_block(run, K, min_score, hits, n_hits, "aln_search_topk");
}

extern "C" int aln_search_topk_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* templates, const aln_gap* gap,
                                        int32_t q_begin, int32_t q_end, int32_t K, float min_score, aln_hit* hits, int32_t* n_hits) {
  if (!hits || !n_hits || !profiles || K < 1 || K > kSelKeep) return ALN_E_ARG;
  ScoreRun run;
  int rc = run.prepare(ctx, nullptr, templates, nullptr, gap, q_begin, q_end, profiles);
  if (rc != ALN_OK) return rc;
  return search_block(run, K, min_score, hits, n_hits, "aln_search_topk_profiles");
}

extern "C" int aln_search_topk_profiles_gaps(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_qgaps* gaps, const aln_seqs* templates,
                                             int32_t align_type, int32_t q_begin, int32_t q_end, int32_t K, float min_score,
                                             aln_hit* hits, int32_t* n_hits) {
  if (!hits || !n_hits || !profiles || !gaps || K < 1 || K > kSelKeep) return ALN_E_ARG;
  ScoreRun run;
  run.qgaps = gaps; run.qgaps_align_type = align_type;
  int rc = run.prepare(ctx, nullptr, templates, nullptr, nullptr, q_begin, q_end, profiles);
  if (rc != ALN_OK) return rc;
  return search_block(run, K, min_score, hits, n_hits, "aln_search_topk_profiles_gaps");
}

#undef STRY
#undef RTRY
