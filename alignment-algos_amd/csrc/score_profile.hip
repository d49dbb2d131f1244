// score_profile.hip — all-vs-all scores and local end cells for queries given as POSITION-SPECIFIC rows (aln_qprofiles), no
// planes (gfx950).
//
// A profile says, for every query position, what each template letter scores there: S[i][j] = rows[i][letter of t[j]].  The row
// sweep of score_sweep.h reads a row's similarities as 32 ints in LDS indexed by the template's code; for a residue query that
// vector is the table row of the query's letter, here it is row i of the profile itself.  So the three kernels below are the
// table kernels of score_only.hip / search_topk.hip with another row source (ProfileRows, score_sweep.h): the device holds the
// rows widened to 32 int32 and an asynchronous 16-byte-per-lane global -> LDS copy brings them into a ring of 32 rows, 8 rows
// (1 KiB) per copy, one copy ahead of the sweep.  Same recurrence, same observers, same results as a full build over the Q x T
// plane of the profile (aln_batch_dp with ALN_SIM_MATRIX) + Optimal.
//   score_local_prof_kernel<R>       find_max's value                      (twin of score_local_kernel<R>)
//   score_global_prof_kernel<R>      the final cell, four non-local types  (twin of score_global_kernel<R>)
//   score_local_end_prof_kernel<R>   find_max's cell of one hit            (twin of score_local_end_kernel<R>)
// ScoreArgs: qcodes is the device rows as bytes, biased so that pool row r starts at qcodes + 128 r; qoff counts ROWS; table32 and
// qsel are unused.  One wave per pair, launched by template length class like their twins (ScoreRun::launch, search_topk.hip).
#include "score_common.h"

namespace aln {

__device__ __forceinline__ const int4* profile_rows(const ScoreArgs& a, int qi) {
  return reinterpret_cast<const int4*>(a.qcodes + a.qoff[qi] * 128);
}

template <int R>
__global__ __launch_bounds__(64) void score_local_prof_kernel(ScoreArgs a) {
  __shared__ __attribute__((aligned(16))) int ring[32 * 32];
  const int lane = threadIdx.x;
  const int ti = a.tsel[blockIdx.x], qi = a.q_begin + blockIdx.y;
  const int4* __restrict__ pr = profile_rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);
  LocalCols<R> cols;
  cols.load(tc, T, a.gi, a.ge);
  int d[R][4];
  int m = sweep_local<R, ProfileRows>(ring, cols, pr, Q - 2, d, NoObserver());
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o));
  if (lane == 0) a.scores[(size_t)blockIdx.y * a.n_t + ti] = (float)m;
}

template <int R>
__global__ __launch_bounds__(64) void score_global_prof_kernel(ScoreArgs a, int free_del, int free_ins) {
  __shared__ __attribute__((aligned(16))) int ring[32 * 32];
  const int lane = threadIdx.x;
  const int ti = a.tsel[blockIdx.x], qi = a.q_begin + blockIdx.y;
  const int4* __restrict__ pr = profile_rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);
  const int gi = a.gi, ge = a.ge;
  float* out = &a.scores[(size_t)blockIdx.y * a.n_t + ti];
  // degenerate shortcuts (dpmatrix.h:375-390), as in score_global_kernel: no interior row or column -> one gap from the origin
  if (Q == 2 || T == 2) {
    int cost = 0;
    if (Q == 2) { const int len = T - 2; cost = (len < 1 || free_del) ? 0 : gi + ge * (len - 1); }
    else { const int len = Q - 2; cost = (len < 1 || free_ins) ? 0 : gi + ge * (len - 1); }
    if (lane == 0) *out = (float)(-cost);
    return;
  }
  GlobalCols<R> cols;
  cols.load(tc, T, gi, ge);
  int best = sweep_global<R, ProfileRows>(ring, cols, pr, Q, free_del, free_ins, NoObserver());
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) best = max(best, __shfl_xor(best, o));
  if (lane == 0) *out = (float)best;
}

// the end cell of a local hit: score_local_end_kernel (search_topk.hip) over a profile's rows; the reduction and the seed rule
// are restated, not shared, because handing the row array to a helper by reference costs registers
template <int R>
__global__ __launch_bounds__(64) void score_local_end_prof_kernel(ScoreArgs a, const int32_t* __restrict__ list, aln_hit* hits, int K) {
  __shared__ __attribute__((aligned(16))) int ring[32 * 32];
  const int lane = threadIdx.x;
  const int slot = list[blockIdx.x];
  const int ti = hits[slot].t, qi = a.q_begin + slot / K;
  const int4* __restrict__ pr = profile_rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);
  LocalCols<R> cols;
  cols.load(tc, T, a.gi, a.ge);
  int d[R][4];
  FirstMaxObserver first;
  const int lmax = sweep_local<R, ProfileRows>(ring, cols, pr, Q - 2, d, first);
  int m = lmax;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o));
  int br = (lmax == m) ? first.lrow : 0x7FFFFFFF;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) br = min(br, __shfl_xor(br, o));
  int bc = (lmax == m && first.lrow == br) ? first.lcol : 0x7FFFFFFF;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) bc = min(bc, __shfl_xor(bc, o));
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

void launch_score_prof(int r, bool local, dim3 grid, hipStream_t stream, const ScoreArgs& s, int free_del, int free_ins) {
  dispatch_r<8>(r, [&](auto rc) {
    constexpr int R = decltype(rc)::value;
    if (local) hipLaunchKernelGGL(score_local_prof_kernel<R>, grid, dim3(64), 0, stream, s);
    else hipLaunchKernelGGL(score_global_prof_kernel<R>, grid, dim3(64), 0, stream, s, free_del, free_ins);
  });
}

void launch_score_local_end_prof(int r, int n, hipStream_t stream, const ScoreArgs& s, const int32_t* list, aln_hit* hits, int K) {
  dispatch_r<8>(r, [&](auto rc) {
    hipLaunchKernelGGL(score_local_end_prof_kernel<decltype(rc)::value>, dim3(n), dim3(64), 0, stream, s, list, hits, K);
  });
}

}  // namespace aln
