// search_qgaps.hip — all-vs-all scoring and search for profiles whose rows carry their own GAP PENALTIES (aln_qgaps) (gfx950).
//
// aln_score_profiles_gaps_vs_all and aln_search_topk_profiles_gaps (include/aln_hip.h has the definition) run the kernels of
// score_only.hip and search_topk.hip over score_sweep_qgaps.h's sweeps: one wave per pair, the whole DP row in VGPRs, ProfileRows'
// LDS ring as the row source, nothing per cell in HBM.  A row's four prices are words 26 .. 29 of its device image and arrive
// with its similarities.  Everything around the kernels — ScoreRun, the slabs, topk_select_kernel, class_list_kernel, the
// end-cell pass — is the constant-gap entries'; only the kernel launched differs (launch_qgaps_score / launch_qgaps_end).
// There is no full-build route: no batch gap model prices a gap by the query position.
#include "score_common.h"
#include "score_sweep_qgaps.h"

namespace aln {

template <int R>
__global__ __launch_bounds__(64) void score_local_qgaps_kernel(ScoreArgs a) {
  __shared__ __attribute__((aligned(16))) int lds[32 * 32];
  const int lane = threadIdx.x;
  const int ti = a.tsel[blockIdx.x], qi = a.q_begin + blockIdx.y;
  const int4* __restrict__ qr = ProfileQuery::rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);
  QGapLocalCols<R> cols;
  cols.load(tc, T);
  int d[R][4];
  int m = sweep_local_qgaps<R>(lds, cols, qr, Q - 2, d, NoObserver());
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o));
  if (lane == 0) a.scores[(size_t)blockIdx.y * a.n_t + ti] = (float)m;
}

// the four non-local align types: the final cell's score
template <int R>
__global__ __launch_bounds__(64) void score_global_qgaps_kernel(ScoreArgs a, int free_del, int free_ins) {
  __shared__ __attribute__((aligned(16))) int lds[32 * 32];
  const int lane = threadIdx.x;
  const int ti = a.tsel[blockIdx.x], qi = a.q_begin + blockIdx.y;
  const int4* __restrict__ qr = ProfileQuery::rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);
  float* out = &a.scores[(size_t)blockIdx.y * a.n_t + ti];
  // degenerate shapes: no interior row -> del(0, T-2), no interior column -> ins(1, Q-2); the prices come straight from the
  // device rows (32 words each)
  if (Q == 2 || T == 2) {
    const int* __restrict__ w = reinterpret_cast<const int*>(qr);
    int cost = 0;
    if (Q == 2) {
      const int len = T - 2;
      cost = (len < 1 || free_del) ? 0 : w[kQGapWord] + w[kQGapWord + 1] * (len - 1);
    } else if (!free_ins && Q >= 3) {
      int part = 0;
      for (int p = 2 + lane; p <= Q - 2; p += 64) part += w[p * 32 + kQGapWord + 3];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o);
      cost = w[32 + kQGapWord + 2] + part;
    }
    if (lane == 0) *out = (float)(-cost);
    return;
  }
  QGapGlobalCols<R> cols;
  cols.load(tc, T);
  int best = sweep_global_qgaps<R>(lds, cols, qr, Q, free_del, free_ins, NoObserver());
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) best = max(best, __shfl_xor(best, o));
  if (lane == 0) *out = (float)best;
}

// the end cell of a local hit: score_local_end_kernel (search_topk.hip) over the gap-row sweep, same reduction and seed rule
template <int R>
__global__ __launch_bounds__(64) void score_local_end_qgaps_kernel(ScoreArgs a, const int32_t* __restrict__ list, aln_hit* hits, int K) {
  __shared__ __attribute__((aligned(16))) int lds[32 * 32];
  const int lane = threadIdx.x;
  const int slot = list[blockIdx.x];
  const int ti = hits[slot].t, qi = a.q_begin + slot / K;
  const int4* __restrict__ qr = ProfileQuery::rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);
  QGapLocalCols<R> cols;
  cols.load(tc, T);
  int d[R][4];
  FirstMaxObserver first;
  const int lmax = sweep_local_qgaps<R>(lds, cols, qr, Q - 2, d, first);
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

void launch_qgaps_score(int r, bool local, dim3 grid, hipStream_t stream, const ScoreArgs& s, int free_del, int free_ins) {
  dispatch_r<8>(r, [&](auto rc) {
    constexpr int R = decltype(rc)::value;
    if (local) hipLaunchKernelGGL(score_local_qgaps_kernel<R>, grid, dim3(64), 0, stream, s);
    else hipLaunchKernelGGL(score_global_qgaps_kernel<R>, grid, dim3(64), 0, stream, s, free_del, free_ins);
  });
}

void launch_qgaps_end(int r, int cnt, hipStream_t stream, const ScoreArgs& s, const int32_t* list, aln_hit* hits, int K) {
  dispatch_r<8>(r, [&](auto rc) {
    hipLaunchKernelGGL(score_local_end_qgaps_kernel<decltype(rc)::value>, dim3(cnt), dim3(64), 0, stream, s, list, hits, K);
  });
}

}  // namespace aln

#undef STRY
#undef RTRY
