// search_align_profile.hip — the alignments of the hits of a PROFILE search, on the device: the kernels of
// aln_hits_align_profiles (gfx950).
//
// A position-specific query (aln_qprofiles) changes one thing about the fused hit alignment of search_align.hip: where a row's
// similarities come from.  The sweep, the strip byte, the observers, the final cell's pointer and both walks are those of
// align_local_hit_kernel / align_global_hit_kernel; the row source is ProfileRows (score_sweep.h) — the rows of the profile,
// 32 int32 each, brought from HBM into a 16-byte-aligned ring of 32 rows in LDS by an asynchronous copy of 8 rows, one copy ahead
// of the sweep — and rows are addressed as in score_profile.hip.
//   align_local_hit_prof_kernel<R>    twin of align_local_hit_kernel<R>:  rows 1 .. q_end, five bits per cell, the local walk
//   align_global_hit_prof_kernel<R>   twin of align_global_hit_kernel<R>: rows 1 .. Q-2, four bits per cell, the walk to the origin
// A profile has no letters, so the identity is counted over CHARACTERS: the query letters the caller gave (the consensus pool, or
// the placeholder pool of ScoreRun) against the templates', exactly the comparison gapped_strings_kernel makes for the lines.
//
// The VM counter.  The row loop of these kernels holds the strip stores (R per row) beside the staging copy, and gfx950 retires
// loads, LDS copies and stores through ONE counter in issue order.  ProfileRows::landed() waits until at most one operation is
// outstanding; it is called right after chunk c + 1 is requested, so chunk c has landed (it is older than everything waited
// for) — and so has every strip store issued so far: once per 8 rows the stores are drained.  That is correct and is what ships:
// a counted wait that leaves the stores in flight was built and measured, and did not separate from this one.  INVARIANT (ScoreRun::upload_profile_rows): a sweep requests at most rows
// 0 .. Q + 13 of its profile and the buffer is padded for that; the local kernel stops at q_end <= Q - 2.  The last copy
// requested is never read: it is drained before the walk (and before the kernel returns early) so that nothing is in flight into
// LDS when the wave ends.
#include "search_align.h"

namespace aln {

__device__ __forceinline__ const int4* align_profile_rows(const ScoreArgs& a, int qi) {   // profile_rows(), score_profile.hip
  return reinterpret_cast<const int4*>(a.qcodes + a.qoff[qi] * 128);
}

template <int R>
__global__ __launch_bounds__(64) void align_local_hit_prof_kernel(ScoreArgs a, AlignArgs g, const char* __restrict__ qch,
                                                                 const char* __restrict__ tch) {
  __shared__ __attribute__((aligned(16))) int ring[32 * 32];
  const int lane = threadIdx.x;
  const int hit = g.list[blockIdx.x];
  const HitDesc hd = g.desc[hit];
  const int ti = hd.t, qi = hd.q, q_end = hd.q_end, t_end = hd.t_end;
  const int4* __restrict__ pr = align_profile_rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const char* __restrict__ qs = qch + a.qoff[qi];              // the query letters share the profiles' offsets
  const char* __restrict__ ts = tch + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);
  constexpr int kPitch = 256 * R;
  uint8_t* strip = g.strip + hd.strip_off;      // row i (2 .. q_end) at strip + (i - 2) * kPitch

  // rows 1 .. q_end (1 <= q_end <= Q - 2: the host sends other pairs elsewhere)
  LocalCols<R> cols;
  cols.load(tc, T, a.gi, a.ge);
  int d[R][4];
  __builtin_assume(q_end >= 1);
  StripObserver<true> bytes;
  bytes.strip = strip; bytes.pitch = kPitch;
  sweep_local<R, ProfileRows>(ring, cols, pr, q_end, d, bytes);
  __threadfence();                                           // the last copy has landed; the walk's lanes read bytes other lanes stored
  __syncthreads();
  const int dend = __shfl(sweep_pick<R>(d, t_end / 256, t_end & 3, 0), (t_end & 255) >> 2);
  PairResult res = {};
  res.best = (float)dend; res.corner = 0.f; res.best_q = q_end; res.best_t = t_end;
  if (!((float)dend == hd.score)) {                          // not the cell the slot's score stands in: refuse the slot
    if (lane == 0) { res.best = 0.f; res.status = ALN_E_ARG; res.n_path = 0; g.res[hit] = res; g.same[hit] = 0; }
    return;
  }

  // ---- the walk back (optimal.h:79-105), as in align_local_hit_kernel -------------------------------------------------------
  int32_t* o = g.trav + (size_t)hit * g.trav_stride * 2;
  const int cap = g.trav_stride;
  int n = 0, same = 0;
  auto sink = [&](int k, int q, int t) {
    if (k < cap) { o[2 * k] = q; o[2 * k + 1] = t; same += (qs[q] == ts[t]) ? 1 : 0; }
  };
  auto emit1 = [&](int q, int t) { if (lane == 0) sink(n, q, t); ++n; };
  emit1(Q - 1, T - 1);
  emit1(q_end, t_end);
  if (strip_walk<kPitch, true>(strip, q_end, t_end, n, sink)) emit1(0, 0);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) same += __shfl_xor(same, off);
  if (lane == 0) {
    res.n_path = n;
    res.status = n <= cap ? 0 : ALN_E_OVERFLOW;
    g.res[hit] = res;
    g.same[hit] = same;
  }
}

template <int R>
__global__ __launch_bounds__(64) void align_global_hit_prof_kernel(ScoreArgs a, AlignArgs g, const char* __restrict__ qch,
                                                                  const char* __restrict__ tch, int free_del, int free_ins) {
  __shared__ __attribute__((aligned(16))) int ring[32 * 32];
  const int lane = threadIdx.x;
  const int hit = g.list[blockIdx.x];
  const HitDesc hd = g.desc[hit];
  const int ti = hd.t, qi = hd.q;
  const int4* __restrict__ pr = align_profile_rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const char* __restrict__ qs = qch + a.qoff[qi];
  const char* __restrict__ ts = tch + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);   // Q >= 3, T >= 3: the host's routing
  const int gi = a.gi, ge = a.ge;
  constexpr int kPitch = 256 * R;
  uint8_t* strip = g.strip + hd.strip_off;      // row i (2 .. Q-2) at strip + (i - 2) * kPitch

  GlobalCols<R> cols;
  cols.load(tc, T, gi, ge);
  GlobalObserver<R> ob(cols, free_del, free_ins ? 0 : ge, Q - 3);
  ob.strip = strip; ob.pitch = kPitch;
  int score = sweep_global<R, ProfileRows>(ring, cols, pr, Q, free_del, free_ins, ob);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) score = max(score, __shfl_xor(score, off));

  int i, j;
  ob.final_cell(free_ins, i, j);
  __threadfence();                                           // the last copy has landed; the walk's lanes read bytes other lanes stored
  __syncthreads();

  // ---- the walk back (optimal.h:56-74): it always runs to a cell of row 1 or column 1, which points at (0,0) -------------------
  int32_t* o = g.trav + (size_t)hit * g.trav_stride * 2;
  const int cap = g.trav_stride;
  int n = 0, same = 0;
  auto sink = [&](int k, int q, int t) {
    if (k < cap) { o[2 * k] = q; o[2 * k + 1] = t; same += (qs[q] == ts[t]) ? 1 : 0; }
  };
  auto emit1 = [&](int q, int t) { if (lane == 0) sink(n, q, t); ++n; };
  emit1(Q - 1, T - 1);
  emit1(i, j);
  strip_walk<kPitch, false>(strip, i, j, n, sink);
  emit1(0, 0);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) same += __shfl_xor(same, off);
  if (lane == 0) {
    PairResult res = {};
    res.best = (float)score; res.corner = 0.f; res.best_q = Q - 1; res.best_t = T - 1;
    res.n_path = n;
    res.status = n <= cap ? 0 : ALN_E_OVERFLOW;
    g.res[hit] = res;
    g.same[hit] = same;
  }
}

// The instantiations kept, by the rule of search_align.hip: no scratch memory, no VGPR spill (DESIGN 4.8f has the table).
constexpr unsigned kFusedProfClasses = 0x1FEu;               // bit R set: class R runs in align_local_hit_prof_kernel<R>
constexpr unsigned kFusedGlobalProfClasses = 0x1FEu;         // bit R set: class R runs in align_global_hit_prof_kernel<R>

unsigned align_prof_classes(bool local) { return local ? kFusedProfClasses : kFusedGlobalProfClasses; }

void launch_align_hit_prof(int r, bool local, int n, hipStream_t stream, const ScoreArgs& s, const AlignArgs& g, const char* qch,
                           const char* tch, int free_del, int free_ins) {
  dispatch_r<8>(r, [&](auto rc) {
    constexpr int R = decltype(rc)::value;
    if (local) hipLaunchKernelGGL(align_local_hit_prof_kernel<R>, dim3(n), dim3(64), 0, stream, s, g, qch, tch);
    else hipLaunchKernelGGL(align_global_hit_prof_kernel<R>, dim3(n), dim3(64), 0, stream, s, g, qch, tch, free_del, free_ins);
  });
}

}  // namespace aln
