// search_pileup.h — what the entries that lay hits out as query-anchored rows share: PileupJob, the job behind
// hit_local_kernel / hit_global_kernel<R, Side, PileupJob> (search_align.h), its argument blocks, the host's restatement of
// one row from a pair list (the batch route) and the launch of the kernel pair.  aln_hits_pileup (search_pileup.hip, whose
// head tells where the bytes come from and how the gap pass is ordered) downloads the rows; aln_hits_weights
// (search_weights.hip) keeps the letters rows of a group of queries on the device and reads the weights off them, and
// aln_hits_purge (search_purge.hip) the purge decision before that (both through search_stack.h's HitStack).  The
// kernels are instantiated ONCE, in search_pileup.hip: launch_pileup_job is an ordinary function defined there.
#pragma once
#include <climits>

#include "search_align.h"

namespace aln {

// Where the rows of a chunk's hits go: the same for every chunk of a call, so it lies on the device once and the kernels'
// argument block carries one pointer to it — the sink reads it after the sweep, and nothing of it is held across the sweep.
struct PileupRows {
  const int32_t* live;      // per hit of the chunk; 0: the record only
  const char* pool;         // the templates' characters (read only where letters are wanted)
  char* letters;            // hit h's row at letters + h * stride, preset to '.' (nullptr: not wanted)
  uint16_t* tpos;           // ... at tpos + h * stride, preset to 0 (nullptr: not wanted)
  aln_hit_span* spans;      // one per hit of the chunk, preset to zero (nullptr: not wanted)
  int64_t stride;
};

struct PileupArgs {
  const int32_t* list;      // blockIdx.x -> hit of the chunk
  const HitDesc* desc;
  uint8_t* strip;
  const PileupRows* rows;
  PairResult* res;          // best = score, n_path, status
  int32_t* same;
};

// The job that piles up.  What strip_walk's entries become: the identity's count, two stores, the lane's bounds.
struct PileupJob {
  typedef PileupArgs Args;
  template <class Letters>
  struct Sink {
    Letters qs, ts;                         // what the identity is counted over
    const char* tch;                        // the template's characters
    char* lrow; uint16_t* prow;             // the hit's two rows (index q - 1)
    aln_hit_span* span;
    int Q, T, live;
    int same = 0, lo = INT_MAX, lo_t = 0, hi = -1, hi_t = 0;
    __device__ __forceinline__ Sink(const Args& g, const ScoreArgs& a, int hit, int, Letters qs_, Letters ts_, const uint8_t*, int Q_,
                                    int T_)
        : qs(qs_), ts(ts_), Q(Q_), T(T_) {
      const PileupRows o = *g.rows;
      tch = o.pool + a.toff[g.desc[hit].t];
      lrow = o.letters ? o.letters + (size_t)hit * o.stride : nullptr;
      prow = o.tpos ? o.tpos + (size_t)hit * o.stride : nullptr;
      span = o.spans ? o.spans + hit : nullptr;
      live = o.live[hit];
    }
    __device__ __forceinline__ void operator()(int, int q, int t) {
      same += (qs[q] == ts[t]) ? 1 : 0;
      if (live && q >= 1 && q <= Q - 2 && t >= 1 && t <= T - 2) {
        if (q < lo) { lo = q; lo_t = t; }
        if (q > hi) { hi = q; hi_t = t; }
        if (prow) prow[q - 1] = (uint16_t)t;
        if (lrow) lrow[q - 1] = tch[t];
      }
    }
    // after the walk: same summed, the span, '-' over the unwritten positions of i_lo .. i_hi (every lane calls it)
    __device__ __forceinline__ void finish() {
      const int mylo = lo, myhi = hi;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        same += __shfl_xor(same, off);
        lo = min(lo, __shfl_xor(lo, off));
        hi = max(hi, __shfl_xor(hi, off));
      }
      if (hi < 0) return;                   // muted, or no interior entry: '.', 0 and the zero span stand (wave-uniform)
      // a query position occurs once in a list, so one lane owns each bound
      lo_t = __shfl(lo_t, __builtin_ctzll(__ballot(mylo == lo)));
      hi_t = __shfl(hi_t, __builtin_ctzll(__ballot(myhi == hi)));
      if (span && threadIdx.x == 0) *span = aln_hit_span{lo, hi, lo_t, hi_t};
      if (lrow) {
        __threadfence();                    // the walk's stores of every lane are visible to every lane (head of search_pileup.hip)
        __syncthreads();
        for (int i = lo + (int)threadIdx.x; i <= hi; i += 64)
          if (lrow[i - 1] == '.') lrow[i - 1] = '-';
      }
    }
    __device__ __forceinline__ int status(int) const { return 0; }
  };
};

// One slot's rows from its pair list, on the host: the definition of include/aln_hip.h restated (the batch route).  lrow / prow:
// the slot's rows, already '.' / 0 over p < Q - 2; span: already zero.
inline void pileup_from_list(const int32_t* l, int n, int64_t Q, int64_t T, const char* tres, char* lrow, uint16_t* prow,
                             aln_hit_span* span) {
  int64_t lo = INT64_MAX, hi = -1, lo_t = 0, hi_t = 0;
  for (int k = 0; k < n; ++k) {
    const int64_t i = l[2 * k], j = l[2 * k + 1];
    if (i < 1 || i > Q - 2 || j < 1 || j > T - 2) continue;
    if (i < lo) { lo = i; lo_t = j; }
    if (i > hi) { hi = i; hi_t = j; }
    if (prow) prow[i - 1] = (uint16_t)j;
    if (lrow) lrow[i - 1] = tres[j];
  }
  if (hi < 0) return;
  if (span) *span = aln_hit_span{(int32_t)lo, (int32_t)hi, (int32_t)lo_t, (int32_t)hi_t};
  if (lrow)
    for (int64_t i = lo; i <= hi; ++i)
      if (lrow[i - 1] == '.') lrow[i - 1] = '-';
}

// launch_hit_job<PileupJob> (search_align.h) behind an ordinary function, defined in search_pileup.hip
int launch_pileup_job(FusedRoute<HitDesc>& fr, const FusedChunk& c, PileupArgs& g);

}  // namespace aln
