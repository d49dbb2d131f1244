// search_align_multi.h — what align_local_multi_kernel (search_align_multi.hip) is handed: how a hit and its transient planes are
// described, where the rounds' results go, and the observer that turns one masked row sweep into both the strip bytes of the
// walk and find_max's end cell.
#pragma once
#include "search_align.h"

namespace aln {

struct MultiDesc {          // one used slot the fused kernel takes, 32 bytes
  int32_t q, t;             // sequence indices in the pools
  int32_t cls;              // template length class 1 .. 8
  int32_t pad;
  int64_t strip_off;        // first byte of the hit's strip: max(Q - 3, 1) rows of 256 cls bytes (rows 2 .. Q-2)
  int64_t mask_off;         // first 32-bit word of the hit's forbidden-cell plane: Q rows of 8 cls words
};

inline void place(MultiDesc& d, size_t strip, size_t mask) { d.strip_off = (int64_t)strip; d.mask_off = (int64_t)mask; }   // FusedRoute::cut

struct MultiArgs {
  const int32_t* list;      // blockIdx.x -> hit of the chunk
  const MultiDesc* desc;
  uint8_t* strip;
  uint32_t* mask;           // zeroed per chunk
  int32_t* trav;            // round a of hit h in TRAVERSAL order (end -> start) at trav + (h * n_rounds + a) * trav_stride * 2
  int trav_stride;
  int n_rounds;             // N = max_alignments
  float min_score;
  PairResult* res;          // [h * n_rounds + a], zeroed per chunk: rounds that are not reported keep n_path 0
  int32_t* same;            // [h * n_rounds + a]
  int32_t* n_found;         // [h]
};

// Both observers of the local sweep at once: the strip byte of every cell (StripObserver, search_align.h) and find_max's
// partial (FirstMaxObserver's rule, score_common.h: the row the lane's running maximum last strictly rose in and the smallest
// of the lane's columns holding it).
struct StripFirstMaxObserver : StripObserver<true> {
  int seen = 0, lrow = 0, lcol = 0;
  template <int R>
  __device__ __forceinline__ void row(int i, const int (&d)[R][4], int lane_max) {
    if (lane_max > seen) {
      seen = lane_max; lrow = i;
#pragma unroll
      for (int r = R - 1; r >= 0; --r)
#pragma unroll
        for (int x = 3; x >= 0; --x) lcol = (d[r][x] == lane_max) ? 4 * (int)threadIdx.x + 256 * r + x : lcol;
    }
  }
};

}  // namespace aln
