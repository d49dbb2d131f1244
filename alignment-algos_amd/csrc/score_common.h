// score_common.h — what the all-vs-all score kernels (score_only.hip) and the top-K search built on them (search_topk.hip) share:
// the DPP helpers of the collapsed recurrence, the kernels' argument block, and ScoreRun, the host side of one all-vs-all
// scoring call cut into steps so that a caller can leave the scores of a slab of query rows in a device buffer of its own.
#pragma once
#include <deque>
#include <vector>

#include "aln_internal.h"

namespace aln {

constexpr int kNegS = -(1 << 28);

template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF>
__device__ __forceinline__ int sdpp(int old, int src) {
  return __builtin_amdgcn_update_dpp(old, src, CTRL, ROW_MASK, BANK_MASK, false);
}
__device__ __forceinline__ int wave_incl_max_s(int v) {
  const int ident = (int)0x80000000;
  v = max(v, sdpp<0x111>(ident, v));
  v = max(v, sdpp<0x112>(ident, v));
  v = max(v, sdpp<0x114>(ident, v));
  v = max(v, sdpp<0x118>(ident, v));
  v = max(v, sdpp<0x142, 0xA>(ident, v));
  v = max(v, sdpp<0x143, 0xC>(ident, v));
  return v;
}

struct ScoreArgs {
  const uint8_t* qcodes; const int64_t* qoff;   // query pool, offsets (n_q + 1)
  const uint8_t* tcodes; const int64_t* toff;   // template pool
  const int32_t* table32;                       // 32 x 32
  const int32_t* tsel;                          // blockIdx.x -> template index (templates are launched by length class)
  const int32_t* qsel;                          // packed kernel: query rows of the slab sorted by length (neighbours share a wave)
  float* scores;                                // rows x n_t
  int q_begin, n_t;
  int gi, ge;
};

// One all-vs-all scoring call (the arguments of aln_score_all_vs_all): prepare() checks them and decides the route, upload()
// puts what the register-resident kernels read on the device, launch() enqueues those kernels for a block of query rows
// into a device buffer of the caller.  Nothing here synchronises; the object must outlive the stream work it enqueued.
struct ScoreRun {
  enum Route { kNothing, kAllFull, kFast };
  aln_ctx* ctx = nullptr;
  const aln_seqs* queries = nullptr; const aln_seqs* templates = nullptr;
  const aln_submatrix* sub = nullptr; const aln_gap* gap = nullptr;
  int32_t q_begin = 0, q_end = 0;
  int rows = 0, n_t = 0;
  bool local = false, packed = false;
  int free_del = 0, free_ins = 0;
  Route route = kNothing;
  std::vector<int32_t> every_t;                 // 0 .. n_t-1 (kAllFull: what score_through_batches takes)
  std::vector<int32_t> long_t;                  // kFast: templates beyond 2048 columns, left to score_through_batches
  std::vector<int32_t> order;                   // kFast: the other templates by length class
  std::vector<int> cls_begin;                   // class r = order[cls_begin[r] .. cls_begin[r+1])
  std::vector<uint8_t> qc, tc;
  int32_t ti[32 * 32];
  int maxQ = 0, maxT = 0;
  double maxs = 0;
  ScoreArgs a = {};
  uint8_t *dq = nullptr, *dt = nullptr; int64_t *dqo = nullptr, *dto = nullptr; int32_t* dtab = nullptr;
  int32_t *dsel = nullptr, *dqsel = nullptr;
  std::deque<std::vector<int32_t>> qorders;     // the packed kernel's length orders: alive until the caller has synchronised

  // the argument checks of aln_score_all_vs_all, in its order; ALN_OK with route == kNothing: no pair to score
  int prepare(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub, const aln_gap* gap,
              int32_t q_begin, int32_t q_end);
  int upload_offsets();                         // qoff / toff only (all a caller of the kAllFull route needs on the device)
  int upload();                                 // kFast: residue codes, offsets, table, class order
  // kFast: scores of query rows [q_begin + row0, q_begin + row0 + nr) against the templates of `order` -> dscores[nr x n_t]
  int launch(int row0, int nr, float* dscores);
  void release();
  ~ScoreRun() { release(); }
};

// scores[(q - q_begin) * ld + col[t]] for the templates of `tlist` through resident batches of full builds
// (col == nullptr: column t, ld == 0: n_t — the layout of aln_score_all_vs_all's result)
int score_through_batches(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                          const aln_gap* gap, int32_t q_begin, int32_t q_end, const std::vector<int32_t>& tlist, float* scores,
                          const int32_t* col = nullptr, size_t ld = 0);

}  // namespace aln
