// search_align.h — what the fused hit-alignment kernels of search_align.hip (residue queries, the table in LDS) and
// search_align_profile.hip (position-specific queries, rows staged into LDS) share: how a hit is described to a kernel, where its
// results go and how a slot's record, list and lines are written for the caller (AlignOut, shared with search_align_multi.hip),
// and the two observers that turn a row sweep into the strip bytes and the final cell's pointer.  The strip byte is
// defined at the head of search_align.hip.  The two walks are restated in each file, not shared (a helper that takes
// the kernel's state by reference costs registers).
#pragma once
#include <algorithm>
#include <cstring>

#include "score_common.h"

namespace aln {

struct HitDesc {            // one used slot a fused kernel takes, 32 bytes
  int32_t q, t;             // sequence indices in the pools
  int32_t q_end, t_end;     // local: the trusted end cell (non-local: unused, 0)
  float score;              // local: the slot's score, D[q_end][t_end] must equal it (non-local: unused, 0)
  int32_t cls;              // template length class 1 .. 8
  int64_t strip_off;        // first byte of the hit's strip: (q_end - 1) rows of 256 cls bytes (non-local: Q - 3 rows)
};

// hit of the chunk -> its length class (class_list_kernel, score_common.h)
struct DescClass {
  const HitDesc* desc;
  __device__ int operator()(int h) const { return desc[h].cls; }
};

struct AlignArgs {
  const int32_t* list;      // blockIdx.x -> hit of the chunk
  const HitDesc* desc;
  uint8_t* strip;
  int32_t* trav;            // hit h's list in TRAVERSAL order (end -> start) at trav + h * trav_stride * 2
  int trav_stride;
  PairResult* res;          // best = score, n_path, status (what gapped_strings_kernel reads)
  int32_t* same;            // identical aligned residues of the list (calcIdentity's count before its "- 2")
};

// The sweeps' observer: the strip byte of every cell (see the head of search_align.hip), one 32-bit store per lane and group.
// SCORE_BIT: bit 4, which only the local walk reads.
template <bool SCORE_BIT>
struct StripObserver : NoObserver {
  uint8_t* strip; int pitch;                    // row i (2 .. last) at strip + (i - 2) * pitch
  uint32_t w = 0;
  __device__ __forceinline__ void cell(int, int x, int m, int e, int f, int pv, int A, int gmx, int key) {
    uint32_t b = (m >= max(e, f)) ? 0u : (e >= f ? 1u : 2u);
    b |= (pv >= A) ? 4u : 0u;
    b |= (gmx >= key) ? 8u : 0u;
    if (SCORE_BIT) b |= (m > 0) ? 16u : 0u;
    w = (x == 0 ? 0u : w) | (b << (8 * x));
  }
  __device__ __forceinline__ void group(int i, int r) {       // the lane's four columns: 256 contiguous bytes per wave
    (reinterpret_cast<uint32_t*>(strip + (size_t)(i - 2) * pitch) + threadIdx.x)[64 * r] = w;
  }
};

// sweep_global's observer: the strip bytes, and what the final cell's pointer (dpmatrix.h:505-534) needs.
//   row():  of column T-2 the first row k <= Q-3 holding the maximal insertion key D[k][T-2] + gek k (gek = ge, or 0 under a free
//           tail insertion).  Row Q-2 costs nothing and equals the match candidate, which comes first: it never wins and is left out.
//   last(): of row Q-2 the match candidate D[Q-2][T-2] and the best deletion with the smallest column holding it (column T-2
//           costs nothing and ties the match).
template <int R>
struct GlobalObserver : StripObserver<false> {
  const GlobalCols<R>& k;
  int free_del, gek, lastk;                     // lastk = Q - 3
  int ikey = kNegS, irow = 0;                   // irow == 0: no candidate (owning lane only)
  int match = kNegS, dlv = kNegS, dlc = 0;      // after last(): wave-uniform
  __device__ __forceinline__ GlobalObserver(const GlobalCols<R>& k_, int free_del_, int gek_, int lastk_)
      : k(k_), free_del(free_del_), gek(gek_), lastk(lastk_) {}
  __device__ __forceinline__ void row(int i, const int (&d)[R][4], int) {
    const int key = sweep_pick<R>(d, k.rs, k.xs, kNegS) + gek * i;
    const bool up = (int)threadIdx.x == k.ls && i <= lastk && key > ikey;   // strictly greater: the smallest row wins ties
    ikey = up ? key : ikey;
    irow = up ? i : irow;
  }
  __device__ __forceinline__ void last(const int (&d)[R][4]) {
    match = __shfl(sweep_pick<R>(d, k.rs, k.xs, kNegS), k.ls);
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int c = 4 * (int)threadIdx.x + 256 * r + x;
        const int len = k.T - 2 - c;
        const int cost = (len < 1 || free_del) ? 0 : k.gi + k.ge * (len - 1);
        const int v = k.in[r][x] ? d[r][x] - cost : kNegS;
        const bool up = v > dlv;                // the lane's columns ascend
        dlv = up ? v : dlv;
        dlc = up ? c : dlc;
      }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {   // value max, column min
      const int ov = __shfl_xor(dlv, off), oc = __shfl_xor(dlc, off);
      const bool take = ov > dlv || (ov == dlv && oc < dlc);
      dlv = take ? ov : dlv;
      dlc = take ? oc : dlc;
    }
  }
};

// Where the results of one slot go, and how they are written (the same for both routes)
struct AlignOut {
  aln_hit_alignment* out; int32_t* pairs; int32_t pair_stride; char* tlines; char* qlines; int32_t line_stride; int32_t* lengths;
  int worst = ALN_OK;
  void note(int st) { if (st < worst) worst = st; }
  // list: n entries, reversed when flip; line: the slot's two lines of `len` chars (nullptr: none)
  void put(size_t slot, int status, float score, float identity, int n, const int32_t* list, bool flip, int len, const char* tl,
           const char* ql) {
    aln_hit_alignment o = {n, status, score, identity};
    if (pairs && status == ALN_OK) {
      const int m = std::min(n, pair_stride);
      int32_t* dst = pairs + slot * (size_t)pair_stride * 2;
      for (int k = 0; k < m; ++k) {
        const int sk = flip ? n - 1 - k : k;
        dst[2 * k] = list[2 * sk]; dst[2 * k + 1] = list[2 * sk + 1];
      }
      if (n > pair_stride) o.status = ALN_E_OVERFLOW;
    }
    if (tlines) {
      char* t = tlines + slot * (size_t)line_stride; char* q = qlines + slot * (size_t)line_stride;
      int wrote = 0;
      if (status == ALN_OK && len >= line_stride) o.status = ALN_E_OVERFLOW;
      else if (status == ALN_OK && len > 0 && tl) { memcpy(t, tl, (size_t)len); memcpy(q, ql, (size_t)len); wrote = len; }
      t[wrote] = 0; q[wrote] = 0;
      if (lengths) lengths[slot] = wrote;
    }
    out[slot] = o;
    note(o.status);
  }
};

// the checks both entries make before ScoreRun's: the hit list, the record array, K, and the two optional output groups
inline bool align_outputs_ok(int32_t K, const aln_hit* hits, const int32_t* n_hits, const aln_hit_alignment* out, const int32_t* pairs,
                             int32_t pair_stride, const char* tlines, const char* qlines, int32_t line_stride, const int32_t* lengths) {
  if (!hits || !n_hits || !out || K < 1 || K > 1024) return false;
  if (pairs ? pair_stride < 2 : false) return false;
  const bool want_lines = tlines || qlines;
  if (want_lines ? (!tlines || !qlines || line_stride < 1) : lengths != nullptr) return false;
  return true;
}

// search_align_profile.hip: the profile twins of align_local_hit_kernel / align_global_hit_kernel for the n hits of g.list, all of
// length class r (s: ScoreArgs of a profile run, score_profile.hip; qch / tch: the character pools of the query letters and the
// templates on the device, which the identity is counted over), and the classes they are kept for (bit R: class R is fused)
unsigned align_prof_classes(bool local);
void launch_align_hit_prof(int r, bool local, int n, hipStream_t stream, const ScoreArgs& s, const AlignArgs& g, const char* qch,
                           const char* tch, int free_del, int free_ins);

}  // namespace aln
