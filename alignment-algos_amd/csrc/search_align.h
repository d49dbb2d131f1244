// search_align.h — what the fused hit-alignment kernels of search_align.hip (one pair of kernels for residue queries, the
// table in LDS, and for position-specific queries, rows staged into LDS) and search_align_multi.hip (several rounds per
// hit) share: how a hit is described to a kernel, where its results go and how a slot's record, list and lines are written for
// the caller (AlignOut, put_fused, pair_desc), the two observers that turn a row sweep into the strip bytes and the final
// cell's pointer, and strip_walk, the walk back through the strip that all three kernels call — and the two of
// search_counts.hip, which tally the walk's entries instead of listing them.  The strip byte is defined at
// the head of search_align.hip.  DESIGN 4.8 found that a helper which takes a kernel's ROW ARRAYS by reference costs
// registers; the walk runs after the sweep on scalar state only (strip, i, j, n), and sharing it costs none.
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
  // The final cell's pointer (dpmatrix.h:505-534), after the sweep: match, deletions from (Q-2, k) k ascending, insertions from
  // (k, T-2) k ascending; a later candidate wins only when strictly greater.  (i, j): the cell the walk starts from.
  __device__ __forceinline__ void final_cell(int free_ins, int& i, int& j) const {
    const int ir = __shfl(irow, k.ls), ik = __shfl(ikey, k.ls);
    const int ilv = ir == 0 ? kNegS : (free_ins ? ik : ik - (k.gi + k.ge * lastk));
    i = lastk + 1; j = k.T - 2;
    if (dlv > match) j = dlc;
    if (ilv > max(match, dlv)) { i = ir; j = k.T - 2; }
  }
};

// The walk back through a hit's strip (row i, 2 .. last, at strip + (i - 2) * PITCH; the byte: head of search_align.hip) from
// the cell (i, j) the caller has already emitted — optimal.h:79-105 under LOCAL, optimal.h:56-74 otherwise.  Entry k of the
// list, in traversal order (end -> start), is handed to sink(k, q, t) by exactly one lane; n counts the entries.  A cell of
// row 1 or column 1 points at (0,0), whose score is 0 (dpmatrix.h:579-599): the walk ends there and the caller emits (0,0)
// itself where its list has it.  Returns true when a LOCAL walk stopped at a cell with both indices > 0 — Optimal's local
// walk stops BEFORE a cell whose score is <= 0 (optimal.h:100), bit 4 — and (0,0) is prepended.  Every branch is wave-uniform.
template <int PITCH, bool LOCAL, class Sink>
__device__ __forceinline__ bool strip_walk(const uint8_t* strip, int i, int j, int& n, Sink&& sink) {
  const int lane = threadIdx.x;
  auto at = [&](int ii, int c) -> uint32_t { return strip[(size_t)(ii - 2) * PITCH + c]; };
  while (i >= 2 && j >= 2) {
    // lane l looks at cell (i - l, j - l): its byte holds the move into it and (LOCAL) the score bit of its diagonal predecessor
    const int ci = i - lane, cj = j - lane;
    const bool valid = ci >= 2 && cj >= 2;
    const uint32_t b = valid ? at(ci, cj - 1) : 0u;
    const bool go = valid && (b & 3u) == 0u && (!LOCAL || (b & 16u) != 0u);
    const unsigned long long m = __ballot(go);
    const int L = (~m == 0ull) ? 64 : __builtin_ctzll(~m);   // lanes 0 .. L-1 step diagonally (LOCAL: onto a cell that is kept)
    if (lane < L) sink(n + lane, ci - 1, cj - 1);
    n += L; i -= L; j -= L;
    if (L == 64) continue;
    if (i < 2 || j < 2) break;
    const uint32_t mv = (uint32_t)__shfl((int)b, L) & 3u;    // not LOCAL: 1 or 2, lane L is valid and did not go
    if (LOCAL && mv == 0u) return true;                      // a match whose predecessor's score is <= 0 (a forbidden cell among them)
    int pi, pj; uint32_t bp = 0;
    if (mv == 1u) {                                          // deletion: the smallest column of row i-1 holding the maximal key
      pi = i - 1; pj = 0;                                    // (the smallest k wins ties: leftwards from column j-2 while bit 2 is set)
      for (int k0 = j - 2; k0 >= 1; k0 -= 64) {
        const int kk = k0 - lane;
        const uint32_t bb = kk >= 1 ? at(i, kk) : 0u;
        const unsigned long long clr = __ballot((bb & 4u) == 0u);
        if (clr) { const int l0 = __builtin_ctzll(clr); pj = k0 - l0; if (LOCAL) bp = (uint32_t)__shfl((int)bb, l0); break; }
      }
    } else {                                                 // insertion: the smallest row of column j-1 holding the maximal key
      pj = j - 1; pi = 0;                                    // (upwards from row i-2 while bit 3 is set)
      for (int k0 = i - 2; k0 >= 1; k0 -= 64) {
        const int kk = k0 - lane;
        const uint32_t bb = kk >= 1 ? at(kk + 1, pj) : 0u;
        const unsigned long long clr = __ballot((bb & 8u) == 0u);
        if (clr) { const int l0 = __builtin_ctzll(clr); pi = k0 - l0; if (LOCAL) bp = (uint32_t)__shfl((int)bb, l0); break; }
      }
    }
    if (pi < 1 || pj < 1) break;                             // (cannot happen: row 1 and column 1 always clear their bits)
    if (LOCAL && (bp & 16u) == 0u) return true;              // the source's score is <= 0
    if (lane == 0) sink(n, pi, pj);
    ++n;
    i = pi; j = pj;
  }
  return false;
}

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

// One record of a fused kernel -> AlignOut::put.  r, same: what the kernel left; Q, T: the pair's lengths; trav: its list in
// traversal order; so, lines: what gapped_strings_kernel left for it and its two lines of line_stride chars (nullptr: no lines)
inline void put_fused(AlignOut& ao, size_t slot, const PairResult& r, int same, int64_t Q, int64_t T, const int32_t* trav,
                      const StrOut* so, const char* lines, int line_stride) {
  const float ident = r.status == 0 ? float(same - 2) / float(std::min(Q, T) - 2) * 100.f : 0.f;   // alignment.h:864
  int len = 0; const char* tl = nullptr; const char* ql = nullptr; int st = r.status;
  if (so && st == 0) {
    if (so->err == ALN_E_OVERFLOW) len = line_stride;          // put() turns it into the record's status
    else if (so->err != ALN_OK) st = so->err;
    else { len = so->length; tl = lines; ql = tl + line_stride; }
  }
  ao.put(slot, st, r.best, ident, r.n_path, trav, true, len, tl, ql);
}

// what gapped_strings_kernel reads of a pair (q, t) whose list a fused kernel wrote
inline PairDesc pair_desc(const aln_seqs* queries, const aln_seqs* templates, int q, int t) {
  PairDesc pd = {};
  pd.Q = (int32_t)(queries->offsets[q + 1] - queries->offsets[q]);
  pd.T = (int32_t)(templates->offsets[t + 1] - templates->offsets[t]);
  pd.q_seq = q; pd.t_seq = t; pd.q_off = queries->offsets[q]; pd.t_off = templates->offsets[t];
  return pd;
}

// The used slots of a hit list by route: the fused kernels' hits (row-major) and the batch route's pairs, each with its slot
struct SlotRoutes {
  std::vector<HitDesc> fast; std::vector<size_t> fast_slot;
  std::vector<int32_t> bq, bt; std::vector<size_t> bslot;
};

// One walk over hits[rows x K] of a prepared run (`queries`: the pool lengths are read from): every n_hits[r] in 0..K, every
// used slot's t in range and, local, its end cell in range, else ALN_E_ARG; each slot described for its route.  The fused
// route takes integer scoring (ScoreRun::kFast), pairs with an interior, templates of up to 2048 columns and the length
// classes an instantiation is kept for — every kept one compiles without scratch memory and without VGPR spills (the masks
// are the side's); hint align_fused_nonlocal = 0 keeps the non-local types out of it.  Writes nothing but `sr`.
inline int route_slots(const ScoreRun& run, const aln_seqs* queries, int32_t K, const aln_hit* hits, const int32_t* n_hits,
                       SlotRoutes& sr) {
  const aln_seqs* templates = run.templates;
  const bool fused_ok = run.route == ScoreRun::kFast && (run.local || run.ctx->hints.align_fused_nonlocal);
  const unsigned fused_classes = run.prof ? (run.local ? ProfileQuery::kFusedLocal : ProfileQuery::kFusedGlobal)
                                          : (run.local ? ResidueQuery::kFusedLocal : ResidueQuery::kFusedGlobal);
  for (int r = 0; r < run.rows; ++r) {
    if (n_hits[r] < 0 || n_hits[r] > K) return ALN_E_ARG;
    const int q = run.q_begin + r;
    const int64_t Q = queries->offsets[q + 1] - queries->offsets[q];
    for (int k = 0; k < n_hits[r]; ++k) {
      const size_t slot = (size_t)r * K + k;
      const aln_hit& h = hits[slot];
      if (h.t < 0 || h.t >= run.n_t) return ALN_E_ARG;
      const int64_t T = templates->offsets[h.t + 1] - templates->offsets[h.t];
      const bool interior = Q >= 3 && T >= 3;
      if (run.local && interior && (h.q_end < 1 || h.q_end > Q - 2 || h.t_end < 1 || h.t_end > T - 2)) return ALN_E_ARG;
      const int cls = (int)((T + 255) / 256);
      if (fused_ok && interior && T <= 2048 && ((fused_classes >> cls) & 1u)) {
        HitDesc d = {q, h.t, 0, 0, 0.f, cls, 0};                 // non-local: the slot's end cell and score are ignored
        if (run.local) { d.q_end = h.q_end; d.t_end = h.t_end; d.score = h.score; }
        sr.fast.push_back(d); sr.fast_slot.push_back(slot);
      } else { sr.bq.push_back(q); sr.bt.push_back(h.t); sr.bslot.push_back(slot); }
    }
  }
  return ALN_OK;
}

// The batch route of hit alignment (search_align.hip): slot_all[k] of pair (qi_all[k], ti_all[k]) is where ao.put() files it
int align_through_batches(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                          const aln_qprofiles* prof, const aln_gap* gap, const std::vector<int32_t>& qi_all,
                          const std::vector<int32_t>& ti_all, const std::vector<size_t>& slot_all, AlignOut& ao);

// the checks both entries make before ScoreRun's: the hit list, the record array, K, and the two optional output groups
inline bool align_outputs_ok(int32_t K, const aln_hit* hits, const int32_t* n_hits, const aln_hit_alignment* out, const int32_t* pairs,
                             int32_t pair_stride, const char* tlines, const char* qlines, int32_t line_stride, const int32_t* lengths) {
  if (!hits || !n_hits || !out || K < 1 || K > 1024) return false;
  if (pairs ? pair_stride < 2 : false) return false;
  const bool want_lines = tlines || qlines;
  if (want_lines ? (!tlines || !qlines || line_stride < 1) : lengths != nullptr) return false;
  return true;
}

}  // namespace aln
