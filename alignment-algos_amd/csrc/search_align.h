// search_align.h — what the fused hit-alignment entries share.  Device: how a hit is described to a kernel (HitDesc), the two
// observers that turn a row sweep into the strip bytes and the final cell's pointer, strip_walk, the walk back through the
// strip, and the ONE pair of kernels around them, hit_local_kernel / hit_global_kernel<R, Side, Job>: what becomes of a walk
// entry is the job's — ListJob here (search_align.hip: the pair list), CountJob in search_counts.h (the column counts),
// PileupJob in search_pileup.h (the query-anchored rows: search_pileup.hip downloads them, search_weights.hip keeps them).
// search_align_multi.hip (several rounds per hit) has a kernel of its own around the same walk.  Host: where a slot's record,
// list and lines go (AlignOut, put_fused, pair_desc), the routing of slots (route_slots) and the fused route's driver that
// the four entries run their chunks through (FusedRoute, over score_common.h's DeviceBufs, STRY / RTRY and launch_classes).
// Around the driver, what the entries over HitDesc share: a hit's strip bytes (hit_strip_bytes), the launch of the kernel pair
// over a job (launch_hit_job), the owner of the per-hit records (HitRecords), the chunks of the entries that list (list_fused_hits), the batch route of the jobs that read pair lists
// on the host (for_list_groups) and what an extern "C" entry does before its body (hit_list_ok, hit_entry).
// The strip byte is defined at the head of search_align.hip.  DESIGN 4.8 found that a helper which takes a kernel's ROW ARRAYS by reference costs
// registers; the walk and the jobs run after the sweep on scalar state only, and sharing them costs none.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

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
template <class Desc>
struct DescClass {
  const Desc* desc;
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

// The job that lists: entry k < cap of the walk into the hit's list, `same` counted over the entries kept.  A job has Args
// (which begin with list, desc, strip and have res, same) and Sink<Letters>: built AFTER the sweep and its fences from the
// argument block and scalars — nothing of a job is live across the sweep, and the kernels' row arrays never reach it —, called
// per entry by exactly one lane, finish() by every lane after the walk, status(n) for the record, `same` for the identity.
struct ListJob {
  typedef AlignArgs Args;
  template <class Letters>
  struct Sink {
    Letters qs, ts;                             // what the identity is counted over
    int32_t* o; int cap;
    int same = 0;
    __device__ __forceinline__ Sink(const Args& g, const ScoreArgs&, int hit, int, Letters qs_, Letters ts_, const uint8_t*, int, int)
        : qs(qs_), ts(ts_), o(g.trav + (size_t)hit * g.trav_stride * 2), cap(g.trav_stride) {}
    __device__ __forceinline__ void operator()(int k, int q, int t) {
      if (k < cap) {
        o[2 * k] = q; o[2 * k + 1] = t;
        same += (qs[q] == ts[t]) ? 1 : 0;
      }
    }
    __device__ __forceinline__ void finish() {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) same += __shfl_xor(same, off);
    }
    __device__ __forceinline__ int status(int n) const { return n <= cap ? 0 : ALN_E_OVERFLOW; }
  };
};

// The two kernels, one wave per hit, templates over the length class, the query side (ResidueQuery, ProfileQuery:
// score_common.h) and the job.  qch / tch: the character pools of the query letters (which share the queries' offsets) and of
// the templates on the device.  A profile has no letters, so its identity is counted over CHARACTERS — the caller's consensus
// pool, or the placeholder pool of ScoreRun, against the templates', exactly the comparison gapped_strings_kernel makes for
// the lines; the residue side counts over codes, never reads the pools and is passed nullptr.
//
// The VM counter, staged side.  The row loop holds the strip stores (R per row) beside the staging copy, and gfx950 retires
// loads, LDS copies and stores through ONE counter in issue order.  ProfileRows::landed() waits until at most one operation is
// outstanding; it is called right after chunk c + 1 is requested, so chunk c has landed (it is older than everything waited
// for) — and so has every strip store issued so far: once per 8 rows the stores are drained.  That is correct and is what ships:
// a counted wait that leaves the stores in flight was built and measured, and did not separate from this one.
// INVARIANT (ScoreRun::upload_profile_rows): a sweep requests at most rows 0 .. Q + 13 of its profile and the buffer is padded
// for that; the local kernel stops at q_end <= Q - 2.  The last copy requested is never read: it is drained before the walk (and
// before the kernel returns early) so that nothing is in flight into LDS when the wave ends.
template <int R, class Side, class Job>
__global__ __launch_bounds__(64) void hit_local_kernel(ScoreArgs a, typename Job::Args g, const char* __restrict__ qch,
                                                      const char* __restrict__ tch) {
  __shared__ __attribute__((aligned(16))) int lds[32 * 32];
  const int lane = threadIdx.x;
  Side::stage(lds, a);
  const int hit = g.list[blockIdx.x];
  const HitDesc hd = g.desc[hit];
  const int ti = hd.t, qi = hd.q, q_end = hd.q_end, t_end = hd.t_end;
  const typename Side::Rows::Src* __restrict__ qr = Side::rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const auto* __restrict__ qs = Side::letters(a.qcodes, qch) + a.qoff[qi];      // what the identity is counted over
  const auto* __restrict__ ts = Side::letters(a.tcodes, tch) + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);
  constexpr int kPitch = 256 * R;
  uint8_t* strip = g.strip + hd.strip_off;      // row i (2 .. q_end) at strip + (i - 2) * kPitch

  // rows 1 .. q_end (1 <= q_end <= Q - 2: the host sends other pairs elsewhere); rows below q_end are not needed
  LocalCols<R> cols;
  cols.load(tc, T, a.gi, a.ge);
  int d[R][4];
  __builtin_assume(q_end >= 1);                 // row 1 always runs, as the host guarantees: no path around it to keep registers for
  StripObserver<true> bytes;
  bytes.strip = strip; bytes.pitch = kPitch;
  sweep_local<R, typename Side::Rows>(lds, cols, qr, q_end, d, bytes);
  if constexpr (Side::kStaged) {
    __threadfence();                                         // the last copy has landed; the walk's lanes read bytes other lanes stored
    __syncthreads();
  }
  // D[q_end][t_end]: row q_end is in d[], column t_end in slot (rs, xs) of lane ls
  const int dend = __shfl(sweep_pick<R>(d, t_end / 256, t_end & 3, 0), (t_end & 255) >> 2);
  PairResult res = {};
  res.best = (float)dend; res.corner = 0.f; res.best_q = q_end; res.best_t = t_end;
  if (!((float)dend == hd.score)) {                          // not the cell the slot's score stands in: refuse the slot
    if (lane == 0) { res.best = 0.f; res.status = ALN_E_ARG; res.n_path = 0; g.res[hit] = res; g.same[hit] = 0; }
    return;
  }
  if constexpr (!Side::kStaged) {
    __threadfence();                                         // the walk's lanes read bytes other lanes stored
    __syncthreads();
  }

  // ---- the walk back (optimal.h:79-105), its entries handed to the job in traversal order ------------------------------------
  typename Job::template Sink<decltype(Side::letters(a.tcodes, tch))> sink(g, a, hit, qi, qs, ts, tc, Q, T);
  int n = 0;
  auto emit1 = [&](int q, int t) { if (lane == 0) sink(n, q, t); ++n; };
  emit1(Q - 1, T - 1);
  emit1(q_end, t_end);
  if (strip_walk<kPitch, true>(strip, q_end, t_end, n, sink)) emit1(0, 0);
  sink.finish();
  if (lane == 0) {
    res.n_path = n;
    res.status = sink.status(n);
    g.res[hit] = res;
    g.same[hit] = sink.same;
  }
}

// The same for the four non-local align types (sweep_global): every row 1 .. Q-2 is swept, and the walk starts at the cell
// the final cell's pointer names.
template <int R, class Side, class Job>
__global__ __launch_bounds__(64) void hit_global_kernel(ScoreArgs a, typename Job::Args g, const char* __restrict__ qch,
                                                       const char* __restrict__ tch, int free_del, int free_ins) {
  __shared__ __attribute__((aligned(16))) int lds[32 * 32];
  const int lane = threadIdx.x;
  Side::stage(lds, a);
  const int hit = g.list[blockIdx.x];
  const HitDesc hd = g.desc[hit];
  const int ti = hd.t, qi = hd.q;
  const typename Side::Rows::Src* __restrict__ qr = Side::rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const auto* __restrict__ qs = Side::letters(a.qcodes, qch) + a.qoff[qi];      // what the identity is counted over
  const auto* __restrict__ ts = Side::letters(a.tcodes, tch) + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);   // Q >= 3, T >= 3: the host's routing
  const int gi = a.gi, ge = a.ge;
  constexpr int kPitch = 256 * R;
  uint8_t* strip = g.strip + hd.strip_off;      // row i (2 .. Q-2) at strip + (i - 2) * kPitch

  GlobalCols<R> cols;
  cols.load(tc, T, gi, ge);
  GlobalObserver<R> ob(cols, free_del, free_ins ? 0 : ge, Q - 3);
  ob.strip = strip; ob.pitch = kPitch;
  int score = sweep_global<R, typename Side::Rows>(lds, cols, qr, Q, free_del, free_ins, ob);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) score = max(score, __shfl_xor(score, off));

  int i, j;
  ob.final_cell(free_ins, i, j);
  __threadfence();                                           // (staged side: the last copy has landed;) the walk's lanes read bytes other lanes stored
  __syncthreads();

  // ---- the walk back (optimal.h:56-74): it always runs to a cell of row 1 or column 1, which points at (0,0) -------------------
  typename Job::template Sink<decltype(Side::letters(a.tcodes, tch))> sink(g, a, hit, qi, qs, ts, tc, Q, T);
  int n = 0;
  auto emit1 = [&](int q, int t) { if (lane == 0) sink(n, q, t); ++n; };
  emit1(Q - 1, T - 1);
  emit1(i, j);
  strip_walk<kPitch, false>(strip, i, j, n, sink);
  emit1(0, 0);
  sink.finish();
  if (lane == 0) {
    PairResult res = {};
    res.best = (float)score; res.corner = 0.f; res.best_q = Q - 1; res.best_t = T - 1;
    res.n_path = n;
    res.status = sink.status(n);
    g.res[hit] = res;
    g.same[hit] = sink.same;
  }
}

// Where the results of one slot go, and how they are written (the same for both routes)
struct AlignOut {
  aln_hit_alignment* out; int32_t* pairs; int32_t pair_stride; char* tlines; char* qlines; int32_t line_stride; int32_t* lengths;
  int worst = ALN_OK;
  void note(int st) { if (st < worst) worst = st; }
  // a slot nothing is reported for: the zero record, empty lines
  void clear(size_t slot) {
    out[slot] = aln_hit_alignment{0, 0, 0.0f, 0.0f};
    if (tlines) { tlines[slot * (size_t)line_stride] = 0; qlines[slot * (size_t)line_stride] = 0; }
    if (lengths) lengths[slot] = 0;
  }
  // ... which the unused slots of a hit list are (n_hits[r] in 0 .. K: route_slots has checked it)
  void clear_unused(int rows, int32_t K, const int32_t* n_hits) {
    for (int r = 0; r < rows; ++r)
      for (int k = n_hits[r]; k < K; ++k) clear((size_t)r * K + k);
  }
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

// the length classes hit_local_kernel / hit_global_kernel are kept for on the run's side
inline unsigned hit_kernel_classes(const ScoreRun& run) {
  return run.prof ? (run.local ? ProfileQuery::kFusedLocal : ProfileQuery::kFusedGlobal)
                  : (run.local ? ResidueQuery::kFusedLocal : ResidueQuery::kFusedGlobal);
}

// One walk over hits[rows x K] of a prepared run (`queries`: the pool lengths are read from): every n_hits[r] in 0..K, every
// used slot's t in range and, with end_cell, its end cell in range, else ALN_E_ARG; each slot described for its route.  The
// fused route takes integer scoring (ScoreRun::kFast), pairs with an interior, templates of up to 2048 columns and the length
// classes of fused_classes, the caller's kernels' mask — every kept instantiation compiles without scratch memory and
// without VGPR spills; hint align_fused_nonlocal = 0 keeps the non-local types out of it.  end_cell: the kernels take the
// slot's end cell and score (hit_local_kernel); without it they are neither read nor checked.  Writes nothing but `sr`.
inline int route_slots(const ScoreRun& run, const aln_seqs* queries, int32_t K, const aln_hit* hits, const int32_t* n_hits,
                       unsigned fused_classes, bool end_cell, SlotRoutes& sr) {
  const aln_seqs* templates = run.templates;
  const bool fused_ok = run.route == ScoreRun::kFast && (run.local || run.ctx->hints.align_fused_nonlocal);
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
      if (end_cell && interior && (h.q_end < 1 || h.q_end > Q - 2 || h.t_end < 1 || h.t_end > T - 2)) return ALN_E_ARG;
      const int cls = (int)((T + 255) / 256);
      if (fused_ok && interior && T <= 2048 && ((fused_classes >> cls) & 1u)) {
        HitDesc d = {q, h.t, 0, 0, 0.f, cls, 0};                 // !end_cell: the slot's end cell and score are ignored
        if (end_cell) { d.q_end = h.q_end; d.t_end = h.t_end; d.score = h.score; }
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

// the check every entry makes before ScoreRun's: the hit list, the record array, K
inline bool hit_list_ok(int32_t K, const aln_hit* hits, const int32_t* n_hits, const aln_hit_alignment* out) {
  return hits && n_hits && out && K >= 1 && K <= 1024;
}
// ... and with it the two optional output groups of the entries that list
inline bool align_outputs_ok(int32_t K, const aln_hit* hits, const int32_t* n_hits, const aln_hit_alignment* out, const int32_t* pairs,
                             int32_t pair_stride, const char* tlines, const char* qlines, int32_t line_stride, const int32_t* lengths) {
  if (!hit_list_ok(K, hits, n_hits, out)) return false;
  if (pairs ? pair_stride < 2 : false) return false;
  const bool want_lines = tlines || qlines;
  if (want_lines ? (!tlines || !qlines || line_stride < 1) : lengths != nullptr) return false;
  return true;
}

// ---- the fused route's driver: what aln_hits_align, aln_hits_align_multi, aln_hits_column_counts and aln_hits_pileup run their
// chunks through ----
constexpr size_t kFusedBudget = (size_t)1 << 30;   // bytes of strips (of masks, of lists, of lines) resident at a time

// (The error exits STRY / RTRY and the buffer owner DeviceBufs: score_common.h.)
struct HitNeed { size_t strip, mask; int cap; };   // of one hit: strip bytes, words of a forbidden-cell plane (0: none), most list entries
struct FusedChunk { size_t h0, n, strip, mask; int trav_stride; int cls_cnt[9]; };   // hits [h0, h0 + n) and what they need together
inline void place(HitDesc& d, size_t strip, size_t) { d.strip_off = (int64_t)strip; }

// The fused hits of one call (Desc: HitDesc, MultiDesc), cut into chunks, and the device state every entry's chunks need.  The
// caller gets its own buffers from `bufs`, and between stage() and launch() enqueues what else its kernels read.
template <class Desc>
struct FusedRoute {
  ScoreRun& run; const aln_seqs* queries; std::vector<Desc>& fast;
  std::vector<FusedChunk> chunks;
  size_t max_n = 1, max_strip = 1, max_mask = 1, max_trav = 1;   // the maxima over the chunks, which size the buffers
  DeviceBufs bufs;
  uint8_t* dstrip = nullptr; Desc* ddesc = nullptr; int32_t *dlist = nullptr, *dfill = nullptr; char *dqch = nullptr, *dtch = nullptr;
  FusedRoute(ScoreRun& r, const aln_seqs* q, std::vector<Desc>& f) : run(r), queries(q), fast(f), bufs(r) {}

  // Every hit has N lists (0: none) of up to need(d).cap entries and, want_lines, N pairs of lines: strips, masks, lists and
  // lines each stay below the budget; hint align_chunk_hits only asks for fewer hits.  Sets the hits' offsets into the chunk.
  template <class Need>
  void cut(int N, bool want_lines, int line_stride, Need&& need) {
    const size_t forced = run.ctx->hints.align_chunk_hits > 0 ? (size_t)run.ctx->hints.align_chunk_hits : (size_t)-1;
    auto close = [&](const FusedChunk& c) {
      chunks.push_back(c);
      max_n = std::max(max_n, c.n); max_strip = std::max(max_strip, c.strip); max_mask = std::max(max_mask, c.mask);
      max_trav = std::max(max_trav, c.n * (size_t)N * c.trav_stride * 2);
    };
    FusedChunk c = {0, 0, 0, 0, 4, {}};
    for (size_t h = 0; h < fast.size(); ++h) {
      const HitNeed nd = need(fast[h]);
      const int ts = std::max(c.trav_stride, nd.cap);
      const bool full = c.n >= forced || c.strip + nd.strip > kFusedBudget || (c.mask + nd.mask) * 4 > kFusedBudget ||
                        (c.n + 1) * (size_t)N * ts * 8 > kFusedBudget ||
                        (want_lines && (c.n + 1) * (size_t)N * 2 * (size_t)line_stride > kFusedBudget);
      if (c.n > 0 && full) {
        close(c);
        c = {h, 0, 0, 0, 4, {}};
      }
      place(fast[h], c.strip, c.mask);
      c.strip += nd.strip; c.mask += nd.mask; c.n++; c.cls_cnt[fast[h].cls]++;
      c.trav_stride = std::max(c.trav_stride, nd.cap);
    }
    if (c.n > 0) close(c);
  }

  // Profiles: the device rows of [q_begin, q_end) are uploaded once when they fit the budget, else (or under the hint) every
  // chunk uploads the rows of its own profiles — hits are row-major, so a chunk's rows are one contiguous range.
  int begin() {
    aln_ctx* ctx = run.ctx;
    if (run.prof)
      run.rows_per_slab = ctx->hints.align_rows_per_chunk != 0 ||
                          ((size_t)(run.prof->offsets[run.q_end] - run.prof->offsets[run.q_begin]) + kProfilePadRows) * 128 > kFusedBudget;
    RTRY(run.upload());
    STRY(bufs.get(dstrip, max_strip));
    STRY(bufs.get(ddesc, max_n));
    STRY(bufs.get(dlist, max_n));
    STRY(bufs.get(dfill, 9));
    return ALN_OK;
  }
  // The two character pools: what lines are laid out from, and what the profile kernels count the identity over
  int upload_pools() {
    aln_ctx* ctx = run.ctx;
    const size_t nq = (size_t)queries->offsets[queries->n_seqs], nt = (size_t)run.templates->offsets[run.n_t];
    STRY(bufs.get(dqch, std::max<size_t>(nq, 1)));
    STRY(bufs.get(dtch, std::max<size_t>(nt, 1)));
    STRY(hipMemcpyAsync(dqch, queries->residues, nq, hipMemcpyHostToDevice, ctx->stream));
    STRY(hipMemcpyAsync(dtch, run.templates->residues, nt, hipMemcpyHostToDevice, ctx->stream));
    return ALN_OK;
  }
  // The chunk's profile rows (where they go per chunk) and descriptors, then also(), the caller's own uploads that stand
  // here in the stream's order, then `fill` zeroed for class_list_kernel
  template <class Also>
  int stage(const FusedChunk& c, Also&& also) {
    aln_ctx* ctx = run.ctx;
    if (run.prof && run.rows_per_slab) RTRY(run.upload_profile_rows(fast[c.h0].q, fast[c.h0 + c.n - 1].q + 1));
    STRY(hipMemcpyAsync(ddesc, fast.data() + c.h0, c.n * sizeof(Desc), hipMemcpyHostToDevice, ctx->stream));
    RTRY(also());
    STRY(hipMemsetAsync(dfill, 0, 9 * 4, ctx->stream));
    return ALN_OK;
  }
  int stage(const FusedChunk& c) { return stage(c, [] { return (int)ALN_OK; }); }

  // The chunk's hits listed by class, then (launch_classes) per class present kernel(side, k, hits of the class, their list,
  // qch, tch): the caller's kernel<R = k, Side> over that list — k at run time, because the callers' class masks decide which
  // R they instantiate; the residue side never reads the pools and is passed nullptr.
  template <class Launch>
  int launch(const FusedChunk& c, Launch&& kernel) {
    aln_ctx* ctx = run.ctx;
    const int n = (int)c.n;
    const DescClass<Desc> dc = {ddesc};
    hipLaunchKernelGGL(class_list_kernel<DescClass<Desc>>, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, dc, n, ClassOff::of(c.cls_cnt), dfill, dlist);
    STRY(hipGetLastError());
    STRY(launch_classes(run.prof != nullptr, c.cls_cnt, [&](auto side, auto rc, int cnt, int off) {
      kernel(side, (int)decltype(rc)::value, cnt, dlist + off, run.prof ? dqch : nullptr, run.prof ? dtch : nullptr);
    }));
    return ALN_OK;
  }
};

// ---- what the entries over HitDesc — aln_hits_align, aln_hits_column_counts, aln_hits_pileup — share around the driver ----

// The strip of a fused hit (HitDesc::strip_off), for cut(): rows 2 .. q_end of a local sweep, rows 2 .. Q-2 of the others
inline size_t hit_strip_bytes(const ScoreRun& run, const aln_seqs* queries, const HitDesc& d) {
  const int rows = run.local ? d.q_end - 1 : (int)(queries->offsets[d.q + 1] - queries->offsets[d.q]) - 3;
  return (size_t)std::max(rows, 1) * 256 * (size_t)d.cls;
}

// One chunk through the kernel pair over a job: per class present hit_local_kernel or hit_global_kernel<R, Side, Job>, by the
// run's align type, over the class's part of the list (g.list is set here; the caller fills the rest of g).  A template the
// caller's .hip file instantiates with its own job, so every compile unit emits its own kernels and no others.  Leaves as
// FusedRoute::launch does: an error exit has synchronized the stream.
template <class Job>
int launch_hit_job(FusedRoute<HitDesc>& fr, const FusedChunk& c, typename Job::Args& g) {
  ScoreRun& run = fr.run;
  const hipStream_t stream = run.ctx->stream;
  return fr.launch(c, [&](auto side, int k, int cnt, const int32_t* list, const char* qch, const char* tch) {
    typedef decltype(side) Side;
    const dim3 grid(cnt), block(64);
    g.list = list;
    constexpr int kLocalMax = ((Side::kFusedLocal >> 8) & 1u) ? 8 : 7;   // a class the mask leaves out never gets here
    if (run.local)
      dispatch_r<kLocalMax>(k, [&](auto rc) {
        hipLaunchKernelGGL((hit_local_kernel<decltype(rc)::value, Side, Job>), grid, block, 0, stream, run.a, g, qch, tch);
      });
    else
      dispatch_r<8>(k, [&](auto rc) {
        hipLaunchKernelGGL((hit_global_kernel<decltype(rc)::value, Side, Job>), grid, block, 0, stream, run.a, g, qch, tch,
                           run.free_del, run.free_ins);
      });
  });
}

// The records the kernels leave per hit (per hit and round: aln_hits_align_multi) — res and same of a job's Args — and their
// host images.  The caller enqueues the download where it stands in its chunk and reads the images after its synchronization.
struct HitRecords {
  PairResult* dres = nullptr; int32_t* dsame = nullptr;
  std::vector<PairResult> hres; std::vector<int32_t> hsame;
  int alloc(DeviceBufs& bufs, size_t n) {
    aln_ctx* ctx = bufs.run.ctx;
    STRY(bufs.get(dsame, n));
    STRY(bufs.get(dres, n));
    hres.resize(n); hsame.resize(n);
    return ALN_OK;
  }
  int enqueue_download(aln_ctx* ctx, size_t n) {
    STRY(hipMemcpyAsync(hres.data(), dres, n * sizeof(PairResult), hipMemcpyDeviceToHost, ctx->stream));
    STRY(hipMemcpyAsync(hsame.data(), dsame, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    return ALN_OK;
  }
  // A chunk's records into their slots, for a job without lists and lines; also(h, slot, Q): what else the caller files for
  // hit h of the chunk
  template <class Also>
  void put(AlignOut& ao, const FusedRoute<HitDesc>& fr, const FusedChunk& c, const std::vector<size_t>& fast_slot, Also&& also) const {
    const aln_seqs* queries = fr.queries; const aln_seqs* templates = fr.run.templates;
    for (size_t h = 0; h < c.n; ++h) {
      const HitDesc& d = fr.fast[c.h0 + h];
      const int64_t Q = queries->offsets[d.q + 1] - queries->offsets[d.q], T = templates->offsets[d.t + 1] - templates->offsets[d.t];
      put_fused(ao, fast_slot[c.h0 + h], hres[h], hsame[h], Q, T, nullptr, nullptr, nullptr, 0);
      also(h, fast_slot[c.h0 + h], Q);
    }
  }
};

// The chunks of fused hits of the entries that list (aln_hits_align, aln_hits_align_profiles, aln_hits_align_profiles_gaps):
// one list each, and the two lines where ao wants them; every record is filed through put_fused.  launch(fr, c, g): the
// caller's kernel pair over ListJob for one chunk (launch_hit_job<ListJob>; search_align_qgaps.h: launch_hit_qgaps_job<ListJob>).
template <class Launch>
int list_fused_hits(ScoreRun& run, const aln_seqs* queries, SlotRoutes& sr, AlignOut& ao, Launch&& launch) {
  aln_ctx* ctx = run.ctx;
  const aln_seqs* templates = run.templates;
  std::vector<HitDesc>& fast = sr.fast;
  const std::vector<size_t>& fast_slot = sr.fast_slot;
  const bool want_lines = ao.tlines != nullptr;
  const int32_t line_stride = ao.line_stride;
  // the most entries a fused hit's list can have
  auto list_cap = [&](const HitDesc& d) {
    if (run.local) return std::min(d.q_end, d.t_end) + 3;
    return (int)std::min(queries->offsets[d.q + 1] - queries->offsets[d.q], templates->offsets[d.t + 1] - templates->offsets[d.t]) + 1;
  };
  FusedRoute<HitDesc> fr(run, queries, fast);
  fr.cut(1, want_lines, line_stride, [&](const HitDesc& d) {
    return HitNeed{hit_strip_bytes(run, queries, d), 0, list_cap(d)};
  });
  const size_t max_n = fr.max_n, max_trav = fr.max_trav;
  int32_t* dtrav = nullptr; PairDesc* dpd = nullptr; StrOut* dso = nullptr; char* dlines = nullptr;
  HitRecords rec;
  RTRY(fr.begin());
  STRY(fr.bufs.get(dtrav, max_trav));
  RTRY(rec.alloc(fr.bufs, max_n));
  std::vector<int32_t> htrav(max_trav);
  std::vector<PairDesc> hpd;
  std::vector<StrOut> hso;
  std::vector<char> hlines;
  if (want_lines || run.prof) RTRY(fr.upload_pools());
  if (want_lines) {
    STRY(fr.bufs.get(dpd, max_n));
    STRY(fr.bufs.get(dso, max_n));
    STRY(fr.bufs.get(dlines, max_n * 2 * (size_t)line_stride));
    hpd.resize(max_n); hso.resize(max_n); hlines.resize(max_n * 2 * (size_t)line_stride);
  }
  for (const FusedChunk& c : fr.chunks) {
    const int n = (int)c.n;
    RTRY(fr.stage(c));
    AlignArgs g = {};
    g.desc = fr.ddesc; g.strip = fr.dstrip; g.trav = dtrav; g.trav_stride = c.trav_stride; g.res = rec.dres; g.same = rec.dsame;
    RTRY(launch(fr, c, g));
    if (want_lines) {
      for (int h = 0; h < n; ++h) hpd[h] = pair_desc(queries, templates, fast[c.h0 + h].q, fast[c.h0 + h].t);
      STRY(hipMemcpyAsync(dpd, hpd.data(), (size_t)n * sizeof(PairDesc), hipMemcpyHostToDevice, ctx->stream));
      StrParams prm = {c.trav_stride, 1, 0, line_stride};
      RTRY(launch_gapped_strings(ctx, n, dpd, rec.dres, dtrav, fr.dqch, fr.dtch, dlines, dso, prm));
      STRY(hipMemcpyAsync(hso.data(), dso, (size_t)n * sizeof(StrOut), hipMemcpyDeviceToHost, ctx->stream));
      STRY(hipMemcpyAsync(hlines.data(), dlines, (size_t)n * 2 * (size_t)line_stride, hipMemcpyDeviceToHost, ctx->stream));
    }
    RTRY(rec.enqueue_download(ctx, c.n));
    if (ao.pairs) STRY(hipMemcpyAsync(htrav.data(), dtrav, (size_t)n * c.trav_stride * 8, hipMemcpyDeviceToHost, ctx->stream));
    STRY(hipStreamSynchronize(ctx->stream));                 // the host vectors above are read by the copies until here
    for (int h = 0; h < n; ++h) {
      const HitDesc& d = fast[c.h0 + h];
      const int64_t Q = queries->offsets[d.q + 1] - queries->offsets[d.q], T = templates->offsets[d.t + 1] - templates->offsets[d.t];
      put_fused(ao, fast_slot[c.h0 + h], rec.hres[h], rec.hsame[h], Q, T, htrav.data() + (size_t)h * c.trav_stride * 2,
                want_lines ? &hso[h] : nullptr, want_lines ? hlines.data() + (size_t)h * 2 * line_stride : nullptr, line_stride);
    }
  }
  return ALN_OK;
}

// The batch route of a job that reads pair lists on the host: the slots of sr.bq / bt / bslot go through
// align_through_batches a group at a time, records and lists into buffers of the group — at most kListGroupBytes of lists,
// and hint align_list_group_slots only asks for fewer slots —, the record is filed (ao.out, ao.note) and, unless the slot
// failed or is a local one whose score is not > 0 (the seed cell's list), per_slot(slot, q, t, list, n_pairs) reads the list.
constexpr size_t kListGroupBytes = (size_t)256 << 20;
template <class PerSlot>
int for_list_groups(ScoreRun& run, const aln_seqs* queries, const SlotRoutes& sr, AlignOut& ao, PerSlot&& per_slot) {
  const aln_seqs* templates = run.templates;
  const std::vector<int32_t>&bq = sr.bq, &bt = sr.bt;
  const int hint = run.ctx->hints.align_list_group_slots;
  const size_t forced = hint > 0 ? (size_t)hint : (size_t)-1;
  std::vector<aln_hit_alignment> grec;
  std::vector<int32_t> gpairs, gq, gt;
  std::vector<size_t> gslot;
  for (size_t b0 = 0, b1; b0 < bq.size(); b0 = b1) {
    int64_t stride = 4;
    for (b1 = b0; b1 < bq.size(); ++b1) {
      const int64_t Q = queries->offsets[bq[b1] + 1] - queries->offsets[bq[b1]];
      const int64_t T = templates->offsets[bt[b1] + 1] - templates->offsets[bt[b1]];
      const int64_t s = std::max(stride, std::min(Q, T) + 3);
      if (b1 > b0 && (b1 - b0 >= forced || (b1 + 1 - b0) * (size_t)s * 8 > kListGroupBytes)) break;
      stride = s;
    }
    const size_t nb = b1 - b0;
    grec.assign(nb, aln_hit_alignment{0, 0, 0.0f, 0.0f});
    gpairs.assign(nb * (size_t)stride * 2, 0);
    gq.assign(bq.begin() + b0, bq.begin() + b1); gt.assign(bt.begin() + b0, bt.begin() + b1);
    gslot.resize(nb);
    for (size_t p = 0; p < nb; ++p) gslot[p] = p;
    AlignOut go = {grec.data(), gpairs.data(), (int32_t)stride, nullptr, nullptr, 0, nullptr};
    const int rc = align_through_batches(run.ctx, queries, templates, run.sub, run.prof, run.gap, gq, gt, gslot, go);
    if (rc != ALN_OK) return rc;
    for (size_t p = 0; p < nb; ++p) {
      const aln_hit_alignment& rec = grec[p];
      ao.out[sr.bslot[b0 + p]] = rec;
      ao.note(rec.status);
      if (rec.status != 0 || (run.local && !(rec.score > 0.f))) continue;
      per_slot(sr.bslot[b0 + p], gq[p], gt[p], gpairs.data() + p * (size_t)stride * 2, rec.n_pairs);
    }
  }
  return ALN_OK;
}

// What an extern "C" entry of the family does before its body: align_routes reset; `ok`, the entry's own argument checks
// (they write nothing and come before ScoreRun's); profile_form: the three pointers prepare() would otherwise read; the run
// prepared in the residue form (queries, sub) or the profile form (profiles, consensus).  body(run, pool): pool is what
// query letters and lengths are read from — run.queries, or the consensus pool of a profile run.
template <class Body>
int hit_entry(aln_ctx* ctx, bool profile_form, const aln_seqs* queries, const aln_qprofiles* profiles, const aln_seqs* consensus,
              const aln_seqs* templates, const aln_submatrix* sub, const aln_gap* gap, int32_t q_begin, int32_t q_end, bool ok,
              Body&& body) {
  if (ctx) ctx->align_routes[0] = ctx->align_routes[1] = 0;
  if (!ok || (profile_form && (!profiles || !templates || !gap))) return ALN_E_ARG;
  ScoreRun run;
  run.consensus = consensus;
  const int rc = profile_form ? run.prepare(ctx, nullptr, templates, nullptr, gap, q_begin, q_end, profiles)
                              : run.prepare(ctx, queries, templates, sub, gap, q_begin, q_end);
  if (rc != ALN_OK) return rc;
  return body(run, consensus ? consensus : run.queries);
}

}  // namespace aln
