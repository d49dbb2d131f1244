// score_common.h — what the all-vs-all score kernels (score_only.hip) and the entries built on them (search_topk.hip,
// search_zscore.hip, search_align.hip, search_counts.hip) share beside the row sweep itself (score_sweep.h): the kernels'
// argument block, the query side a kernel is instantiated for (residues scored through the table, or position-specific rows),
// how work is listed and launched by template length class (ClassOff, class_list_kernel, launch_classes), ScoreRun, the host
// side of one all-vs-all scoring call cut into steps so that a caller can leave the scores of a slab of query rows in a device
// buffer of its own, and what every driver of the family leaves through and owns its device buffers with (STRY / RTRY, DeviceBufs).
#pragma once
#include <algorithm>
#include <deque>
#include <string>
#include <type_traits>
#include <vector>

#include "score_sweep.h"

namespace aln {

struct ScoreArgs {
  const uint8_t* qcodes; const int64_t* qoff;   // query pool, offsets (n_q + 1); profile kernels: the device rows, 128 bytes each,
                                                // biased so that pool row r starts at qcodes + 128 r, and offsets in rows
  const uint8_t* tcodes; const int64_t* toff;   // template pool
  const int32_t* table32;                       // 32 x 32
  const int32_t* tsel;                          // blockIdx.x -> template index (templates are launched by length class)
  const int32_t* qsel;                          // packed kernel: query rows of the slab sorted by length (neighbours share a wave)
  float* scores;                                // rows x n_t
  int q_begin, n_t;
  int gi, ge;
};

// ---- the query side ------------------------------------------------------------------------------------------------------------
// A position-specific query (aln_qprofiles) says, for every query position, what each template letter scores there: S[i][j] =
// rows[i][letter of t[j]].  The sweeps read a row's similarities as 32 ints in LDS indexed by the template's code; for a residue
// query that vector is the table row of the query's letter, for a profile it is row i of the profile itself.  So every kernel
// around a sweep is ONE template over the query side, which says where the rows come from and nothing else:
//   Rows          the sweep's row source (score_sweep.h)
//   stage()       what the kernel's 4 KiB of LDS (__shared__ __attribute__((aligned(16))) int lds[32 * 32]) holds before the sweep
//   rows()        the global pointer handed to the sweep for query qi
//   kStaged       the side copies rows into LDS asynchronously while the sweep runs: a kernel must drain the last copy before
//                 its wave ends, and such a query has no letters of its own (the identity is counted over characters)
//   letters()     of a pool's codes and its characters, the one an alignment's identity is counted over (search_align.hip)
//   kFusedLocal / kFusedGlobal   bit R set: class R runs in hit_local_kernel<R> / hit_global_kernel<R> (search_align.h), under
//                 ListJob (search_align.hip), CountJob (search_counts.hip) and PileupJob (search_pileup.hip)
//   kFusedMulti   bit R set: class R runs in align_local_multi_kernel<R> (search_align_multi.hip)
// The row arrays never leave the kernel and the sweeps' text does not change with the side.
struct ResidueQuery {
  typedef TableRows Rows;
  static constexpr bool kStaged = false;
  // R = 8 of the local kernel is not kept for this side, so that class goes the batch route.  It was dropped for 24 VGPRs
  // spilled into AGPRs; as the kernel stands today it would compile to 237 VGPRs and none (4.8j has the
  // figures).  The mask is a route, and changing a route is a change of behaviour of its own.
  static constexpr unsigned kFusedLocal = 0x0FEu, kFusedGlobal = 0x1FEu;
  static constexpr unsigned kFusedMulti = 0x0FEu;                                       // R = 8 spills 12 VGPRs
  static __device__ __forceinline__ void stage(int* lds, const ScoreArgs& a) {          // the 32 x 32 table
    for (int k = threadIdx.x; k < 32 * 32; k += 64) lds[k] = a.table32[k];
    __syncthreads();
  }
  static __device__ __forceinline__ const uint8_t* rows(const ScoreArgs& a, int qi) { return a.qcodes + a.qoff[qi]; }
  static __device__ __forceinline__ const uint8_t* letters(const uint8_t* codes, const char*) { return codes; }
};
// ScoreArgs of a profile run: qcodes is the device rows as bytes, biased so that pool row r starts at qcodes + 128 r; qoff counts
// ROWS; table32 and qsel are unused.  The LDS is ProfileRows' ring of 32 rows, 8 rows (1 KiB) per copy, one copy ahead of the sweep.
struct ProfileQuery {
  typedef ProfileRows Rows;
  static constexpr bool kStaged = true;
  static constexpr unsigned kFusedLocal = 0x1FEu, kFusedGlobal = 0x1FEu;                // no scratch, no VGPR spill
  static constexpr unsigned kFusedMulti = 0x0FEu;                                       // R = 8 spills 20 VGPRs
  static __device__ __forceinline__ void stage(int*, const ScoreArgs&) {}
  static __device__ __forceinline__ const int4* rows(const ScoreArgs& a, int qi) {
    return reinterpret_cast<const int4*>(a.qcodes + a.qoff[qi] * 128);
  }
  static __device__ __forceinline__ const char* letters(const uint8_t*, const char* chars) { return chars; }
};

// A template of T <= 2048 columns is of length class R = ceil(T / 256): the groups of 256 columns a wave sweeps.
// dispatch_r calls f(std::integral_constant<int, R>) for the runtime class r (1 .. RMAX; a larger r takes RMAX).
template <int RMAX, class F>
inline void dispatch_r(int r, F&& f) {
  if constexpr (RMAX > 1) {
    if (r < RMAX) return dispatch_r<RMAX - 1>(r, f);
  }
  f(std::integral_constant<int, RMAX>());
}

struct ClassOff {
  int off[9];
  // a list that holds cnt[c] slots of class c, class by class: class c starts at off[c]
  static ClassOff of(const int (&cnt)[9]) {
    ClassOff co = {};
    for (int k = 1; k < 9; ++k) co.off[k] = co.off[k - 1] + cnt[k - 1];
    return co;
  }
};

// One launch per length class present (cnt[1 .. 8]; class 0 is the full-build route's and never launched here): calls
// f(side, std::integral_constant<int, R>(), cnt[R], ClassOff::of(cnt).off[R]) — side: ProfileQuery() or ResidueQuery() — which
// launches the caller's kernel<R, Side> over the class's part of the list, and stops at the first launch that failed.
template <class F>
inline hipError_t launch_classes(bool profiles, const int (&cnt)[9], F&& f) {
  const ClassOff co = ClassOff::of(cnt);
  for (int k = 1; k <= 8; ++k) {
    if (cnt[k] == 0) continue;
    dispatch_r<8>(k, [&](auto rc) {
      if (profiles) f(ProfileQuery(), rc, cnt[k], co.off[k]);
      else f(ResidueQuery(), rc, cnt[k], co.off[k]);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// list[off[c] ..) = the slots h < n_slots with cls(h) == c (cls(h) < 0: unused slot), in no particular order; fill[9] starts at 0
template <class ClassOf>
__global__ __launch_bounds__(256) void class_list_kernel(ClassOf cls_of, int n_slots, ClassOff co, int32_t* fill, int32_t* list) {
  __shared__ int lc[9], lb[9];
  const int tid = threadIdx.x;
  const int h = blockIdx.x * 256 + tid;
  if (tid < 9) lc[tid] = 0;
  __syncthreads();
  int cls = -1, my = 0;
  if (h < n_slots) {
    cls = cls_of(h);
    if (cls >= 0) my = atomicAdd(&lc[cls], 1);
  }
  __syncthreads();
  if (tid < 9 && lc[tid]) lb[tid] = co.off[tid] + atomicAdd(&fill[tid], lc[tid]);
  __syncthreads();
  if (cls >= 0) list[lb[cls] + my] = h;
}

// What Optimal::find_max (optimal.h:108-124) needs of a local sweep (score_local_end_kernel, search_topk.hip, tells how it is
// reduced): per lane the row at which the running maximum last strictly improved and — inside that rare branch — the smallest
// of the lane's columns holding it.
struct FirstMaxObserver : NoObserver {
  int seen = 0, lrow = 0, lcol = 0;
  // the lane's maximum rose in row i exactly when row i's maximum exceeds the old one, and then equals it
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

// One all-vs-all scoring call (the arguments of aln_score_all_vs_all): prepare() checks them and decides the route, upload()
// puts what the register-resident kernels read on the device, launch() enqueues those kernels for a block of query rows
// into a device buffer of the caller.  Nothing here synchronises but an error exit (STRY / RTRY below, which leave the device
// state to release()'s later callers); the object must outlive the stream work it enqueued.
// The query side is either a residue pool scored through `sub` or a pool of position-specific profiles (aln_qprofiles: `prof`
// set, no `sub`).  For profiles `queries` is a placeholder pool the run makes itself — the profiles' offsets, every interior
// residue alphabet[0] — so that lengths are read in one place and the full-build route has residues to create batches with.
struct ScoreRun {
  enum Route { kNothing, kAllFull, kFast };
  aln_ctx* ctx = nullptr;
  const aln_seqs* queries = nullptr; const aln_seqs* templates = nullptr;
  const aln_submatrix* sub = nullptr; const aln_gap* gap = nullptr;
  const aln_qprofiles* prof = nullptr;          // the query side is profiles
  std::string ph_res; aln_seqs ph = {};         // ... and their placeholder pool
  const aln_seqs* consensus = nullptr;          // profiles, set before prepare(): a pool of query letters that must share the
                                                // profiles' offsets (aln_hits_align_profiles); checked, never encoded or scored
  const aln_qgaps* qgaps = nullptr;             // profiles, set before prepare(): the rows carry their own gap penalties
  int32_t qgaps_align_type = 0;                 // (aln_score_profiles_gaps_vs_all).  prepare() then takes no `gap` but this align
                                                // type, runs that entry's checks in its order, and the route is kFast or an error:
                                                // never kAllFull, never long_t
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
  int32_t* dprows = nullptr; size_t dprows_bytes = 0;   // profiles: the resident rows, 32 int32 each (upload_profile_rows)
  std::vector<int32_t> hrows;                   // ... their host image, alive until the caller has synchronised
  bool rows_per_slab = false;                   // profiles: launch() uploads the rows of its own block (set before upload())
  std::deque<std::vector<int32_t>> qorders;     // the packed kernel's length orders: alive until the caller has synchronised

  // the argument checks of aln_score_all_vs_all, in its order; ALN_OK with route == kNothing: no pair to score
  // (profiles: queries and sub NULL; the checks of aln_score_profiles_vs_all, in its order, the consensus pool's directly
  // after the descriptor's)
  int prepare(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub, const aln_gap* gap,
              int32_t q_begin, int32_t q_end, const aln_qprofiles* prof = nullptr);
  int upload_offsets();                         // qoff / toff only (all a caller of the kAllFull route needs on the device)
  int upload();                                 // kFast: residue codes (or profile rows), offsets, table, class order
  int upload_profile_rows(int32_t qa, int32_t qb);   // kFast, profiles: the rows of profiles [qa, qb) become the resident ones
  // kFast: scores of query rows [q_begin + row0, q_begin + row0 + nr) against the templates of `order` -> dscores[nr x n_t]
  int launch(int row0, int nr, float* dscores);
  void release();                               // idempotent
  ~ScoreRun() { release(); }
};

// The family's one error exit.  Both leave the enclosing function (`ctx` in scope: a local, or ScoreRun's member) only after
// the stream has been synchronised, so whatever an owner frees afterwards — a DeviceBufs of that function or of its caller,
// ScoreRun's destructor — is never freed under work in flight, as long as every exit past the first enqueue goes through
// them.  Every .hip file that sees them #undefs both at its end.
#define STRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { ctx->last_error = std::string(#expr) + ": " + hipGetErrorString(e_); hipStreamSynchronize(ctx->stream); return ALN_E_HIP; } } while (0)
#define RTRY(expr) do { int r_ = (expr); if (r_ != ALN_OK) { hipStreamSynchronize(ctx->stream); return r_; } } while (0)

// Device buffers with an owner: freed, and the run's device state released, when it goes out of scope
struct DeviceBufs {
  ScoreRun& run;
  std::vector<void*> owned;
  explicit DeviceBufs(ScoreRun& r) : run(r) {}
  DeviceBufs(const DeviceBufs&) = delete;
  ~DeviceBufs() { for (void* p : owned) hipFree(p); run.release(); }
  template <class T>
  hipError_t get(T*& p, size_t count) {
    const hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e == hipSuccess) owned.push_back(p);
    return e;
  }
};

// The kernels of a run with gap rows (search_qgaps.hip), length class r = 1 .. 8: the scores of a grid of (template, query row)
// pairs — local, or one of the four other align types — and the end cells of `cnt` listed local hits.  Enqueue only; the caller
// reads hipGetLastError (launch_classes does).
void launch_qgaps_score(int r, bool local, dim3 grid, hipStream_t stream, const ScoreArgs& s, int free_del, int free_ins);
void launch_qgaps_end(int r, int cnt, hipStream_t stream, const ScoreArgs& s, const int32_t* list, aln_hit* hits, int K);

// scores[(q - q_begin) * ld + col[t]] for the templates of `tlist` through resident batches of full builds
// (col == nullptr: column t, ld == 0: n_t — the layout of aln_score_all_vs_all's result).  prof != nullptr: `queries` is the
// profiles' placeholder pool, `sub` is not read and every batch is built from ALN_SIM_MATRIX planes expanded on the host.
int score_through_batches(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                          const aln_gap* gap, int32_t q_begin, int32_t q_end, const std::vector<int32_t>& tlist, float* scores,
                          const int32_t* col = nullptr, size_t ld = 0, const aln_qprofiles* prof = nullptr);

// The similarity source of one resident batch of the full-build route: the table, or (prof != nullptr) the Q x T planes of the
// batch's pairs expanded on the host — S[i][j] = rows[(off + i) * n + index(t[j])] inside, 0 on the sentinel rows and columns.
// The object owns the planes and must outlive the aln_batch_dp call that reads `sim`.
struct BatchSim {
  aln_sim sim = aln_sim();
  std::vector<float> planes; std::vector<int64_t> plane_off;
  void set(const aln_submatrix* sub, const aln_qprofiles* prof, const aln_seqs* templates, size_t n_pairs, const int32_t* qi,
           const int32_t* ti);
};
// bytes of planes a Q x T pair of such a batch holds on the device (score + pointer planes, padded rows; + the similarity plane)
inline size_t batch_pair_bytes(size_t Q, size_t T, bool with_sim_plane) { return Q * (T + 16) * (with_sim_plane ? 12 : 8); }

constexpr size_t kBatchPlaneBudget = (size_t)12 << 30;   // bytes of planes one resident batch of the full-build route may hold
constexpr size_t kBatchMaxPairs = 65536;                 // ... and the most pairs of a batch cut from a pair list

// Cuts the pair list (qi[k], ti[k]), k < n, into successive resident batches [g0, g1): the first pair is always taken, then the
// group stops before the pair that would exceed the plane budget, or at kBatchMaxPairs.  Start from BatchGroup(); next() is false
// when the list is used up.  max_q, max_t, max_sum: the largest Q, T and Q + T of the group (list and line strides).
struct BatchGroup {
  size_t g0 = 0, g1 = 0;
  int64_t max_q = 0, max_t = 0, max_sum = 0;
  bool next(const aln_seqs* queries, const aln_seqs* templates, const int32_t* qi, const int32_t* ti, size_t n, bool with_sim_plane) {
    g0 = g1; max_q = max_t = max_sum = 0;
    size_t bytes = 0;
    while (g1 < n && g1 - g0 < kBatchMaxPairs) {
      const int64_t Q = queries->offsets[qi[g1] + 1] - queries->offsets[qi[g1]];
      const int64_t T = templates->offsets[ti[g1] + 1] - templates->offsets[ti[g1]];
      const size_t need = batch_pair_bytes((size_t)Q, (size_t)T, with_sim_plane);
      if (g1 > g0 && bytes + need > kBatchPlaneBudget) break;
      bytes += need; max_q = std::max(max_q, Q); max_t = std::max(max_t, T); max_sum = std::max(max_sum, Q + T); ++g1;
    }
    return g1 > g0;
  }
};

}  // namespace aln
