// search_align.hip — the alignments of search hits, on the device: aln_hits_align (gfx950).
//
// aln_search_topk reports, per hit, the cell the optimal local alignment ends in.  Traceback through the collapsed recurrence of
// score_only.hip needs neither scores nor (prev_q, prev_t) pointers: five bits per cell, all of them comparisons between values
// the row sweep already holds, say which candidate won and where a gap jump lands.  So one wave per hit
//   align_local_hit_kernel<R>   sweeps rows 1 .. q_end (sweep_local, score_sweep.h), writes ONE byte per cell into a
//                               transient strip of its own, walks back from the given end cell through that strip, writes
//                               Optimal's pair list and counts the identities;
//   class_list_kernel           (score_common.h) lists a chunk's hits by template length class R = ceil(T / 256);
//   gapped_strings_kernel       (gapped_strings.hip, unchanged) lays the two lines of every list out.
// No aln_batch, no planes, no find_max.  The strip byte of row i (2 .. q_end), column slot c:
//   bits 0-1  the move INTO cell (i, c+1): 0 match, 1 deletion, 2 insertion — the reference tries match, deletions (k ascending),
//             insertions (k ascending) and a later candidate wins only when strictly greater (dpmatrix.h:607-649): with m, e, f
//             the three maxima, match if m >= max(e, f), else deletion if e >= f, else insertion.  (Candidates are clipped at 0
//             before they are compared; the walk only ever reads the move of a cell whose score is > 0, where the clip is idle.)
//   bit 2     cell (i-1, c) as a deletion source: an earlier column of row i-1 already holds at least its key D + ge k
//             (the sweep's pv >= A).  The smallest k wins ties, so a deletion into (i, j) walks row i-1 leftwards from
//             column j-2 while the bit is set and lands on the first clear one.
//   bit 3     cell (i-1, c) as an insertion source: an earlier row of column c already holds at least its key (gmx_old >= m + ge row);
//             the walk goes upwards in column j-1 from row i-2.
//   bit 4     D[i-1][c] > 0: Optimal's local walk stops BEFORE a cell whose score is <= 0 (optimal.h:100).
// Bits 2-4 of row i describe row i-1, whose values the sweep holds while it computes row i: the last row the walk needs them
// for is q_end - 1.  Rows 1 and columns 1 need no move: their cells point at the origin (dpmatrix.h:579-599).
//   align_global_hit_kernel<R>  the same for the four non-local align types (sweep_global): every row 1 .. Q-2 is swept, since
//                               Optimal starts at (Q-1, T-1); the byte has bits 0-3 only (nothing is clipped, so the move rule is
//                               the reference's at every interior cell, dpmatrix.h:447-486, and no walk stops at a score); the
//                               final cell's pointer (dpmatrix.h:505-534) comes from row Q-2, still in registers, and from what
//                               the row observer kept of column T-2; the walk always runs to a cell of row 1 or column 1, then (0,0).
// Everything the kernels do not take — templates beyond 2048 columns, scoring systems ScoreRun sends through full builds, pairs
// without an interior, a length class an instantiation was not kept for — goes through resident batches inside the call.
// aln_hits_align_profiles is the same call for the hits of a profile search: the same host driver (align_block), the same two
// kernels instantiated for the profile side, and batches built from the profiles' planes for what those do not take.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "search_align.h"

namespace aln {

constexpr size_t kAlignBudget = (size_t)1 << 30;   // bytes of strips (and of lists, and of lines) resident at a time

// Both kernels are templates over the query side (ResidueQuery, ProfileQuery: score_common.h).  qch / tch: the character pools
// of the query letters (which share the queries' offsets) and of the templates on the device.  A profile has no letters, so its
// identity is counted over CHARACTERS — the caller's consensus pool, or the placeholder pool of ScoreRun, against the templates',
// exactly the comparison gapped_strings_kernel makes for the lines; the residue side counts over codes, never reads the pools
// and is passed nullptr.
//
// The VM counter, staged side.  The row loop holds the strip stores (R per row) beside the staging copy, and gfx950 retires
// loads, LDS copies and stores through ONE counter in issue order.  ProfileRows::landed() waits until at most one operation is
// outstanding; it is called right after chunk c + 1 is requested, so chunk c has landed (it is older than everything waited
// for) — and so has every strip store issued so far: once per 8 rows the stores are drained.  That is correct and is what ships:
// a counted wait that leaves the stores in flight was built and measured, and did not separate from this one.
// INVARIANT (ScoreRun::upload_profile_rows): a sweep requests at most rows 0 .. Q + 13 of its profile and the buffer is padded
// for that; the local kernel stops at q_end <= Q - 2.  The last copy requested is never read: it is drained before the walk (and
// before the kernel returns early) so that nothing is in flight into LDS when the wave ends.
template <int R, class Side>
__global__ __launch_bounds__(64) void align_local_hit_kernel(ScoreArgs a, AlignArgs g, const char* __restrict__ qch,
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

  // ---- the walk back (optimal.h:79-105), emitted in traversal order ---------------------------------------------------------
  int32_t* o = g.trav + (size_t)hit * g.trav_stride * 2;
  const int cap = g.trav_stride;
  int n = 0, same = 0;
  auto sink = [&](int k, int q, int t) {
    if (k < cap) {
      o[2 * k] = q; o[2 * k + 1] = t;
      same += (qs[q] == ts[t]) ? 1 : 0;
    }
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

template <int R, class Side>
__global__ __launch_bounds__(64) void align_global_hit_kernel(ScoreArgs a, AlignArgs g, const char* __restrict__ qch,
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
  int32_t* o = g.trav + (size_t)hit * g.trav_stride * 2;
  const int cap = g.trav_stride;
  int n = 0, same = 0;
  auto sink = [&](int k, int q, int t) {
    if (k < cap) {
      o[2 * k] = q; o[2 * k + 1] = t;
      same += (qs[q] == ts[t]) ? 1 : 0;
    }
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

// The batch route over the listed slots: aln_batch_create + aln_batch_dp + aln_batch_optimal / _strings, in the groups
// BatchGroup (score_common.h) cuts under the plane budget.  prof != nullptr: `queries` holds the query
// letters (the consensus pool or the placeholder), `sub` is not read and every batch is built from the planes of its own pairs
// (BatchSim), which its budget counts.  (Declared in search_align.h: search_counts.hip tallies the lists of this route.)
int align_through_batches(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                          const aln_qprofiles* prof, const aln_gap* gap, const std::vector<int32_t>& qi_all,
                          const std::vector<int32_t>& ti_all, const std::vector<size_t>& slot_all, AlignOut& ao) {
  std::vector<int32_t> n, st, pairs, len;
  std::vector<float> sc, ident;
  std::vector<char> tl, ql;
  BatchGroup grp;
  while (grp.next(queries, templates, qi_all.data(), ti_all.data(), qi_all.size(), prof != nullptr)) {
    const size_t g0 = grp.g0;
    const int32_t np = (int32_t)(grp.g1 - g0), stride = (int32_t)std::max<int64_t>(std::min(grp.max_q, grp.max_t) + 3, 4);
    const int32_t ls = (int32_t)(grp.max_sum + 2);
    n.assign((size_t)np, 0); st.assign((size_t)np, 0); pairs.assign((size_t)np * stride * 2, 0);
    sc.assign((size_t)np, 0.f); ident.assign((size_t)np, 0.f); len.assign((size_t)np, 0);
    BatchSim bs;
    bs.set(sub, prof, templates, (size_t)np, qi_all.data() + g0, ti_all.data() + g0);
    aln_batch* bb = nullptr;
    int rc = aln_batch_create(ctx, queries, templates, np, qi_all.data() + g0, ti_all.data() + g0, 0, &bb);
    if (rc == ALN_OK) rc = aln_batch_dp(bb, &bs.sim, gap, ALN_FWD, ALN_DP_AUTO, 0);
    if (rc == ALN_OK) rc = aln_batch_optimal(bb, sc.data(), n.data(), pairs.data(), stride, st.data());
    if (rc == ALN_OK) {
      tl.assign((size_t)np * ls, 0); ql.assign((size_t)np * ls, 0);
      rc = aln_batch_optimal_strings(bb, nullptr, ident.data(), nullptr, tl.data(), ql.data(), ls, len.data());
      if (rc == ALN_E_STARTPAIR) rc = ALN_OK;                 // reported per slot
    }
    if (bb) aln_batch_destroy(bb);
    if (rc != ALN_OK) return rc;
    for (int32_t p = 0; p < np; ++p)
      ao.put(slot_all[g0 + p], st[p], sc[p], ident[p], st[p] == 0 ? n[p] : 0, pairs.data() + (size_t)p * stride * 2, false, len[p],
             tl.data() + (size_t)p * ls, ql.data() + (size_t)p * ls);
  }
  return ALN_OK;
}

// The shared body of aln_hits_align and aln_hits_align_profiles (run: prepared; `queries`: the pool the query letters and
// lengths are read from — run.queries, or the consensus pool of a profile run): the slot checks, the routes, the chunks of
// fused hits, the batches.
static int align_block(ScoreRun& run, const aln_seqs* queries, int32_t K, const aln_hit* hits, const int32_t* n_hits,
                       aln_hit_alignment* out, int32_t* pairs, int32_t pair_stride, char* tlines, char* qlines, int32_t line_stride,
                       int32_t* lengths) {
  aln_ctx* ctx = run.ctx;
  const aln_seqs* templates = run.templates;
  const aln_qprofiles* prof = run.prof;
  const int32_t q_begin = run.q_begin;
  const bool want_lines = tlines || qlines;
  int rc;
  const int rows = run.rows, n_t = run.n_t;
  if (rows == 0) return ALN_OK;
  // a fused hit's strip rows and the most entries its list can have
  auto strip_rows = [&](const HitDesc& d) {
    return run.local ? d.q_end - 1 : (int)(queries->offsets[d.q + 1] - queries->offsets[d.q]) - 3;
  };
  auto list_cap = [&](const HitDesc& d) {
    if (run.local) return std::min(d.q_end, d.t_end) + 3;
    return (int)std::min(queries->offsets[d.q + 1] - queries->offsets[d.q], templates->offsets[d.t + 1] - templates->offsets[d.t]) + 1;
  };

  // one walk: every used slot validated and described for its route (nothing is written before it ends)
  SlotRoutes sr;
  if ((rc = route_slots(run, queries, K, hits, n_hits, sr)) != ALN_OK) return rc;
  std::vector<HitDesc>& fast = sr.fast;
  const std::vector<size_t>& fast_slot = sr.fast_slot;
  const std::vector<int32_t>&bq = sr.bq, &bt = sr.bt;
  const std::vector<size_t>& bslot = sr.bslot;
  ctx->align_routes[0] = (int64_t)fast.size(); ctx->align_routes[1] = (int64_t)bq.size();
  AlignOut ao = {out, pairs, pair_stride, tlines, qlines, line_stride, lengths};
  for (int r = 0; r < rows; ++r)
    for (int k = std::max(n_hits[r], 0); k < K; ++k) {
      const size_t slot = (size_t)r * K + k;
      const aln_hit_alignment zero = {0, 0, 0.0f, 0.0f};
      out[slot] = zero;
      if (tlines) { tlines[slot * (size_t)line_stride] = 0; qlines[slot * (size_t)line_stride] = 0; }
      if (lengths) lengths[slot] = 0;
    }

  // chunks of fused hits: strips, lists and lines each stay below the budget; the hint only asks for fewer
  struct Chunk { size_t h0, n; size_t strip; int trav_stride; int cls_cnt[9]; };
  std::vector<Chunk> chunks;
  {
    const size_t forced = ctx->hints.align_chunk_hits > 0 ? (size_t)ctx->hints.align_chunk_hits : (size_t)-1;
    Chunk c = {0, 0, 0, 4, {0, 0, 0, 0, 0, 0, 0, 0, 0}};
    for (size_t h = 0; h < fast.size(); ++h) {
      HitDesc& d = fast[h];
      const size_t need = (size_t)std::max(strip_rows(d), 1) * 256 * (size_t)d.cls;
      const int ts = std::max(c.trav_stride, list_cap(d));
      const bool full = c.n >= forced || c.strip + need > kAlignBudget || (c.n + 1) * (size_t)ts * 8 > kAlignBudget ||
                        (want_lines && (c.n + 1) * 2 * (size_t)line_stride > kAlignBudget);
      if (c.n > 0 && full) {
        chunks.push_back(c);
        c = {h, 0, 0, 4, {0, 0, 0, 0, 0, 0, 0, 0, 0}};
      }
      d.strip_off = (int64_t)c.strip;
      c.strip += need; c.n++; c.cls_cnt[d.cls]++;
      c.trav_stride = std::max(c.trav_stride, list_cap(d));
    }
    if (c.n > 0) chunks.push_back(c);
  }

  if (!chunks.empty()) {
    size_t max_n = 1, max_strip = 1, max_trav = 1;
    for (const Chunk& c : chunks) {
      max_n = std::max(max_n, c.n); max_strip = std::max(max_strip, c.strip);
      max_trav = std::max(max_trav, c.n * (size_t)c.trav_stride * 2);
    }
    uint8_t* dstrip = nullptr; HitDesc* ddesc = nullptr; int32_t *dlist = nullptr, *dfill = nullptr, *dtrav = nullptr, *dsame = nullptr;
    PairResult* dres = nullptr; PairDesc* dpd = nullptr; StrOut* dso = nullptr; char *dlines = nullptr, *dqch = nullptr, *dtch = nullptr;
    auto cleanup = [&]() {
      hipFree(dstrip); hipFree(ddesc); hipFree(dlist); hipFree(dfill); hipFree(dtrav); hipFree(dsame); hipFree(dres); hipFree(dpd);
      hipFree(dso); hipFree(dlines); hipFree(dqch); hipFree(dtch);
      run.release();
    };
#define STRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { ctx->last_error = std::string(#expr) + ": " + hipGetErrorString(e_); hipStreamSynchronize(ctx->stream); cleanup(); return ALN_E_HIP; } } while (0)
#define RTRY(expr) do { int r_ = (expr); if (r_ != ALN_OK) { hipStreamSynchronize(ctx->stream); cleanup(); return r_; } } while (0)
    // profiles: the device rows of [q_begin, q_end) are uploaded once when they fit the budget, else (or under the hint) every
    // chunk uploads the rows of its own profiles — hits are row-major, so a chunk's rows are one contiguous range
    if (prof)
      run.rows_per_slab = ctx->hints.align_rows_per_chunk != 0 ||
                          ((size_t)(prof->offsets[run.q_end] - prof->offsets[q_begin]) + kProfilePadRows) * 128 > kAlignBudget;
    RTRY(run.upload());
    STRY(hipMalloc((void**)&dstrip, max_strip));
    STRY(hipMalloc((void**)&ddesc, max_n * sizeof(HitDesc)));
    STRY(hipMalloc((void**)&dlist, max_n * 4));
    STRY(hipMalloc((void**)&dfill, 9 * 4));
    STRY(hipMalloc((void**)&dtrav, max_trav * 4));
    STRY(hipMalloc((void**)&dsame, max_n * 4));
    STRY(hipMalloc((void**)&dres, max_n * sizeof(PairResult)));
    std::vector<PairResult> hres(max_n);
    std::vector<int32_t> hsame(max_n), htrav(max_trav);
    std::vector<PairDesc> hpd;
    std::vector<StrOut> hso;
    std::vector<char> hlines;
    if (want_lines || prof) {              // the profile kernels count the identity over the characters
      const size_t nq = (size_t)queries->offsets[queries->n_seqs], nt = (size_t)templates->offsets[n_t];
      STRY(hipMalloc((void**)&dqch, std::max<size_t>(nq, 1)));
      STRY(hipMalloc((void**)&dtch, std::max<size_t>(nt, 1)));
      STRY(hipMemcpyAsync(dqch, queries->residues, nq, hipMemcpyHostToDevice, ctx->stream));
      STRY(hipMemcpyAsync(dtch, templates->residues, nt, hipMemcpyHostToDevice, ctx->stream));
    }
    if (want_lines) {
      STRY(hipMalloc((void**)&dpd, max_n * sizeof(PairDesc)));
      STRY(hipMalloc((void**)&dso, max_n * sizeof(StrOut)));
      STRY(hipMalloc((void**)&dlines, max_n * 2 * (size_t)line_stride));
      hpd.resize(max_n); hso.resize(max_n); hlines.resize(max_n * 2 * (size_t)line_stride);
    }
    for (const Chunk& c : chunks) {
      const int n = (int)c.n;
      ClassOff co = {};
      for (int k = 1; k < 9; ++k) co.off[k] = co.off[k - 1] + c.cls_cnt[k - 1];
      if (prof && run.rows_per_slab) RTRY(run.upload_profile_rows(fast[c.h0].q, fast[c.h0 + c.n - 1].q + 1));
      STRY(hipMemcpyAsync(ddesc, fast.data() + c.h0, (size_t)n * sizeof(HitDesc), hipMemcpyHostToDevice, ctx->stream));
      STRY(hipMemsetAsync(dfill, 0, 9 * 4, ctx->stream));
      const DescClass dc = {ddesc};
      hipLaunchKernelGGL(class_list_kernel<DescClass>, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, dc, n, co, dfill, dlist);
      STRY(hipGetLastError());
      AlignArgs g = {};
      g.desc = ddesc; g.strip = dstrip; g.trav = dtrav; g.trav_stride = c.trav_stride; g.res = dres; g.same = dsame;
      for (int k = 1; k <= 8; ++k) {
        if (c.cls_cnt[k] == 0) continue;
        g.list = dlist + co.off[k];
        auto launch = [&](auto side) {
          typedef decltype(side) Side;
          const dim3 grid(c.cls_cnt[k]), block(64);
          const char *qch = Side::kStaged ? dqch : nullptr, *tch = Side::kStaged ? dtch : nullptr;
          constexpr int kLocalMax = ((Side::kFusedLocal >> 8) & 1u) ? 8 : 7;   // a class the mask leaves out never gets here
          if (run.local)
            dispatch_r<kLocalMax>(k, [&](auto rc) {
              hipLaunchKernelGGL((align_local_hit_kernel<decltype(rc)::value, Side>), grid, block, 0, ctx->stream, run.a, g, qch, tch);
            });
          else
            dispatch_r<8>(k, [&](auto rc) {
              hipLaunchKernelGGL((align_global_hit_kernel<decltype(rc)::value, Side>), grid, block, 0, ctx->stream, run.a, g, qch, tch,
                                 run.free_del, run.free_ins);
            });
        };
        if (prof) launch(ProfileQuery());
        else launch(ResidueQuery());
        STRY(hipGetLastError());
      }
      if (want_lines) {
        for (int h = 0; h < n; ++h) hpd[h] = pair_desc(queries, templates, fast[c.h0 + h].q, fast[c.h0 + h].t);
        STRY(hipMemcpyAsync(dpd, hpd.data(), (size_t)n * sizeof(PairDesc), hipMemcpyHostToDevice, ctx->stream));
        StrParams prm = {c.trav_stride, 1, 0, line_stride};
        RTRY(launch_gapped_strings(ctx, n, dpd, dres, dtrav, dqch, dtch, dlines, dso, prm));
        STRY(hipMemcpyAsync(hso.data(), dso, (size_t)n * sizeof(StrOut), hipMemcpyDeviceToHost, ctx->stream));
        STRY(hipMemcpyAsync(hlines.data(), dlines, (size_t)n * 2 * (size_t)line_stride, hipMemcpyDeviceToHost, ctx->stream));
      }
      STRY(hipMemcpyAsync(hres.data(), dres, (size_t)n * sizeof(PairResult), hipMemcpyDeviceToHost, ctx->stream));
      STRY(hipMemcpyAsync(hsame.data(), dsame, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
      if (pairs) STRY(hipMemcpyAsync(htrav.data(), dtrav, (size_t)n * c.trav_stride * 8, hipMemcpyDeviceToHost, ctx->stream));
      STRY(hipStreamSynchronize(ctx->stream));                 // the host vectors above are read by the copies until here
      for (int h = 0; h < n; ++h) {
        const HitDesc& d = fast[c.h0 + h];
        const int64_t Q = queries->offsets[d.q + 1] - queries->offsets[d.q], T = templates->offsets[d.t + 1] - templates->offsets[d.t];
        put_fused(ao, fast_slot[c.h0 + h], hres[h], hsame[h], Q, T, htrav.data() + (size_t)h * c.trav_stride * 2,
                  want_lines ? &hso[h] : nullptr, want_lines ? hlines.data() + (size_t)h * 2 * line_stride : nullptr, line_stride);
      }
    }
#undef STRY
#undef RTRY
    cleanup();
  }
  if (!bq.empty()) {
    rc = align_through_batches(ctx, queries, templates, run.sub, prof, run.gap, bq, bt, bslot, ao);
    if (rc != ALN_OK) return rc;
  }
  return ao.worst;
}

}  // namespace aln

using namespace aln;

extern "C" int aln_hits_align(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                              const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K, const aln_hit* hits,
                              const int32_t* n_hits, aln_hit_alignment* out, int32_t* pairs, int32_t pair_stride, char* tlines,
                              char* qlines, int32_t line_stride, int32_t* lengths) {
  if (ctx) ctx->align_routes[0] = ctx->align_routes[1] = 0;
  if (!align_outputs_ok(K, hits, n_hits, out, pairs, pair_stride, tlines, qlines, line_stride, lengths)) return ALN_E_ARG;
  ScoreRun run;
  int rc = run.prepare(ctx, queries, templates, sub, gap, q_begin, q_end);
  if (rc != ALN_OK) return rc;
  return align_block(run, run.queries, K, hits, n_hits, out, pairs, pair_stride, tlines, qlines, line_stride, lengths);
}

// The same for the hits of a profile search.  The query letters — the lines and the identity need them, the scores never do —
// are the caller's consensus pool or, without one, the placeholder pool the run builds for profiles.
extern "C" int aln_hits_align_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus,
                                       const aln_seqs* templates, const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                                       const aln_hit* hits, const int32_t* n_hits, aln_hit_alignment* out, int32_t* pairs,
                                       int32_t pair_stride, char* tlines, char* qlines, int32_t line_stride, int32_t* lengths) {
  if (ctx) ctx->align_routes[0] = ctx->align_routes[1] = 0;
  if (!profiles || !templates || !gap) return ALN_E_ARG;
  if (!align_outputs_ok(K, hits, n_hits, out, pairs, pair_stride, tlines, qlines, line_stride, lengths)) return ALN_E_ARG;
  ScoreRun run;
  run.consensus = consensus;
  int rc = run.prepare(ctx, nullptr, templates, nullptr, gap, q_begin, q_end, profiles);
  if (rc != ALN_OK) return rc;
  return align_block(run, consensus ? consensus : run.queries, K, hits, n_hits, out, pairs, pair_stride, tlines, qlines,
                     line_stride, lengths);
}

extern "C" int aln_hits_align_last_routes(const aln_ctx* ctx, int64_t out[2]) {
  if (!ctx || !out) return ALN_E_ARG;
  out[0] = ctx->align_routes[0]; out[1] = ctx->align_routes[1];
  return ALN_OK;
}
