// search_align.hip — the alignments of search hits, on the device: aln_hits_align (gfx950).
//
// aln_search_topk reports, per hit, the cell the optimal local alignment ends in.  Traceback through the collapsed recurrence of
// score_only.hip needs neither scores nor (prev_q, prev_t) pointers: five bits per cell, all of them comparisons between values
// the row sweep already holds, say which candidate won and where a gap jump lands.  So one wave per hit
//   hit_local_kernel<R, Side, ListJob>   (search_align.h) sweeps rows 1 .. q_end (sweep_local, score_sweep.h), writes ONE byte per cell into a
//                               transient strip of its own, walks back from the given end cell through that strip and hands
//                               every entry to its job: ListJob writes Optimal's pair list and counts the identities;
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
//   hit_global_kernel<R, Side, ListJob>  the same for the four non-local align types (sweep_global): every row 1 .. Q-2 is swept, since
//                               Optimal starts at (Q-1, T-1); the byte has bits 0-3 only (nothing is clipped, so the move rule is
//                               the reference's at every interior cell, dpmatrix.h:447-486, and no walk stops at a score); the
//                               final cell's pointer (dpmatrix.h:505-534) comes from row Q-2, still in registers, and from what
//                               the row observer kept of column T-2; the walk always runs to a cell of row 1 or column 1, then (0,0).
// Everything the kernels do not take — templates beyond 2048 columns, scoring systems ScoreRun sends through full builds, pairs
// without an interior, a length class an instantiation was not kept for — goes through resident batches inside the call.
// aln_hits_align_profiles is the same call for the hits of a profile search: the same host driver (align_block), the same two
// kernels instantiated for the profile side, and batches built from the profiles' planes for what those do not take.
// The chunks of fused hits run through FusedRoute (search_align.h), which aln_hits_align_multi, aln_hits_column_counts and
// aln_hits_pileup share; the entries' prologue (hit_entry) and the launch of the kernel pair (launch_hit_job) stand there too.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "search_align.h"

namespace aln {

// The batch route over the listed slots: aln_batch_create + aln_batch_dp + aln_batch_optimal / _strings, in the groups
// BatchGroup (score_common.h) cuts under the plane budget.  prof != nullptr: `queries` holds the query
// letters (the consensus pool or the placeholder), `sub` is not read and every batch is built from the planes of its own pairs
// (BatchSim), which its budget counts.  (Declared in search_align.h: for_list_groups there runs it for the jobs that read
// their lists on the host.)
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
  int rc;
  const int rows = run.rows;
  if (rows == 0) return ALN_OK;
  // one walk: every used slot validated and described for its route (nothing is written before it ends)
  SlotRoutes sr;
  if ((rc = route_slots(run, queries, K, hits, n_hits, hit_kernel_classes(run), run.local, sr)) != ALN_OK) return rc;
  std::vector<HitDesc>& fast = sr.fast;
  const std::vector<int32_t>&bq = sr.bq, &bt = sr.bt;
  const std::vector<size_t>& bslot = sr.bslot;
  ctx->align_routes[0] = (int64_t)fast.size(); ctx->align_routes[1] = (int64_t)bq.size();
  AlignOut ao = {out, pairs, pair_stride, tlines, qlines, line_stride, lengths};
  ao.clear_unused(rows, K, n_hits);

  // chunks of fused hits: one list each, and the two lines where wanted
  if (!fast.empty()) {
    rc = list_fused_hits(run, queries, sr, ao, [](FusedRoute<HitDesc>& fr, const FusedChunk& c, AlignArgs& g) {
      return launch_hit_job<ListJob>(fr, c, g);
    });
    if (rc != ALN_OK) return rc;
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
  return hit_entry(ctx, false, queries, nullptr, nullptr, templates, sub, gap, q_begin, q_end,
                   align_outputs_ok(K, hits, n_hits, out, pairs, pair_stride, tlines, qlines, line_stride, lengths),
                   [&](ScoreRun& run, const aln_seqs* pool) {
                     return align_block(run, pool, K, hits, n_hits, out, pairs, pair_stride, tlines, qlines, line_stride, lengths);
                   });
}

// The same for the hits of a profile search.  The query letters — the lines and the identity need them, the scores never do —
// are the caller's consensus pool or, without one, the placeholder pool the run builds for profiles.
extern "C" int aln_hits_align_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus,
                                       const aln_seqs* templates, const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                                       const aln_hit* hits, const int32_t* n_hits, aln_hit_alignment* out, int32_t* pairs,
                                       int32_t pair_stride, char* tlines, char* qlines, int32_t line_stride, int32_t* lengths) {
  return hit_entry(ctx, true, nullptr, profiles, consensus, templates, nullptr, gap, q_begin, q_end,
                   align_outputs_ok(K, hits, n_hits, out, pairs, pair_stride, tlines, qlines, line_stride, lengths),
                   [&](ScoreRun& run, const aln_seqs* pool) {
                     return align_block(run, pool, K, hits, n_hits, out, pairs, pair_stride, tlines, qlines, line_stride, lengths);
                   });
}

extern "C" int aln_hits_align_last_routes(const aln_ctx* ctx, int64_t out[2]) {
  if (!ctx || !out) return ALN_E_ARG;
  out[0] = ctx->align_routes[0]; out[1] = ctx->align_routes[1];
  return ALN_OK;
}

#undef STRY
#undef RTRY
