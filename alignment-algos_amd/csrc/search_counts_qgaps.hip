// search_counts_qgaps.hip — the column counts of the hits of a search under position-specific gap penalties, on the device:
// aln_hits_column_counts_profiles_gaps (gfx950).
//
// The second job over search_align_qgaps.h's kernel pair: hit_local_qgaps_kernel / hit_global_qgaps_kernel<R, CountJob>, the job
// being search_counts.h's, unchanged — one integer atomicAdd per list entry into the call's 32-wide count rows, `covered` in the
// spare column.  The alignment of a slot is the list aln_hits_align_profiles_gaps reports for it, and the record is that entry's
// without pairs and lines.  A pair without an interior has no interior entry and contributes nothing: the host files its
// record (NoInterior) and that is all.  There is no batch route.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "search_align_qgaps.h"
#include "search_counts.h"

namespace aln {

// The body of aln_hits_column_counts_profiles_gaps (run: prepared with gap rows; `queries`: hit_entry_qgaps' pool), after
// count_block (search_counts.hip): the slot checks, the weights, the chunks of fused hits, the records of the other pairs.
static int count_block_qgaps(ScoreRun& run, const aln_seqs* queries, int32_t K, const aln_hit* hits, const int32_t* n_hits,
                             const int32_t* weights, aln_hit_alignment* out, int32_t* counts, int32_t* covered) {
  aln_ctx* ctx = run.ctx;
  const aln_seqs* templates = run.templates;
  const int rows = run.rows;
  if (rows == 0) return ALN_OK;
  const int n_alpha = run.prof->n;
  const int64_t row0 = queries->offsets[run.q_begin];
  const size_t n_rows = (size_t)(queries->offsets[run.q_end] - row0);

  // route_slots_qgaps' walk (every used slot validated and described for its route), then the weights; nothing written before
  SlotRoutes sr;
  int rc = route_slots_qgaps(run, queries, K, hits, n_hits, sr);
  if (rc != ALN_OK) return rc;
  std::vector<HitDesc>& fast = sr.fast;
  if (weights)
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < n_hits[r]; ++k)
        if (weights[(size_t)r * K + k] < 0 || weights[(size_t)r * K + k] > 65535) return ALN_E_ARG;
  auto weight_of = [&](size_t slot) { return weights ? weights[slot] : 1; };
  ctx->align_routes[0] = (int64_t)fast.size(); ctx->align_routes[1] = (int64_t)sr.bq.size();

  memset(counts, 0, n_rows * (size_t)n_alpha * 4);
  if (covered) memset(covered, 0, n_rows * 4);
  AlignOut ao = {out, nullptr, 0, nullptr, nullptr, 0, nullptr};
  ao.clear_unused(rows, K, n_hits);

  // chunks of fused hits (count_fused_hits, search_counts.h)
  if (!fast.empty()) {
    rc = count_fused_hits(run, queries, sr, row0, n_rows, n_alpha, counts, covered, ao, weight_of,
                          [](FusedRoute<HitDesc>& fr, const FusedChunk& c, CountArgs& g) { return launch_hit_qgaps_job<CountJob>(fr, c, g); });
    if (rc != ALN_OK) return rc;
  }

  // the pairs without an interior: the record aln_hits_align_profiles_gaps writes without pairs and lines, no contribution
  for (size_t p = 0; p < sr.bq.size(); ++p) {
    const int32_t q = sr.bq[p], t = sr.bt[p];
    const int64_t qo = queries->offsets[q], Q = queries->offsets[q + 1] - qo;
    const int64_t to = templates->offsets[t], T = templates->offsets[t + 1] - to;
    const NoInterior ni(run, q, Q, T);
    int same = 0;
    for (int k = 0; k < ni.n; ++k) same += queries->residues[qo + ni.list[2 * k]] == templates->residues[to + ni.list[2 * k + 1]] ? 1 : 0;
    ao.put(sr.bslot[p], ALN_OK, ni.score, float(same - 2) / float(std::min(Q, T) - 2) * 100.f, ni.n, ni.list, false, 0, nullptr, nullptr);
  }
  return ao.worst;
}

}  // namespace aln

using namespace aln;

extern "C" int aln_hits_column_counts_profiles_gaps(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_qgaps* gaps,
                                                    const aln_seqs* consensus, const aln_seqs* templates, int32_t align_type,
                                                    int32_t q_begin, int32_t q_end, int32_t K, const aln_hit* hits,
                                                    const int32_t* n_hits, const int32_t* weights, aln_hit_alignment* out,
                                                    int32_t* counts, int32_t* covered) {
  return hit_entry_qgaps(ctx, profiles, gaps, consensus, templates, align_type, q_begin, q_end, hit_list_ok(K, hits, n_hits, out) && counts,
                         [&](ScoreRun& run, const aln_seqs* pool) {
                           return count_block_qgaps(run, pool, K, hits, n_hits, weights, out, counts, covered);
                         });
}

#undef STRY
#undef RTRY
