// search_counts.hip — the column counts of search hits, on the device: aln_hits_column_counts (gfx950).
//
// The step from one search round to the next needs, per query position, how often each template letter stands under it in
// the alignments of the query's hits: one small integer matrix per query, not the alignments.  So the two kernels of
// search_align.h are instantiated here with another job behind the same sweep and walk:
//   hit_local_kernel<R, Side, CountJob>    sweep_local + StripObserver<true> + the score check + strip_walk;
//   hit_global_kernel<R, Side, CountJob>   sweep_global + GlobalObserver + final_cell + strip_walk.
// One wave per hit.  The job's sink counts `same` for the identity (the record is aln_hits_align's), keeps the lane's smallest and
// largest interior query row, and issues ONE integer atomicAdd of the slot's weight into the call's count rows — row
// (offsets[q] - offsets[q_begin] + i), 32 int32 wide as the profile side's device rows are, column = the template letter's
// code; nothing reads the old value.  Within a hit every query row occurs once, so adds collide only between hits of one
// query, and integer adds commute: the result is exact whatever the order.  After the walk the wave reduces the two bounds
// and adds the weight to the spare column 31 (`covered`) of rows i_lo .. i_hi, 64 rows per step.  There is no list, no line
// buffer and no gapped_strings_kernel; the rows are zeroed once per call and downloaded once at its end.
// A slot that must not contribute — weight 0, a local score <= 0 (the seed cell's list) — still needs its record: the host
// passes weight 0 for it and the kernel leaves the adds out.  A local slot whose sweep score differs from .score returns
// before the walk.  Everything the kernels do not take goes through for_list_groups (search_align.h) — align_through_batches
// with pair lists wanted, a group of slots at a time —, whose lists the host tallies into the same outputs.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "search_counts.h"   // CountArgs, CountJob: the job, which search_counts_qgaps.hip instantiates too

namespace aln {

// The shared body of aln_hits_column_counts and aln_hits_column_counts_profiles (run: prepared; `queries`: the pool the query
// letters and lengths are read from — hit_entry's pool, search_align.h): the slot checks, the routes, the chunks of fused
// hits, the batches.
static int count_block(ScoreRun& run, const aln_seqs* queries, int32_t K, const aln_hit* hits, const int32_t* n_hits,
                       const int32_t* weights, aln_hit_alignment* out, int32_t* counts, int32_t* covered) {
  aln_ctx* ctx = run.ctx;
  const aln_seqs* templates = run.templates;
  const aln_qprofiles* prof = run.prof;
  const int32_t q_begin = run.q_begin;
  const int rows = run.rows;
  if (rows == 0) return ALN_OK;
  const int n_alpha = prof ? prof->n : run.sub->n;
  const char* alphabet = prof ? prof->alphabet : run.sub->alphabet;
  const int64_t row0 = queries->offsets[q_begin];
  const size_t n_rows = (size_t)(queries->offsets[run.q_end] - row0);

  // route_slots' walk (every used slot validated and described for its route), then the weights; nothing written before
  SlotRoutes sr;
  int rc = route_slots(run, queries, K, hits, n_hits, hit_kernel_classes(run), run.local, sr);
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
                          [](FusedRoute<HitDesc>& fr, const FusedChunk& c, CountArgs& g) { return launch_hit_job<CountJob>(fr, c, g); });
    if (rc != ALN_OK) return rc;
  }

  // the batch route (for_list_groups, search_align.h): every surviving slot's pair list tallied here
  if (!sr.bq.empty()) {
    int idx[256];
    for (int i = 0; i < 256; ++i) idx[i] = -1;
    for (int i = 0; i < n_alpha; ++i) idx[(unsigned char)alphabet[i]] = i;
    rc = for_list_groups(run, queries, sr, ao, [&](size_t slot, int32_t q, int32_t t, const int32_t* l, int n_pairs) {
      const int w = weight_of(slot);
      if (w <= 0) return;
      const int64_t qo = queries->offsets[q], Q = queries->offsets[q + 1] - qo;
      const int64_t to = templates->offsets[t], T = templates->offsets[t + 1] - to;
      int64_t lo = INT64_MAX, hi = -1;
      for (int k = 0; k < n_pairs; ++k) {
        const int64_t i = l[2 * k], j = l[2 * k + 1];
        if (i < 1 || i > Q - 2 || j < 1 || j > T - 2) continue;
        const int a = idx[(unsigned char)templates->residues[to + j]];
        if (a >= 0) counts[(size_t)(qo - row0 + i) * n_alpha + a] += w;
        lo = std::min(lo, i); hi = std::max(hi, i);
      }
      if (covered)
        for (int64_t i = lo; i <= hi; ++i) covered[qo - row0 + i] += w;
    });
    if (rc != ALN_OK) return rc;
  }
  return ao.worst;
}

}  // namespace aln

using namespace aln;

extern "C" int aln_hits_column_counts(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                                      const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K, const aln_hit* hits,
                                      const int32_t* n_hits, const int32_t* weights, aln_hit_alignment* out, int32_t* counts,
                                      int32_t* covered) {
  return hit_entry(ctx, false, queries, nullptr, nullptr, templates, sub, gap, q_begin, q_end, hit_list_ok(K, hits, n_hits, out) && counts,
                   [&](ScoreRun& run, const aln_seqs* pool) {
                     return count_block(run, pool, K, hits, n_hits, weights, out, counts, covered);
                   });
}

extern "C" int aln_hits_column_counts_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus,
                                               const aln_seqs* templates, const aln_gap* gap, int32_t q_begin, int32_t q_end,
                                               int32_t K, const aln_hit* hits, const int32_t* n_hits, const int32_t* weights,
                                               aln_hit_alignment* out, int32_t* counts, int32_t* covered) {
  return hit_entry(ctx, true, nullptr, profiles, consensus, templates, nullptr, gap, q_begin, q_end, hit_list_ok(K, hits, n_hits, out) && counts,
                   [&](ScoreRun& run, const aln_seqs* pool) {
                     return count_block(run, pool, K, hits, n_hits, weights, out, counts, covered);
                   });
}

#undef STRY
#undef RTRY
