// search_align_qgaps.hip — the alignments of the hits of a search under position-specific gap penalties, on the device:
// aln_hits_align_profiles_gaps (gfx950).  include/aln_hip.h has the definition of the alignment.
//
// aln_hits_align_profiles' call for a run whose profile rows carry their own del_init / del_extn / ins_init / ins_extn: one
// wave per hit,
//   hit_local_qgaps_kernel<R, ListJob>    (search_align_qgaps.h) sweep_local_qgaps + StripObserver<true> + the score check + strip_walk;
//   hit_global_qgaps_kernel<R, ListJob>   sweep_global_qgaps + QGapGlobalObserver + final_cell + strip_walk;
//   class_list_kernel, gapped_strings_kernel as in search_align.hip.
// The strip byte is the one defined at the head of search_align.hip; search_align_qgaps.h tells why its bits 2 and 3 stay valid
// under per-row prices.  The chunks run through search_align.h's list_fused_hits, the driver aln_hits_align_profiles uses.
// There is no batch route: every pair with an interior takes the kernels (all eight length classes, all five align types),
// and a pair without one (Q = 2 or T = 2) is filed by the host in closed form (NoInterior), its lines by host_strings.cpp's
// general procedure, which gapped_strings_kernel mirrors for exactly such lists.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "search_align_qgaps.h"

namespace aln {

// The slots without an interior (sr.bq / bt / bslot), filed as the batch route of aln_hits_align_profiles files them: record,
// list, and the two lines with their length.  `queries`: the pool the query letters are read from.
static void file_without_interior(const ScoreRun& run, const aln_seqs* queries, const SlotRoutes& sr, bool want_lines,
                                  int32_t line_stride, AlignOut& ao) {
  const aln_seqs* templates = run.templates;
  std::vector<char> tl, ql;
  for (size_t p = 0; p < sr.bq.size(); ++p) {
    const int32_t q = sr.bq[p], t = sr.bt[p];
    const int64_t qo = queries->offsets[q], Q = queries->offsets[q + 1] - qo;
    const int64_t to = templates->offsets[t], T = templates->offsets[t + 1] - to;
    const char* qs = queries->residues + qo; const char* ts = templates->residues + to;
    const NoInterior ni(run, q, Q, T);
    int same = 0;
    for (int k = 0; k < ni.n; ++k) same += qs[ni.list[2 * k]] == ts[ni.list[2 * k + 1]] ? 1 : 0;
    const float ident = float(same - 2) / float(std::min(Q, T) - 2) * 100.f;   // alignment.h:864
    int st = ALN_OK, len = 0;
    if (want_lines) {
      aln_alignment ali = {};
      ali.n_pairs = ni.n; ali.pair_off = 0;
      len = aln_gapped_length((int32_t)T, &ali, 1, ni.list);
      if (len >= line_stride) len = line_stride;                  // put() turns it into the record's status
      else {
        tl.assign((size_t)len + 1, 0); ql.assign((size_t)len + 1, 0);
        const int rc = aln_gapped_strings(qs, (int32_t)Q, ts, (int32_t)T, &ali, 1, ni.list, tl.data(), ql.data(), len + 1);
        if (rc != ALN_OK) { st = rc; len = 0; }
      }
    }
    ao.put(sr.bslot[p], st, ni.score, st == ALN_OK ? ident : 0.f, st == ALN_OK ? ni.n : 0, ni.list, false, len, tl.data(), ql.data());
  }
}

// The body of aln_hits_align_profiles_gaps (run: prepared with gap rows; `queries`: hit_entry_qgaps' pool): the slot checks, the
// two routes, the chunks of fused hits (list_fused_hits, search_align.h), the pairs without an interior.
static int align_block_qgaps(ScoreRun& run, const aln_seqs* queries, int32_t K, const aln_hit* hits, const int32_t* n_hits,
                             aln_hit_alignment* out, int32_t* pairs, int32_t pair_stride, char* tlines, char* qlines,
                             int32_t line_stride, int32_t* lengths) {
  aln_ctx* ctx = run.ctx;
  const bool want_lines = tlines || qlines;
  int rc;
  const int rows = run.rows;
  if (rows == 0) return ALN_OK;
  // one walk: every used slot validated and described for its route (nothing is written before it ends)
  SlotRoutes sr;
  if ((rc = route_slots_qgaps(run, queries, K, hits, n_hits, sr)) != ALN_OK) return rc;
  ctx->align_routes[0] = (int64_t)sr.fast.size(); ctx->align_routes[1] = (int64_t)sr.bq.size();
  AlignOut ao = {out, pairs, pair_stride, tlines, qlines, line_stride, lengths};
  ao.clear_unused(rows, K, n_hits);

  // chunks of fused hits: search_align.h's driver over the gap-row kernel pair
  if (!sr.fast.empty()) {
    rc = list_fused_hits(run, queries, sr, ao, [](FusedRoute<HitDesc>& fr, const FusedChunk& c, AlignArgs& g) {
      return launch_hit_qgaps_job<ListJob>(fr, c, g);
    });
    if (rc != ALN_OK) return rc;
  }
  file_without_interior(run, queries, sr, want_lines, line_stride, ao);
  return ao.worst;
}

}  // namespace aln

using namespace aln;

extern "C" int aln_hits_align_profiles_gaps(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_qgaps* gaps,
                                            const aln_seqs* consensus, const aln_seqs* templates, int32_t align_type,
                                            int32_t q_begin, int32_t q_end, int32_t K, const aln_hit* hits, const int32_t* n_hits,
                                            aln_hit_alignment* out, int32_t* pairs, int32_t pair_stride, char* tlines, char* qlines,
                                            int32_t line_stride, int32_t* lengths) {
  return hit_entry_qgaps(ctx, profiles, gaps, consensus, templates, align_type, q_begin, q_end,
                         align_outputs_ok(K, hits, n_hits, out, pairs, pair_stride, tlines, qlines, line_stride, lengths),
                         [&](ScoreRun& run, const aln_seqs* pool) {
                           return align_block_qgaps(run, pool, K, hits, n_hits, out, pairs, pair_stride, tlines, qlines, line_stride,
                                                    lengths);
                         });
}

#undef STRY
#undef RTRY
