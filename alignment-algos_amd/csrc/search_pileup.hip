// search_pileup.hip — the query-anchored pileup of search hits, on the device: aln_hits_pileup (gfx950).
//
// What is read off a search round — sequence weights, purging, gap statistics, a consensus, the MSA handed on — wants one
// fixed-width row per hit whose column is the query position: the template residue aligned to it, or a gap.  The list of a hit
// is 8 B per entry and has to be scattered on the host; the row is 1 B (letters) + 2 B (template positions) per query position
// and needs nothing further.  So the two kernels of search_align.h are instantiated here with a third job behind the same sweep
// and walk:
//   hit_local_kernel<R, Side, PileupJob>    sweep_local + StripObserver<true> + the score check + strip_walk;
//   hit_global_kernel<R, Side, PileupJob>   sweep_global + GlobalObserver + final_cell + strip_walk.
// One wave per hit.  The job's sink counts `same` for the identity (the record is aln_hits_align's), and for an interior entry
// (q, t) stores t as 2 bytes into the hit's tpos row and the template's CHARACTER as 1 byte into its letters row, both at index
// q - 1, each only where that output is wanted, and keeps the lane's smallest and largest interior q with the t that belongs to
// each.  After the walk the wave reduces the two bounds, writes the span, and turns every position of i_lo .. i_hi that no entry
// wrote into '-', 64 positions per step.
//
// Where the bytes come from.  The rows of a chunk live in two device buffers of `stride` = the block's longest Q - 2 entries per
// hit.  Before every launch the host memsets the chunk's letters to '.', its tpos and its spans to 0 — in the stream's order, so
// a kernel never meets what an earlier chunk or call left — and the kernels only ever overwrite: a slot that is muted (below),
// a local slot that is refused before the walk and every position outside i_lo .. i_hi keep '.' / 0 / {0,0,0,0} as the definition
// wants them.  The host copies Q - 2 entries per slot into the caller's arrays, which it has zeroed in full: that is the padding.
//
// Ordering of the gap pass.  It reads letters bytes that OTHER lanes of the wave stored during the walk (a diagonal run is
// stored by up to 64 lanes, a jump's entry by lane 0).  Between the last of those stores and the first of those loads stand
// __threadfence(); __syncthreads(); — the pair the kernels place between the sweep's strip stores and the walk.  The fence is a
// sequentially consistent fence at agent scope: every lane's stores have left for L2 before it completes and the vector L1 is
// invalidated after it, so a line that another wave of the CU pulled in earlier (rows of two hits may share a cache line: the
// stride is not padded) is not read stale; the barrier keeps any lane from loading before every lane has passed its fence.  The
// block is one wave and finish() is called by every lane under wave-uniform conditions, so the barrier is reached by all 64.
// The '.' the pass tests for was written by the memset, an earlier operation of the stream.  ('.' is taken not to be a letter of
// the templates' alphabet: a pileup could not show it.)
//
// The character pool.  `Letters` of the residue side are codes, so the pool is not among the sink's constructor arguments: it
// rides behind the job's Args (PileupRows; FusedRoute::upload_pools() puts the pool on the device for both sides) and the hit's
// offset into it is toff[desc[hit].t], the offset of the codes.  The kernels' signatures are untouched.
// A slot that must not contribute but needs its record — a local score <= 0, the seed cell's list — is muted by a per-hit flag
// from the host (live == 0), as CountJob is muted by weight 0: its sink counts `same` and stores nothing.  A local slot whose
// sweep score differs from .score returns before the walk.  Everything the kernels do not take goes through for_list_groups
// (search_align.h) — align_through_batches with pair lists wanted —, from whose lists the host fills the same outputs.
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "search_pileup.h"

namespace aln {

// PileupRows, PileupArgs, PileupJob and pileup_from_list stand in search_pileup.h, which aln_hits_weights (search_weights.hip)
// shares; the kernels are instantiated here alone, behind launch_pileup_job.
int launch_pileup_job(FusedRoute<HitDesc>& fr, const FusedChunk& c, PileupArgs& g) { return launch_hit_job<PileupJob>(fr, c, g); }

// The shared body of aln_hits_pileup and aln_hits_pileup_profiles (run: prepared; `queries`: the pool the query lengths are
// read from — hit_entry's pool, search_align.h): the stride check, the slot checks, the routes, the chunks of fused hits,
// the batches.
static int pileup_block(ScoreRun& run, const aln_seqs* queries, int32_t K, const aln_hit* hits, const int32_t* n_hits,
                        aln_hit_alignment* out, aln_hit_span* spans, char* letters, uint16_t* tpos, int32_t line_stride) {
  aln_ctx* ctx = run.ctx;
  const aln_seqs* templates = run.templates;
  const int rows = run.rows;
  if (rows == 0) return ALN_OK;
  const bool want_rows = letters || tpos;
  int64_t maxw = 0;                                          // the longest Q - 2 of the block
  for (int q = run.q_begin; q < run.q_end; ++q) maxw = std::max<int64_t>(maxw, queries->offsets[q + 1] - queries->offsets[q] - 2);
  if (want_rows && line_stride < maxw) return ALN_E_ARG;
  maxw = std::max<int64_t>(maxw, 1);                         // ... which is the device rows' stride

  // route_slots' walk (every used slot validated and described for its route); nothing written before
  SlotRoutes sr;
  int rc = route_slots(run, queries, K, hits, n_hits, hit_kernel_classes(run), run.local, sr);
  if (rc != ALN_OK) return rc;
  std::vector<HitDesc>& fast = sr.fast;
  const std::vector<size_t>& fast_slot = sr.fast_slot;
  ctx->align_routes[0] = (int64_t)fast.size(); ctx->align_routes[1] = (int64_t)sr.bq.size();

  // the outputs in full: zero everywhere, then '.' over the Q - 2 positions of every used slot
  const size_t n_slots = (size_t)rows * K, ls = want_rows ? (size_t)line_stride : 0;
  if (letters) memset(letters, 0, n_slots * ls);
  if (tpos) memset(tpos, 0, n_slots * ls * 2);
  if (spans) memset(spans, 0, n_slots * sizeof(aln_hit_span));
  AlignOut ao = {out, nullptr, 0, nullptr, nullptr, 0, nullptr};
  ao.clear_unused(rows, K, n_hits);
  for (int r = 0; r < rows; ++r) {
    const int64_t w = queries->offsets[run.q_begin + r + 1] - queries->offsets[run.q_begin + r] - 2;
    if (letters && w > 0)
      for (int k = 0; k < n_hits[r]; ++k) memset(letters + ((size_t)r * K + k) * ls, '.', (size_t)w);
  }

  // chunks of fused hits.  cut() is asked for one "pair of lines" of maxw bytes per hit, which is the 2 maxw bytes of a tpos row
  // (the letters row is half of that), and for lists of no entries: strips and each row buffer stay below the budget.
  if (!fast.empty()) {
    FusedRoute<HitDesc> fr(run, queries, fast);
    std::vector<int32_t> fast_live(fast.size());
    for (size_t h = 0; h < fast.size(); ++h) fast_live[h] = (run.local && !(fast[h].score > 0.f)) ? 0 : 1;
    fr.cut(1, want_rows, (int)std::min<int64_t>(maxw, INT_MAX),
           [&](const HitDesc& d) { return HitNeed{hit_strip_bytes(run, queries, d), 0, 0}; });
    const size_t max_n = fr.max_n, dw = (size_t)maxw;
    int32_t* dlive = nullptr; char* dlet = nullptr; uint16_t* dpos = nullptr; aln_hit_span* dspan = nullptr; PileupRows* drows = nullptr;
    HitRecords rec;
    RTRY(fr.begin());
    STRY(fr.bufs.get(dlive, max_n));
    RTRY(rec.alloc(fr.bufs, max_n));
    if (letters) STRY(fr.bufs.get(dlet, max_n * dw));
    if (tpos) STRY(fr.bufs.get(dpos, max_n * dw));
    if (spans) STRY(fr.bufs.get(dspan, max_n));
    STRY(fr.bufs.get(drows, 1));
    std::vector<char> hlet(letters ? max_n * dw : 0);
    std::vector<uint16_t> hpos(tpos ? max_n * dw : 0);
    std::vector<aln_hit_span> hspan(spans ? max_n : 0);
    RTRY(fr.upload_pools());                                   // the templates' characters, on both sides
    const PileupRows where = {dlive, fr.dtch, dlet, dpos, dspan, (int64_t)dw};   // (alive until the first chunk's synchronisation)
    STRY(hipMemcpyAsync(drows, &where, sizeof(where), hipMemcpyHostToDevice, ctx->stream));
    for (const FusedChunk& c : fr.chunks) {
      const size_t n = c.n;
      RTRY(fr.stage(c, [&]() -> int {
        STRY(hipMemcpyAsync(dlive, fast_live.data() + c.h0, n * 4, hipMemcpyHostToDevice, ctx->stream));
        if (dlet) STRY(hipMemsetAsync(dlet, '.', n * dw, ctx->stream));
        if (dpos) STRY(hipMemsetAsync(dpos, 0, n * dw * 2, ctx->stream));
        if (dspan) STRY(hipMemsetAsync(dspan, 0, n * sizeof(aln_hit_span), ctx->stream));
        return ALN_OK;
      }));
      PileupArgs g = {};
      g.desc = fr.ddesc; g.strip = fr.dstrip; g.rows = drows; g.res = rec.dres; g.same = rec.dsame;
      RTRY(launch_pileup_job(fr, c, g));
      RTRY(rec.enqueue_download(ctx, n));
      if (dlet) STRY(hipMemcpyAsync(hlet.data(), dlet, n * dw, hipMemcpyDeviceToHost, ctx->stream));
      if (dpos) STRY(hipMemcpyAsync(hpos.data(), dpos, n * dw * 2, hipMemcpyDeviceToHost, ctx->stream));
      if (dspan) STRY(hipMemcpyAsync(hspan.data(), dspan, n * sizeof(aln_hit_span), hipMemcpyDeviceToHost, ctx->stream));
      STRY(hipStreamSynchronize(ctx->stream));                 // the host vectors above are read by the copies until here
      rec.put(ao, fr, c, fast_slot, [&](size_t h, size_t slot, int64_t Q) {
        if (letters) memcpy(letters + slot * ls, hlet.data() + h * dw, (size_t)(Q - 2));
        if (tpos) memcpy(tpos + slot * ls, hpos.data() + h * dw, (size_t)(Q - 2) * 2);
        if (spans) spans[slot] = hspan[h];
      });
    }
  }

  // the batch route (for_list_groups, search_align.h): every surviving slot's pair list laid out here
  if (!sr.bq.empty()) {
    rc = for_list_groups(run, queries, sr, ao, [&](size_t slot, int32_t q, int32_t t, const int32_t* l, int n_pairs) {
      const int64_t Q = queries->offsets[q + 1] - queries->offsets[q];
      const int64_t to = templates->offsets[t], T = templates->offsets[t + 1] - to;
      pileup_from_list(l, n_pairs, Q, T, templates->residues + to, letters ? letters + slot * ls : nullptr,
                       tpos ? tpos + slot * ls : nullptr, spans ? spans + slot : nullptr);
    });
    if (rc != ALN_OK) return rc;
  }
  return ao.worst;
}

static bool pileup_outputs_ok(int32_t K, const aln_hit* hits, const int32_t* n_hits, const aln_hit_alignment* out, const char* letters,
                              const uint16_t* tpos, int32_t line_stride) {
  return hit_list_ok(K, hits, n_hits, out) && !((letters || tpos) && line_stride < 1);
}

}  // namespace aln

using namespace aln;

extern "C" int aln_hits_pileup(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                               const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K, const aln_hit* hits,
                               const int32_t* n_hits, aln_hit_alignment* out, aln_hit_span* spans, char* letters, uint16_t* tpos,
                               int32_t line_stride) {
  return hit_entry(ctx, false, queries, nullptr, nullptr, templates, sub, gap, q_begin, q_end,
                   pileup_outputs_ok(K, hits, n_hits, out, letters, tpos, line_stride), [&](ScoreRun& run, const aln_seqs* pool) {
                     return pileup_block(run, pool, K, hits, n_hits, out, spans, letters, tpos, line_stride);
                   });
}

extern "C" int aln_hits_pileup_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus,
                                        const aln_seqs* templates, const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                                        const aln_hit* hits, const int32_t* n_hits, aln_hit_alignment* out, aln_hit_span* spans,
                                        char* letters, uint16_t* tpos, int32_t line_stride) {
  return hit_entry(ctx, true, nullptr, profiles, consensus, templates, nullptr, gap, q_begin, q_end,
                   pileup_outputs_ok(K, hits, n_hits, out, letters, tpos, line_stride), [&](ScoreRun& run, const aln_seqs* pool) {
                     return pileup_block(run, pool, K, hits, n_hits, out, spans, letters, tpos, line_stride);
                   });
}

#undef STRY
#undef RTRY
