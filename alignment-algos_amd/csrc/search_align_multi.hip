// search_align_multi.hip — several non-intersecting local alignments per search hit, on the device: aln_hits_align_multi and,
// for the hits of a profile search, aln_hits_align_multi_profiles (gfx950).
//
// Round 0 of a hit is Optimal's alignment (what aln_hits_align returns); round a >= 1 is Optimal's alignment of the matrix in
// which every aligned pair of the rounds before is forbidden: D = 0 there, everything else the reference's recurrence
// (include/aln_hip.h has the rule).  One wave per hit runs all rounds inside one launch:
//   align_local_multi_kernel<R, Side>   (Side: residue queries through the table, or position-specific rows staged into LDS)
//                                 per round: sweep_local_masked (score_sweep.h) over ALL rows 1 .. Q-2 — the end cell is not
//                                 known in advance — observed for the strip byte of every cell (search_align.hip defines it) and
//                                 for find_max's end cell (score_local_end_kernel's rule) in the SAME sweep; the walk back of
//                                 hit_local_kernel (search_align.h) through the strip; the list, the identity count, and one bit per
//                                 aligned pair into the hit's forbidden-cell plane (1/8 B per cell) for the rounds that follow.
// The walk needs no change: a forbidden cell holds 0 when the next row's strip byte takes its score bit, so a walk that reaches
// one — diagonally or as a gap source — stops before it, as Optimal's does (optimal.h:100).  It is strip_walk (search_align.h), the
// one hit_local_kernel calls, with a sink that also sets the pair's bit.  (DESIGN 4.8's finding is about helpers that take
// a kernel's row arrays by reference; the walk's state is scalars after the sweep, and sharing it cost no register: 4.8i.)
//   class_list_kernel, gapped_strings_kernel   unchanged: the lines of every (hit, round) list in one launch.
// Templates beyond the kept classes, scoring systems ScoreRun sends through full builds and pairs without an interior go
// through resident batches inside the call, round by round, on ALN_SIM_MATRIX planes expanded and masked on the host (a
// profile's planes in every round, round 0 included: there is no table to build from).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "search_align_multi.h"

namespace aln {

// One template over the query side (ResidueQuery, ProfileQuery: score_common.h), as the kernels of search_align.h are.  qch /
// tch: the character pools of the query letters and of the templates on the device — the staged side has no letters of its own
// and counts the identity over CHARACTERS (the consensus pool or the placeholder, exactly what gapped_strings_kernel lays out);
// the residue side counts over codes, never reads the pools and is passed nullptr.
//
// The staged side, round after round.  Every round's sweep calls Rows::first() again: chunks 0 and 1 go into slots 0 and 1 of
// the ring.  The round before left ONE copy requested that nothing reads (the chunk after its last row's) and up to 32 stale
// rows in the ring.  The stale rows are harmless — a sweep reads row i only after landed() has returned for the chunk that
// holds it, and that chunk was requested by THIS sweep.  The copy is not: it targets one of the four slots, which the new
// round's copies target too, and nothing but the counter's order would keep it from landing on top of them.  So the wave
// drains its VM counter (s_waitcnt vmcnt(0)) directly after every sweep, which is before either way out of the round — the
// break of a round that is not reported and the walk of one that is (whose fence waits for the strip stores anyway) — and so
// before the next round's first() and before the wave ends: no copy targets LDS after the wave has gone.  The ring is private
// to the wave, so the drain needs no barrier of its own; it stands next to the fence + barrier pair that the walk needs.
// INVARIANT (ScoreRun::upload_profile_rows): a sweep over rows 1 .. Q-2 requests at most rows 0 .. Q + 13 of its profile.
// The mask words stay what they were: set by atomicOr, made visible by fence + barrier, read through plain loads.
template <int R, class Side>
__global__ __launch_bounds__(64) void align_local_multi_kernel(ScoreArgs a, MultiArgs g, const char* __restrict__ qch,
                                                              const char* __restrict__ tch) {
  __shared__ __attribute__((aligned(16))) int lds[32 * 32];
  const int lane = threadIdx.x;
  Side::stage(lds, a);
  const int hit = g.list[blockIdx.x];
  const MultiDesc hd = g.desc[hit];
  const int ti = hd.t, qi = hd.q;
  const typename Side::Rows::Src* __restrict__ qr = Side::rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const auto* __restrict__ qs = Side::letters(a.qcodes, qch) + a.qoff[qi];      // what the identity is counted over
  const auto* __restrict__ ts = Side::letters(a.tcodes, tch) + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);   // Q >= 3, T >= 3: the host's routing
  constexpr int kPitch = 256 * R;
  uint8_t* strip = g.strip + hd.strip_off;      // row i (2 .. Q-2) at strip + (i - 2) * kPitch
  uint32_t* mask = g.mask + hd.mask_off;        // row i (0 .. Q-1) at mask + i * 8 R
  const int cap = g.trav_stride;
  auto drain = [] { if constexpr (Side::kStaged) asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };   // the round's last copy

  LocalCols<R> cols;
  cols.load(tc, T, a.gi, a.ge);
  int found = 0;
  for (int round = 0; round < g.n_rounds; ++round) {
    // ---- the sweep: strip bytes + find_max (optimal.h:108-124; the reduction and the seed rule of score_local_end_kernel) ------
    int d[R][4];
    StripFirstMaxObserver ob;
    ob.strip = strip; ob.pitch = kPitch;
    int lmax;
    if (round == 0) lmax = sweep_local_masked<R, false, typename Side::Rows>(lds, cols, qr, Q - 2, mask, d, ob);   // nothing is forbidden yet: no mask loads
    else lmax = sweep_local_masked<R, true, typename Side::Rows>(lds, cols, qr, Q - 2, mask, d, ob);
    drain();                                                   // before EITHER way out of the round: the break below, the walk
    int m = lmax;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o));
    int br = (lmax == m) ? ob.lrow : 0x7FFFFFFF;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) br = min(br, __shfl_xor(br, o));
    int bc = (lmax == m && ob.lrow == br) ? ob.lcol : 0x7FFFFFFF;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) bc = min(bc, __shfl_xor(bc, o));
    int seed = 0;
    if (m > 0) {
      const int cl = T - 2;
      seed = __shfl(sweep_pick<R>(d, cl / 256, cl & 3, 0), (cl & 255) >> 2);
    }
    const bool seed_wins = (m == 0) || (seed == m);
    const int q_end = seed_wins ? Q - 2 : br, t_end = seed_wins ? T - 2 : bc;
    // reported: score >= min_score and, after round 0, > 0; the first round that is not ends the hit (all wave-uniform)
    if ((round > 0 && m <= 0) || !((float)m >= g.min_score)) break;
    __threadfence();                                           // the walk's lanes read bytes other lanes stored
    __syncthreads();

    // ---- the walk back (optimal.h:79-105), emitted in traversal order; every aligned pair is forbidden from now on ------------
    const bool more = round + 1 < g.n_rounds;
    int32_t* o = g.trav + ((size_t)hit * g.n_rounds + round) * cap * 2;
    int n = 0, same = 0;
    auto forbid = [&](int q, int t) {                          // an alignment has one cell per row: no two lanes share a word
      if (more) atomicOr(mask + (size_t)q * (8 * R) + (t >> 5), 1u << (t & 31));
    };
    auto sink = [&](int k, int q, int t) {
      if (k < cap) { o[2 * k] = q; o[2 * k + 1] = t; same += (qs[q] == ts[t]) ? 1 : 0; }
    };
    auto emit1 = [&](int q, int t) { if (lane == 0) sink(n, q, t); ++n; };
    emit1(Q - 1, T - 1);
    emit1(q_end, t_end);
    if (lane == 0) forbid(q_end, t_end);
    // a list the caller's stride truncates still forbids all its cells
    if (strip_walk<kPitch, true>(strip, q_end, t_end, n, [&](int k, int q, int t) { sink(k, q, t); forbid(q, t); })) emit1(0, 0);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) same += __shfl_xor(same, off);
    if (lane == 0) {
      PairResult res = {};
      res.best = (float)m; res.corner = 0.f; res.best_q = q_end; res.best_t = t_end;
      res.n_path = n;
      res.status = n <= cap ? 0 : ALN_E_OVERFLOW;
      g.res[(size_t)hit * g.n_rounds + round] = res;
      g.same[(size_t)hit * g.n_rounds + round] = same;
    }
    ++found;
    __threadfence();                                           // the next sweep's lanes read mask words other lanes changed, and
    __syncthreads();                                           // overwrite strip bytes this walk read
  }
  if (lane == 0) g.n_found[hit] = found;
}

// Is round `a` with this score reported?
static bool reported(int a, float score, float min_score) { return score >= min_score && (a == 0 || score > 0.f); }

// The batch route, round by round over the slots still alive: aln_batch_create + aln_batch_dp + aln_batch_optimal / _strings,
// in the groups BatchGroup (score_common.h) cuts under the plane budget.  Round 0 is built from the table
// itself, exactly as aln_hits_align builds it; later rounds from the pairs' Q x T planes, expanded on the host with every
// forbidden cell at -(round 0's score + 1).  prof != nullptr: `queries` holds the query letters (the consensus pool or the
// placeholder), `sub` is not read and EVERY round, round 0 included, is built from the planes of its pairs, expanded by the
// profile plane source (BatchSim, score_common.h) and, after round 0, masked in place.
static int multi_through_batches(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                                 const aln_qprofiles* prof, const aln_gap* gap, const std::vector<int32_t>& qi_all,
                                 const std::vector<int32_t>& ti_all, const std::vector<size_t>& slot_all, int N, float min_score,
                                 int32_t* n_found, AlignOut& ao) {
  int idx[256];
  for (int i = 0; i < 256; ++i) idx[i] = -1;
  if (!prof)                                                   // side: the table's letter index (profiles: BatchSim has its own)
    for (int i = 0; i < sub->n; ++i) idx[(unsigned char)sub->alphabet[i]] = i;
  const size_t np_all = qi_all.size();
  std::vector<std::vector<int32_t>> forbidden(np_all);       // per pair: (i, j) of every aligned pair so far
  std::vector<float> neg(np_all, 0.f);
  std::vector<size_t> alive(np_all);
  for (size_t p = 0; p < np_all; ++p) alive[p] = p;
  std::vector<int32_t> n, st, pairs, len, aq, at;
  std::vector<float> sc, ident, planes;
  std::vector<int64_t> plane_off;
  std::vector<char> tl, ql;
  for (int a = 0; a < N && !alive.empty(); ++a) {
    std::vector<size_t> next;
    aq.resize(alive.size()); at.resize(alive.size());          // the round's pair list: the slots still alive
    for (size_t k = 0; k < alive.size(); ++k) { aq[k] = qi_all[alive[k]]; at[k] = ti_all[alive[k]]; }
    BatchGroup grp;
    while (grp.next(queries, templates, aq.data(), at.data(), alive.size(), a > 0 || prof != nullptr)) {
      const size_t g0 = grp.g0;
      const int32_t np = (int32_t)(grp.g1 - g0), stride = (int32_t)std::max<int64_t>(std::min(grp.max_q, grp.max_t) + 3, 4);
      const int32_t ls = (int32_t)(grp.max_sum + 2);
      const int32_t *gq = aq.data() + g0, *gt = at.data() + g0;
      n.assign((size_t)np, 0); st.assign((size_t)np, 0); pairs.assign((size_t)np * stride * 2, 0);
      sc.assign((size_t)np, 0.f); ident.assign((size_t)np, 0.f); len.assign((size_t)np, 0);
      aln_sim sim = aln_sim();
      BatchSim bs;
      auto forbid_in = [&](float* S, int64_t T, size_t p) {
        for (size_t e = 0; e < forbidden[p].size(); e += 2) S[(int64_t)forbidden[p][e] * T + forbidden[p][e + 1]] = neg[p];
      };
      if (prof) {                                              // side: the planes of the group's pairs, every round
        bs.set(nullptr, prof, templates, (size_t)np, gq, gt);
        for (int32_t k = 0; k < np && a > 0; ++k)
          forbid_in(bs.planes.data() + bs.plane_off[k], templates->offsets[gt[k] + 1] - templates->offsets[gt[k]], alive[g0 + k]);
        sim = bs.sim;
      } else if (a == 0) { sim.kind = ALN_SIM_SUBMATRIX; sim.sub = *sub; }
      else {
        plane_off.assign((size_t)np + 1, 0);
        for (int32_t k = 0; k < np; ++k) {
          const int64_t Q = queries->offsets[gq[k] + 1] - queries->offsets[gq[k]], T = templates->offsets[gt[k] + 1] - templates->offsets[gt[k]];
          plane_off[k + 1] = plane_off[k] + Q * T;
        }
        planes.assign((size_t)plane_off[np], 0.f);
        for (int32_t k = 0; k < np; ++k) {
          const int64_t q0 = queries->offsets[gq[k]], Q = queries->offsets[gq[k] + 1] - q0;
          const int64_t t0 = templates->offsets[gt[k]], T = templates->offsets[gt[k] + 1] - t0;
          float* S = planes.data() + plane_off[k];
          for (int64_t i = 1; i <= Q - 2; ++i) {
            const float* row = sub->table + (size_t)idx[(unsigned char)queries->residues[q0 + i]] * sub->n;   // letters: checked by prepare()
            for (int64_t j = 1; j <= T - 2; ++j) S[i * T + j] = row[idx[(unsigned char)templates->residues[t0 + j]]];
          }
          forbid_in(S, T, alive[g0 + k]);
        }
        sim.kind = ALN_SIM_MATRIX; sim.planes = planes.data(); sim.plane_off = plane_off.data();
      }
      aln_batch* bb = nullptr;
      int rc = aln_batch_create(ctx, queries, templates, np, gq, gt, 0, &bb);
      if (rc == ALN_OK) rc = aln_batch_dp(bb, &sim, gap, ALN_FWD, ALN_DP_AUTO, 0);
      if (rc == ALN_OK) rc = aln_batch_optimal(bb, sc.data(), n.data(), pairs.data(), stride, st.data());
      if (rc == ALN_OK) {
        tl.assign((size_t)np * ls, 0); ql.assign((size_t)np * ls, 0);
        rc = aln_batch_optimal_strings(bb, nullptr, ident.data(), nullptr, tl.data(), ql.data(), ls, len.data());
        if (rc == ALN_E_STARTPAIR) rc = ALN_OK;                 // reported per alignment
      }
      if (bb) aln_batch_destroy(bb);
      if (rc != ALN_OK) return rc;
      for (int32_t k = 0; k < np; ++k) {
        const size_t p = alive[g0 + k];
        if (!reported(a, sc[k], min_score)) continue;           // the hit ends here
        const int cnt = st[k] == 0 ? n[k] : 0;
        const int32_t* list = pairs.data() + (size_t)k * stride * 2;
        ao.put(slot_all[p] * (size_t)N + a, st[k], sc[k], ident[k], cnt, list, false, len[k], tl.data() + (size_t)k * ls,
               ql.data() + (size_t)k * ls);
        n_found[slot_all[p]] = a + 1;
        if (st[k] != 0 || a + 1 >= N) continue;                 // no list to forbid: the hit ends with this record
        const int64_t Q = queries->offsets[gq[k] + 1] - queries->offsets[gq[k]], T = templates->offsets[gt[k] + 1] - templates->offsets[gt[k]];
        if (a == 0) neg[p] = -(sc[k] + 1.f);
        for (int e = 0; e < cnt; ++e)
          if (list[2 * e] >= 1 && list[2 * e] <= Q - 2 && list[2 * e + 1] >= 1 && list[2 * e + 1] <= T - 2) {
            forbidden[p].push_back(list[2 * e]); forbidden[p].push_back(list[2 * e + 1]);
          }
        next.push_back(p);
      }
    }
    alive.swap(next);
  }
  return ALN_OK;
}

// The shared body of aln_hits_align_multi and aln_hits_align_multi_profiles (run: prepared; `queries`: the pool the query
// letters and lengths are read from — run.queries, or the consensus pool of a profile run).  Lines that differ with the query
// side are marked "side:".
static int multi_block(ScoreRun& run, const aln_seqs* queries, int32_t K, const aln_hit* hits, const int32_t* n_hits, int N,
                       float min_score, int32_t* n_found, aln_hit_alignment* out, int32_t* pairs, int32_t pair_stride, char* tlines,
                       char* qlines, int32_t line_stride, int32_t* lengths) {
  aln_ctx* ctx = run.ctx;
  const aln_seqs* templates = run.templates;
  const aln_qprofiles* prof = run.prof;
  const bool want_lines = tlines || qlines;
  const int rows = run.rows;
  if (rows == 0) return ALN_OK;
  auto q_len = [&](int q) { return (int64_t)(queries->offsets[q + 1] - queries->offsets[q]); };
  auto t_len = [&](int t) { return (int64_t)(templates->offsets[t + 1] - templates->offsets[t]); };

  // one walk: validate every used slot and describe it for its route (nothing is written before it ends).  The kernel finds
  // every round's end cell itself: the slots' are neither read nor checked.  side: the instantiations kept — every one
  // compiles without scratch memory and without VGPR spills
  SlotRoutes sr;
  int rc = route_slots(run, queries, K, hits, n_hits, prof ? ProfileQuery::kFusedMulti : ResidueQuery::kFusedMulti, false, sr);
  if (rc != ALN_OK) return rc;
  std::vector<MultiDesc> fast;                                 // (HitDesc is only route_slots' carrier here: its end cell and score stay 0)
  for (const HitDesc& d : sr.fast) fast.push_back(MultiDesc{d.q, d.t, d.cls, 0, 0, 0});
  const std::vector<size_t>& fast_slot = sr.fast_slot;
  const std::vector<int32_t>&bq = sr.bq, &bt = sr.bt;
  const std::vector<size_t>& bslot = sr.bslot;
  ctx->align_routes[0] = (int64_t)fast.size(); ctx->align_routes[1] = (int64_t)bq.size();
  AlignOut ao = {out, pairs, pair_stride, tlines, qlines, line_stride, lengths};
  for (size_t s = 0; s < (size_t)rows * K; ++s) {              // every record starts as "not reported"
    n_found[s] = 0;
    for (int a = 0; a < N; ++a) ao.clear(s * N + a);
  }

  // chunks of fused hits: a strip, a forbidden-cell plane, N lists and, where wanted, N pairs of lines each
  if (!fast.empty()) {
    FusedRoute<MultiDesc> fr(run, queries, fast);
    fr.cut(N, want_lines, line_stride, [&](const MultiDesc& d) {
      const int64_t Q = q_len(d.q), T = t_len(d.t);
      return HitNeed{(size_t)std::max<int64_t>(Q - 3, 1) * 256 * (size_t)d.cls, (size_t)Q * 8 * (size_t)d.cls, (int)std::min(Q, T) + 1};
    });
    const size_t max_n = fr.max_n, max_trav = fr.max_trav, max_e = max_n * (size_t)N;
    uint32_t* dmask = nullptr; int32_t *dtrav = nullptr, *dfound = nullptr;
    PairDesc* dpd = nullptr; StrOut* dso = nullptr; char* dlines = nullptr;
    HitRecords rec;                                            // N records per hit
    RTRY(fr.begin());
    STRY(fr.bufs.get(dmask, fr.max_mask));
    STRY(fr.bufs.get(dtrav, max_trav));
    STRY(fr.bufs.get(dfound, max_n));
    RTRY(rec.alloc(fr.bufs, max_e));
    std::vector<int32_t> hfound(max_n), htrav(max_trav);
    std::vector<PairDesc> hpd;
    std::vector<StrOut> hso;
    std::vector<char> hlines;
    if (want_lines || prof) RTRY(fr.upload_pools());
    if (want_lines) {
      STRY(fr.bufs.get(dpd, max_e));
      STRY(fr.bufs.get(dso, max_e));
      STRY(fr.bufs.get(dlines, max_e * 2 * (size_t)line_stride));
      hpd.resize(max_e); hso.resize(max_e); hlines.resize(max_e * 2 * (size_t)line_stride);
    }
    for (const FusedChunk& c : fr.chunks) {
      const int n = (int)c.n;
      const size_t ne = (size_t)n * N;
      RTRY(fr.stage(c));
      STRY(hipMemsetAsync(dmask, 0, c.mask * 4, ctx->stream));
      STRY(hipMemsetAsync(rec.dres, 0, ne * sizeof(PairResult), ctx->stream));   // rounds that are not reported: n_path 0, empty lines
      STRY(hipMemsetAsync(rec.dsame, 0, ne * 4, ctx->stream));
      MultiArgs g = {};
      g.desc = fr.ddesc; g.strip = fr.dstrip; g.mask = dmask; g.trav = dtrav; g.trav_stride = c.trav_stride; g.n_rounds = N;
      g.min_score = min_score; g.res = rec.dres; g.same = rec.dsame; g.n_found = dfound;
      RTRY(fr.launch(c, [&](auto side, int k, int cnt, const int32_t* list, const char* qch, const char* tch) {
        typedef decltype(side) Side;
        g.list = list;
        constexpr int kMax = ((Side::kFusedMulti >> 8) & 1u) ? 8 : 7;   // a class the mask leaves out never gets here
        dispatch_r<kMax>(k, [&](auto rc) {
          hipLaunchKernelGGL((align_local_multi_kernel<decltype(rc)::value, Side>), dim3(cnt), dim3(64), 0, ctx->stream, run.a, g, qch, tch);
        });
      }));
      if (want_lines) {
        for (int h = 0; h < n; ++h)
          std::fill_n(hpd.begin() + (size_t)h * N, N, pair_desc(queries, templates, fast[c.h0 + h].q, fast[c.h0 + h].t));
        STRY(hipMemcpyAsync(dpd, hpd.data(), ne * sizeof(PairDesc), hipMemcpyHostToDevice, ctx->stream));
        StrParams prm = {c.trav_stride, 1, 0, line_stride};
        RTRY(launch_gapped_strings(ctx, (int)ne, dpd, rec.dres, dtrav, fr.dqch, fr.dtch, dlines, dso, prm));
        STRY(hipMemcpyAsync(hso.data(), dso, ne * sizeof(StrOut), hipMemcpyDeviceToHost, ctx->stream));
        STRY(hipMemcpyAsync(hlines.data(), dlines, ne * 2 * (size_t)line_stride, hipMemcpyDeviceToHost, ctx->stream));
      }
      RTRY(rec.enqueue_download(ctx, ne));
      STRY(hipMemcpyAsync(hfound.data(), dfound, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
      if (pairs) STRY(hipMemcpyAsync(htrav.data(), dtrav, ne * c.trav_stride * 8, hipMemcpyDeviceToHost, ctx->stream));
      STRY(hipStreamSynchronize(ctx->stream));                 // the host vectors above are read by the copies until here
      for (int h = 0; h < n; ++h) {
        const MultiDesc& d = fast[c.h0 + h];
        const int64_t Q = q_len(d.q), T = t_len(d.t);
        const size_t slot = fast_slot[c.h0 + h];
        n_found[slot] = hfound[h];
        for (int a = 0; a < hfound[h]; ++a) {
          const size_t e = (size_t)h * N + a;
          put_fused(ao, slot * (size_t)N + a, rec.hres[e], rec.hsame[e], Q, T, htrav.data() + e * c.trav_stride * 2,
                    want_lines ? &hso[e] : nullptr, want_lines ? hlines.data() + e * 2 * line_stride : nullptr, line_stride);
        }
      }
    }
  }
  if (!bq.empty()) {
    rc = multi_through_batches(ctx, queries, templates, run.sub, prof, run.gap, bq, bt, bslot, N, min_score, n_found, ao);
    if (rc != ALN_OK) return rc;
  }
  return ao.worst;
}

}  // namespace aln

using namespace aln;

extern "C" int aln_hits_align_multi(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                                    const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K, const aln_hit* hits,
                                    const int32_t* n_hits, int32_t max_alignments, float min_score, int32_t* n_found,
                                    aln_hit_alignment* out, int32_t* pairs, int32_t pair_stride, char* tlines, char* qlines,
                                    int32_t line_stride, int32_t* lengths) {
  const bool ok = n_found && max_alignments >= 1 && max_alignments <= 16 &&
                  align_outputs_ok(K, hits, n_hits, out, pairs, pair_stride, tlines, qlines, line_stride, lengths);
  return hit_entry(ctx, false, queries, nullptr, nullptr, templates, sub, gap, q_begin, q_end, ok, [&](ScoreRun& run, const aln_seqs* pool) {
    if (!run.local) return (int)ALN_E_ARG;
    return multi_block(run, pool, K, hits, n_hits, max_alignments, min_score, n_found, out, pairs, pair_stride, tlines, qlines,
                       line_stride, lengths);
  });
}

// The same for the hits of a profile search.  The query letters — the lines and the identity need them, the scores never do —
// are the caller's consensus pool or, without one, the placeholder pool the run builds for profiles.
extern "C" int aln_hits_align_multi_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus,
                                             const aln_seqs* templates, const aln_gap* gap, int32_t q_begin, int32_t q_end,
                                             int32_t K, const aln_hit* hits, const int32_t* n_hits, int32_t max_alignments,
                                             float min_score, int32_t* n_found, aln_hit_alignment* out, int32_t* pairs,
                                             int32_t pair_stride, char* tlines, char* qlines, int32_t line_stride, int32_t* lengths) {
  const bool ok = n_found && max_alignments >= 1 && max_alignments <= 16 &&
                  align_outputs_ok(K, hits, n_hits, out, pairs, pair_stride, tlines, qlines, line_stride, lengths);
  return hit_entry(ctx, true, nullptr, profiles, consensus, templates, nullptr, gap, q_begin, q_end, ok, [&](ScoreRun& run, const aln_seqs* pool) {
    if (!run.local) return (int)ALN_E_ARG;
    return multi_block(run, pool, K, hits, n_hits, max_alignments, min_score, n_found, out, pairs, pair_stride, tlines, qlines,
                       line_stride, lengths);
  });
}

#undef STRY
#undef RTRY
