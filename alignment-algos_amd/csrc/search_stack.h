// search_stack.h — the letters rows of a group of consecutive queries, resident on the device in slot order, and what is read
// off them: what aln_hits_weights (search_weights.hip) and aln_hits_purge (search_purge.hip) share on the host.
//   HitStack       the routing of a block's slots (route_slots, then the alphabet: nothing is written before both have passed),
//                  the group sizing under the budgets, and per group the construction of the stack: preset to '.', the fused
//                  hits chunk by chunk through FusedRoute, launch_pileup_job and the scatter, the batch slots through
//                  for_list_groups, laid out on the host (pileup_from_list) and uploaded; the records filed as they come down.
//   StackWeights   the buffers of the four weight launches over a complete group, the launches, the download and the filing of
//                  weights, raw, counts and covered.
// The kernels are instantiated ONCE, in search_weights.hip, behind two ordinary functions (launch_scatter_rows,
// launch_weight_kernels), as the pileup kernels are behind launch_pileup_job.  aln_hits_pssm (search_pssm.hip) runs
// aln_hits_purge's body, purge_block, with a hook over every group's count rows (StackHook, below).
#pragma once
#include <algorithm>
#include <climits>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "search_pileup.h"

namespace aln {

constexpr size_t kStackBudget = (size_t)1 << 30;        // bytes of letters rows resident at a time
constexpr int kSpareCol = 31;                           // the alphabet has at most 30 letters: k_p, or covered

struct WeightQuery {        // one query row of the group
  int64_t row;              // the count row of its position 0 (query row 1), relative to the group's first count row
  int32_t len;              // Q - 2
  int32_t pad;
};

// scatter_rows_kernel over the n hits of a chunk: row h of src into slot[h] of the stack (search_weights.hip)
int launch_scatter_rows(aln_ctx* ctx, const char* src, char* stack, const int32_t* slot, int64_t stride, size_t n);

// The four launches over a complete group of gn queries (search_weights.hip): the tally into np, the slots' sums into raw, the
// weights into wt and, cnt != nullptr, the g_rows count rows under the weights (zeroed first: the sentinel rows stay zero).
struct WeightLaunch {
  const char* stack; int64_t stride; int K; size_t gn, g_rows;
  const WeightQuery* qr; const int8_t* idx; int w_max;
  int32_t *np, *wt, *cnt; int64_t* raw;
};
int launch_weight_kernels(aln_ctx* ctx, const WeightLaunch& w);

struct StackGroup {         // queries [g0, g0 + gn) of the block: slots from slot0, g_rows count rows from row grow0 of the pool
  size_t g0, gn, slot0, g_rows;
  int64_t grow0;
};

struct HitStack {
  ScoreRun& run; const aln_seqs* queries; int32_t K;
  SlotRoutes sr;
  AlignOut ao;
  int8_t idx[256];                                      // character -> index in the alphabet, -1 for every other byte
  int n_alpha = 0;
  int64_t row0 = 0, maxw = 1;                           // the block's first count row; its longest Q - 2
  size_t n_rows = 0, dw = 1, group = 1, max_grows = 1;  // count rows of the block; the stride; rows and most count rows of a group
  DeviceBufs own;
  char* dstack = nullptr; int8_t* didx = nullptr; WeightQuery* dqr = nullptr;
  std::vector<WeightQuery> hqr;
  std::vector<char> hrow;

  HitStack(ScoreRun& r, const aln_seqs* q, int32_t K_, aln_hit_alignment* out)
      : run(r), queries(q), K(K_), ao{out, nullptr, 0, nullptr, nullptr, 0, nullptr}, own(r) {}

  // route_slots' walk (every used slot validated and described for its route), then the alphabet; nothing written before
  int route(const aln_hit* hits, const int32_t* n_hits) {
    n_alpha = run.prof ? run.prof->n : run.sub->n;
    const char* alphabet = run.prof ? run.prof->alphabet : run.sub->alphabet;
    row0 = queries->offsets[run.q_begin];
    n_rows = (size_t)(queries->offsets[run.q_end] - row0);
    for (int q = run.q_begin; q < run.q_end; ++q) maxw = std::max<int64_t>(maxw, queries->offsets[q + 1] - queries->offsets[q] - 2);
    const int rc = route_slots(run, queries, K, hits, n_hits, hit_kernel_classes(run), run.local, sr);
    if (rc != ALN_OK) return rc;
    memset(idx, -1, sizeof idx);
    for (int i = 0; i < n_alpha; ++i) {
      if (alphabet[i] == '.' || alphabet[i] == '-') return ALN_E_ARG;      // the pileup could not show them as letters
      idx[(unsigned char)alphabet[i]] = (int8_t)i;
    }
    run.ctx->align_routes[0] = (int64_t)sr.fast.size(); run.ctx->align_routes[1] = (int64_t)sr.bq.size();
    return ALN_OK;
  }

  // Groups of consecutive queries: as many rows as keep the stack below the budget and, row_bytes > 0, what else a caller keeps
  // per query row below it too; the hint only asks for fewer.  stride_align: what the stride is rounded up to (the padding
  // holds '.').  Then the stack, the table and the queries' records on the device.
  int alloc(size_t stride_align, size_t row_bytes) {
    aln_ctx* ctx = run.ctx;
    const size_t rows = (size_t)run.rows;
    dw = ((size_t)maxw + stride_align - 1) / stride_align * stride_align;
    group = std::max<size_t>(kStackBudget / ((size_t)K * dw), 1);
    if (row_bytes > 0) group = std::min(group, std::max<size_t>(kStackBudget / row_bytes, 1));
    if (ctx->hints.weights_group_rows > 0) group = std::min(group, (size_t)ctx->hints.weights_group_rows);
    group = std::min(std::min(group, rows), (size_t)32768);    // (a group's rows are a launch's blockIdx.y)
    for (size_t g0 = 0; g0 < rows; g0 += group) {
      const size_t g1 = std::min(g0 + group, rows);
      max_grows = std::max(max_grows, (size_t)(queries->offsets[run.q_begin + g1] - queries->offsets[run.q_begin + g0]));
    }
    STRY(own.get(dstack, group * K * dw));
    STRY(own.get(didx, 256));
    STRY(own.get(dqr, group));
    STRY(hipMemcpyAsync(didx, idx, sizeof idx, hipMemcpyHostToDevice, ctx->stream));        // (alive until the first synchronisation)
    hqr.resize(group);
    hrow.resize(dw);
    return ALN_OK;
  }

  // Group by group: the stack built, the group's records filed, then body(group) over the complete stack.  body leaves with
  // the stream synchronised.  who: the entry's name, for an error's text.
  template <class Body>
  int build(const char* who, Body&& body) {
    aln_ctx* ctx = run.ctx;
    const aln_seqs* templates = run.templates;
    const size_t rows = (size_t)run.rows;
    size_t f0 = 0, b0 = 0;                                     // the group's first fused hit and first batch slot (both row-major)
    for (size_t g0 = 0; g0 < rows; g0 += group) {
      const size_t g1 = std::min(g0 + group, rows), gn = g1 - g0;
      const size_t slot0 = g0 * K, slot1 = g1 * K;
      const int64_t grow0 = queries->offsets[run.q_begin + g0];
      const size_t g_rows = (size_t)(queries->offsets[run.q_begin + g1] - grow0);
      size_t f1 = f0, b1 = b0;
      while (f1 < sr.fast.size() && sr.fast_slot[f1] < slot1) ++f1;
      while (b1 < sr.bq.size() && sr.bslot[b1] < slot1) ++b1;
      for (size_t r = 0; r < gn; ++r) {
        const int64_t o = queries->offsets[run.q_begin + g0 + r];
        hqr[r] = WeightQuery{o - grow0 + 1, (int32_t)(queries->offsets[run.q_begin + g0 + r + 1] - o - 2), 0};
      }
      STRY(hipMemcpyAsync(dqr, hqr.data(), gn * sizeof(WeightQuery), hipMemcpyHostToDevice, ctx->stream));
      STRY(hipMemsetAsync(dstack, '.', gn * K * dw, ctx->stream));

      // the group's fused hits, chunk by chunk: the rows of a chunk, then their move into the stack
      if (f1 > f0) {
        std::vector<HitDesc> fast(sr.fast.begin() + f0, sr.fast.begin() + f1);
        const std::vector<size_t> fast_slot(sr.fast_slot.begin() + f0, sr.fast_slot.begin() + f1);
        FusedRoute<HitDesc> fr(run, queries, fast);
        std::vector<int32_t> fast_live(fast.size()), fast_at(fast.size());
        for (size_t h = 0; h < fast.size(); ++h) {
          fast_live[h] = (run.local && !(fast[h].score > 0.f)) ? 0 : 1;
          fast_at[h] = (int32_t)(fast_slot[h] - slot0);
        }
        fr.cut(1, true, (int)std::min<int64_t>(maxw, INT_MAX),
               [&](const HitDesc& d) { return HitNeed{hit_strip_bytes(run, queries, d), 0, 0}; });
        const size_t max_n = fr.max_n;
        int32_t *dlive = nullptr, *dat = nullptr; char* dlet = nullptr; PileupRows* drows = nullptr;
        HitRecords rec;
        RTRY(fr.begin());
        STRY(fr.bufs.get(dlive, max_n));
        STRY(fr.bufs.get(dat, max_n));
        RTRY(rec.alloc(fr.bufs, max_n));
        STRY(fr.bufs.get(dlet, max_n * dw));
        STRY(fr.bufs.get(drows, 1));
        RTRY(fr.upload_pools());                                 // the templates' characters, on both sides
        const PileupRows where = {dlive, fr.dtch, dlet, nullptr, nullptr, (int64_t)dw};   // (alive until the first chunk's synchronisation)
        STRY(hipMemcpyAsync(drows, &where, sizeof(where), hipMemcpyHostToDevice, ctx->stream));
        for (const FusedChunk& c : fr.chunks) {
          const size_t n = c.n;
          RTRY(fr.stage(c, [&]() -> int {
            STRY(hipMemcpyAsync(dlive, fast_live.data() + c.h0, n * 4, hipMemcpyHostToDevice, ctx->stream));
            STRY(hipMemcpyAsync(dat, fast_at.data() + c.h0, n * 4, hipMemcpyHostToDevice, ctx->stream));
            STRY(hipMemsetAsync(dlet, '.', n * dw, ctx->stream));
            return ALN_OK;
          }));
          PileupArgs g = {};
          g.desc = fr.ddesc; g.strip = fr.dstrip; g.rows = drows; g.res = rec.dres; g.same = rec.dsame;
          RTRY(launch_pileup_job(fr, c, g));
          RTRY(launch_scatter_rows(ctx, dlet, dstack, dat, (int64_t)dw, n));
          RTRY(rec.enqueue_download(ctx, n));
          STRY(hipStreamSynchronize(ctx->stream));               // the records' host images are read by the copies until here
          rec.put(ao, fr, c, fast_slot, [](size_t, size_t, int64_t) {});
        }
      }

      // the group's batch slots (for_list_groups, search_align.h): every surviving slot's row laid out here and uploaded
      if (b1 > b0) {
        SlotRoutes gs;
        gs.bq.assign(sr.bq.begin() + b0, sr.bq.begin() + b1);
        gs.bt.assign(sr.bt.begin() + b0, sr.bt.begin() + b1);
        gs.bslot.assign(sr.bslot.begin() + b0, sr.bslot.begin() + b1);
        int up = ALN_OK;
        const int rc = for_list_groups(run, queries, gs, ao, [&](size_t slot, int32_t q, int32_t t, const int32_t* l, int n_pairs) {
          const int64_t Q = queries->offsets[q + 1] - queries->offsets[q];
          const int64_t to = templates->offsets[t], T = templates->offsets[t + 1] - to;
          if (Q < 3 || up != ALN_OK) return;
          memset(hrow.data(), '.', (size_t)(Q - 2));
          pileup_from_list(l, n_pairs, Q, T, templates->residues + to, hrow.data(), nullptr, nullptr);
          if (hipMemcpyAsync(dstack + (slot - slot0) * dw, hrow.data(), (size_t)(Q - 2), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
              hipStreamSynchronize(ctx->stream) != hipSuccess) {   // hrow is written again for the next slot
            ctx->last_error = std::string(who) + ": upload of a batch slot's row failed";
            up = ALN_E_HIP;
          }
        });
        RTRY(rc);
        RTRY(up);
      }

      RTRY(body(StackGroup{g0, gn, slot0, g_rows, grow0}));      // the stack is complete
      f0 = f1; b0 = b1;
    }
    return ALN_OK;
  }
};

// The weights of a complete group and the counts under them: buffers, the four launches, the download, the filing.  Outputs:
// weights (required) and raw rows x K, counts and covered in aln_hits_column_counts' layout; each but weights may be nullptr.
// keep_rows: the weighted count rows are made and stay on the device (dcnt, 32 int32 each, covered in column kSpareCol) also
// when neither counts nor covered is downloaded — aln_hits_pssm reads them there.
struct StackWeights {
  HitStack& st; int32_t w_max;
  int32_t* weights; int64_t* raw; int32_t* counts; int32_t* covered;
  bool want_counts, keep_rows;
  int32_t *dnp = nullptr, *dcnt = nullptr, *dwt = nullptr; int64_t* draw = nullptr;
  std::vector<int32_t> hcnt;

  StackWeights(HitStack& s, int32_t w_max_, int32_t* weights_, int64_t* raw_, int32_t* counts_, int32_t* covered_,
               bool keep_rows_ = false)
      : st(s), w_max(w_max_), weights(weights_), raw(raw_), counts(counts_), covered(covered_), want_counts(counts_ || covered_),
        keep_rows(keep_rows_) {}

  // what a slot or count row nothing reaches holds
  void clear() {
    const size_t n_slots = (size_t)st.run.rows * st.K;
    memset(weights, 0, n_slots * 4);
    if (raw) memset(raw, 0, n_slots * 8);
    if (counts) memset(counts, 0, st.n_rows * (size_t)st.n_alpha * 4);
    if (covered) memset(covered, 0, st.n_rows * 4);
  }
  int alloc() {
    aln_ctx* ctx = st.run.ctx;
    STRY(st.own.get(dnp, st.max_grows * 32));
    if (want_counts || keep_rows) STRY(st.own.get(dcnt, st.max_grows * 32));
    STRY(st.own.get(dwt, st.group * st.K));
    STRY(st.own.get(draw, st.group * st.K));
    hcnt.resize(want_counts ? st.max_grows * 32 : 0);
    return ALN_OK;
  }
  // the tally, the slots' sums, the weights, the weighted tally; what comes down; leaves with the stream synchronised
  int group(const StackGroup& g) {
    aln_ctx* ctx = st.run.ctx;
    const size_t K = (size_t)st.K;
    const WeightLaunch w = {st.dstack, (int64_t)st.dw, (int)st.K, g.gn, g.g_rows, st.dqr, st.didx, (int)w_max,
                            dnp, dwt, dcnt, draw};
    RTRY(launch_weight_kernels(ctx, w));
    if (want_counts) STRY(hipMemcpyAsync(hcnt.data(), dcnt, g.g_rows * 128, hipMemcpyDeviceToHost, ctx->stream));
    STRY(hipMemcpyAsync(weights + g.slot0, dwt, g.gn * K * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (raw) STRY(hipMemcpyAsync(raw + g.slot0, draw, g.gn * K * 8, hipMemcpyDeviceToHost, ctx->stream));
    STRY(hipStreamSynchronize(ctx->stream));
    if (want_counts) {
      const size_t base = (size_t)(g.grow0 - st.row0);
      for (size_t r = 0; r < g.g_rows; ++r) {
        if (counts) memcpy(counts + (base + r) * (size_t)st.n_alpha, hcnt.data() + r * 32, (size_t)st.n_alpha * 4);
        if (covered) covered[base + r] = hcnt[r * 32 + kSpareCol];
      }
    }
    return ALN_OK;
  }
};

// The shared body of aln_hits_purge and aln_hits_purge_profiles (search_purge.hip), which aln_hits_pssm (search_pssm.hip) runs
// too: with `after` the weighted count rows of a group stay on the device (sw.dcnt) and after(st, sw, group) reads them there,
// once the group's weights have come down; it leaves with the stream synchronised.
using StackHook = std::function<int(HitStack&, StackWeights&, const StackGroup&)>;
int purge_block(ScoreRun& run, const aln_seqs* queries, int32_t K, const aln_hit* hits, const int32_t* n_hits,
                int32_t max_identity, int32_t min_overlap, int32_t w_max, aln_hit_alignment* out, aln_hit_purge* purge,
                int32_t* weights, int64_t* raw, int32_t* counts, int32_t* covered, const StackHook* after = nullptr);

}  // namespace aln
