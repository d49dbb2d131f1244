// score_only.hip — all-vs-all local alignment SCORES, no planes (BASELINE config 5) (gfx950).
//
// The score Optimal reports for a local build is find_max over the matrix (optimal.h:90-93, :108-124): the
// maximum cell of the DPMatrix::build_forw_local_dpm_nonlinear_gaps recurrence (dpmatrix.h:538-689).  When nobody
// needs cells or pointers nothing per-cell has to touch HBM: one wave per (query, template) pair sweeps the rows
// with the whole state in VGPRs — the same collapsed recurrence as dp_affine_tag.hip, without tags:
//   E(j) by a DPP max-plus prefix scan of A(k) = D[i-1][k] + ge k, F by a per-column running max of D[k][c] + ge k,
//   best = max3(match, E, F) + S, clipped at 0, running maximum per lane.
// The sweep itself is score_sweep.h's (sweep_local, sweep_global); only the packed 16-bit kernel below carries its own.
// Algorithmic bytes per pair: |q| + |t| residue bytes in, 4 bytes out (~0 B/cell) — the kernel is
// bound by VALU issue (about 6 half-rate + 8 full-rate instructions per cell), not by HBM.
// Grid: x = template index, y = query index inside the caller's row block; templates are replicated on every GPU,
// query rows are what ranks shard.
// Queries given as POSITION-SPECIFIC rows (aln_qprofiles) run the same two kernels, instantiated for the profile side
// (ProfileQuery, score_common.h): same recurrence, same results as a full build over the Q x T plane of the profile
// (aln_batch_dp with ALN_SIM_MATRIX) + Optimal; only where a row's 32 similarities in LDS come from differs (ProfileRows,
// score_sweep.h).  There is no packed kernel for them.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "score_common.h"
#include "score_sweep_qgaps.h"   // kQGapWord: where a device row keeps its gap prices

namespace aln {

// One kernel per job for both query sides (ResidueQuery, ProfileQuery: score_common.h); one wave per pair.
template <int R, class Side>
__global__ __launch_bounds__(64) void score_local_kernel(ScoreArgs a) {
  __shared__ __attribute__((aligned(16))) int lds[32 * 32];
  const int lane = threadIdx.x;
  Side::stage(lds, a);
  const int ti = a.tsel[blockIdx.x], qi = a.q_begin + blockIdx.y;
  const typename Side::Rows::Src* __restrict__ qr = Side::rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);
  LocalCols<R> cols;
  cols.load(tc, T, a.gi, a.ge);
  int d[R][4];
  int m = sweep_local<R, typename Side::Rows>(lds, cols, qr, Q - 2, d, NoObserver());
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o));
  if (lane == 0) a.scores[(size_t)blockIdx.y * a.n_t + ti] = (float)m;
}


// ---- the four non-local align types: the score Optimal reports is the FINAL cell's (optimal.h:56-74) ---------------------------
template <int R, class Side>
__global__ __launch_bounds__(64) void score_global_kernel(ScoreArgs a, int free_del, int free_ins) {
  __shared__ __attribute__((aligned(16))) int lds[32 * 32];
  const int lane = threadIdx.x;
  Side::stage(lds, a);
  const int ti = a.tsel[blockIdx.x], qi = a.q_begin + blockIdx.y;
  const typename Side::Rows::Src* __restrict__ qr = Side::rows(a, qi);
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const int Q = (int)(a.qoff[qi + 1] - a.qoff[qi]), T = (int)(a.toff[ti + 1] - a.toff[ti]);
  const int gi = a.gi, ge = a.ge;
  float* out = &a.scores[(size_t)blockIdx.y * a.n_t + ti];
  // degenerate shortcuts (dpmatrix.h:375-390): no interior row or column -> one gap from the origin, never clipped
  if (Q == 2 || T == 2) {
    int cost = 0;
    if (Q == 2) { const int len = T - 2; cost = (len < 1 || free_del) ? 0 : gi + ge * (len - 1); }
    else { const int len = Q - 2; cost = (len < 1 || free_ins) ? 0 : gi + ge * (len - 1); }
    if (lane == 0) *out = (float)(-cost);
    return;
  }
  GlobalCols<R> cols;
  cols.load(tc, T, gi, ge);
  int best = sweep_global<R, typename Side::Rows>(lds, cols, qr, Q, free_del, free_ins, NoObserver());
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) best = max(best, __shfl_xor(best, o));
  if (lane == 0) *out = (float)best;
}


// ---- two queries per wave in packed 16-bit lanes --------------------------------------------------------------------
// v_max_i32 issues at half rate on gfx950 and so does v_pk_max_i16 — which does two.  When every intermediate fits in 15 bits
// (checked on the host) the low half of each register carries query A and the high half query B against the same template:
// the recurrence, the DPP prefix scans and the one-column shift act on both halves at once, the substitution score comes
// from a per-row table of packed pairs (tab[qA[i]][c], tab[qB[i]][c]) that 32 lanes rebuild in LDS for every row.
typedef short s2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s2 as_s2(int v) { return __builtin_bit_cast(s2, v); }
__device__ __forceinline__ int as_i(s2 v) { return __builtin_bit_cast(int, v); }
__device__ __forceinline__ s2 dup2(int v) { return as_s2((v & 0xFFFF) | (v << 16)); }
__device__ __forceinline__ s2 pmax(s2 a, s2 b) { return __builtin_elementwise_max(a, b); }
constexpr int kNeg16 = -12000;          // "minus infinity" of the packed kernel: below every real value, clear of int16 wrap-around

__device__ __forceinline__ s2 wave_incl_max_pk(s2 v) {
  const int ident = (int)0x80008000;
  v = pmax(v, as_s2(sdpp<0x111>(ident, as_i(v))));
  v = pmax(v, as_s2(sdpp<0x112>(ident, as_i(v))));
  v = pmax(v, as_s2(sdpp<0x114>(ident, as_i(v))));
  v = pmax(v, as_s2(sdpp<0x118>(ident, as_i(v))));
  v = pmax(v, as_s2(sdpp<0x142, 0xA>(ident, as_i(v))));
  v = pmax(v, as_s2(sdpp<0x143, 0xC>(ident, as_i(v))));
  return v;
}

template <int R>
__global__ __launch_bounds__(64) void score_local_pk_kernel(ScoreArgs a, int n_rows) {
  __shared__ int tab[32 * 32];
  __shared__ int prow[2][32];           // packed substitution row of the current query residues, double-buffered by row parity
  const int lane = threadIdx.x;
  for (int k = lane; k < 32 * 32; k += 64) tab[k] = a.table32[k];
  __syncthreads();
  const int ti = a.tsel[blockIdx.x];
  const int rowA = a.qsel[2 * blockIdx.y], rowB_ = a.qsel[(2 * blockIdx.y + 1 < n_rows) ? 2 * blockIdx.y + 1 : 2 * blockIdx.y];
  const int qiA = a.q_begin + rowA, qiB = a.q_begin + rowB_;
  const uint8_t* __restrict__ qcA = a.qcodes + a.qoff[qiA];
  const uint8_t* __restrict__ qcB = a.qcodes + a.qoff[qiB];
  const uint8_t* __restrict__ tc = a.tcodes + a.toff[ti];
  const int QA = (int)(a.qoff[qiA + 1] - a.qoff[qiA]), QB = (int)(a.qoff[qiB + 1] - a.qoff[qiB]);
  const int T = (int)(a.toff[ti + 1] - a.toff[ti]);
  const int Qm = QA > QB ? QA : QB, Qs = QA > QB ? QB : QA;
  const int gi = a.gi, ge = a.ge;
  const int cb = 4 * lane;
  const int gime = gi - ge;
  const s2 zero2 = dup2(0), neg2 = dup2(kNeg16);

  int code4[R][4], inm[R][4];
  s2 gec[R][4], ekc[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int c = cb + 256 * r + x;
      int code = kCodeTail;
      if (c < T) code = tc[c];
      code4[r][x] = code * 4;
      gec[r][x] = dup2(ge * c);
      ekc[r][x] = dup2(ge * c + gime);
      inm[r][x] = ((unsigned)(c - 1) < (unsigned)(T - 2)) ? -1 : 0;
    }
  s2 d[R][4], gmx[R][4], cv[R], ak[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    cv[r] = neg2;
#pragma unroll
    for (int x = 0; x < 4; ++x) { d[r][x] = zero2; gmx[r][x] = neg2; ak[r][x] = neg2; }
  }
  s2 lmax = zero2, snap = zero2;
  // the packed substitution row of query row i: lanes 0..31 build it (residue indices clamped for the shorter query)
  auto build_row = [&](int i) {
    if (lane < 32) {
      const int ia = i < QA ? i : QA - 1, ib = i < QB ? i : QB - 1;
      const int va = tab[(int)qcA[ia] * 32 + lane], vb = tab[(int)qcB[ib] * 32 + lane];
      prow[i & 1][lane] = (va & 0xFFFF) | (vb << 16);
    }
    __syncthreads();
  };
  auto row_at = [&](int i, int c4) -> s2 {
    return as_s2(*reinterpret_cast<const int*>(reinterpret_cast<const char*>(prow[i & 1]) + c4));
  };
  auto finish_row = [&]() {
    s2 sk = neg2;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      s2 tk = neg2;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        s2 A = d[r][x] + gec[r][x];
        if (r == 0 && x == 0) A = (lane == 0) ? neg2 : A;    // column 0 is never a source
        ak[r][x] = A;
        tk = pmax(tk, A);
      }
      lmax = pmax(pmax(lmax, pmax(d[r][0], d[r][1])), pmax(d[r][2], d[r][3]));
      const s2 ik = wave_incl_max_pk(tk);
      const s2 ek = as_s2(sdpp<0x138>(as_i(neg2), as_i(ik)));
      cv[r] = pmax(sk, ek);
      sk = pmax(sk, as_s2(__builtin_amdgcn_readlane(as_i(ik), 63)));
    }
  };
  if (Qs < 3) snap = zero2;                                  // a query without interior rows scores 0
  if (Qm >= 3) {
    build_row(1);
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const s2 h = pmax(row_at(1, code4[r][x]), zero2);
        d[r][x] = as_s2(as_i(h) & inm[r][x]);
      }
    finish_row();
    if (Qs - 2 == 1) snap = lmax;
  }
  for (int i = 2; i <= Qm - 2; ++i) {
    build_row(i);
    const s2 roff = dup2(gi + ge * (i - 2));
    const s2 rowB = dup2(ge * (i - 1));
    s2 bk[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      s2 pv = cv[r];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const s2 m = d[r][x];
        const s2 e = pv - ekc[r][x];
        const s2 f = gmx[r][x] - roff;
        bk[r][x] = pmax(pmax(m, e), f);
        pv = pmax(pv, ak[r][x]);
        gmx[r][x] = pmax(gmx[r][x], m + rowB);
      }
    }
    int prev_k = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int uk = sdpp<0x138>(0, as_i(bk[r][3]));
      if (r > 0) uk = (lane == 0) ? prev_k : uk;
      prev_k = __builtin_amdgcn_readlane(as_i(bk[r][3]), 63);
      const bool masked = (r == 0) || (256 * (r + 1) > T - 1);
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int c = cb + 256 * r + x;
        const s2 sv = row_at(i, code4[r][x]);
        s2 h = pmax(((x == 0) ? as_s2(uk) : bk[r][x - 1]) + sv, zero2);
        if (r == 0 && x == 1) h = (c == 1) ? pmax(sv, zero2) : h;
        if (masked) h = as_s2(as_i(h) & inm[r][x]);
        d[r][x] = h;
      }
    }
    finish_row();
    if (i == Qs - 2) snap = lmax;                            // the shorter query ends here; later rows of its half are not its own
  }
  // the longer query's half of lmax, the shorter one's half of snap
  const int full = as_i(lmax), part = as_i(snap);
  int mA = (short)(((QA >= QB) ? full : part) & 0xFFFF);
  int mB = (short)((((QB >= QA) ? full : part) >> 16) & 0xFFFF);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { mA = max(mA, __shfl_xor(mA, o)); mB = max(mB, __shfl_xor(mB, o)); }
  if (lane == 0) {
    a.scores[(size_t)rowA * a.n_t + ti] = (float)mA;
    if (rowB_ != rowA) a.scores[(size_t)rowB_ * a.n_t + ti] = (float)mB;
  }
}

// The general route: scores[(q - q_begin) * ld + col[t]] for the templates listed in `tlist`, through resident batches of full
// DP builds (aln_batch_dp picks the kernel: tagged keys, int32 rows, exact-order scans) + Optimal's score — what the reference does
// for every pair, kept for what the register-resident kernels above do not take: templates beyond 2048 columns, fractional tables
// or gaps.  Pairs are grouped so that one group's planes stay below ~12 GB.
int score_through_batches(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                          const aln_gap* gap, int32_t q_begin, int32_t q_end, const std::vector<int32_t>& tlist, float* scores,
                          const int32_t* col, size_t ld, const aln_qprofiles* prof) {
  if (ld == 0) ld = (size_t)templates->n_seqs;
  const size_t budget = kBatchPlaneBudget;      // (no BatchGroup: the pairs are made as they are grouped, and there is no pair limit)
  std::vector<int32_t> qi, tix;
  std::vector<float> sc;
  std::vector<int32_t> st;
  auto flush = [&]() -> int {
    if (qi.empty()) return ALN_OK;
    aln_batch* bb = nullptr;
    BatchSim bs;
    bs.set(sub, prof, templates, qi.size(), qi.data(), tix.data());
    int rc = aln_batch_create(ctx, queries, templates, (int32_t)qi.size(), qi.data(), tix.data(), 0, &bb);
    if (rc == ALN_OK) rc = aln_batch_dp(bb, &bs.sim, gap, ALN_FWD, ALN_DP_AUTO, 0);
    sc.resize(qi.size()); st.resize(qi.size());
    if (rc == ALN_OK) rc = aln_batch_optimal(bb, sc.data(), nullptr, nullptr, 0, st.data());
    if (bb) aln_batch_destroy(bb);
    if (rc != ALN_OK) return rc;
    for (size_t k = 0; k < qi.size(); ++k) {
      if (st[k] != 0) return st[k];
      scores[(size_t)(qi[k] - q_begin) * ld + (col ? col[tix[k]] : tix[k])] = sc[k];
    }
    qi.clear(); tix.clear();
    return ALN_OK;
  };
  size_t bytes = 0;
  for (int32_t t : tlist) {
    const size_t T = (size_t)(templates->offsets[t + 1] - templates->offsets[t]);
    for (int32_t q = q_begin; q < q_end; ++q) {
      const size_t Q = (size_t)(queries->offsets[q + 1] - queries->offsets[q]);
      const size_t need = batch_pair_bytes(Q, T, prof != nullptr);
      if (!qi.empty() && bytes + need > budget) { int rc = flush(); if (rc) return rc; bytes = 0; }
      qi.push_back(q); tix.push_back(t); bytes += need;
    }
  }
  return flush();
}

void BatchSim::set(const aln_submatrix* sub, const aln_qprofiles* prof, const aln_seqs* templates, size_t n_pairs,
                   const int32_t* qi, const int32_t* ti) {
  if (!prof) { sim.kind = ALN_SIM_SUBMATRIX; sim.sub = *sub; return; }
  int idx[256];
  for (int i = 0; i < 256; ++i) idx[i] = -1;
  for (int i = 0; i < prof->n; ++i) idx[(unsigned char)prof->alphabet[i]] = i;
  plane_off.assign(n_pairs + 1, 0);
  for (size_t p = 0; p < n_pairs; ++p) {
    const int64_t Q = prof->offsets[qi[p] + 1] - prof->offsets[qi[p]], T = templates->offsets[ti[p] + 1] - templates->offsets[ti[p]];
    plane_off[p + 1] = plane_off[p] + Q * T;
  }
  planes.assign((size_t)plane_off[n_pairs], 0.f);
  for (size_t p = 0; p < n_pairs; ++p) {
    const int64_t off = prof->offsets[qi[p]], Q = prof->offsets[qi[p] + 1] - off;
    const int64_t t0 = templates->offsets[ti[p]], T = templates->offsets[ti[p] + 1] - t0;
    float* S = planes.data() + plane_off[p];
    for (int64_t i = 1; i <= Q - 2; ++i) {
      const float* row = prof->rows + (size_t)(off + i) * prof->n;
      for (int64_t j = 1; j <= T - 2; ++j) S[i * T + j] = row[idx[(unsigned char)templates->residues[t0 + j]]];   // checked by prepare()
    }
  }
  sim.kind = ALN_SIM_MATRIX;
  sim.planes = planes.data();
  sim.plane_off = plane_off.data();
}

int ScoreRun::prepare(aln_ctx* ctx_, const aln_seqs* queries_, const aln_seqs* templates_, const aln_submatrix* sub_,
                      const aln_gap* gap_, int32_t q_begin_, int32_t q_end_, const aln_qprofiles* prof_) {
  ctx = ctx_; queries = queries_; templates = templates_; sub = sub_; gap = gap_; q_begin = q_begin_; q_end = q_end_; prof = prof_;
  route = kNothing;
  if (!ctx || !templates || (qgaps ? !prof : !gap) || (prof ? false : (!queries || !sub))) return ALN_E_ARG;
  if (q_begin < 0 || q_end > (prof ? prof->n_seqs : queries->n_seqs) || q_begin > q_end) return ALN_E_ARG;
  if (!qgaps && gap->model != ALN_GAP_AFFINE_CONST) return ALN_E_ARG;
  const int32_t align_type = qgaps ? qgaps_align_type : gap->align_type;
  if (align_type < 0 || align_type > 4) return ALN_E_ARG;
  local = align_type == ALN_LOCAL;
  free_del = (align_type == ALN_LOCAL || align_type == ALN_SEMI_LOCAL || align_type == ALN_LOCAL_GLOBAL);
  free_ins = (align_type == ALN_LOCAL || align_type == ALN_SEMI_LOCAL || align_type == ALN_GLOBAL_LOCAL);
  if (prof) {
    if (prof->n < 1 || prof->n > 30 || !prof->alphabet || !prof->rows || !prof->offsets || prof->n_seqs < 0) return ALN_E_ARG;
    for (int s = 0; s < prof->n_seqs; ++s)
      if (prof->offsets[s + 1] - prof->offsets[s] < 2) return ALN_E_ARG;
    if (consensus) {
      if (consensus->n_seqs != prof->n_seqs || !consensus->offsets || !consensus->residues) return ALN_E_ARG;
      for (int s = 0; s <= prof->n_seqs; ++s)
        if (consensus->offsets[s] != prof->offsets[s]) return ALN_E_ARG;
    }
    // gap rows live in words 26 .. 29 of a device row (score_sweep_qgaps.h)
    if (qgaps && (prof->n > 26 || !qgaps->del_init || !qgaps->del_extn || !qgaps->ins_init || !qgaps->ins_extn)) return ALN_E_ARG;
    ph_res.assign((size_t)prof->offsets[prof->n_seqs], prof->alphabet[0]);
    for (int s = 0; s < prof->n_seqs; ++s) { ph_res[(size_t)prof->offsets[s]] = '^'; ph_res[(size_t)prof->offsets[s + 1] - 1] = '$'; }
    ph.n_seqs = prof->n_seqs; ph.offsets = prof->offsets; ph.residues = ph_res.data();
    queries = &ph;
  } else if (!sub->alphabet || !sub->table || sub->n < 1 || sub->n > 30) return ALN_E_ARG;
  ALN_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const float gi = qgaps ? 0.f : gap->gap_init, ge = qgaps ? 0.f : gap->gap_extn;
  rows = q_end - q_begin; n_t = templates->n_seqs;
  every_t.resize((size_t)n_t);
  for (int t = 0; t < n_t; ++t) every_t[t] = t;
  if (q_begin == q_end || n_t == 0) return ALN_OK;
  // fractional gaps or table values: full builds in the exact-order kernels (the reference's arithmetic), batch by batch
  // (a profile run first finishes its checks: no batch would look at the templates' letters for it)
  bool integral = (gi == (float)(int)gi) && (ge == (float)(int)ge) && gi >= 0 && ge >= 0;
  if (!integral && !prof) { route = kAllFull; return ALN_OK; }
  const int n_alpha = prof ? prof->n : sub->n;
  const char* alphabet = prof ? prof->alphabet : sub->alphabet;
  int idx[256];
  for (int i = 0; i < 256; ++i) idx[i] = -1;
  for (int i = 0; i < n_alpha; ++i) idx[(unsigned char)alphabet[i]] = i;
  maxs = 0;
  for (int i = 0; i < 32 * 32; ++i) ti[i] = 0;
  if (prof) {
    // maxs over the interior rows of the whole pool (a sentinel row's values are never read)
    for (int s = 0; s < prof->n_seqs && integral; ++s)
      for (int64_t k = (prof->offsets[s] + 1) * prof->n; k < (prof->offsets[s + 1] - 1) * prof->n; ++k) {
        const float v = prof->rows[k];
        if (!(v == (float)(int)v)) { integral = false; break; }
        maxs = std::max(maxs, fabs((double)v));
      }
  } else {
    for (int i = 0; i < sub->n; ++i)
      for (int j = 0; j < sub->n; ++j) {
        float v = sub->table[i * sub->n + j];
        if (!(v == (float)(int)v)) { route = kAllFull; return ALN_OK; }
        ti[i * 32 + j] = (int32_t)v;
        maxs = std::max(maxs, fabs((double)v));
      }
  }
  auto encode = [&](const aln_seqs* s, std::vector<uint8_t>& codes, int& maxlen) -> int {
    const int64_t total = s->offsets[s->n_seqs];
    codes.resize((size_t)total);
    for (int64_t k = 0; k < total; ++k) {
      unsigned char ch = (unsigned char)s->residues[k];
      int c = (ch == '^') ? kCodeHead : (ch == '$') ? kCodeTail : idx[ch];
      if (c < 0) return ALN_E_RESIDUE;
      codes[(size_t)k] = (uint8_t)c;
    }
    maxlen = 0;
    for (int i = 0; i < s->n_seqs; ++i) {
      int64_t len = s->offsets[i + 1] - s->offsets[i];
      if (len < 2) return ALN_E_ARG;
      maxlen = std::max<int>(maxlen, (int)len);
    }
    return ALN_OK;
  };
  int rc;
  if ((rc = encode(queries, qc, maxQ)) != ALN_OK) return rc;
  if ((rc = encode(templates, tc, maxT)) != ALN_OK) return rc;
  if (maxT > kMaxLen || maxQ > kMaxLen) return ALN_E_TOO_LONG;
  if (qgaps) {
    // Gap rows: no full-build route exists, so what the other entries send there is refused.  The entries READ of the whole
    // pool are checked — del_* at rows 0 .. Q-2 and ins_* at rows 1 .. Q-2 of every profile — and no other: a negative one
    // first (ALN_E_ARG), then a fractional row entry or gap value and the value bound with G, their maximum, in place of gi
    // and ge (ALN_E_NOT_INTEGRAL).
    if (maxT > 2048) return ALN_E_TOO_LONG;
    const float* const arr[4] = {qgaps->del_init, qgaps->del_extn, qgaps->ins_init, qgaps->ins_extn};
    double G = 0;
    bool gaps_integral = true;
    for (int s = 0; s < prof->n_seqs; ++s)
      for (int w = 0; w < 4; ++w)
        for (int64_t r = prof->offsets[s] + (w < 2 ? 0 : 1); r < prof->offsets[s + 1] - 1; ++r) {
          const float v = arr[w][r];
          if (v < 0) return ALN_E_ARG;
          if (!(std::floor(v) == v)) gaps_integral = false;       // (a NaN included)
          else G = std::max(G, (double)v);
        }
    if (!integral || !gaps_integral) return ALN_E_NOT_INTEGRAL;
    if (!((maxs + G) * ((double)maxQ + std::min(maxT, 2048)) + G + maxs < 8388608.0)) return ALN_E_NOT_INTEGRAL;
  }
  if (!integral) { route = kAllFull; return ALN_OK; }              // profiles: a fractional entry or gap
  if ((maxs + ge) * ((double)maxQ + std::min(maxT, 2048)) + gi + maxs >= 8388608.0) { route = kAllFull; return ALN_OK; }
  route = kFast;
  // Templates are launched by length class: a wave sweeps 256 R columns, so a template of T columns needs
  // R = ceil(T / 256) groups; one launch per class keeps short templates from paying for the longest one.
  cls_begin.assign(10, 0);
  {
    std::vector<std::vector<int32_t>> by(9);
    for (int t = 0; t < n_t; ++t) {
      const int T = (int)(templates->offsets[t + 1] - templates->offsets[t]);
      if (T > 2048) long_t.push_back(t);            // beyond the register-resident kernels: full builds
      else by[(T + 255) / 256].push_back(t);
    }
    for (int r = 1; r <= 8; ++r) { cls_begin[r] = (int)order.size(); order.insert(order.end(), by[r].begin(), by[r].end()); }
    cls_begin[9] = (int)order.size();
  }
  // packed 16-bit lanes (two queries per wave) when every intermediate provably fits: best local score <= maxs * min(Q,T),
  // A keys add ge * column, the "minus infinity" -12000 must stay below every real candidate and clear of wrap-around
  const int fastT = std::min(maxT, 2048);                // (longer templates do not run in these kernels)
  const double L = (double)std::max(maxQ, fastT), best = maxs * (double)std::min(maxQ, fastT);
  packed = !prof && local && best + ge * L + maxs < 30000.0 && ge * L + gi + maxs < 8000.0 && maxs < 2048.0 && ctx->hints.score_packed;
  return ALN_OK;
}

void ScoreRun::release() {
  hipFree(dq); hipFree(dt); hipFree(dqo); hipFree(dto); hipFree(dtab); hipFree(dsel); hipFree(dqsel); hipFree(dprows);
  dq = dt = nullptr; dqo = dto = nullptr; dtab = dsel = dqsel = nullptr; dprows = nullptr; dprows_bytes = 0;
}

// (The member functions below leave through score_common.h's STRY / RTRY over the member ctx; what they allocated is released
// by the caller's DeviceBufs or by the destructor.)
int ScoreRun::upload_offsets() {
  STRY(hipMalloc((void**)&dqo, (size_t)(queries->n_seqs + 1) * 8)); STRY(hipMalloc((void**)&dto, (size_t)(n_t + 1) * 8));
  STRY(hipMemcpyAsync(dqo, queries->offsets, (size_t)(queries->n_seqs + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  STRY(hipMemcpyAsync(dto, templates->offsets, (size_t)(n_t + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  return ALN_OK;
}

// Profiles: rows [offsets[qa], offsets[qb]) of the pool, widened to 32 int32 (letters n .. 31 and both sentinel rows 0), 128-byte
// aligned (hipMalloc's alignment, 128 bytes per row).  INVARIANT: the allocation ends kProfilePadRows rows (zeros) behind the last
// row — a sweep requests the 8-row chunks its rows 1 .. Q-2 lie in plus the one after (ProfileRows, score_sweep.h), i.e. at most
// rows .. Q + 13 of its profile, of which the last profile's reach past the pool's end.  A sweep that reads the rows through an
// order (PermutedProfileRows, search_zscore.hip) requests ENTRIES 0 .. Q + 13 of that order instead, every one of them a
// row index below Q: the order is padded (order_stride, same file), and no copy of such a sweep leaves its profile.
int ScoreRun::upload_profile_rows(int32_t qa, int32_t qb) {
  const int64_t r0 = prof->offsets[qa], r1 = prof->offsets[qb];
  const size_t n_rows = (size_t)(r1 - r0) + kProfilePadRows;
  if (n_rows * 128 > dprows_bytes) {
    hipFree(dprows); dprows = nullptr; dprows_bytes = 0;
    STRY(hipMalloc((void**)&dprows, n_rows * 128));
    dprows_bytes = n_rows * 128;
  }
  hrows.assign(n_rows * 32, 0);
  for (int32_t s = qa; s < qb; ++s)
    for (int64_t r = prof->offsets[s] + 1; r < prof->offsets[s + 1] - 1; ++r)
      for (int k = 0; k < prof->n; ++k) hrows[(size_t)(r - r0) * 32 + k] = (int32_t)prof->rows[(size_t)r * prof->n + k];
  if (qgaps)   // the rows' gap prices, words kQGapWord .. + 3: the entries read (prepare() checked them) and no other
    for (int32_t s = qa; s < qb; ++s)
      for (int64_t r = prof->offsets[s]; r < prof->offsets[s + 1] - 1; ++r) {
        int32_t* w = &hrows[(size_t)(r - r0) * 32 + kQGapWord];
        w[0] = (int32_t)qgaps->del_init[r]; w[1] = (int32_t)qgaps->del_extn[r];
        if (r > prof->offsets[s]) { w[2] = (int32_t)qgaps->ins_init[r]; w[3] = (int32_t)qgaps->ins_extn[r]; }
      }
  STRY(hipMemcpyAsync(dprows, hrows.data(), n_rows * 128, hipMemcpyHostToDevice, ctx->stream));
  a.qcodes = reinterpret_cast<const uint8_t*>(dprows) - r0 * 128;
  return ALN_OK;
}

int ScoreRun::upload() {
  STRY(hipMalloc((void**)&dt, tc.size()));
  if (!prof) {
    STRY(hipMalloc((void**)&dq, qc.size())); STRY(hipMalloc((void**)&dtab, sizeof ti));
    STRY(hipMemcpyAsync(dq, qc.data(), qc.size(), hipMemcpyHostToDevice, ctx->stream));
  }
  STRY(hipMemcpyAsync(dt, tc.data(), tc.size(), hipMemcpyHostToDevice, ctx->stream));
  RTRY(upload_offsets());
  if (!prof) STRY(hipMemcpyAsync(dtab, ti, sizeof ti, hipMemcpyHostToDevice, ctx->stream));
  a.qcodes = dq; a.qoff = dqo; a.tcodes = dt; a.toff = dto; a.table32 = dtab;
  if (prof && !rows_per_slab) RTRY(upload_profile_rows(q_begin, q_end));
  a.q_begin = q_begin; a.n_t = n_t; a.gi = qgaps ? 0 : (int)gap->gap_init; a.ge = qgaps ? 0 : (int)gap->gap_extn;
  STRY(hipMalloc((void**)&dsel, (size_t)n_t * 4));
  if (!order.empty()) STRY(hipMemcpyAsync(dsel, order.data(), order.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if (packed) STRY(hipMalloc((void**)&dqsel, (size_t)rows * 4));
  return ALN_OK;
}

int ScoreRun::launch(int row0, int nrows, float* dscores) {
  const dim3 block(64);
  // blockIdx.y is limited to 65535: walk the query rows in slabs.  The packed kernel pairs queries of similar length (a wave
  // runs to the longer one's last row): every slab's length order goes to the device before the slab's first launch, into its own
  // region of dqsel (slab starting at row r0 -> dqsel + r0), so no launch can see another slab's order (the kernels run
  // asynchronously on ctx->stream) and the host vector lives until the caller's synchronisation.
  if (packed) {
    qorders.emplace_back((size_t)nrows);
    std::vector<int32_t>& qo_all = qorders.back();
    for (int r0 = 0; r0 < nrows; r0 += 32768) {
      const int nr = std::min(32768, nrows - r0);
      int32_t* qo = qo_all.data() + r0;
      for (int k = 0; k < nr; ++k) qo[k] = k;
      std::stable_sort(qo, qo + nr, [&](int32_t x, int32_t y) {
        return queries->offsets[q_begin + row0 + r0 + x + 1] - queries->offsets[q_begin + row0 + r0 + x] <
               queries->offsets[q_begin + row0 + r0 + y + 1] - queries->offsets[q_begin + row0 + r0 + y];
      });
    }
    STRY(hipMemcpyAsync(dqsel + row0, qo_all.data(), (size_t)nrows * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  if (prof && rows_per_slab) RTRY(upload_profile_rows(q_begin + row0, q_begin + row0 + nrows));
  int cls_cnt[9] = {};                                    // `order` holds the templates class by class, from class 1 on
  for (int r = 1; r <= 8; ++r) cls_cnt[r] = cls_begin[r + 1] - cls_begin[r];
  for (int r0 = 0; r0 < nrows; r0 += 32768) {
    const int nr = std::min(32768, nrows - r0);
    STRY(launch_classes(prof != nullptr, cls_cnt, [&](auto side, auto rc, int nc, int off) {
      typedef decltype(side) Side;
      constexpr int R = decltype(rc)::value;
      ScoreArgs s = a;
      s.q_begin = q_begin + row0 + r0;
      s.scores = dscores + (size_t)r0 * n_t;
      s.tsel = dsel + off;
      s.qsel = dqsel ? dqsel + row0 + r0 : nullptr;
      const dim3 grid(nc, packed ? (nr + 1) / 2 : nr);   // packed: two query rows per wave
      if (qgaps) launch_qgaps_score(R, local, grid, ctx->stream, s, free_del, free_ins);               // (profiles only, never packed)
      else if (packed) hipLaunchKernelGGL(score_local_pk_kernel<R>, grid, block, 0, ctx->stream, s, nr);   // (residues only: no side)
      else if (local) hipLaunchKernelGGL((score_local_kernel<R, Side>), grid, block, 0, ctx->stream, s);
      else hipLaunchKernelGGL((score_global_kernel<R, Side>), grid, block, 0, ctx->stream, s, free_del, free_ins);
    }));
  }
  return ALN_OK;
}

}  // namespace aln

using namespace aln;

// The shared body of aln_score_all_vs_all and aln_score_profiles_vs_all (run: prepared)
static int score_block(ScoreRun& run, float* scores) {
  aln_ctx* ctx = run.ctx;
  const std::vector<int32_t>* full_t = &run.every_t;     // the templates that go through full builds
  if (run.route != ScoreRun::kAllFull) {
    const size_t n = (size_t)run.rows * run.n_t;
    DeviceBufs bufs(run);                                  // this scope: the score buffer is freed and the run released BEFORE
    float* dsc = nullptr;                                  // the full builds below, which want the memory
    STRY(bufs.get(dsc, n));
    RTRY(run.upload());
    RTRY(run.launch(0, run.rows, dsc));
    STRY(hipMemcpyAsync(scores, dsc, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    STRY(hipStreamSynchronize(ctx->stream));
    full_t = &run.long_t;
  }
  if (full_t->empty()) return ALN_OK;
  return score_through_batches(ctx, run.queries, run.templates, run.sub, run.gap, run.q_begin, run.q_end, *full_t, scores, nullptr, 0, run.prof);
}

// The score Optimal reports for queries[q_begin .. q_end) against every template: scores[(q - q_begin) * n_t + t].
// Replaces (q_end - q_begin) x n_t constructions of DPMatrix(q, t, AASubstitutionEval, fwd, align_type) + Optimal(align_type):
// find_max for local alignments, the final cell's score for the four other align types.
extern "C" int aln_score_all_vs_all(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                                    const aln_gap* gap, int32_t q_begin, int32_t q_end, float* scores) {
  if (!scores) return ALN_E_ARG;
  ScoreRun run;
  int rc = run.prepare(ctx, queries, templates, sub, gap, q_begin, q_end);
  if (rc != ALN_OK || run.route == ScoreRun::kNothing) return rc;
  return score_block(run, scores);
}

// The same for position-specific queries: replaces as many fills of a Q x T SimilarityMatrix from a position-dependent
// Evaluator::similarity + DPMatrix + Optimal constructions.
extern "C" int aln_score_profiles_vs_all(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* templates, const aln_gap* gap,
                                         int32_t q_begin, int32_t q_end, float* scores) {
  if (!scores || !profiles) return ALN_E_ARG;
  ScoreRun run;
  int rc = run.prepare(ctx, nullptr, templates, nullptr, gap, q_begin, q_end, profiles);
  if (rc != ALN_OK || run.route == ScoreRun::kNothing) return rc;
  return score_block(run, scores);
}

// The same for profiles whose rows carry their own gap penalties (include/aln_hip.h): the kernels of search_qgaps.hip
extern "C" int aln_score_profiles_gaps_vs_all(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_qgaps* gaps, const aln_seqs* templates,
                                              int32_t align_type, int32_t q_begin, int32_t q_end, float* scores) {
  if (!scores || !profiles || !gaps) return ALN_E_ARG;
  ScoreRun run;
  run.qgaps = gaps; run.qgaps_align_type = align_type;
  int rc = run.prepare(ctx, nullptr, templates, nullptr, nullptr, q_begin, q_end, profiles);
  if (rc != ALN_OK || run.route == ScoreRun::kNothing) return rc;
  return score_block(run, scores);
}

#undef STRY
#undef RTRY
