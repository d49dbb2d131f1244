// score_sweep_qgaps.h — score_sweep.h's row sweeps for profiles whose ROWS carry their own gap penalties (aln_qgaps), device only.
//
// Siblings of sweep_local / sweep_global, not policies of them: every existing user of score_sweep.h compiles from unchanged
// text (DESIGN 4.8t has the code-object comparison).  The recurrence is the collapsed one with every gap cost replaced
// (include/aln_hip.h, aln_score_profiles_gaps_vs_all, has the definition):
//   deletion   from (i-1, k) into (i, j) skips L = j-1-k template residues and is priced by the row it LEAVES:
//              gi' + ge' (L-1), gi' = del_init[i-1], ge' = del_extn[i-1].  Both are wave-uniform, so the keys keep their shape,
//                A(k) = D[i-1][k] + ge' k,   E(c+1) = prefix max of A - (ge' c + gi' - ge'),
//              and what LocalCols holds as gec / ekc becomes one multiply-add per cell over the lane's column index (cix).
//              finish_row of row i-1 runs while that row's prices are at hand; the loop of row i keeps them in two scalars.
//   insertion  from (k, c) into (i, c+1) skips the profile positions k+1 .. i-1, each at its own price:
//              ins_init[k+1] + sum_{p=k+2..i-1} ins_extn[p].  With X[p] = sum_{u=2..p} ins_extn[u] (X[1] = 0) that is
//              ins_init[k+1] - X[k+1] + X[i-1], so the per-column running maximum holds D[k][c] - ins_init[k+1] + X[k+1] and is
//              read as f = gmx - X[i-1]; X is one scalar accumulated as the rows go by, and the update for k = i-1 in the loop
//              of row i needs row i's own prices, which that loop has just read.
// With all four arrays constant (gi, ge) every D equals sweep_local's / sweep_global's: A, E and f are the same numbers, the
// running maximum is theirs minus gi.
// Where a row's prices live: words 26 .. 29 of its 128-byte device image (del_init, del_extn, ins_init, ins_extn; hence an
// alphabet of at most 26 letters — words 30 and 31 stay 0, the template sentinels' codes index them).  They ride ProfileRows'
// global -> LDS copies; a wave reads them with one wave-uniform LDS read per row, directly after ProfileRows::row(i) has made
// row i readable, and moves them to SGPRs.  ProfileRows::landed()'s reasoning is untouched: no new global load.
// Value range (ScoreRun::prepare): with G the largest price read, (maxs + G) (maxQ + maxT) + G + maxs < 2^23.  Every key is a
// cell value plus or minus at most one gap cost or one of ge' k <= G T, X <= G Q, so it stays below 2^23 in magnitude, far
// inside int32 and clear of the "minus infinity" -2^28; the multiply-adds take G < 2^21 and a column index clamped to T - 1 <
// 2^11 (cix), both inside v_mad_i32_i24's signed 24-bit operands.  Columns beyond T - 1 are never a source of an interior one.
#pragma once
#include "score_sweep.h"

namespace aln {

constexpr int kQGapWord = 26;                // the first of a device row's four gap words

struct RowGaps { int dgi, dge, igi, ige; };  // del_init, del_extn, ins_init, ins_extn of one profile row, in SGPRs
__device__ __forceinline__ RowGaps sweep_row_gaps(const int* ring, int qrow) {
  const int* w = reinterpret_cast<const int*>(reinterpret_cast<const char*>(ring) + qrow) + kQGapWord;
  RowGaps g;
  g.dgi = __builtin_amdgcn_readfirstlane(w[0]);
  g.dge = __builtin_amdgcn_readfirstlane(w[1]);
  g.igi = __builtin_amdgcn_readfirstlane(w[2]);
  g.ige = __builtin_amdgcn_readfirstlane(w[3]);
  return g;
}

// ---- local -------------------------------------------------------------------------------------------------------------------
template <int R>
struct QGapLocalCols {
  int code4[R][4], cix[R][4], inm[R][4];
  int T;
  __device__ __forceinline__ void load(const uint8_t* tc, int T_) {
    T = T_;
    const int cb = 4 * (int)threadIdx.x;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int c = cb + 256 * r + x;
        int code = kCodeTail;
        if (c < T) code = tc[c];
        code4[r][x] = code * 4;
        cix[r][x] = min(c, T - 1);                                      // the column index of the keys, clamped (see above)
        inm[r][x] = ((unsigned)(c - 1) < (unsigned)(T - 2)) ? -1 : 0;
      }
  }
};

// sweep_local for gap rows: rows 1 .. last of the profile at qc (ProfileRows' source), row `last` left in d[], the lane's
// maximum returned.  End gaps are free, so row 0's prices and the head and tail costs play no part.
template <int R, class Obs>
__device__ __forceinline__ int sweep_local_qgaps(const int* ring, const QGapLocalCols<R>& k, const int4* qc, int last,
                                                 int (&d)[R][4], Obs&& obs) {
  const int lane = threadIdx.x;
  const int cb = 4 * lane;
  const int T = k.T;
  int gmx[R][4], cv[R], ak[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    cv[r] = kNegS;
#pragma unroll
    for (int x = 0; x < 4; ++x) { d[r][x] = 0; gmx[r][x] = kNegS; }
  }
  int lmax = 0;
  int pge = 0, pgime = 0;                                      // del_extn and del_init - del_extn of the row held in d[]
  auto finish_row = [&]() {
    int sk = kNegS;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int tk = kNegS;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        int A = __mul24(pge, k.cix[r][x]) + d[r][x];
        if (r == 0 && x == 0) A = (lane == 0) ? kNegS : A;   // column 0 is never a source
        ak[r][x] = A;
        tk = max(tk, A);
      }
      lmax = max(max(lmax, d[r][0]), d[r][1]);
      lmax = max(max(lmax, d[r][2]), d[r][3]);
      const int ik = wave_incl_max_s(tk);
      const int ek = sdpp<0x138>(kNegS, ik);
      cv[r] = max(sk, ek);
      sk = max(sk, __builtin_amdgcn_readlane(ik, 63));
    }
  };
  if (last >= 1) {
    const int qrow = ProfileRows::first(ring, qc);
    const RowGaps g = sweep_row_gaps(ring, qrow);
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int h = max(sweep_tab_at(ring, qrow, k.code4[r][x]), 0);
        d[r][x] = h & k.inm[r][x];
      }
    pge = g.dge; pgime = g.dgi - g.dge;
    finish_row();
    obs.row(1, d, lmax);
  }
  int xsum = 0;                                                // X[i-1]
  for (int i = 2; i <= last; ++i) {
    const int qrow = ProfileRows::row(ring, qc, i);
    const RowGaps g = sweep_row_gaps(ring, qrow);
    const int roff = xsum;
    xsum += g.ige;                                             // X[i]
    const int rowB = xsum - g.igi;
    int bk[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int pv = cv[r];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int m = d[r][x];
        const int A = ak[r][x];
        const int e = pv - (__mul24(pge, k.cix[r][x]) + pgime);
        const int f = gmx[r][x] - roff;
        bk[r][x] = max(max(m, e), f);
        obs.cell(r, x, m, e, f, pv, A, gmx[r][x], m + rowB);
        pv = max(pv, A);
        gmx[r][x] = max(gmx[r][x], m + rowB);
      }
      obs.group(i, r);
    }
    int prev_k = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int uk = sdpp<0x138>(0, bk[r][3]);
      if (r > 0) uk = (lane == 0) ? prev_k : uk;
      prev_k = __builtin_amdgcn_readlane(bk[r][3], 63);
      const bool masked = (r == 0) || (256 * (r + 1) > T - 1);
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int c = cb + 256 * r + x;
        const int s = sweep_tab_at(ring, qrow, k.code4[r][x]);
        int h = max(((x == 0) ? uk : bk[r][x - 1]) + s, 0);
        if (r == 0 && x == 1) h = (c == 1) ? max(s, 0) : h;  // column 1 (lane 0 only): free insertion from the origin
        if (masked) h &= k.inm[r][x];                        // columns 0 and >= T-1 stay 0
        d[r][x] = h;
      }
    }
    pge = g.dge; pgime = g.dgi - g.dge;
    finish_row();
    obs.row(i, d, lmax);
  }
  return lmax;
}

// ---- non-local -----------------------------------------------------------------------------------------------------------------
template <int R>
struct QGapGlobalCols {
  int code4[R][4], cix[R][4]; bool in[R][4];
  int T;
  int rs, xs, ls;                                                  // column T-2: its (wave-uniform) slot and lane
  __device__ __forceinline__ void load(const uint8_t* tc, int T_) {
    T = T_;
    const int cb = 4 * (int)threadIdx.x;
    const int cl = T - 2;
    rs = cl / 256; xs = cl & 3; ls = (cl & 255) >> 2;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int c = cb + 256 * r + x;
        int code = kCodeTail;
        if (c < T) code = tc[c];
        code4[r][x] = code * 4;
        cix[r][x] = min(c, T - 1);
        in[r][x] = (unsigned)(c - 1) < (unsigned)(T - 2);
      }
  }
};

// sweep_global for gap rows (Q >= 3 and T >= 3): rows 1 .. Q-2 and the final cell; the lane's candidate for its score.
//   head deletion into (1, j)        del(0, j-1): row 0's prices, read from the ring's slot 0
//   head insertion into (i, 1)       ins(1, i-1) = ins_init[1] + X[i-1]
//   final cell from (Q-2, k)         del(Q-2, T-2-k): the prices of the last row finished
//   final cell from (k, T-2)         ins(k+1, Q-2): the running maximum of column T-2 minus X[Q-2]
// each 0 where the align type makes that end gap free.
template <int R, class Obs>
__device__ __forceinline__ int sweep_global_qgaps(const int* ring, const QGapGlobalCols<R>& k, const int4* qc, int Q,
                                                  int free_del, int free_ins, Obs&& obs) {
  const int lane = threadIdx.x;
  const int cb = 4 * lane;
  const int T = k.T, ls = k.ls;
  int d[R][4], gmx[R][4], cv[R], ak[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    cv[r] = kNegS;
#pragma unroll
    for (int x = 0; x < 4; ++x) { d[r][x] = kNegS; gmx[r][x] = kNegS; }
  }
  int clast = kNegS;
  int pgi = 0, pge = 0;                                            // del_init and del_extn of the row held in d[]
  auto finish_row = [&]() {
    int sk = kNegS;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int tk = kNegS;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int A = __mul24(pge, k.cix[r][x]) + d[r][x];       // non-interior cells hold "minus infinity": never a source
        ak[r][x] = A;
        tk = max(tk, A);
      }
      const int ik = wave_incl_max_s(tk);
      const int ek = sdpp<0x138>(kNegS, ik);
      cv[r] = max(sk, ek);
      sk = max(sk, __builtin_amdgcn_readlane(ik, 63));
    }
    const int v = sweep_pick<R>(d, k.rs, k.xs, kNegS);
    clast = max(clast, lane == ls ? v : kNegS);
  };
  int igi1;                                                        // ins_init[1]: the head insertion's
  {
    const int qrow = ProfileRows::first(ring, qc);
    const RowGaps g0 = sweep_row_gaps(ring, 0);                    // row 0, the '^' row, prices the head deletion
    const RowGaps g = sweep_row_gaps(ring, qrow);
    igi1 = g.igi;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int c = cb + 256 * r + x;
        const int cost = (c >= 2 && !free_del) ? g0.dgi + __mul24(g0.dge, k.cix[r][x] - 2) : 0;
        d[r][x] = k.in[r][x] ? sweep_tab_at(ring, qrow, k.code4[r][x]) - cost : kNegS;
      }
    pgi = g.dgi; pge = g.dge;
    finish_row();
    obs.row(1, d, clast);
  }
  int xsum = 0;                                                    // X[i-1]
  for (int i = 2; i <= Q - 2; ++i) {
    const int qrow = ProfileRows::row(ring, qc, i);
    const RowGaps g = sweep_row_gaps(ring, qrow);
    const int roff = xsum;
    xsum += g.ige;                                                 // X[i]
    const int rowB = xsum - g.igi;
    const int col1 = free_ins ? 0 : igi1 + roff;                   // column 1: one insertion from the origin, ins(1, i-1)
    const int pgime = pgi - pge;
    int bk[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int pv = cv[r];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int m = d[r][x];
        const int A = ak[r][x];
        const int e = pv - (__mul24(pge, k.cix[r][x]) + pgime);
        const int f = gmx[r][x] - roff;
        bk[r][x] = max(max(m, e), f);
        obs.cell(r, x, m, e, f, pv, A, gmx[r][x], m + rowB);
        pv = max(pv, A);
        gmx[r][x] = max(gmx[r][x], m + rowB);
      }
      obs.group(i, r);
    }
    int prev_k = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int uk = sdpp<0x138>(0, bk[r][3]);
      if (r > 0) uk = (lane == 0) ? prev_k : uk;
      prev_k = __builtin_amdgcn_readlane(bk[r][3], 63);
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int c = cb + 256 * r + x;
        const int s = sweep_tab_at(ring, qrow, k.code4[r][x]);
        int h = ((x == 0) ? uk : bk[r][x - 1]) + s;
        if (r == 0 && x == 1) h = (c == 1) ? s - col1 : h;
        d[r][x] = k.in[r][x] ? h : kNegS;
      }
    }
    pgi = g.dgi; pge = g.dge;
    finish_row();
    obs.row(i, d, clast);
  }
  // ---- the final cell: row Q-2 is in d[] with its prices in pgi / pge, gmx holds rows <= Q-3, xsum is X[Q-2] -------------
  obs.last(d);
  int best = (lane == ls) ? sweep_pick<R>(d, k.rs, k.xs, kNegS) : kNegS;
  int dl = kNegS;                                                  // deletion from (Q-2, k): del(Q-2, T-2-k)
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int len = T - 2 - k.cix[r][x];
      const int cost = (len < 1 || free_del) ? 0 : pgi + __mul24(pge, len - 1);
      dl = max(dl, k.in[r][x] ? d[r][x] - cost : kNegS);
    }
  best = max(best, dl);
  int il;                                                          // insertion from (k, T-2): ins(k+1, Q-2)
  if (free_ins) il = clast;
  else {
    const int g = sweep_pick<R>(gmx, k.rs, k.xs, kNegS);           // max over k <= Q-3 of D[k][T-2] - ins_init[k+1] + X[k+1]
    il = (lane == ls && Q >= 4) ? g - xsum : kNegS;
  }
  return max(best, il);
}

}  // namespace aln
