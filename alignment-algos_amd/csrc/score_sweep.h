// score_sweep.h — the register-resident row sweep of the collapsed recurrence, 32-bit, device only.
//
// One wave holds a whole DP row in VGPRs: lane l owns columns 256 r + 4 l + x (r < R groups, x < 4).  Per row
//   E(j) comes from a DPP max-plus prefix scan of A(k) = D[i-1][k] + ge k, F from a per-column running max of D[k][c] + ge k,
//   best = max3(match, E, F) + S.
// Two recurrences live here, each as a pair "column state" (built once per template) + "sweep" (run once per query string):
//   LocalCols<R>  + sweep_local   clipped at 0, end gaps free, columns outside the interior masked to 0        (dpmatrix.h:538-689)
//   GlobalCols<R> + sweep_global  the four non-local align types: no clip, "minus infinity" outside the interior,
//                                 end gaps priced per align type, the final cell included                      (dpmatrix.h:375-534)
// Users: score_only.hip (scores), search_topk.hip (end cells), search_zscore.hip (one sweep per shuffle; a profile's rows in a
// permuted order, through a source of its own), search_align.hip (four or five bits per cell into a strip) — each kernel of
// these once, instantiated for residue queries and for queries given as position-specific rows (the query side,
// score_common.h) — and search_align_multi.hip (sweep_local_masked: the local sweep over a plane of forbidden cells).  What a user sees of
// a sweep beyond its result goes through an observer, where a row's similarities come from through a row source; the packed
// 16-bit kernel of score_only.hip has its own types and its own sweep.
#pragma once
#include "aln_internal.h"

namespace aln {

constexpr int kNegS = -(1 << 28);

template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF>
__device__ __forceinline__ int sdpp(int old, int src) {
  return __builtin_amdgcn_update_dpp(old, src, CTRL, ROW_MASK, BANK_MASK, false);
}
__device__ __forceinline__ int wave_incl_max_s(int v) {
  const int ident = (int)0x80000000;
  v = max(v, sdpp<0x111>(ident, v));
  v = max(v, sdpp<0x112>(ident, v));
  v = max(v, sdpp<0x114>(ident, v));
  v = max(v, sdpp<0x118>(ident, v));
  v = max(v, sdpp<0x142, 0xA>(ident, v));
  v = max(v, sdpp<0x143, 0xC>(ident, v));
  return v;
}

// ---- row sources ---------------------------------------------------------------------------------------------------------------
// A sweep reads S[i][c] as one LDS word at base + (byte offset of row i's 32 ints, wave-uniform) + 4 * (template code of column
// c).  Where the offset comes from is the row source, a policy of sweep_local / sweep_global (template parameter Rows; Src is
// what the global pointer handed to the sweep points to):
//   first(lds, src)     the offset of row 1; called once, before anything else
//   row(lds, src, i)    the offset of row i >= 2, called once per row in ascending order: the hook in which a source stages
//                       what later rows need
__device__ __forceinline__ int sweep_tab_at(const int* tab, int qrow, int c4) {
  return *reinterpret_cast<const int*>(reinterpret_cast<const char*>(tab) + qrow + c4);
}

// The default: a 32 x 32 substitution table in LDS, row i is the table row of query code qc[i] (128 bytes per code), and the
// code of row i + 1 is fetched while row i is computed.  kInSweep: its three lines stay spelled out in the sweeps, under
// `if constexpr`, and this struct only names them.  Routed through first() / row() like any other source the same loads reach
// the optimiser in another shape (the address of qc[i + 1] is formed differently) and nine instantiations of
// score_global_kernel, score_shuffled_kernel and hit_global_kernel change their SGPR spills.
struct TableRows {
  typedef uint8_t Src;
  static constexpr bool kInSweep = true;
};

// A position-specific query (ProfileQuery, score_common.h): the device holds row i of the profile as 32 int32 (128 bytes; letters n .. 31
// and the two sentinel rows are 0), rows contiguous, so 8 rows are the 1 KiB that ONE 16-byte-per-lane global -> LDS copy writes
// lane-linearly.  LDS holds a ring of 32 rows (4 chunks of 8, the 4 KiB of the table it replaces): row i sits in slot i & 31.
// Chunk c + 1 is requested when the sweep enters chunk c, then the source waits until at most that one copy is outstanding, i.e.
// until chunk c has landed (copies complete in order; the loop holds no other global load that would make the compiler drain
// them early).  The slot chunk c + 1 overwrites was last read three chunks ago.  The copy of the chunk after the last row's is
// requested as well and never read: the buffer is padded by kProfilePadRows rows for it (ScoreRun::upload_profile_rows).
constexpr int kProfilePadRows = 16;
struct ProfileRows {
  typedef int4 Src;
  static constexpr bool kInSweep = false;
  static __device__ __forceinline__ void fill(const int* ring, const int4* src, int c) {
    typedef __attribute__((address_space(3))) void* lds_t;
    typedef __attribute__((address_space(1))) void* glb_t;
    __builtin_amdgcn_global_load_lds((glb_t)(src + c * 64 + (int)threadIdx.x), (lds_t)(ring + (c & 3) * 256), 16, 0, 0);
  }
  static __device__ __forceinline__ void landed() { asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); }
  static __device__ __forceinline__ int first(const int* ring, const int4* src) {
    fill(ring, src, 0); fill(ring, src, 1); landed();
    return 128;
  }
  static __device__ __forceinline__ int row(const int* ring, const int4* src, int i) {
    if ((i & 7) == 0) { fill(ring, src, (i >> 3) + 1); landed(); }
    return (i & 31) * 128;
  }
};

// What a user of sweep_local or sweep_global may watch.  The default watches nothing and compiles to nothing.
struct NoObserver {
  // cell(r, x, m, e, f, pv, A, gmx, key): a cell (group r, slot x) of row i-1 while row i is computed.  m, e, f are the three
  // maxima row i's cell to its right chooses from; pv >= A says an earlier column of row i-1 holds at least this cell's deletion
  // key, gmx >= key that an earlier row of the column holds at least its insertion key.  Then group(i, r): the lane's four cells
  // of the group are through.
  __device__ __forceinline__ void cell(int, int, int, int, int, int, int, int, int) {}
  __device__ __forceinline__ void group(int, int) {}
  // row(i, d, lane_max): row i is in d[]; lane_max is the lane's maximum over rows 1 .. i (sweep_global: over rows 1 .. i of
  // column T-2, in the lane that owns it)
  template <int R>
  __device__ __forceinline__ void row(int, const int (&)[R][4], int) {}
  // last(d), sweep_global only: the last row, Q-2, is in d[] and the final cell is next
  template <int R>
  __device__ __forceinline__ void last(const int (&)[R][4]) {}
};

// ---- local -------------------------------------------------------------------------------------------------------------------
template <int R>
struct LocalCols {
  int code4[R][4], gec[R][4], ekc[R][4], inm[R][4];
  int T, gi, ge;
  __device__ __forceinline__ void load(const uint8_t* tc, int T_, int gi_, int ge_) {
    T = T_; gi = gi_; ge = ge_;
    const int cb = 4 * (int)threadIdx.x;
    const int gime = gi - ge;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int c = cb + 256 * r + x;
        int code = kCodeTail;
        if (c < T) code = tc[c];
        code4[r][x] = code * 4;
        gec[r][x] = ge * c;
        ekc[r][x] = ge * c + gime;                                      // E(c+1) = prefix max - ekc
        inm[r][x] = ((unsigned)(c - 1) < (unsigned)(T - 2)) ? -1 : 0;   // interior column: scores are >= 0, so "& mask" zeroes the rest
      }
  }
};

// Rows 1 .. last of the query codes qc (last <= Q - 2; last < 1: no row).  Leaves row `last` in d[] (all 0 without a row) and
// returns the lane's maximum over every cell it computed.  The sweep owns that maximum and both inner loops stay in this
// function: an observer that keeps the maximum by reference, or a helper that takes the row arrays by reference, costs
// registers and with them waves per SIMD.
template <int R, class Rows = TableRows, class Obs>
__device__ __forceinline__ int sweep_local(const int* tab, const LocalCols<R>& k, const typename Rows::Src* qc, int last,
                                           int (&d)[R][4], Obs&& obs) {
  const int lane = threadIdx.x;
  const int cb = 4 * lane;
  const int gi = k.gi, ge = k.ge, T = k.T;
  int gmx[R][4], cv[R], ak[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    cv[r] = kNegS;
#pragma unroll
    for (int x = 0; x < 4; ++x) { d[r][x] = 0; gmx[r][x] = kNegS; }
  }
  int lmax = 0;
  // prefix-scan preparation on the row held in d[] (ak = D + ge c, cv[r] = the maximum of the keys left of the lane's group r)
  // + running maximum
  auto finish_row = [&]() {
    int sk = kNegS;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int tk = kNegS;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        int A = d[r][x] + k.gec[r][x];
        if (r == 0 && x == 0) A = (lane == 0) ? kNegS : A;   // column 0 is never a source
        ak[r][x] = A;
        tk = max(tk, A);
      }
      lmax = max(max(lmax, d[r][0]), d[r][1]);               // two v_max3 per group
      lmax = max(max(lmax, d[r][2]), d[r][3]);
      const int ik = wave_incl_max_s(tk);
      const int ek = sdpp<0x138>(kNegS, ik);
      cv[r] = max(sk, ek);
      sk = max(sk, __builtin_amdgcn_readlane(ik, 63));
    }
  };
  if (last >= 1) {
    // row 1 (dpmatrix.h:579-590): local mode -> end gaps are free: clip(S[1][c])
    int qrow;
    if constexpr (Rows::kInSweep) qrow = (int)qc[1] * 128;
    else qrow = Rows::first(tab, qc);
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int h = max(sweep_tab_at(tab, qrow, k.code4[r][x]), 0);
        d[r][x] = h & k.inm[r][x];
      }
    finish_row();
    obs.row(1, d, lmax);
  }
  int qcode_next = 0;
  if constexpr (Rows::kInSweep) qcode_next = (last >= 2) ? (int)qc[2] : 0;
  for (int i = 2; i <= last; ++i) {                         // dpmatrix.h:607-649
    int qrow;
    if constexpr (Rows::kInSweep) {
      qrow = qcode_next * 128;
      if (i + 1 <= last) qcode_next = (int)qc[i + 1];
    } else qrow = Rows::row(tab, qc, i);
    const int roff = gi + ge * (i - 2);
    const int rowB = ge * (i - 1);
    int bk[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int pv = cv[r];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int m = d[r][x];
        const int A = ak[r][x];
        const int e = pv - k.ekc[r][x];
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
        const int s = sweep_tab_at(tab, qrow, k.code4[r][x]);
        int h = max(((x == 0) ? uk : bk[r][x - 1]) + s, 0);
        if (r == 0 && x == 1) h = (c == 1) ? max(s, 0) : h;  // column 1 (lane 0 only): free insertion from the origin (:593-599)
        if (masked) h &= k.inm[r][x];                        // columns 0 and >= T-1 stay 0
        d[r][x] = h;
      }
    }
    finish_row();
    obs.row(i, d, lmax);
  }
  return lmax;
}

// sweep_local with a set of FORBIDDEN cells (search_align_multi.hip): one bit per cell, row i of the pair at
// mask + i * 8 R words, column c in bit c & 31 of word c / 32 — a lane's four columns of group r are nibble (lane & 7) of word
// 8 r + lane / 8, one 32-byte-per-8-lanes load per group and row.  D is forced to 0 where the bit is set, directly after the
// cell is formed and before anything reads it: row 1, column 1 with its free insertion from the origin and the edge groups
// included; as a gap source or a diagonal predecessor such a cell is then an ordinary zero cell.  MASKED == false reads no
// mask and is sweep_local's recurrence.  A sibling, not a policy of sweep_local: every existing user of that function compiles
// from unchanged text (DESIGN 4.8h has the metadata comparison).  The mask is written by earlier rounds of the same wave, so it
// is read through plain loads, never as __restrict__ / invariant data.
// Rows: the row source, as in sweep_local — the table's three lines spelled out under `if constexpr`, every other source
// through first() / row().  A STAGED source (ProfileRows) shares the wave's one VM counter with the mask loads (R per row) and
// with the observer's strip stores (R per row); gfx950 retires all of them in issue order.  Two things follow (DESIGN 4.8k
// quotes the waits of the compiled loop):
//   landed()   waits until at most ONE operation is outstanding, directly after chunk c + 1 is requested.  Whatever else is in
//              flight, chunk c was requested eight rows (or, in first(), one instruction) before chunk c + 1, so it is never the
//              newest outstanding operation and has landed when the wait returns.  More traffic only makes the wait stronger.
//   order      the mask words of row i are requested BEFORE Rows::row(i): on a fill row landed() then covers them too (they are
//              older than the copy), so the wait the compiler adds for them finds them there.  That wait is NOT counted: with
//              copies into LDS among the outstanding operations the compiler waits for a plain load with s_waitcnt vmcnt(0) —
//              once per masked row, before the second inner loop's first cell, behind the row's strip stores (on the table
//              side the same place reads vmcnt(3), vmcnt(2) for R = 2).  So in the MASKED rounds every row drains its stores,
//              and a fill row drains the copy it has just requested: chunk c + 1 lands in the row that asks for it, seven rows
//              before its first use, hidden by the first inner loop only.  Round 0 (MASKED == false) has no such wait and
//              keeps the copy one chunk ahead.  Requested after the copy, the mask words would change nothing about the
//              drain and lose landed()'s cover; counting that wait by hand is the follow-up DESIGN 4.8k names.
template <int R, bool MASKED, class Rows = TableRows, class Obs>
__device__ __forceinline__ int sweep_local_masked(const int* tab, const LocalCols<R>& k, const typename Rows::Src* qc, int last,
                                                  const uint32_t* mask, int (&d)[R][4], Obs&& obs) {
  const int lane = threadIdx.x;
  const int cb = 4 * lane;
  const int gi = k.gi, ge = k.ge, T = k.T;
  const uint32_t* mlane = mask + (lane >> 3);
  const int msh = 4 * (lane & 7);
  int gmx[R][4], cv[R], ak[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    cv[r] = kNegS;
#pragma unroll
    for (int x = 0; x < 4; ++x) { d[r][x] = 0; gmx[r][x] = kNegS; }
  }
  int lmax = 0;
  auto finish_row = [&]() {
    int sk = kNegS;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int tk = kNegS;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        int A = d[r][x] + k.gec[r][x];
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
    uint32_t mw1[R];                                         // row 1's mask words: requested before the first copies
#pragma unroll
    for (int r = 0; r < R; ++r) mw1[r] = MASKED ? mlane[8 * R + 8 * r] : 0u;
    int qrow;
    if constexpr (Rows::kInSweep) qrow = (int)qc[1] * 128;
    else qrow = Rows::first(tab, qc);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint32_t nib = mw1[r] >> msh;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int h = max(sweep_tab_at(tab, qrow, k.code4[r][x]), 0);
        d[r][x] = ((nib >> x) & 1u) ? 0 : (h & k.inm[r][x]);
      }
    }
    finish_row();
    obs.row(1, d, lmax);
  }
  int qcode_next = 0;
  if constexpr (Rows::kInSweep) qcode_next = (last >= 2) ? (int)qc[2] : 0;
  for (int i = 2; i <= last; ++i) {
    int qrow;
    if constexpr (Rows::kInSweep) {
      qrow = qcode_next * 128;
      if (i + 1 <= last) qcode_next = (int)qc[i + 1];
    }
    uint32_t mw[R];
#pragma unroll
    for (int r = 0; r < R; ++r) mw[r] = MASKED ? mlane[(size_t)i * (8 * R) + 8 * r] : 0u;
    if constexpr (!Rows::kInSweep) qrow = Rows::row(tab, qc, i);   // after the mask words are requested (see above)
    const int roff = gi + ge * (i - 2);
    const int rowB = ge * (i - 1);
    int bk[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int pv = cv[r];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int m = d[r][x];
        const int A = ak[r][x];
        const int e = pv - k.ekc[r][x];
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
      const uint32_t nib = mw[r] >> msh;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int c = cb + 256 * r + x;
        const int s = sweep_tab_at(tab, qrow, k.code4[r][x]);
        int h = max(((x == 0) ? uk : bk[r][x - 1]) + s, 0);
        if (r == 0 && x == 1) h = (c == 1) ? max(s, 0) : h;  // column 1 (lane 0 only): free insertion from the origin
        if (masked) h &= k.inm[r][x];                        // columns 0 and >= T-1 stay 0
        if (MASKED) h = ((nib >> x) & 1u) ? 0 : h;           // a forbidden cell
        d[r][x] = h;
      }
    }
    finish_row();
    obs.row(i, d, lmax);
  }
  return lmax;
}

// this lane's value in slot (rs, xs) of a row (rs, xs wave-uniform); `none` where the slot does not exist
template <int R>
__device__ __forceinline__ int sweep_pick(const int (&v)[R][4], int rs, int xs, int none) {
  int o = none;
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int x = 0; x < 4; ++x) o = (r == rs && x == xs) ? v[r][x] : o;
  return o;
}

// ---- non-local -----------------------------------------------------------------------------------------------------------------
// Values may be negative, so columns outside the interior are kept at "minus infinity" instead of being masked to 0; row 1 and
// column 1 pay (or not: free end gaps, aasubalib.h:34-49,60-75) the gap from the origin (dpmatrix.h:409-426); the final cell
// (dpmatrix.h:505-534) is the best of the last interior cell, a deletion from the last interior row and an insertion from the
// last interior column, each free or priced by the align type.
template <int R>
struct GlobalCols {
  int code4[R][4], gec[R][4], ekc[R][4]; bool in[R][4];
  int T, gi, ge;
  int rs, xs, ls;                                                  // column T-2, the last interior one: its (wave-uniform) slot and lane
  __device__ __forceinline__ void load(const uint8_t* tc, int T_, int gi_, int ge_) {
    T = T_; gi = gi_; ge = ge_;
    const int cb = 4 * (int)threadIdx.x;
    const int gime = gi - ge;
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
        gec[r][x] = ge * c;
        ekc[r][x] = ge * c + gime;
        in[r][x] = (unsigned)(c - 1) < (unsigned)(T - 2);
      }
  }
};

// Rows 1 .. Q-2 and the final cell (Q >= 3 and T >= 3: the callers deal with the degenerate shapes).  Returns the lane's
// candidate for the final cell's score; the maximum over the wave is the score.  Both inner loops stay in this function, as in
// sweep_local; the row array stays in it too, and an observer sees the last row through last(): handing d[] out by reference
// moved the registers of score_global_kernel and score_shuffled_kernel.
template <int R, class Rows = TableRows, class Obs>
__device__ __forceinline__ int sweep_global(const int* tab, const GlobalCols<R>& k, const typename Rows::Src* qc, int Q,
                                            int free_del, int free_ins, Obs&& obs) {
  const int lane = threadIdx.x;
  const int cb = 4 * lane;
  const int gi = k.gi, ge = k.ge, T = k.T, ls = k.ls;
  int d[R][4], gmx[R][4], cv[R], ak[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    cv[r] = kNegS;
#pragma unroll
    for (int x = 0; x < 4; ++x) { d[r][x] = kNegS; gmx[r][x] = kNegS; }
  }
  int clast = kNegS;                                               // max over rows of D[k][T-2] (free insertions into the final cell)
  auto finish_row = [&]() {
    int sk = kNegS;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int tk = kNegS;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int A = d[r][x] + k.gec[r][x];                     // non-interior cells hold "minus infinity": never a source
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
  {
    // row 1 (dpmatrix.h:409-418): one deletion from the origin, free if the template's head gap is
    int qrow;
    if constexpr (Rows::kInSweep) qrow = (int)qc[1] * 128;
    else qrow = Rows::first(tab, qc);
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int c = cb + 256 * r + x;
        const int cost = (c >= 2 && !free_del) ? gi + ge * (c - 2) : 0;
        d[r][x] = k.in[r][x] ? sweep_tab_at(tab, qrow, k.code4[r][x]) - cost : kNegS;
      }
    finish_row();
    obs.row(1, d, clast);
  }
  int qcode_next = 0;
  if constexpr (Rows::kInSweep) qcode_next = (Q >= 4) ? (int)qc[2] : 0;
  for (int i = 2; i <= Q - 2; ++i) {                               // dpmatrix.h:447-486
    int qrow;
    if constexpr (Rows::kInSweep) {
      qrow = qcode_next * 128;
      if (i + 1 <= Q - 2) qcode_next = (int)qc[i + 1];
    } else qrow = Rows::row(tab, qc, i);
    const int roff = gi + ge * (i - 2);
    const int rowB = ge * (i - 1);
    const int col1 = free_ins ? 0 : roff;                          // column 1: one insertion from the origin (:421-426)
    int bk[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int pv = cv[r];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int m = d[r][x];
        const int A = ak[r][x];
        const int e = pv - k.ekc[r][x];
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
        const int s = sweep_tab_at(tab, qrow, k.code4[r][x]);
        int h = ((x == 0) ? uk : bk[r][x - 1]) + s;
        if (r == 0 && x == 1) h = (c == 1) ? s - col1 : h;
        d[r][x] = k.in[r][x] ? h : kNegS;
      }
    }
    finish_row();
    obs.row(i, d, clast);
  }
  // ---- the final cell (dpmatrix.h:505-534): row Q-2 is in d[], gmx holds rows <= Q-3, clast every row of column T-2 -----
  obs.last(d);
  int best = (lane == ls) ? sweep_pick<R>(d, k.rs, k.xs, kNegS) : kNegS;   // match: D[Q-2][T-2] (the final cell's similarity is 0)
  int dl = kNegS;                                                  // deletion from (Q-2, k), k = 1 .. T-2 (k = T-2 costs nothing)
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int c = cb + 256 * r + x;
      const int len = T - 2 - c;
      const int cost = (len < 1 || free_del) ? 0 : gi + ge * (len - 1);
      dl = max(dl, k.in[r][x] ? d[r][x] - cost : kNegS);
    }
  best = max(best, dl);
  int il;                                                          // insertion from (k, T-2), k = 1 .. Q-2
  if (free_ins) il = clast;
  else {
    const int g = sweep_pick<R>(gmx, k.rs, k.xs, kNegS);           // max over k <= Q-3 of D[k][T-2] + ge k
    il = (lane == ls && Q >= 4) ? g - (gi + ge * (Q - 3)) : kNegS;
  }
  return max(best, il);
}

}  // namespace aln
