// search_zscore.hip — shuffle z-scores of search hits: the background sample of every hit scored and reduced on the device (gfx950).
//
// A raw local score is length- and composition-biased; the classic remedy places it against the scores of the SAME template
// with permutations of the query.  That is n_shuffles x (number of hits) score-only alignments — the work score_only.hip's
// register-resident row sweep was built for — and nothing but two 64-bit sums per hit has to leave the device:
//   shuffle_queries_kernel         residue queries, one thread per (query row, shuffle): the permuted residue codes, sentinels in place
//   shuffle_orders_kernel          profile queries, one thread per (query row, shuffle): the order of the rows as uint16 indices
//   class_list_kernel              (score_common.h) the used hit slots listed by template length class R = ceil(T / 256), over
//                                  a plain array of template indices: any align type, any hit list
//   score_shuffled_kernel<R,LOCAL,Side>  one wave per (listed slot, group of shuffles): the template-side state of
//                                  score_local_kernel<R> / score_global_kernel<R> is built ONCE, then the row sweep
//                                  (score_sweep.h) runs once per shuffle of the group; score and score^2 are summed in 64 bits
//                                  and leave the wave as two atomic adds (integer addition: the result does not depend on the order)
// aln_hits_zscores permutes a query's residues; a position-specific query (aln_qprofiles) has rows instead, so shuffle s of
// profile q is the profile with its interior rows in another order — the order the header's rule gives for the list 0 .. L-1.
// Permuted profiles are never materialised (n_shuffles x rows x 128 B per query, written once and read back): the device holds
// ONE copy of a profile's rows (ScoreRun::upload_profile_rows, 32 int32 per row) and a wave reads it in permuted order.  That
// copy is shared by the K x n_shuffles sweeps of the query and stays in L2; a shuffle costs 2 B per row.
// Both entries run one driver (zscores_block): query rows are handled a chunk at a time so that the shuffled strings (or orders)
// and the accumulators stay below 1 GiB each.  Hits on templates beyond 2048 columns go the way they go in
// aln_score_all_vs_all: the host materialises the same permutations (the same statement of the rule, search_zscore.h) and
// score_through_batches scores them through full builds.
#include <cstdio>
#include <string>
#include <vector>

#include "search_zscore.h"

namespace aln {

// ---- the orders ------------------------------------------------------------------------------------------------------------
// An order of a profile of Q rows is `stride` uint16: entry 0 is 0 (the '^' row), entry 1 + i is 1 + a[i] (a: the header's rule
// on 0 .. L-1, L = Q - 2), every entry from Q - 1 on is 0.  INVARIANT (beside the one of ScoreRun::upload_profile_rows): stride =
// Q + 14 rounded up to a multiple of 8 and every order starts 16-byte aligned — a sweep requests the 8-row chunks its rows
// 1 .. Q-2 lie in plus the one after, i.e. entries 0 .. Q + 13, eight at a time as one aligned 16-byte scalar load; the entries
// behind Q - 2 are requested and never used as rows of the recurrence, so they name row 0, a valid row of zeros.  Every entry is
// < Q: no copy reads outside its profile.
__host__ __device__ __forceinline__ int64_t order_stride(int64_t Q) { return (Q + 14 + 7) & ~(int64_t)7; }

struct ShuffleArgs {
  const uint8_t* qcodes; const int64_t* qoff;   // query pool (orders: qcodes is not read; qoff: the profiles' offsets, in rows)
  const int64_t* poff;                          // nr + 1: row r's shuffles start at entry poff[r] of the pool (no used slot: none)
  void* pool;                                   // strings: |q| bytes each; orders: order_stride(|q|) uint16 each
  int q_first, nr, S;                           // q_first: query index of the chunk's row 0
  uint32_t seed;
};

// Fisher-Yates is serial per string; the strings are independent.  The string lives in global memory: a swap is two byte
// loads and two byte stores that stay in L2, and the whole pass is a small fraction of the scoring that follows.
__global__ __launch_bounds__(256) void shuffle_queries_kernel(ShuffleArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)a.nr * a.S) return;
  const int row = (int)(e / a.S), s = (int)(e % a.S);
  const int64_t p0 = a.poff[row];
  if (a.poff[row + 1] == p0) return;
  const int q = a.q_first + row;
  const int Q = (int)(a.qoff[q + 1] - a.qoff[q]);
  const uint8_t* __restrict__ src = a.qcodes + a.qoff[q];
  uint8_t* dst = static_cast<uint8_t*>(a.pool) + p0 + (int64_t)s * Q;
  for (int i = 0; i < Q; ++i) dst[i] = src[i];
  shuffle_interior(a.seed, (uint32_t)q, (uint32_t)s, dst + 1, Q - 2);
}

__global__ __launch_bounds__(256) void shuffle_orders_kernel(ShuffleArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)a.nr * a.S) return;
  const int row = (int)(e / a.S), s = (int)(e % a.S);
  const int64_t p0 = a.poff[row];
  if (a.poff[row + 1] == p0) return;
  const int q = a.q_first + row;
  const int Q = (int)(a.qoff[q + 1] - a.qoff[q]);
  const int stride = (int)order_stride(Q);
  uint16_t* dst = static_cast<uint16_t*>(a.pool) + p0 + (int64_t)s * stride;
  for (int i = 0; i < stride; ++i) dst[i] = (uint16_t)(i < Q - 1 ? i : 0);
  shuffle_interior(a.seed, (uint32_t)q, (uint32_t)s, dst + 1, Q - 2);
}

// ---- the row source of a permuted profile -------------------------------------------------------------------------------------
// ProfileRows (score_sweep.h) with a gather: the same ring of 32 rows, the same request one chunk ahead, the same
// s_waitcnt vmcnt(1) — but lane l of the copy for chunk c reads 16 bytes of row order[8 c + l / 8], part l % 8.  The LDS side of
// the copy is lane-linear whatever the lanes' source addresses are, so the ring holds the permuted rows in sweep order and
// nothing else changes.  The eight indices of a chunk are 16 bytes at a wave-uniform, 16-byte-aligned address, read through the
// constant address space: ONE scalar load, counted by lgkmcnt, so the copies' vmcnt accounting is untouched (an ordinary
// global load of the indices would make the compiler drain the copy in flight with vmcnt(0)).  The orders were written by an
// earlier launch on the same stream, so the scalar cache cannot hold a stale line of them.  Each lane picks its 16 bits with
// three selects and a shift.
struct PermutedSrc {
  const int4* rows;                             // row 0 of the profile (the resident copy)
  const uint16_t* order;                        // this shuffle's order
};
struct PermutedProfileRows {
  typedef PermutedSrc Src;
  static constexpr bool kInSweep = false;
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ void fill(const int* ring, const PermutedSrc* src, int c) {
    typedef __attribute__((address_space(3))) void* lds_t;
    typedef __attribute__((address_space(1))) void* glb_t;
    typedef const __attribute__((address_space(4))) u32x4* idx_t;
    const u32x4 w = *(idx_t)(uintptr_t)(src->order + 8 * c);
    const int lane = (int)threadIdx.x;                       // rows 2 k and 2 k + 1 of the chunk share word k = lane / 16
    const unsigned lo = (lane & 16) ? w.y : w.x, hi = (lane & 16) ? w.w : w.z;
    const unsigned pair = (lane & 32) ? hi : lo;
    const int r = (int)((pair >> ((lane & 8) * 2)) & 0xFFFFu);
    __builtin_amdgcn_global_load_lds((glb_t)(src->rows + r * 8 + (lane & 7)), (lds_t)(ring + (c & 3) * 256), 16, 0, 0);
  }
  static __device__ __forceinline__ void landed() { asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); }
  // A wave runs several sweeps over one ring.  When first() is called again the previous sweep's last copy (its never-read
  // chunk) may still be in flight and its last rows' LDS reads may just have been issued.  The reads: every one of them feeds
  // the score the wave reduced before it came here, and the explicit lgkmcnt(0) below makes "they have all returned" a fact of
  // the instruction stream, not of timing.  The copy: copies complete in issue order, so it lands before chunks 0 and 1 of this
  // sweep do, whichever slot it writes, and the vmcnt(1) that follows retires it together with chunk 0.
  static __device__ __forceinline__ int first(const int* ring, const PermutedSrc* src) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    fill(ring, src, 0); fill(ring, src, 1); landed();
    return 128;
  }
  static __device__ __forceinline__ int row(const int* ring, const PermutedSrc* src, int i) {
    if ((i & 7) == 0) { fill(ring, src, (i >> 3) + 1); landed(); }
    return (i & 31) * 128;
  }
};

struct ZScoreArgs {
  ScoreArgs a;                                  // a.q_begin: query index of the chunk's row 0; residues: a.qcodes is not read
  const int32_t* list;                          // blockIdx.x -> slot of the chunk
  const int32_t* slot_t;                        // slot -> template index
  const int64_t* poff; const void* pool;        // the shuffled strings, or the orders (ShuffleArgs)
  unsigned long long* acc;                      // slot -> { sum, sum of squares }
  int K, S, G;                                  // G: shuffles per wave; blockIdx.y = group
  int free_del, free_ins;
};

// The template-side state of score_local_kernel<R> / score_global_kernel<R> (score_sweep.h) is built once, the sweep runs once
// per shuffle of the group.  Side (score_common.h) says what a shuffle is: the residue side sweeps shuffle s's own string, the
// staged side sweeps the one resident profile through shuffle s's order (a PermutedSrc on the stack).  The two calls are
// spelled out under `if constexpr`: a generic lambda over the per-shuffle source moved the registers of six residue
// instantiations.  For the same reason both sides' operands (stride, pr, o0; q0) are formed in the prologue, each
// dead on the other side and dropped by the compiler: one typed pointer for both sides reordered instructions in the prologues of
// several instantiations, and forming pr inside the loops moved the registers of the staged ones (4.8j).
template <int R, bool LOCAL, class Side>
__global__ __launch_bounds__(64) void score_shuffled_kernel(ZScoreArgs z) {
  __shared__ __attribute__((aligned(16))) int lds[32 * 32];
  const int lane = threadIdx.x;
  Side::stage(lds, z.a);
  const int slot = z.list[blockIdx.x];
  const int row = slot / z.K, ti = z.slot_t[slot], qi = z.a.q_begin + row;
  const int s0 = blockIdx.y * z.G, n_s = min(z.G, z.S - s0);
  const int Q = (int)(z.a.qoff[qi + 1] - z.a.qoff[qi]), T = (int)(z.a.toff[ti + 1] - z.a.toff[ti]);
  const int stride = (int)order_stride(Q);                                                   // staged side only
  const int4* __restrict__ pr = ProfileQuery::rows(z.a, qi);
  const uint16_t* __restrict__ o0 = static_cast<const uint16_t*>(z.pool) + z.poff[row] + (int64_t)s0 * stride;
  const uint8_t* __restrict__ q0 = static_cast<const uint8_t*>(z.pool) + z.poff[row] + (int64_t)s0 * Q;   // residue side only
  const uint8_t* __restrict__ tc = z.a.tcodes + z.a.toff[ti];
  long long sum = 0, sumsq = 0;
  auto add = [&](int m) {                                      // one shuffle's score, reduced over the wave
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o));
    sum += m; sumsq += (long long)m * m;
  };
  if constexpr (LOCAL) {
    LocalCols<R> cols;
    cols.load(tc, T, z.a.gi, z.a.ge);
    for (int s = 0; s < n_s; ++s) {
      int d[R][4];
      if constexpr (Side::kStaged) {
        const PermutedSrc src = {pr, o0 + (size_t)s * stride};
        add(sweep_local<R, PermutedProfileRows>(lds, cols, &src, Q - 2, d, NoObserver()));
      } else add(sweep_local<R>(lds, cols, q0 + (size_t)s * Q, Q - 2, d, NoObserver()));
    }
  } else if (Q == 2 || T == 2) {
    // degenerate shortcuts of score_global_kernel: one gap from the origin, the same for every shuffle
    int cost = 0;
    if (Q == 2) { const int len = T - 2; cost = (len < 1 || z.free_del) ? 0 : z.a.gi + z.a.ge * (len - 1); }
    else { const int len = Q - 2; cost = (len < 1 || z.free_ins) ? 0 : z.a.gi + z.a.ge * (len - 1); }
    sum = -(long long)cost * n_s; sumsq = (long long)cost * cost * n_s;
  } else {
    GlobalCols<R> cols;
    cols.load(tc, T, z.a.gi, z.a.ge);
    for (int s = 0; s < n_s; ++s) {
      if constexpr (Side::kStaged) {
        const PermutedSrc src = {pr, o0 + (size_t)s * stride};
        add(sweep_global<R, PermutedProfileRows>(lds, cols, &src, Q, z.free_del, z.free_ins, NoObserver()));
      } else add(sweep_global<R>(lds, cols, q0 + (size_t)s * Q, Q, z.free_del, z.free_ins, NoObserver()));
    }
  }
  // the last sweep's never-read chunk: nothing in flight into LDS at the end
  if constexpr (Side::kStaged) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (lane == 0) {
    atomicAdd(&z.acc[2 * (size_t)slot], (unsigned long long)sum);
    atomicAdd(&z.acc[2 * (size_t)slot + 1], (unsigned long long)sumsq);
  }
}

// The shared body of aln_hits_zscores and aln_hits_zscores_profiles (run: prepared).  Query lengths are read from run.queries —
// for profiles the placeholder pool, which shares the profiles' offsets.  What depends on the query side is marked "side:".
static int zscores_block(ScoreRun& run, int32_t K, const aln_hit* hits, const int32_t* n_hits, int32_t S, uint32_t seed,
                         aln_hit_stats* stats) {
  aln_ctx* ctx = run.ctx;
  const aln_seqs *queries = run.queries, *templates = run.templates;
  const aln_qprofiles* prof = run.prof;
  const int32_t q_begin = run.q_begin;
  const int rows = run.rows, n_t = run.n_t;
  if (rows == 0) return ALN_OK;
  for (int r = 0; r < rows; ++r) {
    if (n_hits[r] < 0 || n_hits[r] > K) return ALN_E_ARG;
    for (int k = 0; k < n_hits[r]; ++k) {
      const int32_t t = hits[(size_t)r * K + k].t;
      if (t < 0 || t >= n_t) return ALN_E_ARG;
    }
  }
  if (run.route == ScoreRun::kAllFull) return ALN_E_NOT_INTEGRAL;
  auto write_chunk = [&](int r0, int nr, const long long* acc) {   // acc: the chunk's { sum, sumsq } per slot
    for (int r = 0; r < nr; ++r)
      for (int k = 0; k < K; ++k) {
        const size_t g = (size_t)(r0 + r) * K + k, c = (size_t)r * K + k;
        aln_hit_stats o = {0, 0, 0, 0.0f};
        if (k < n_hits[r0 + r]) {
          o.sum = acc[2 * c]; o.sumsq = acc[2 * c + 1]; o.n = S;
          o.z = z_of(S, hits[g].score, o.sum, o.sumsq);
        }
        stats[g] = o;
      }
  };
  if (run.route == ScoreRun::kNothing) {           // no template, hence no used slot
    write_chunk(0, rows, nullptr);
    return ALN_OK;
  }
  auto len_of = [&](int r) -> int64_t { return queries->offsets[q_begin + r + 1] - queries->offsets[q_begin + r]; };
  // side: the pool entries the S shuffles of a query of Q positions take — bytes of strings, or uint16 of orders
  auto pool_entries = [&](int64_t Q) -> int64_t { return (int64_t)S * (prof ? order_stride(Q) : Q); };
  const size_t entry_bytes = prof ? 2 : 1;

  // side: the device rows of profiles go up once for [q_begin, q_end) when they fit the budget, else (or by the hint) chunk by chunk
  if (prof)
    run.rows_per_slab = ctx->hints.zscore_rows_per_chunk != 0 ||
                        ((size_t)(prof->offsets[run.q_end] - prof->offsets[q_begin]) + kProfilePadRows) * 128 > kZBudget;

  // chunks of query rows: shuffled strings or orders (per row with a used slot), accumulators (16 B x K per row) and, side:
  // where a chunk uploads its own, the device rows (128 B per profile row)
  struct Chunk { int r0, nr; size_t pool, rowbytes; };
  std::vector<Chunk> chunks;
  {
    const int cap = (int)std::min<size_t>((size_t)0x7FFFFFFF / (size_t)K, kZBudget / ((size_t)K * 16));
    const int forced = ctx->hints.zscore_chunk_rows;
    const int max_rows = forced > 0 ? std::min(forced, cap) : cap;   // a forced size is an upper bound: the budgets still hold
    Chunk c = {0, 0, 0, (size_t)kProfilePadRows * 128};
    for (int r = 0; r < rows; ++r) {
      const size_t need = n_hits[r] > 0 ? (size_t)pool_entries(len_of(r)) * entry_bytes : 0;
      const size_t rneed = run.rows_per_slab ? (size_t)len_of(r) * 128 : 0;
      if (c.nr > 0 && (c.nr >= max_rows || c.pool + need > kZBudget || c.rowbytes + rneed > kZBudget)) {
        chunks.push_back(c); c = {r, 0, 0, (size_t)kProfilePadRows * 128};
      }
      c.nr++; c.pool += need; c.rowbytes += rneed;
    }
    chunks.push_back(c);
  }
  size_t max_pool = prof ? 16 : 1; int max_nr = 1;       // side: an order is fetched 16 bytes at a time
  for (const Chunk& c : chunks) { max_pool = std::max(max_pool, c.pool); max_nr = std::max(max_nr, c.nr); }

  DeviceBufs bufs(run);                                  // every exit below is STRY / RTRY (score_common.h), or the last line
  uint8_t* dpool = nullptr; int64_t* dpoff = nullptr; int32_t *dslot = nullptr, *dlist = nullptr, *dfill = nullptr;
  unsigned long long* dacc = nullptr;
  RTRY(run.upload());
  const size_t max_slots = (size_t)max_nr * K;
  STRY(bufs.get(dpool, max_pool));
  STRY(bufs.get(dpoff, (size_t)max_nr + 1));
  STRY(bufs.get(dslot, max_slots));
  STRY(bufs.get(dlist, max_slots));
  STRY(bufs.get(dfill, 9));
  STRY(bufs.get(dacc, max_slots * 2));
  std::vector<int64_t> poff((size_t)max_nr + 1);
  std::vector<int32_t> slot_t(max_slots);
  std::vector<long long> acc(max_slots * 2);
  std::vector<int32_t> fcol((size_t)n_t, 0), long_list;
  std::vector<float> long_sc, shuf_rows;
  std::vector<long long> lsum, lsumsq;
  std::vector<int64_t> shuf_off, perm;
  std::string shuf;
  const int n_groups = (S + kShufGroup - 1) / kShufGroup, G = (S + n_groups - 1) / n_groups;   // groups of equal size

  for (const Chunk& c : chunks) {
    const int r0 = c.r0, nr = c.nr, n_slots = nr * K;
    int cls_cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    poff[0] = 0;
    for (int r = 0; r < nr; ++r) {
      poff[(size_t)r + 1] = poff[r] + (n_hits[r0 + r] > 0 ? pool_entries(len_of(r0 + r)) : 0);
      for (int k = 0; k < K; ++k) {
        int32_t t = -1;
        if (k < n_hits[r0 + r]) {
          t = hits[(size_t)(r0 + r) * K + k].t;
          const int64_t T = templates->offsets[t + 1] - templates->offsets[t];
          cls_cnt[T > 2048 ? 0 : (int)((T + 255) / 256)]++;
        }
        slot_t[(size_t)r * K + k] = t;
      }
    }
    int n_used = 0;
    for (int k = 0; k < 9; ++k) n_used += cls_cnt[k];
    if (n_used > cls_cnt[0]) {
      if (run.rows_per_slab) RTRY(run.upload_profile_rows(q_begin + r0, q_begin + r0 + nr));
      STRY(hipMemcpyAsync(dpoff, poff.data(), (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
      STRY(hipMemcpyAsync(dslot, slot_t.data(), (size_t)n_slots * 4, hipMemcpyHostToDevice, ctx->stream));
      STRY(hipMemsetAsync(dfill, 0, 9 * 4, ctx->stream));
      STRY(hipMemsetAsync(dacc, 0, (size_t)n_slots * 16, ctx->stream));
      const ShuffleArgs sh = {run.dq, run.dqo, dpoff, dpool, q_begin + r0, nr, S, seed};
      const dim3 sgrid((unsigned)(((long long)nr * S + 255) / 256));
      if (prof) hipLaunchKernelGGL(shuffle_orders_kernel, sgrid, dim3(256), 0, ctx->stream, sh);      // side: which shuffle kernel
      else hipLaunchKernelGGL(shuffle_queries_kernel, sgrid, dim3(256), 0, ctx->stream, sh);
      STRY(hipGetLastError());
      const SlotClass sc = {dslot, run.dto};
      hipLaunchKernelGGL(class_list_kernel<SlotClass>, dim3((n_slots + 255) / 256), dim3(256), 0, ctx->stream, sc, n_slots, ClassOff::of(cls_cnt), dfill, dlist);
      STRY(hipGetLastError());
      ZScoreArgs z = {};
      z.a = run.a; z.a.q_begin = q_begin + r0;          // (after upload_profile_rows: it sets a.qcodes)
      z.slot_t = dslot; z.poff = dpoff; z.pool = dpool; z.acc = dacc; z.K = K; z.S = S; z.G = G;
      z.free_del = run.free_del; z.free_ins = run.free_ins;
      STRY(launch_classes(prof != nullptr, cls_cnt, [&](auto side, auto rc, int cnt, int off) {
        typedef decltype(side) Side;
        constexpr int R = decltype(rc)::value;
        z.list = dlist + off;
        const dim3 grid(cnt, n_groups);
        if (run.local) hipLaunchKernelGGL((score_shuffled_kernel<R, true, Side>), grid, dim3(64), 0, ctx->stream, z);
        else hipLaunchKernelGGL((score_shuffled_kernel<R, false, Side>), grid, dim3(64), 0, ctx->stream, z);
      }));
      STRY(hipMemcpyAsync(acc.data(), dacc, (size_t)n_slots * 16, hipMemcpyDeviceToHost, ctx->stream));
      STRY(hipStreamSynchronize(ctx->stream));
    } else std::fill(acc.begin(), acc.begin() + (size_t)n_slots * 2, 0LL);
    // hits on templates beyond 2048 columns: the same permutations made here (search_zscore.h) and scored through full builds
    // row by row, shuffles [sa, sa + nb) at a time
    if (cls_cnt[0] > 0)
      for (int r = 0; r < nr; ++r) {
        long_list.clear();
        for (int k = 0; k < n_hits[r0 + r]; ++k) {
          const int32_t t = slot_t[(size_t)r * K + k];
          if (templates->offsets[t + 1] - templates->offsets[t] <= 2048) continue;
          if (std::find(long_list.begin(), long_list.end(), t) == long_list.end()) { fcol[t] = (int32_t)long_list.size(); long_list.push_back(t); }
        }
        if (long_list.empty()) continue;
        const int q = q_begin + r0 + r;
        const int64_t Q = len_of(r0 + r);
        const size_t ld = long_list.size();
        lsum.assign(ld, 0); lsumsq.assign(ld, 0);
        // side: residue strings all at once; permuted copies of the profile's rows, at most kZBudget bytes of them at a time
        const int per = prof ? (int)std::max<size_t>(1, std::min<size_t>((size_t)S, kZBudget / ((size_t)Q * prof->n * 4))) : S;
        for (int sa = 0; sa < S; sa += per) {
          const int nb = std::min(per, S - sa);
          shuf_off.resize((size_t)nb + 1);
          for (int b = 0; b <= nb; ++b) shuf_off[b] = (int64_t)b * Q;
          aln_qprofiles sp = {};
          if (prof) {                                    // the placeholder letters, and the rows in shuffle sa + b's order
            const int n_alpha = prof->n;
            const int64_t L = Q - 2;
            const float* src = prof->rows + (size_t)prof->offsets[q] * n_alpha;
            shuf_rows.assign((size_t)nb * Q * n_alpha, 0.f);
            shuf.assign((size_t)nb * Q, prof->alphabet[0]);
            perm.resize((size_t)std::max<int64_t>(L, 1));
            for (int b = 0; b < nb; ++b) {
              shuf[(size_t)b * Q] = '^'; shuf[(size_t)(b + 1) * Q - 1] = '$';
              for (int64_t i = 0; i < L; ++i) perm[i] = i;
              shuffle_interior(seed, (uint32_t)q, (uint32_t)(sa + b), perm.data(), (int)L);
              float* dst = shuf_rows.data() + (size_t)b * Q * n_alpha;
              for (int64_t i = 0; i < L; ++i)
                std::copy(src + (size_t)(1 + perm[i]) * n_alpha, src + (size_t)(2 + perm[i]) * n_alpha, dst + (size_t)(1 + i) * n_alpha);
            }
            sp = {nb, shuf_off.data(), shuf_rows.data(), n_alpha, prof->alphabet};
          } else {                                       // the query's letters, shuffled
            shuf.resize((size_t)nb * Q);
            for (int b = 0; b < nb; ++b) {
              std::copy(queries->residues + queries->offsets[q], queries->residues + queries->offsets[q + 1], shuf.begin() + (size_t)b * Q);
              shuffle_interior(seed, (uint32_t)q, (uint32_t)(sa + b), &shuf[(size_t)b * Q] + 1, (int)(Q - 2));   // '^' and '$' stay
            }
          }
          const aln_seqs sq = {nb, shuf_off.data(), shuf.data()};
          long_sc.assign((size_t)nb * ld, 0.f);
          RTRY(score_through_batches(ctx, &sq, templates, run.sub, run.gap, 0, nb, long_list, long_sc.data(), fcol.data(), ld,
                                     prof ? &sp : nullptr));
          for (size_t j = 0; j < ld; ++j)
            for (int b = 0; b < nb; ++b) { const long long v = (long long)long_sc[(size_t)b * ld + j]; lsum[j] += v; lsumsq[j] += v * v; }
        }
        for (int k = 0; k < n_hits[r0 + r]; ++k) {
          const int32_t t = slot_t[(size_t)r * K + k];
          if (templates->offsets[t + 1] - templates->offsets[t] <= 2048) continue;
          acc[2 * ((size_t)r * K + k)] = lsum[fcol[t]]; acc[2 * ((size_t)r * K + k) + 1] = lsumsq[fcol[t]];
        }
      }
    write_chunk(r0, nr, acc.data());
  }
  return ALN_OK;
}

}  // namespace aln

using namespace aln;

extern "C" int aln_hits_zscores(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                                const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K, const aln_hit* hits,
                                const int32_t* n_hits, int32_t n_shuffles, uint32_t seed, aln_hit_stats* stats) {
  if (!hits || !n_hits || !stats || K < 1 || K > 1024 || n_shuffles < 1 || n_shuffles > 4096) return ALN_E_ARG;
  ScoreRun run;
  int rc = run.prepare(ctx, queries, templates, sub, gap, q_begin, q_end);
  if (rc != ALN_OK) return rc;
  return zscores_block(run, K, hits, n_hits, n_shuffles, seed, stats);
}

// The same for the hits of a profile search: shuffle s permutes the profile's interior rows.
extern "C" int aln_hits_zscores_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* templates, const aln_gap* gap,
                                         int32_t q_begin, int32_t q_end, int32_t K, const aln_hit* hits, const int32_t* n_hits,
                                         int32_t n_shuffles, uint32_t seed, aln_hit_stats* stats) {
  if (!hits || !n_hits || !stats || K < 1 || K > 1024 || n_shuffles < 1 || n_shuffles > 4096) return ALN_E_ARG;
  ScoreRun run;
  int rc = run.prepare(ctx, nullptr, templates, nullptr, gap, q_begin, q_end, profiles);
  if (rc != ALN_OK) return rc;
  return zscores_block(run, K, hits, n_hits, n_shuffles, seed, stats);
}

#undef STRY
#undef RTRY
