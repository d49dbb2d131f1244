// enumerate.hip — Waterman-style near-optimal alignment enumeration on the resident DP planes (gfx950).
//
// Reference: ConstrainedNearOptimal (cw.h:68-284) and UnconstrainedNearOptimal (ucw.h:64-236): a depth-first
// branching traceback from the final cell; at a branch node every predecessor (match, then row q0-1 for
// i = t0-2..1 descending, then column t0-1 for j = q0-2..1 descending) whose forward score plus the reverse
// score so far minus the gap exceeds the threshold starts a new alignment (the first one continues in the
// current slot, later ones copy the state before the node); opt_path follows stored pointers until the
// template's SuboptFlags bit flips.  Discovery order decides the position of every alignment in the set.
//
// Device representation: alignments only ever grow by prepend(), so they form a trie — a node is one aligned
// pair plus a link to the pair after it; an alignment is (head node, score); "copy the alignment" is copying
// two words.  One wave walks one pair's DFS with an explicit stack of branch frames; the candidate scan of a
// branch node is done 64 predecessors at a time (ballot keeps the reference's order); fp32 sums are formed in
// the written order (f + r > thr, (f + r) - g > thr, score = r - g).  The host then sorts (score, index)
// with the same std::sort / std::partial_sort call the reference uses (alignment.h:922-932) and asks the
// device to unroll only the surviving alignments.
#include "enum_common.h"

namespace aln {

__global__ __launch_bounds__(64) void enumerate_kernel(const PairDesc* __restrict__ pairs, int pair, EvalDev proto,
                                                       const uint8_t* __restrict__ qcodes, const uint8_t* __restrict__ tcodes,
                                                       const float* __restrict__ tgi, const float* __restrict__ tge,
                                                       const float* __restrict__ Hbase, const uint32_t* __restrict__ Pbase,
                                                       const float* __restrict__ Sbase, EnumArgs a) {
  {
    const size_t bi = blockIdx.x;                 // position inside the group: every pool is sliced by it
    pair = a.pair_list ? a.pair_list[bi] : pair + (int)bi;
    a.node_pair += bi * a.node_cap; a.node_next += bi * a.node_cap;
    a.head += bi * a.ali_cap; a.score += bi * a.ali_cap;
    a.stack += bi * (size_t)a.stack_cap * kFrameWords;
    a.flags += (size_t)(a.pair_list ? pair : (int)bi) * (size_t)a.flags_stride;   // flag rows are indexed by the pair's place in the batch
    a.out += bi * 4;
  }
  const PairDesc pd = pairs[pair];
  EvalDev e = proto;
  e.Q = pd.Q; e.T = pd.T; e.ld = pd.ld;
  e.qc = qcodes ? qcodes + pd.q_off : nullptr;
  e.tc = tcodes ? tcodes + pd.t_off : nullptr;
  e.tgi = tgi ? tgi + pd.t_off : nullptr;
  e.tge = tge ? tge + pd.t_off : nullptr;
  bind_table_model(e, proto, pd);
  e.S = Sbase ? Sbase + pd.plane_off : nullptr;
  auto HV = [&](int i, int j) -> float { return load_score(Hbase, pd.plane_off, pd.ld, i, j, a.h_mode); };
  const int ld = pd.ld, lane = threadIdx.x;
  const int Q = pd.Q, T = pd.T;
  const bool cw = a.kind == ALN_ENUM_CW;

  uint32_t n_as = (uint32_t)a.first_slot + 1;   // as.push_back(SingleAlignment())  cw.h:82 / ucw.h:78
  uint32_t n_nodes = 0;
  int status = 0;
  // Lane 0 writes the pools, every lane reads them back through L2.  A store is only waited for (one memory round trip) right
  // before the next cross-lane read: `dirty` marks stores in flight, flush() is the s_waitcnt.  (Lane 0 re-reading a word it
  // wrote itself needs no wait: same lane, same address, program order.)
  bool dirty = false;
  auto flush = [&]() { if (dirty) { __builtin_amdgcn_s_waitcnt(0); dirty = false; } };
  if (lane == 0) { st_u(&a.head[a.first_slot], kNoNode); st_f(&a.score[a.first_slot], 0.f); }
  dirty = true;
  flush();

  const float top = HV(Q - 1, T - 1);
  float thr = (1.f - a.delta_ratio) * top;       // cw.h:86-88
  { float alt = top - 0.1f; thr = (alt < thr) ? alt : thr; }

  auto prepend = [&](int k, int q, int t) {     // as[k].prepend(q,t): a new trie node in front of the list
    if (n_nodes >= a.node_cap) { status = ALN_E_OVERFLOW; return; }
    if (lane == 0) {
      a.node_pair[n_nodes] = ((uint32_t)q << 16) | (uint32_t)t;
      a.node_next[n_nodes] = ld_u(&a.head[k]);
      st_u(&a.head[k], n_nodes);
    }
    ++n_nodes;
    dirty = true;
  };
  auto set_score = [&](int k, float s) { if (lane == 0) st_f(&a.score[k], s); dirty = true; };
  auto base_case = [&](int q0, int t0, int k0) {   // cw.h:100-108 / ucw.h:93-101
    prepend(k0, q0, t0);
    prepend(k0, 0, 0);
    flush();
    float s = ld_f(&a.score[k0]);
    s += HV(q0, t0);
    set_score(k0, s);
  };
  // the pointer-following loop of opt_path (cw.h:242-272 / ucw.h:207-228); returns the cell it stopped at.
  // 64 cells of the current diagonal are examined at once (lane l: cell (q0-l, t0-l)): the leading run of cells whose
  // stored pointer is the match pointer is taken in one step — their trie nodes are written in parallel, their
  // similarities are summed in path order (fp32 is not associative) — and a gap cell ends the run with one jump.
  auto walk = [&](int& q0, int& t0, int k0, bool force) {
    const bool flag = cw ? !a.flags[t0] : false;
    float sc = ld_f(&a.score[k0]);
    uint32_t hd = ld_u(&a.head[k0]);
    while (t0 > 1 && q0 > 1 && status == 0) {
      const int q = q0 - lane, t = t0 - lane;
      bool stop = !(q > 1 && t > 1);
      if (!stop && cw && !force && ((a.flags[t] != 0) == flag)) stop = true;   // the template's SuboptFlags bit flipped: branch point
      int pq = 0, pt = 0; float sv = 0.f, g = 0.f;
      if (!stop) {
        const uint32_t p = load_ptr_word(Pbase, pd.plane_off, ld, q, t, a.ptr_mode);
        decode_ptr(p, a.ptr_mode, q, t, pq, pt);
        sv = dev_sim(e, q, t);
      }
      const bool diag = !stop && pq == q - 1 && pt == t - 1;
      const unsigned long long m_end = __ballot(!diag);
      const int F = m_end ? __builtin_ctzll(m_end) : 64;          // first cell that is not a plain match step
      const bool gap_cell = F < 64 && !(((__ballot(stop)) >> F) & 1ull);
      const int n_proc = gap_cell ? F + 1 : F;
      if (n_proc == 0) break;
      if (n_nodes + (uint32_t)n_proc > a.node_cap) { status = ALN_E_OVERFLOW; break; }
      if (lane < n_proc) {
        a.node_pair[n_nodes + lane] = ((uint32_t)q << 16) | (uint32_t)t;
        a.node_next[n_nodes + lane] = lane == 0 ? hd : n_nodes + lane - 1;
      }
      hd = n_nodes + n_proc - 1;
      n_nodes += n_proc;
      if (gap_cell && lane == F) {
        if (q - pq == 1) g = dev_deletion(e, pt, t);
        else g = dev_insertion(e, pq, q, pt, t);
      }
      sc = add_in_path_order(sc, sv, n_proc);       // sc += sim (then sc -= 0 for a match step), in path order
      if (gap_cell) {
        sc -= __shfl(g, F);
        q0 = __shfl(pq, F); t0 = __shfl(pt, F);
      } else { q0 -= n_proc; t0 -= n_proc; }
    }
    if (lane == 0) { st_u(&a.head[k0], hd); st_f(&a.score[k0], sc); }
    dirty = true;
  };

  // Depth-first search with an explicit stack of branch frames.  A pending call is either
  //   CALL_BRANCH: branch(q,t,k,force)      or      CALL_OPT: opt_path(q,t,k,force)
  enum { CALL_NONE = 0, CALL_BRANCH = 1, CALL_OPT = 2 };
  int call = CALL_BRANCH, cq = Q - 1, ct = T - 1, ck = a.first_slot; bool cforce = false;
  int sp = 0;
  long guard = 0;
  while ((call != CALL_NONE || sp > 0) && status == 0) {
    if (++guard > (1L << 40)) { status = ALN_E_OVERFLOW; break; }
    flush();
    if (call == CALL_OPT) {
      call = CALL_NONE;
      int q0 = cq, t0 = ct; const int k0 = ck; const bool force = cforce;
      if (q0 == 1 || t0 == 1) { base_case(q0, t0, k0); continue; }           // cw.h:220-228
      walk(q0, t0, k0, force);
      if (cw) { call = CALL_BRANCH; cq = q0; ct = t0; ck = k0; cforce = force; }   // branch(pq,pt,k0,force)  cw.h:276
      else base_case(q0, t0, k0);                                                    // ucw.h:232-234
      continue;
    }
    if (call == CALL_BRANCH) {
      call = CALL_NONE;
      const int q0 = cq, t0 = ct, k0 = ck;
      if (q0 == 1 || t0 == 1) { base_case(q0, t0, k0); continue; }
      if (cw && cforce) { call = CALL_OPT; cforce = true; continue; }                          // cw.h:205-209
      if (n_as > a.user_limit) { call = CALL_OPT; cforce = true; continue; }                   // cw.h:127-140 / ucw.h:110-121
      if ((uint32_t)sp >= a.stack_cap) { status = ALN_E_OVERFLOW; break; }
      const uint32_t ch = ld_u(&a.head[k0]);
      const float cs = ld_f(&a.score[k0]);
      const float r = cs + dev_sim(e, q0, t0);
      if (lane == 0) {
        uint32_t* f = a.stack + (size_t)sp * kFrameWords;
        st_u(f + 0, (uint32_t)q0); st_u(f + 1, (uint32_t)t0); st_u(f + 2, (uint32_t)k0); st_u(f + 3, 0u);
        st_u(f + 4, ch); st_u(f + 5, __float_as_uint(cs)); st_u(f + 6, __float_as_uint(r));
      }
      dirty = true;
      ++sp;
      continue;
    }
    // ---- resume the branch frame on top of the stack: scan for the next accepted candidate ----
    uint32_t* f = a.stack + (size_t)(sp - 1) * kFrameWords;
    const int q0 = (int)ld_u(f + 0), t0 = (int)ld_u(f + 1), k0 = (int)ld_u(f + 2), cursor = (int)ld_u(f + 3);
    const uint32_t curr_head = ld_u(f + 4);
    const float curr_score = __uint_as_float(ld_u(f + 5)), r = __uint_as_float(ld_u(f + 6));
    const int k = (cursor == 0) ? k0 : (int)n_as;         // k = as.size() after every accepted candidate's subtree
    const int ndel = t0 - 2, nins = q0 - 2;
    const int ncand = 1 + ndel + nins;
    int found = -1; float fg = 0.f; int fq = 0, ft = 0;
    if (e.model == ALN_GAP_AFFINE_CONST) {
      // Constant affine gaps: the candidate's cell and its gap cost are pure arithmetic, so the scan is written without a single
      // branch around a load — 16 x 64 score loads are in flight per trip and one HBM round trip (~2 us) covers 1024 candidates.
      // (With loads inside the if/else ladder below the compiler has to wait for each one before the next group.)
      constexpr int kTrip = 16;
      const bool fdel = (e.align_type == ALN_LOCAL || e.align_type == ALN_SEMI_LOCAL || e.align_type == ALN_LOCAL_GLOBAL);
      const bool fins = (e.align_type == ALN_LOCAL || e.align_type == ALN_SEMI_LOCAL || e.align_type == ALN_GLOBAL_LOCAL);
      const uint16_t* H16p = reinterpret_cast<const uint16_t*>(Hbase) + pd.plane_off;
      const float* H32p = Hbase + pd.plane_off;
      for (int base = cursor; base < ncand && found < 0; base += 64 * kTrip) {
        int cq[kTrip], ct[kTrip]; float fsc[kTrip];
#pragma unroll
        for (int u = 0; u < kTrip; ++u) {
          const int idx = base + 64 * u + lane;
          const bool isdel = idx <= ndel;                       // idx 0 (match) has the same row
          int q = isdel ? q0 - 1 : q0 - 2 - (idx - ndel - 1);
          int t = idx == 0 ? t0 - 1 : isdel ? t0 - 1 - idx : t0 - 1;
          const bool in = idx < ncand;
          q = in ? q : q0 - 1; t = in ? t : t0 - 1;            // lanes past the end read a harmless cell
          cq[u] = q; ct[u] = t;
        }
        if (a.h_mode == 0) {
#pragma unroll
          for (int u = 0; u < kTrip; ++u) fsc[u] = H32p[(size_t)cq[u] * ld + ct[u]];
        } else {
#pragma unroll
          for (int u = 0; u < kTrip; ++u) fsc[u] = (float)H16p[(size_t)cq[u] * ld + ct[u]];
        }
#pragma unroll
        for (int u = 0; u < kTrip; ++u) {
          if (found >= 0 || base + 64 * u >= ncand) break;
          const int idx = base + 64 * u + lane;
          const int q = cq[u], t = ct[u];
          float g = 0.f;
          if (idx != 0) {
            if (idx <= ndel) {                                  // aasubalib.h:27-51
              const int len = t0 - t - 1;
              g = (len < 1 || (fdel && (t == 0 || t0 == T - 1))) ? 0.f : e.gi + e.ge * (float)(len - 1);
            } else {                                            // aasubalib.h:53-77
              const int len = q0 - q - 1;
              g = (len < 1 || (fins && (q == 0 || q0 == Q - 1))) ? 0.f : e.gi + e.ge * (float)(len - 1);
            }
          }
          const bool ok = idx < ncand && (idx == 0 ? fsc[u] + r > thr : fsc[u] + r - g > thr);
          const unsigned long long m = __ballot(ok);
          if (m) {
            const int l = __builtin_ctzll(m);
            found = base + 64 * u + l;
            fg = __shfl(g, l); fq = __shfl(q, l); ft = __shfl(t, l);
          }
        }
      }
    } else {
    // 4 x 64 candidates per trip: the score loads of all four groups are in flight together, the ballots keep the order
      for (int base = cursor; base < ncand && found < 0; base += 256) {
        bool ok[4]; float g[4]; int pq[4], pt[4];
  #pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int idx = base + 64 * u + lane;
          ok[u] = false; g[u] = 0.f; pq[u] = 0; pt[u] = 0;
          if (idx < ncand) {
            if (idx == 0) {                                     // match, cw.h:151-162
              pq[u] = q0 - 1; pt[u] = t0 - 1;
              const float fsc = HV(pq[u], pt[u]);
              ok[u] = fsc + r > thr;
            } else if (idx <= ndel) {                           // deletions i = t0-2 .. 1, cw.h:166-178
              pq[u] = q0 - 1; pt[u] = t0 - 1 - idx;
              const float fsc = HV(pq[u], pt[u]);
              g[u] = dev_deletion(e, pt[u], t0);
              ok[u] = fsc + r - g[u] > thr;
            } else {                                            // insertions j = q0-2 .. 1, cw.h:182-194
              pq[u] = q0 - 2 - (idx - ndel - 1); pt[u] = t0 - 1;
              const float fsc = HV(pq[u], pt[u]);
              g[u] = dev_insertion(e, pq[u], q0, pt[u], t0);
              ok[u] = fsc + r - g[u] > thr;
            }
          }
        }
  #pragma unroll
        for (int u = 0; u < 4; ++u) {
          const unsigned long long m = __ballot(ok[u]);
          if (m && found < 0) {
            const int l = __builtin_ctzll(m);
            found = base + 64 * u + l;
            fg = __shfl(g[u], l); fq = __shfl(pq[u], l); ft = __shfl(pt[u], l);
          }
        }
      }
  }
    if (found < 0) {
      --sp;                                                 // branch() returns
      if (cursor == 0) {                                    // k == k0: nothing passed, finish along stored pointers
        call = CALL_OPT; cq = q0; ct = t0; ck = k0; cforce = true;   // cw.h:196-203 / ucw.h:186-191
      }
      continue;
    }
    if ((uint32_t)k == n_as) {                              // as.push_back(curr)
      if (n_as >= a.ali_cap) { status = ALN_E_OVERFLOW; break; }
      if (lane == 0) { st_u(&a.head[n_as], curr_head); st_f(&a.score[n_as], curr_score); }
      dirty = true;
      ++n_as;
    }
    prepend(k, q0, t0);
    set_score(k, r - fg);
    if (lane == 0) st_u(f + 3, (uint32_t)(found + 1));
    dirty = true;
    if (cw) { call = CALL_OPT; cq = fq; ct = ft; ck = k; cforce = false; }      // opt_path(cand,k,false)
    else { call = CALL_BRANCH; cq = fq; ct = ft; ck = k; cforce = false; }      // ucw: branch(cand,k)
  }
  if (lane == 0) { a.out[0] = (int32_t)n_as; a.out[1] = (int32_t)n_nodes; a.out[2] = status; }
}

// unroll selected alignments: one wave per alignment walks the trie (list order = head -> end)
__global__ __launch_bounds__(64) void enum_unroll_kernel(const uint32_t* __restrict__ node_pair, const uint32_t* __restrict__ node_next,
                                                         const uint8_t* __restrict__ node_len,
                                                         const uint32_t* __restrict__ head, const int32_t* __restrict__ sel, int nsel,
                                                         int32_t* __restrict__ out_pairs, int32_t* __restrict__ out_n, int stride) {
  const int s = blockIdx.x;
  if (s >= nsel) return;
  const int n = unroll_alignment(node_pair, node_next, node_len, head[sel[s]], out_pairs + (size_t)s * stride * 2, stride);
  if (threadIdx.x == 0) out_n[s] = n;
}

// ---- batched form (BASELINE config 4): every pair of a group in one launch ----
// one wave per (pair, slot): slot's alignment index comes from sel[]; -1 = empty, 0 = the pair's Optimal alignment
// (taken from the traceback list, which is stored end -> start), otherwise a trie walk.
__global__ __launch_bounds__(64) void enum_unroll_all_kernel(const uint32_t* __restrict__ node_pair, const uint32_t* __restrict__ node_next,
                                                             const uint8_t* __restrict__ node_len,
                                                             const uint32_t* __restrict__ head, size_t node_stride, int n_pools, uint32_t ali_cap,
                                                             const int32_t* __restrict__ sel, int K, const int32_t* __restrict__ pair_list,
                                                             const int32_t* __restrict__ path,
                                                             int path_stride, const PairResult* __restrict__ res,
                                                             int32_t* __restrict__ out_pairs, int32_t* __restrict__ out_n, int stride,
                                                             int out_by_pair) {
  // blockIdx.y = position of the pair inside its group (pools and sel are group-local); gp = its index in the batch.  The outputs
  // are group-local too, unless the group is the whole batch (out_by_pair): then they are laid out in batch order, whatever
  // order the pairs were launched in, and the host takes them with one copy.
  const int p = blockIdx.y, k = blockIdx.x;
  const int gp = pair_list[p];
  const int idx = sel[(size_t)p * K + k];
  const size_t op = out_by_pair ? (size_t)gp : (size_t)p;
  int32_t* o = out_pairs ? out_pairs + (op * K + k) * stride * 2 : nullptr;
  if (idx < 0) { if (threadIdx.x == 0) out_n[op * K + k] = 0; return; }
  if (idx == 0) {
    const int n = res[gp].n_path;
    const int32_t* src = path + (size_t)gp * path_stride * 2;
    if (o) for (int i = threadIdx.x; i < n && i < stride; i += 64) { o[2 * i] = src[2 * (n - 1 - i)]; o[2 * i + 1] = src[2 * (n - 1 - i) + 1]; }
    if (threadIdx.x == 0) out_n[op * K + k] = n;
    return;
  }
  // a slice per pair (one-wave kernels: n_pools = 0) or the pool workgroup p of enumerate_par.hip used (enum_pool_of)
  const size_t nbase = n_pools ? (size_t)enum_pool_of((uint32_t)p, (uint32_t)n_pools) * node_stride : (size_t)p * node_stride;
  const int n = unroll_alignment(node_pair + nbase, node_next + nbase, node_len ? node_len + nbase : nullptr,
                                 head[(size_t)p * ali_cap + idx], o, stride);
  if (threadIdx.x == 0) out_n[op * K + k] = n;
}

// {score, parent slot, t0, candidate} of every slot of every finished set, packed in set order of the launch: one D2H copy
__global__ __launch_bounds__(256) void enum_pack_sets_kernel(const float* __restrict__ score, const uint32_t* __restrict__ slot_info,
                                                            uint32_t ali_cap, const int64_t* __restrict__ off, uint32_t* __restrict__ out) {
  const int g = blockIdx.x;
  const int64_t o = off[g];
  const int n = (int)(off[g + 1] - o);
  for (int k = threadIdx.x; k < n; k += 256) {
    uint32_t* r = out + (size_t)(o + k) * 4;
    r[0] = __float_as_uint(score[(size_t)g * ali_cap + k]);
    if (slot_info) { const uint32_t* si = slot_info + ((size_t)g * ali_cap + k) * 3; r[1] = si[0]; r[2] = si[1]; r[3] = si[2]; }
    else { r[1] = 0u; r[2] = 0u; r[3] = 0u; }
  }
}

}  // namespace aln

// ---------------------------------------------------------------------------------------------------------
// Host: aln_batch_enumerate (one pair) and aln_batch_enumerate_all (every pair of the batch, BASELINE config 4) over one set of
// rules — DESIGN.md 4.6e.
#include <algorithm>
#include <chrono>
#include <thread>
#include <cstdio>
#include <cstring>

using namespace aln;

namespace {
// The error exit of this file, over a local or member `ctx`.  It synchronizes the stream before it returns: what the caller's
// EnumBufs then frees may be in use by a kernel still in flight.
#define ETRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { ctx->last_error = std::string(#expr) + ": " + hipGetErrorString(e_); hipStreamSynchronize(ctx->stream); return ALN_E_HIP; } } while (0)

// Device buffers (and aln_batch_enumerate_all's four timing events) with an owner: freed when it goes out of scope
struct EnumBufs {
  std::vector<void*> owned;
  hipEvent_t evs[4] = {nullptr, nullptr, nullptr, nullptr};
  EnumBufs() = default;
  EnumBufs(const EnumBufs&) = delete;
  ~EnumBufs() { for (void* p : owned) hipFree(p); for (auto ev : evs) if (ev) hipEventDestroy(ev); }
  template <class T>
  hipError_t get(T*& p, size_t count) {
    const hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e == hipSuccess) owned.push_back(p);
    return e;
  }
};

struct SortKey {
  float score; int32_t idx;
  bool operator<(const SortKey& o) const { return score > o.score; }   // alignment.h:104-105 "higher score first"
};
// NOaliParams::user_limit when the caller leaves it 0: the enumerators' own hard-coded / default limits — cw.h:76 (1000000),
// ucw.h:72 (100000), kscw.h:172 via NOaliParams::default_user_limit (noalib.cpp:19-20: 100000).  One rule for both entry points.
uint32_t default_user_limit(const aln_noa* noa) {
  if (noa->user_limit) return noa->user_limit;
  return noa->kind == ALN_ENUM_CW ? 1000000u : 100000u;
}
bool pruned_kind(int kind) { return kind == ALN_ENUM_KSCW || kind == ALN_ENUM_CRCW; }
// CRCW's own parameters (NOaliParams::sort_limit 100, max_overlap 0.30: noalib.cpp:18,21); false: not usable
bool set_cr_params(EnumArgs& a, const aln_noa* noa, int maxT) {
  a.sort_limit = noa->sort_limit ? noa->sort_limit : 100u;
  a.max_overlap = noa->max_overlap;
  a.cr_tpad = (maxT + 7) & ~7;
  return a.sort_limit >= 1 && a.sort_limit <= 512 && a.k_limit >= 1;
}
size_t cr_lds_bytes(const EnumArgs& a) { return (size_t)a.cand_cap * 8 + (size_t)a.sort_limit * 9 * 4; }

// ---- the several-waves-per-pair search (enumerate_par.hip) -------------------------------------------------------------
// LDS of one workgroup: flags + template codes + query codes (16-byte padded) + the 32 x 32 table
size_t par_lds_bytes(int maxQ, int maxT, int waves = 0) {           // + KSCW's candidate arrays: 256 x (sum, index) per wave
  return (size_t)((maxT + 15) & ~15) * 2 + (size_t)((maxQ + 15) & ~15) + 4096 + (size_t)waves * 256 * 8;
}
// waves per pair: context hint "enum_waves" (1 = the one-wave kernel, 2..16), else 16; 0 = not usable
int par_waves(const aln_batch* b, int kind) {
  if (kind != ALN_ENUM_CW && kind != ALN_ENUM_UCW && kind != ALN_ENUM_KSCW) return 0;
  const int h = b->ctx->hints.enum_waves;
  if (h == 1 || par_lds_bytes(b->maxQ, b->maxT, 16) > 58000 || b->maxQ > 65535 || b->maxT > 65535) return 0;
  if (h >= 2) return std::min(h, 16);
  return 16;                      // measured on 1024 config-4 pairs: 16 waves 0.33 s, 8 waves 0.48 s, 4 waves 0.75 s, one wave 4.6 s
}

// ---- what both entries fix before they allocate ------------------------------------------------------------------------
struct EnumSetup {
  bool ks, cr;          // a pruned enumerator (they share the frame layout and the uid array); CRCW
  bool sub, tpos;       // similarities come from residue codes, not from the S plane; gaps depend on the position
  size_t frame_words;   // words of one frame of the one-wave kernels' stack
  bool usable;          // k_limit and CRCW's parameters are in range.  The entries reject a search that is not only after the planes
                        // were made full and the traceback ran (as they always have), so the verdict waits here for them
  EnumArgs a;           // the search's parameters: everything but pools, capacities, flags and outputs
  EvalDev proto;
};
// The argument and state checks both entries share, in the order both apply them behind their own null-pointer checks, and the
// search's parameters from noa and the batch.  Q, T: the largest sequences of the pairs searched; first_slot: the seed's place.
int enum_setup(const aln_batch* b, const aln_noa* noa, const uint8_t* flags, int Q, int T, int first_slot, int flags_stride, EnumSetup& s) {
  if (!b->have_dp || b->have_sub || b->direction != ALN_FWD) return ALN_E_STATE;
  s.ks = pruned_kind(noa->kind);
  s.cr = noa->kind == ALN_ENUM_CRCW;
  if ((noa->kind == ALN_ENUM_CW || s.ks) && !flags) return ALN_E_ARG;
  if (noa->kind != ALN_ENUM_CW && noa->kind != ALN_ENUM_UCW && !s.ks) return ALN_E_ARG;
  EnumArgs& a = s.a;
  a = {};
  a.kind = noa->kind; a.user_limit = default_user_limit(noa); a.delta_ratio = noa->delta_ratio; a.first_slot = first_slot;
  a.k_limit = s.ks ? (noa->k_limit ? noa->k_limit : 16u) : 0u;
  a.cand_cap = (uint32_t)(Q + T);
  a.stack_cap = (uint32_t)(Q + T + 8);
  a.ptr_mode = b->ptr_mode; a.h_mode = b->h_mode;
  a.int_sums = b->ptr_mode != 0;                       // tagged planes exist only for integer tables and gaps with bounded scores
  a.flags_stride = flags_stride;
  s.usable = a.k_limit <= 64u && (!s.cr || set_cr_params(a, noa, T));
  s.frame_words = s.ks ? 8 + 4 * a.k_limit : kFrameWords;
  EvalDev& proto = s.proto;
  proto = {};
  proto.model = b->gapdev.model; proto.align_type = b->gapdev.align_type;
  proto.gi = b->gapdev.gi; proto.ge = b->gapdev.ge;
  proto.sim_kind = (b->sim_kind == ALN_SIM_SUBMATRIX) ? ALN_SIM_SUBMATRIX : ALN_SIM_MATRIX;
  proto.tablef = b->d_tablef;
  proto.tcn = b->d_tcn; proto.deltab = b->d_deltab; proto.deltab_off = b->d_deltab_off; proto.instab = b->d_instab;
  s.sub = b->sim_kind == ALN_SIM_SUBMATRIX;
  s.tpos = b->gapdev.model != ALN_GAP_AFFINE_CONST;
  return ALN_OK;
}

// The one launch of a search: kernel, block and LDS bytes by (cr, ks, pw) — pw: waves per pair of the several-wave kernel, 0: a
// one-wave kernel — over `grid` workgroups, the first of which works on `pair` (or on a.pair_list[0])
void launch_search(const aln_batch* b, const EnumSetup& s, const EnumArgs& a, int pw, int grid, int pair) {
  auto kernel = enumerate_kernel;                      // (the four search kernels share one signature)
  unsigned block = 64; size_t lds = 0;
  if (s.cr) { kernel = enumerate_cr_kernel; lds = cr_lds_bytes(a); }
  else if (pw) { kernel = enumerate_par_kernel; block = 64u * pw; lds = par_lds_bytes(b->maxQ, b->maxT, pw); }
  else if (s.ks) { kernel = enumerate_ks_kernel; lds = (size_t)a.cand_cap * 8; }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, b->ctx->stream, b->d_pairs, pair, s.proto,
                     s.sub ? b->d_qcodes : nullptr, s.sub ? b->d_tcodes : nullptr, s.tpos ? b->d_tgi : nullptr, s.tpos ? b->d_tge : nullptr,
                     b->d_H, b->d_P, s.sub ? nullptr : b->d_S, a);
}

// Block maxima of pairs [pair0, pair0 + np) for the pruned candidate scan (constant affine gaps, sequences up to 4096): fills
// a.rowmax / a.colmax (one buffer of bufs, the columns' part 256-byte aligned behind the rows') or leaves them null when the
// model does not qualify or the arrays would not pay.
int make_blockmax(aln_batch* b, EnumArgs& a, int pair0, int np, EnumBufs& bufs) {
  if (b->gapdev.model != ALN_GAP_AFFINE_CONST || b->maxQ > 4096 || b->maxT > 4096 || !(b->gapdev.gi >= 0.f) || !(b->gapdev.ge >= 0.f)) return ALN_OK;
  a.bm_rows = b->maxQ; a.bm_cols = b->maxT; a.nbt = (b->maxT + 63) / 64; a.nbq = (b->maxQ + 63) / 64; a.bm_pair0 = pair0;
  const size_t nr = (size_t)np * a.bm_rows * a.nbt, nc = (size_t)np * a.bm_cols * a.nbq;
  if ((nr + nc) * 4 > ((size_t)8 << 30)) return ALN_OK;
  aln_ctx* ctx = b->ctx;
  const size_t nr_pad = (nr + 63) & ~(size_t)63;
  float* bm = nullptr;
  if (bufs.get(bm, nr_pad + nc) != hipSuccess) {
    (void)hipGetLastError();
    return ALN_OK;                                           // no memory for the shortcut: scan everything
  }
  hipLaunchKernelGGL(enum_blockmax_kernel, dim3(a.nbq, np), dim3(256), 0, ctx->stream, b->d_pairs, (const int32_t*)nullptr, pair0, b->d_H,
                     b->h_mode, bm, bm + nr_pad, a.bm_rows, a.bm_cols, a.nbt, a.nbq, pair0);
  ETRY(hipGetLastError());
  a.rowmax = bm; a.colmax = bm + nr_pad;
  return ALN_OK;
}

// ---- pools ---------------------------------------------------------------------------------------------------------------
// the large pools of aln_batch_enumerate_all live with the batch: a slot of b->enum_scratch grows to the largest request
hipError_t scratch(aln_batch* b, aln_batch::EnumSlot slot, size_t bytes, void** out) {
  aln_batch::Scratch& sc = b->enum_scratch[slot];
  if (sc.bytes < bytes) {
    hipFree(sc.p); sc.p = nullptr; sc.bytes = 0;
    hipError_t e = hipMalloc(&sc.p, bytes);
    if (e != hipSuccess) return e;
    sc.bytes = bytes;
  }
  *out = sc.p;
  return hipSuccess;
}
// ... unless the hint enum_keep_pools is 0: then they are freed when aln_batch_enumerate_all returns, on every exit
struct ScratchRelease {
  aln_batch* b;
  ~ScratchRelease() {
    if (!b->ctx->hints.enum_keep_pools) for (auto& sc : b->enum_scratch) { hipFree(sc.p); sc.p = nullptr; sc.bytes = 0; }
  }
};

// Sizes and allocates the pools of one search of gn pairs, one workgroup per pair, from a.node_cap and a.ali_cap per pair;
// aln_batch_enumerate is gn = 1.  The large pools, an EnumSlot each, are the kept scratch of the batch `kept`, or with
// kept = nullptr owned by bufs like everything else (aln_batch_enumerate: its 48 Mi-node default pool must not stay resident).
// Node pool: a slice per pair for the one-wave kernels; pools handed out in chunks for the several-wave kernel (a pair that
// needs ten times the average takes it from the pairs that need a tenth).  serial_after: a one-wave kernel may search again
// in the same pools (aln_batch_enumerate's kParSerial relaunch), so the stack is there under the several-wave kernel too.
int alloc_pools(aln_ctx* ctx, const EnumSetup& s, EnumArgs& a, int gn, int pw, bool serial_after, EnumBufs& bufs, aln_batch* kept) {
  auto big = [&](aln_batch::EnumSlot slot, size_t bytes, void** p) {
    return kept ? scratch(kept, slot, bytes, p) : bufs.get(*(uint8_t**)p, bytes);
  };
  size_t pool_nodes = (size_t)gn * a.node_cap;
  if (pw) {
    a.n_pools = (uint32_t)((pool_nodes + 0xFFFF0000u - 1) / 0xFFFF0000u);          // 32-bit node indices: < 2^32 nodes per pool
    a.n_chunks = (uint32_t)std::max<size_t>(1, pool_nodes / a.n_pools / kChunkNodes);
    pool_nodes = (size_t)a.n_pools * a.n_chunks * kChunkNodes;
    ETRY(bufs.get(a.chunk_next, a.n_pools));
    ETRY(hipMemsetAsync(a.chunk_next, 0, 4 * (size_t)a.n_pools, ctx->stream));
  }
  const size_t slots = (size_t)gn * a.ali_cap;
  ETRY(big(aln_batch::kEnumNodePair, pool_nodes * 4, (void**)&a.node_pair));
  ETRY(big(aln_batch::kEnumNodeNext, pool_nodes * 4, (void**)&a.node_next));
  if (pw) ETRY(big(aln_batch::kEnumNodeLen, pool_nodes, (void**)&a.node_len));
  ETRY(big(aln_batch::kEnumHead, slots * 4, (void**)&a.head));
  ETRY(big(aln_batch::kEnumScore, slots * 4, (void**)&a.score));
  if (pw) {
    ETRY(big(aln_batch::kEnumTask, slots * kTaskWords * 4, (void**)&a.task));
    ETRY(hipMemsetAsync(a.task, 0, slots * kTaskWords * 4, ctx->stream));          // ready words: ticket + 1, never 0
    ETRY(big(aln_batch::kEnumSlotInfo, slots * 12, (void**)&a.slot_info));
  }
  if (!pw || serial_after) ETRY(bufs.get(a.stack, (size_t)gn * a.stack_cap * s.frame_words));
  if (s.ks) ETRY(bufs.get(a.uid, slots));
  if (s.cr) {
    ETRY(bufs.get(a.cr_ali, (size_t)gn * a.sort_limit * a.cr_tpad));
    ETRY(bufs.get(a.cr_reg, (size_t)gn * a.cr_tpad));
  }
  ETRY(bufs.get(a.out, (size_t)gn * 4));
  return ALN_OK;
}

// ---- the set -----------------------------------------------------------------------------------------------------------
// The reference's set order from the slot tree enumerate_par_kernel recorded (see its header): pre-order, siblings by
// (t0 of the branch node ascending, candidate index ascending).  info = 3 words per slot (parent, t0, candidate), `stride` words
// apart, valid for slots > first; slots <= first keep their places.  old_of_new[k] = slot that holds the set's k-th alignment.
void slot_order(int n_as, int first, const uint32_t* info, int stride, std::vector<int32_t>& old_of_new) {
  old_of_new.resize(n_as);
  for (int k = 0; k <= first && k < n_as; ++k) old_of_new[k] = k;
  if (n_as <= first + 1) return;
  const int m = n_as - first - 1;
  std::vector<std::pair<uint64_t, int32_t>> ch(m);
  for (int k = 0; k < m; ++k) {
    const uint32_t* si = info + (size_t)(first + 1 + k) * stride;
    ch[k].first = ((uint64_t)si[0] << 40) | ((uint64_t)(si[1] & 0xFFFFFu) << 20) | (uint64_t)(si[2] & 0xFFFFFu);
    ch[k].second = first + 1 + k;
  }
  std::sort(ch.begin(), ch.end());
  std::vector<int32_t> beg(n_as + 1, 0);                      // children of slot p: ch[beg[p] .. beg[p+1])
  for (int k = 0; k < m; ++k) ++beg[(ch[k].first >> 40) + 1];
  for (int p = 0; p < n_as; ++p) beg[p + 1] += beg[p];
  std::vector<std::pair<int32_t, int32_t>> st;               // (slot, next child)
  int counter = first;
  old_of_new[counter++] = first;
  st.emplace_back(first, beg[first]);
  while (!st.empty()) {
    auto& top = st.back();
    if (top.second == beg[top.first + 1]) { st.pop_back(); continue; }
    const int32_t c = ch[top.second++].second;
    old_of_new[counter++] = c;
    st.emplace_back(c, beg[c]);
  }
}
// The set behind the several-wave kernel: its order (slot_order), and the scores of the slots from `first` on in that order.
// raw: the slots' score words, raw_stride words apart.
void set_order(int n_as, int first, const uint32_t* info, int info_stride, const uint32_t* raw, int raw_stride,
               std::vector<int32_t>& old_of_new, float* scores) {
  slot_order(n_as, first, info, info_stride, old_of_new);
  for (int k = first; k < n_as; ++k) memcpy(&scores[k], raw + (size_t)old_of_new[k] * raw_stride, 4);
}
// AlignmentSet::sortSet(number_suboptimal) — alignment.h:922-932, same libstdc++ calls on the same order of keys.  keys: what
// the set keeps, in its new order; idx = the place before.
void sort_set(const float* scores, int n_as, int mx, std::vector<SortKey>& keys) {
  keys.resize(n_as);
  for (int k = 0; k < n_as; ++k) { keys[k].score = scores[k]; keys[k].idx = k; }
  if (mx >= n_as) std::sort(keys.begin(), keys.end());
  else if (mx > 0) { std::partial_sort(keys.begin(), keys.begin() + mx, keys.end()); keys.erase(keys.begin() + mx, keys.end()); }
}

// ---- every pair of the batch -------------------------------------------------------------------------------------------
// aln_batch_enumerate_all's search of one group of pairs, one workgroup per pair, each with its own slice of the pools: allocate,
// search, order the sets, unroll and copy out.  pw: waves per pair of the several-wave kernel (cw / ucw / kscw), 0: a one-wave
// kernel.  A pair whose set outgrows user_limit under the several-wave kernel comes back as kParSerial and goes to serial_todo:
// a one-wave kernel searches it again with the same capacities.  A pair whose pools overflowed goes to `again`, unless this is
// the last round.  What the retry loop of the entry does with the two lists is its policy.
struct GroupRun {
  // the call
  aln_batch* b; aln_ctx* ctx; const aln_noa* noa; const EnumSetup& s;
  EnumBufs& call;                                // its events time the search and the unroll kernel
  const uint8_t* d_flags; const std::vector<PairResult>& res;
  int32_t K; int32_t* n_out; float* scores; int32_t* lengths; int32_t* pairs; int32_t pair_stride; int32_t* status;
  uint32_t node_cap, ali_cap;                    // per pair, of the current round
  std::vector<int32_t> again, serial_todo;
  // the group
  const int32_t* ids = nullptr; int gn = 0; bool last_round = false; int pw = 0;
  EnumArgs a = {};
  int32_t* d_list = nullptr;
  std::vector<int32_t> hout, sel, hlens;
  std::vector<char> deferred;                    // 1: searched again, nothing is reported now; 2: failed, nothing to order, lengths still reported
  std::vector<int64_t> off;                      // the sets' slots, packed: pair g's slot k is record off[g] + k
  std::vector<uint32_t> packed;                  // {score, parent, t0, candidate} per slot
  float ms_search = 0.f, ms_unroll = 0.f;

  int alloc(EnumBufs& g) {
    a = s.a;
    a.node_cap = node_cap; a.ali_cap = ali_cap;
    { const int rc = alloc_pools(ctx, s, a, gn, pw, false, g, b); if (rc) return rc; }
    ETRY(g.get(d_list, (size_t)gn));
    ETRY(hipMemcpyAsync(d_list, ids, (size_t)gn * 4, hipMemcpyHostToDevice, ctx->stream));
    a.flags = d_flags; a.pair_list = d_list;
    return ALN_OK;
  }
  int search() {
    ETRY(hipEventRecord(call.evs[0], ctx->stream));
    launch_search(b, s, a, pw, gn, 0);
    ETRY(hipGetLastError());
    ETRY(hipEventRecord(call.evs[1], ctx->stream));
    hout.resize((size_t)gn * 4);
    ETRY(hipMemcpyAsync(hout.data(), a.out, hout.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    ETRY(hipStreamSynchronize(ctx->stream));
    return ALN_OK;
  }
  // per pair: what becomes of it (reported, searched again, failed), then sortSet on (score, index) keys picks the survivors
  int order_sets(EnumBufs& g) {
    sel.assign((size_t)gn * K, -1);
    deferred.assign(gn, 0);
    off.assign(gn + 1, 0);
    for (int gi = 0; gi < gn; ++gi) {
      const int p = ids[gi];
      for (int w = 0; w < 3; ++w) b->enum_usage[(size_t)p * 4 + w] = hout[4 * gi + w];
      b->enum_usage[(size_t)p * 4 + 3] = pw ? hout[4 * gi + 3] : 0;       // tickets of the several-wave kernel's task ring
      status[p] = hout[4 * gi + 2] ? hout[4 * gi + 2] : res[p].status;
      n_out[p] = 0;
      off[gi + 1] = off[gi];
      if (status[p] == kParSerial) { status[p] = 0; serial_todo.push_back(p); deferred[gi] = 1; continue; }
      if (status[p] == ALN_E_OVERFLOW && !last_round &&
          (pw || (uint32_t)hout[4 * gi + 1] >= a.node_cap - 64u || (uint32_t)hout[4 * gi] >= a.ali_cap)) { again.push_back(p); deferred[gi] = 1; continue; }
      if (status[p] != 0) { deferred[gi] = 2; continue; }
      off[gi + 1] = off[gi] + hout[4 * gi];
    }
    // one gather + one copy instead of two small copies per pair: {score, parent, t0, candidate} per slot
    const size_t total_slots = (size_t)off[gn];
    packed.resize(total_slots * 4);
    if (total_slots) {
      uint32_t* d_packed = nullptr; int64_t* d_off = nullptr;
      ETRY(scratch(b, aln_batch::kEnumPacked, total_slots * 16, (void**)&d_packed));
      ETRY(g.get(d_off, (size_t)gn + 1));
      ETRY(hipMemcpyAsync(d_off, off.data(), (size_t)(gn + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
      hipLaunchKernelGGL(enum_pack_sets_kernel, dim3(gn), dim3(256), 0, ctx->stream, a.score, pw ? a.slot_info : (const uint32_t*)nullptr, a.ali_cap, d_off, d_packed);
      ETRY(hipGetLastError());
      ETRY(hipMemcpyAsync(packed.data(), d_packed, total_slots * 16, hipMemcpyDeviceToHost, ctx->stream));
      ETRY(hipStreamSynchronize(ctx->stream));
    }
    // per pair, on host threads: the reference's set order (slot tree), then AlignmentSet::sortSet
    const int mx = noa->number_suboptimal;
    auto work = [&](int tid, int nthreads) {
      std::vector<int32_t> order; std::vector<float> scv; std::vector<SortKey> keys;
      for (int gi = tid; gi < gn; gi += nthreads) {
        if (deferred[gi]) continue;
        const int p = ids[gi];
        const int n_as = hout[4 * gi];
        const uint32_t* rec = packed.data() + (size_t)off[gi] * 4;
        scv.resize(n_as);
        if (pw) set_order(n_as, 1, rec + 1, 4, rec, 4, order, scv.data());
        else for (int k = 1; k < n_as; ++k) memcpy(&scv[k], rec + 4 * (size_t)k, 4);
        scv[0] = b->islocal ? res[p].best : res[p].corner;
        sort_set(scv.data(), n_as, mx, keys);
        int keep = (int)keys.size();
        if (keep > K) { status[p] = ALN_E_OVERFLOW; keep = K; }     // the caller's K slots are too few for this set
        n_out[p] = keep;
        for (int k = 0; k < keep; ++k) {
          sel[(size_t)gi * K + k] = pw ? order[keys[k].idx] : keys[k].idx;
          scores[(size_t)p * K + k] = keys[k].score;
        }
      }
    };
    const int nthreads = (int)std::max(1u, std::min({std::thread::hardware_concurrency(), 16u, (unsigned)((total_slots >> 14) + 1)}));
    if (nthreads == 1) work(0, 1);
    else {
      std::vector<std::thread> th;
      for (int t = 0; t < nthreads; ++t) th.emplace_back(work, t, nthreads);
      for (auto& t : th) t.join();
    }
    return ALN_OK;
  }
  // unroll every survivor on the device
  int unroll(EnumBufs& g) {
    const int n = b->n_pairs;
    int32_t *d_sel = nullptr, *d_lens = nullptr, *d_lists = nullptr;
    ETRY(g.get(d_sel, sel.size()));
    ETRY(g.get(d_lens, sel.size()));
    if (pairs) ETRY(scratch(b, aln_batch::kEnumLists, sel.size() * (size_t)pair_stride * 8, (void**)&d_lists));
    ETRY(hipMemcpyAsync(d_sel, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    ETRY(hipEventRecord(call.evs[2], ctx->stream));
    hipLaunchKernelGGL(enum_unroll_all_kernel, dim3(K, gn), dim3(64), 0, ctx->stream, a.node_pair, a.node_next,
                       pw ? a.node_len : (const uint8_t*)nullptr, a.head,
                       pw ? (size_t)a.n_chunks * kChunkNodes : (size_t)a.node_cap, pw ? (int)a.n_pools : 0, a.ali_cap,
                       d_sel, K, d_list, b->d_path, b->path_stride, b->d_res, d_lists, d_lens, pairs ? pair_stride : (1 << 30),
                       gn == n ? 1 : 0);
    ETRY(hipGetLastError());
    ETRY(hipEventRecord(call.evs[3], ctx->stream));
    hlens.resize(sel.size());
    ETRY(hipMemcpyAsync(hlens.data(), d_lens, sel.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    const bool in_place = pairs && gn == n;             // every pair of the batch: laid out in batch order by the kernel, one copy
    if (in_place) ETRY(hipMemcpyAsync(pairs, d_lists, sel.size() * (size_t)pair_stride * 8, hipMemcpyDeviceToHost, ctx->stream));
    ETRY(hipStreamSynchronize(ctx->stream));
    for (int gi = 0; gi < gn; ++gi) {
      const int p = ids[gi];
      if (deferred[gi] == 1) continue;
      for (int k = 0; k < K; ++k) lengths[(size_t)p * K + k] = hlens[(size_t)(gn == n ? p : gi) * K + k];
      if (pairs && !in_place)
        ETRY(hipMemcpy(pairs + (size_t)p * K * pair_stride * 2, d_lists + (size_t)gi * K * pair_stride * 2, (size_t)K * pair_stride * 8,
                       hipMemcpyDeviceToHost));
    }
    ETRY(hipEventElapsedTime(&ms_search, call.evs[0], call.evs[1]));
    ETRY(hipEventElapsedTime(&ms_unroll, call.evs[2], call.evs[3]));
    b->enum_search_ms += ms_search; b->enum_unroll_ms += ms_unroll;
    return ALN_OK;
  }
  int run(const int32_t* ids_, int gn_, bool last_round_, int pw_) {
    ids = ids_; gn = gn_; last_round = last_round_; pw = pw_;
    auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    EnumBufs g;                                  // the group's own buffers (the large pools are the batch's: b->enum_scratch)
    double tm[5];                                // enum_debug: host seconds of the group's phases
    int rc;
    tm[0] = now();
    if ((rc = alloc(g)) != ALN_OK) return rc;
    tm[1] = now();
    if ((rc = search()) != ALN_OK) return rc;
    tm[2] = now();
    if ((rc = order_sets(g)) != ALN_OK) return rc;
    tm[3] = now();
    if ((rc = unroll(g)) != ALN_OK) return rc;
    tm[4] = now();
    if (ctx->hints.enum_debug) {
      uint32_t used = 0;
      if (pw) hipMemcpy(&used, a.chunk_next, 4, hipMemcpyDeviceToHost);      // (pool 0)
      long long nodes = 0, slots = 0; int novf = 0;
      for (int gi = 0; gi < gn; ++gi) { nodes += (uint32_t)hout[4 * gi + 1]; slots += hout[4 * gi]; novf += hout[4 * gi + 2] != 0; }
      fprintf(stderr, "[enumerate_all] group of %d pairs, %d waves/pair, node_cap %u ali_cap %u: search %.2f ms, unroll %.2f ms, again %zu, serial %zu; chunks %u of %u, nodes %lld, slots %lld, failed %d\n",
              gn, pw, a.node_cap, a.ali_cap, ms_search, ms_unroll, again.size(), serial_todo.size(), used, a.n_chunks, nodes, slots, novf);
      fprintf(stderr, "[enumerate_all]   host seconds: alloc %.3f, search + sync %.3f, sets %.3f, unroll + copy %.3f\n", tm[1] - tm[0], tm[2] - tm[1],
              tm[3] - tm[2], tm[4] - tm[3]);
    }
    return ALN_OK;
  }
};
}  // namespace

extern "C" int aln_batch_enumerate(aln_batch* b, int32_t pair, const aln_noa* noa, const uint8_t* flags, aln_alignment* out,
                                   int32_t max_alignments, int32_t* pairs, int64_t pairs_capacity, int32_t* n_out) {
  if (!b || !noa || !out || !pairs || !n_out || pair < 0 || pair >= b->n_pairs) return ALN_E_ARG;
  const PairDesc& d = b->h_pairs[pair];
  // n_existing < 0: the set starts with the pair's Optimal alignment, like the drivers (aa_ali.cpp:83);
  // otherwise the caller's set already holds n_existing alignments whose scores take part in sortSet.
  const bool seed_opt = noa->n_existing < 0;
  const int n_ex = seed_opt ? 1 : noa->n_existing;
  EnumSetup s;
  { const int rc = enum_setup(b, noa, flags, d.Q, d.T, n_ex, 0, s); if (rc) return rc; }
  aln_ctx* ctx = b->ctx;
  ALN_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  { const int rc = ensure_full(b); if (rc) return rc; }      // the searches read scores and plain pointer words
  if (!seed_opt && n_ex > 0 && !noa->existing_scores) return ALN_E_ARG;
  std::vector<PairResult> res(b->n_pairs);
  std::vector<int32_t> optpath((size_t)b->path_stride * 2);
  if (seed_opt) {
    int rc = launch_traceback(b, false);
    if (rc) return rc;
    ETRY(hipMemcpyAsync(res.data(), b->d_res, sizeof(PairResult) * b->n_pairs, hipMemcpyDeviceToHost, ctx->stream));
    ETRY(hipMemcpyAsync(optpath.data(), b->d_path + (size_t)pair * b->path_stride * 2, optpath.size() * 4,
                        hipMemcpyDeviceToHost, ctx->stream));
    ETRY(hipStreamSynchronize(ctx->stream));
    if (res[pair].status != 0) return res[pair].status;
  }
  if (!s.usable) return ALN_E_ARG;

  const int stride = b->path_stride;
  std::vector<SortKey> keys;                            // the kept set; idx < n_ex: a slot that was there before the search
  std::vector<int32_t> uids, lists, lens;              // uid per slot; the kept alignments the search created, in set order
  {
    EnumBufs bufs;                                      // every device buffer of the search: freed before the outputs are assembled
    EnumArgs a = s.a;
    a.ali_cap = a.user_limit + 65536u + (uint32_t)n_ex;
    a.node_cap = 48u << 20;
    if (ctx->hints.enum_node_cap > 0) a.node_cap = (uint32_t)ctx->hints.enum_node_cap;
    const int pw = par_waves(b, noa->kind);            // cw / ucw / kscw: several waves search the pair (enumerate_par.hip)
    // its node pool comes in chunks, and the kParSerial relaunch slices the same pool by node_cap: node_cap itself is whole chunks
    if (pw) a.node_cap = std::max(a.node_cap, kChunkNodes) / kChunkNodes * kChunkNodes;
    { const int rc = alloc_pools(ctx, s, a, 1, pw, true, bufs, nullptr); if (rc) return rc; }
    uint8_t* d_flags = nullptr;
    ETRY(bufs.get(d_flags, (size_t)d.T));
    if (flags) ETRY(hipMemcpyAsync(d_flags, flags, (size_t)d.T, hipMemcpyHostToDevice, ctx->stream));
    else ETRY(hipMemsetAsync(d_flags, 1, (size_t)d.T, ctx->stream));
    a.flags = d_flags;
    if (pw || noa->kind == ALN_ENUM_KSCW) { const int rc = make_blockmax(b, a, pair, 1, bufs); if (rc) return rc; }

    int32_t hout[4] = {0, 0, 0, 0};
    auto search = [&](int waves) -> int {
      launch_search(b, s, a, waves, 1, pair);
      ETRY(hipGetLastError());
      ETRY(hipMemcpyAsync(hout, a.out, 12, hipMemcpyDeviceToHost, ctx->stream));
      ETRY(hipStreamSynchronize(ctx->stream));
      return ALN_OK;
    };
    { const int rc = search(pw); if (rc) return rc; }
    bool used_par = pw != 0;
    if (used_par && hout[2] == kParSerial) {            // the set outgrows user_limit: the serial order decides what is cut
      used_par = false;
      const int rc = search(0);
      if (rc) return rc;
    }
    if (hout[2] != 0) return hout[2];
    const int n_as = hout[0];
    std::vector<float> scores(n_as);
    std::vector<int32_t> old_of_new;                    // set position -> slot (identity after the one-wave kernel)
    if (used_par) {
      std::vector<uint32_t> info((size_t)n_as * 3), raw(n_as);
      ETRY(hipMemcpyAsync(info.data(), a.slot_info, info.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
      ETRY(hipMemcpyAsync(raw.data() + n_ex, a.score + n_ex, (size_t)(n_as - n_ex) * 4, hipMemcpyDeviceToHost, ctx->stream));
      ETRY(hipStreamSynchronize(ctx->stream));
      set_order(n_as, n_ex, info.data(), 3, raw.data(), 1, old_of_new, scores.data());
    } else {
      ETRY(hipMemcpyAsync(scores.data() + n_ex, a.score + n_ex, (size_t)(n_as - n_ex) * 4, hipMemcpyDeviceToHost, ctx->stream));
      ETRY(hipStreamSynchronize(ctx->stream));
    }
    if (seed_opt) scores[0] = b->islocal ? res[pair].best : res[pair].corner;
    else for (int k = 0; k < n_ex; ++k) scores[k] = noa->existing_scores[k];
    if (s.ks) uids.assign(n_as, -1);
    if (s.ks && used_par) {                             // uid = the alignment's place at creation (kscw.h:262), the seed's is 1 (:121)
      for (int k = n_ex; k < n_as; ++k) uids[k] = k == n_ex ? 1 : k;
    } else if (s.ks) {
      ETRY(hipMemcpy(uids.data() + n_ex, a.uid + n_ex, (size_t)(n_as - n_ex) * 4, hipMemcpyDeviceToHost));
    }
    sort_set(scores.data(), n_as, noa->number_suboptimal, keys);
    *n_out = (int)keys.size();
    if (*n_out > max_alignments) return ALN_E_OVERFLOW;   // too few records: the caller retries with *n_out of them

    // unroll the survivors on the device
    std::vector<int32_t> sel;
    for (const SortKey& key : keys) if (key.idx >= n_ex) sel.push_back(used_par ? old_of_new[key.idx] : key.idx);
    lists.resize((size_t)std::max<size_t>(sel.size(), 1) * stride * 2);
    lens.resize(std::max<size_t>(sel.size(), 1));
    if (!sel.empty()) {
      int32_t *d_sel = nullptr, *d_lists = nullptr, *d_lens = nullptr;
      ETRY(bufs.get(d_sel, sel.size()));
      ETRY(bufs.get(d_lists, lists.size()));
      ETRY(bufs.get(d_lens, sel.size()));
      ETRY(hipMemcpyAsync(d_sel, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, ctx->stream));
      hipLaunchKernelGGL(enum_unroll_kernel, dim3((unsigned)sel.size()), dim3(64), 0, ctx->stream, a.node_pair, a.node_next,
                         used_par ? a.node_len : (const uint8_t*)nullptr, a.head,
                         d_sel, (int)sel.size(), d_lists, d_lens, stride);
      ETRY(hipGetLastError());
      ETRY(hipMemcpyAsync(lists.data(), d_lists, lists.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
      ETRY(hipMemcpyAsync(lens.data(), d_lens, sel.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
      ETRY(hipStreamSynchronize(ctx->stream));
    }
  }
  // assemble outputs in set order
  const int n_keep = (int)keys.size();
  const std::string qs(b->q_res.data() + d.q_off, d.Q), ts(b->t_res.data() + d.t_off, d.T);
  int64_t off = 0;
  size_t si = 0;
  for (int k = 0; k < n_keep; ++k) {
    const int idx = keys[k].idx;
    const int32_t* src; int len;
    std::vector<int32_t> tmp;
    if (idx < n_ex && !seed_opt) {        // one of the caller's own alignments: only its new position is reported
      out[k].score = keys[k].score; out[k].identity = 0.f; out[k].uid = -1; out[k].n_pairs = -1; out[k].pair_off = idx;
      continue;
    }
    if (idx < n_ex) {
      len = res[pair].n_path;
      tmp.resize((size_t)len * 2);
      for (int i = 0; i < len; ++i) { tmp[2 * i] = optpath[2 * (len - 1 - i)]; tmp[2 * i + 1] = optpath[2 * (len - 1 - i) + 1]; }
      src = tmp.data();
    } else {
      len = lens[si];
      src = lists.data() + si * (size_t)stride * 2;
      ++si;
      if (len < 0) return ALN_E_OVERFLOW;
    }
    if (off + len > pairs_capacity) return ALN_E_OVERFLOW;
    memcpy(pairs + 2 * off, src, (size_t)len * 8);
    out[k].score = keys[k].score;
    out[k].uid = (idx < n_ex) ? -1 : s.ks ? uids[idx] : (noa->kind == ALN_ENUM_CW ? 0 : -1);   // cw.h:83 sets uid 0 on its seed; copies inherit it
    out[k].n_pairs = len;
    out[k].pair_off = off;
    out[k].identity = aln_identity(qs.c_str(), d.Q, ts.c_str(), d.T, pairs + 2 * off, len);
    off += len;
  }
  return ALN_OK;
}

extern "C" int aln_batch_enumerate_all(aln_batch* b, const aln_noa* noa, const uint8_t* flags, int32_t flags_stride,
                                       uint32_t node_cap_per_pair, uint32_t ali_cap_per_pair, int32_t K, int32_t* n_out, float* scores,
                                       int32_t* lengths, int32_t* pairs, int32_t pair_stride, int32_t* status) {
  if (!b || !noa || !n_out || !scores || !lengths || !status || K <= 0) return ALN_E_ARG;
  EnumSetup s;
  int rc = enum_setup(b, noa, flags, b->maxQ, b->maxT, 1, flags ? flags_stride : 0, s);
  if (rc) return rc;
  if (pairs && pair_stride < b->path_stride) return ALN_E_ARG;
  aln_ctx* ctx = b->ctx;
  ScratchRelease release{b};
  ALN_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int n = b->n_pairs;
  if (n == 0) return ALN_OK;
  rc = ensure_full(b);                                        // the searches read scores and plain pointer words
  if (rc) return rc;
  // every set starts with the pair's Optimal alignment (aa_ali.cpp:83)
  rc = launch_traceback(b, false);
  if (rc) return rc;
  if (!s.usable) return ALN_E_ARG;

  EnumBufs bufs;
  uint8_t* d_flags = nullptr;
  const size_t fl_bytes = flags ? (flags_stride ? (size_t)n * flags_stride : (size_t)b->maxT) : (size_t)b->maxT;
  ETRY(bufs.get(d_flags, fl_bytes));
  if (flags) ETRY(hipMemcpyAsync(d_flags, flags, fl_bytes, hipMemcpyHostToDevice, ctx->stream));
  else ETRY(hipMemsetAsync(d_flags, 1, fl_bytes, ctx->stream));
  for (auto& ev : bufs.evs) ETRY(hipEventCreate(&ev));
  std::vector<PairResult> res(n);
  ETRY(hipMemcpyAsync(res.data(), b->d_res, sizeof(PairResult) * n, hipMemcpyDeviceToHost, ctx->stream));
  ETRY(hipStreamSynchronize(ctx->stream));
  // what the previous search of this batch used, if there was one: the pairs are launched heaviest first (below)
  std::vector<int32_t> prior_nodes;
  if ((int)b->enum_usage.size() == 4 * n && ctx->hints.enum_heavy_first) {
    prior_nodes.resize(n);
    for (int p = 0; p < n; ++p) prior_nodes[p] = b->enum_usage[(size_t)p * 4 + 1];
  }
  b->enum_usage.assign((size_t)n * 4, 0);
  b->enum_search_ms = b->enum_unroll_ms = 0.f;
  const int pw0 = par_waves(b, noa->kind);
  if (pw0 || noa->kind == ALN_ENUM_KSCW) {   // block maxima of every pair's score plane, once (the pruned scans of enumerate_par.hip / enumerate_ks.hip)
    rc = make_blockmax(b, s.a, 0, n, bufs);
    if (rc) return rc;
  }
  for (int p = 0; p < n; ++p) { status[p] = 0; n_out[p] = 0; }

  // The search runs for GROUPS of pairs, one workgroup per pair, each with its own slice of the pools.  Round 0 is every pair
  // with the caller's capacities.  A near-optimal search can need anything between nothing (an unrelated pair) and tens of
  // millions of trie nodes (a 2000-residue homolog at DELTA_RATIO 0.01: 2-21 M), so pairs whose node or alignment pool
  // overflowed are searched again, in groups sized to a device-memory budget, with four times the capacity — up to
  // enum_pool_retries times (context hint, default 2: 16 x the caller's capacities).
  const size_t kPoolBudget = (size_t)48 << 30;                       // bytes of pools of one group
  std::vector<int32_t> todo((size_t)n);
  for (int p = 0; p < n; ++p) todo[p] = p;
  // Workgroup g of a launch searches pair todo[g], and workgroups start in index order as residency frees up.  A search's length is
  // unknown beforehand (nothing, or 27 M trie nodes), and the longest pair bounds a launch — unless it starts first.  When this
  // batch has been searched before (refinement rounds, a sweep over DELTA_RATIO, bench.py's second call), the pairs go in the
  // order of what they used then, heaviest first; results are stored per pair and do not depend on the order.
  if (!prior_nodes.empty())
    std::stable_sort(todo.begin(), todo.end(), [&](int32_t x, int32_t y) { return prior_nodes[x] > prior_nodes[y]; });
  else if (ctx->hints.enum_heavy_first) {
    // no history yet: the alignment's score is the cheapest hint there is — the threshold window (1 - DELTA_RATIO) * score widens
    // with it, and related sequences (long, high-scoring paths) are the ones that branch
    auto key = [&](int32_t p) { return b->islocal ? res[p].best : res[p].corner; };
    std::stable_sort(todo.begin(), todo.end(), [&](int32_t x, int32_t y) { return key(x) > key(y); });
  }
  GroupRun g{b, ctx, noa, s, bufs, d_flags, res, K, n_out, scores, lengths, pairs, pair_stride, status,
             node_cap_per_pair ? node_cap_per_pair : (1u << 20), ali_cap_per_pair ? ali_cap_per_pair : 65536u};
  const int max_round = std::max(0, std::min(ctx->hints.enum_pool_retries, 3));
  // The alignment pool never has to be larger than what the reference's own brake allows: once the set is larger than user_limit every
  // branch is forced down the optimal path (cw.h:127-140), and only the candidates of the frames still on the stack are added —
  // fewer than (Q + T) per frame.  A pair that overflowed its alignment slots is therefore retried until its pool has that size
  // (beyond the enum_pool_retries rounds if need be), and then returns the user_limit-truncated set instead of ALN_E_OVERFLOW.
  const uint64_t limit_cap64 = (uint64_t)s.a.user_limit + 65536ull + (uint64_t)(b->maxQ + b->maxT) * 16ull;
  const uint32_t limit_cap = (uint32_t)std::min<uint64_t>(limit_cap64, 0x7FFFFFFFull);
  for (int round = 0; !todo.empty(); ++round) {
    if (g.ali_cap > limit_cap) g.ali_cap = limit_cap;
    // the last round: the retries are used up and the alignment pool has reached the size user_limit bounds
    const bool final_round = round >= max_round && (g.ali_cap >= limit_cap || round >= max_round + 12);
    g.again.clear(); g.serial_todo.clear();
    for (int pass = 0; pass < 2; ++pass) {                // pass 1: the pairs pass 0's several-wave search handed back
      const std::vector<int32_t>& list = pass == 0 ? todo : g.serial_todo;
      if (list.empty()) continue;
      const std::vector<int32_t> ids_all(list);          // (a group appends to serial_todo)
      const int pw = pass == 0 ? pw0 : 0;
      const size_t per_pair = (size_t)g.node_cap * 8 + (size_t)g.ali_cap * (s.ks ? 12 : 8) +
                              (pw ? (size_t)g.ali_cap * (kTaskWords * 4 + 12) : (size_t)s.a.stack_cap * s.frame_words * 4) +
                              (pairs ? (size_t)K * pair_stride * 8 : 0) + (s.cr ? (size_t)s.a.sort_limit * s.a.cr_tpad * 2 + (size_t)s.a.cr_tpad * 4 : 0);
      size_t gmax = std::max<size_t>(1, kPoolBudget / per_pair);
      if (round == 0 && pass == 0) gmax = ids_all.size();               // the caller sized round 0
      gmax = (ids_all.size() + (ids_all.size() + gmax - 1) / gmax - 1) / ((ids_all.size() + gmax - 1) / gmax);   // groups of equal size
      for (size_t g0 = 0; g0 < ids_all.size(); g0 += gmax) {
        rc = g.run(ids_all.data() + g0, (int)std::min(gmax, ids_all.size() - g0), final_round, pw);
        if (rc != ALN_OK) return rc;
      }
    }
    todo.swap(g.again);
    if (final_round) break;
    if (g.node_cap <= (1u << 29)) g.node_cap *= 4;
    if (g.ali_cap <= (1u << 22)) g.ali_cap *= 4;
  }
  int worst = ALN_OK;
  for (int p = 0; p < n; ++p) if (status[p] != 0 && worst == ALN_OK) worst = status[p];
  for (int p = 0; p < n; ++p) if (status[p] == ALN_E_OVERFLOW) worst = ALN_E_OVERFLOW;
  return worst;
}
#undef ETRY

extern "C" int aln_batch_last_enum_usage(aln_batch* b, int32_t* alignments, int32_t* nodes) {
  if (!b) return ALN_E_ARG;
  if ((int)b->enum_usage.size() != 4 * b->n_pairs) return ALN_E_STATE;
  for (int p = 0; p < b->n_pairs; ++p) {
    if (alignments) alignments[p] = b->enum_usage[4 * p];
    if (nodes) nodes[p] = b->enum_usage[4 * p + 1];
  }
  return ALN_OK;
}

extern "C" int aln_batch_last_enum_tasks(aln_batch* b, int32_t* tasks) {
  if (!b || !tasks) return ALN_E_ARG;
  if ((int)b->enum_usage.size() != 4 * b->n_pairs) return ALN_E_STATE;
  for (int p = 0; p < b->n_pairs; ++p) tasks[p] = b->enum_usage[4 * p + 3];
  return ALN_OK;
}

extern "C" int aln_batch_last_enum_ms(aln_batch* b, float* search_ms, float* unroll_ms) {
  if (!b) return ALN_E_ARG;
  if (search_ms) *search_ms = b->enum_search_ms;
  if (unroll_ms) *unroll_ms = b->enum_unroll_ms;
  return ALN_OK;
}
