/*
 * aln_hip.h — C ABI of the MI355X (gfx950) alignment engine, libalnhip.so.
 *
 * The reference (christang/alignment-algos) has no ABI boundary: its hot path is the header
 * template DPMatrix<S1,S2,Etype> driven by CRTP Evaluator plugins (evaluator.h:20-97) and
 * walked by Enumerator classes (enumerator.h:20-25).  This header is the boundary a
 * maintainer binds instead (INTEGRATION.md shows the C++ shim): each entry point names the
 * reference interface it replaces.  Plain pointers and sizes only; the caller owns every host
 * buffer, the library owns device memory inside aln_ctx / aln_batch.  Calls on one ctx are
 * serialised by the caller; different ctx objects may be used from different threads.
 *
 * Index conventions are the reference's: a sequence includes its '^' head and '$' tail
 * sentinels (sequence.cpp:15-16, fastaio.h:126,137), Q = query size, T = template size,
 * matrices are Q x T row-major, DPCell::null is -1 (dpmatrix.cpp:15).
 *
 * Return codes: 0 = ok; negative values mirror the reference's throw sites so that a C++
 * wrapper can rethrow the same std::string (aln_error_string()).
 */
#ifndef ALN_HIP_H
#define ALN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- enums (values equal the reference's) ------------------------------------------- */
enum aln_align_t {            /* alib.h:20-26 */
  ALN_GLOBAL_LOCAL = 0, ALN_GLOBAL = 1, ALN_LOCAL_GLOBAL = 2, ALN_LOCAL = 3, ALN_SEMI_LOCAL = 4
};
enum aln_direction_t { ALN_FWD = 1, ALN_REV = 2 };   /* dpmatrix.h:23-26 */

enum aln_gap_model {
  ALN_GAP_AFFINE_CONST = 0,     /* AASubstitutionEval::deletion/insertion, aasubalib.h:27-77 */
  ALN_GAP_AFFINE_TPOS_MIN = 1,  /* Hmap2Eval / HMAPaliEval, hmap2_eval.h:41-95 (min of the two template positions) */
  ALN_GAP_DEL_TABLE_INS_TPOS = 2, /* Gn2Eval, gn2_eval.h:100-165: deletion(t1,t2) is a per-template table (vv_gi/vv_ge/vv_cd + the
                                   8100 distance rule, materialised by the caller), insertion = (gi[t1] + ge[t1]*(di-2)) + cn[t1] */
  ALN_GAP_TABLES = 3            /* any Evaluator whose deletion() depends on (t1,t2) and whose insertion() depends on (t1, q2-q1)
                                   away from the query ends: both functions materialised by the caller (aln_lowering.h does it
                                   for an arbitrary evaluator.h plugin; covers GnoaliEval, gnoalib.h:90-185) */
};

enum aln_sim_kind {
  ALN_SIM_SUBMATRIX = 0,        /* residue codes + substitution table, aasubalib.h:17-25 + submatrix.h:36-38 */
  ALN_SIM_MATRIX = 1,           /* caller-materialised SimilarityMatrix planes (any Evaluator::similarity + post_process) */
  ALN_SIM_HMAP2 = 2             /* Hmap2Eval::similarity + post_process computed on the device, hmap2_eval.h:27-39,98-101 */
};

enum aln_dp_algo {
  ALN_DP_AUTO = 0,              /* O(n^2) running-max kernel when every value is a small integer, else exact */
  ALN_DP_EXACT = 1,             /* exact-order O(n^3) kernel: literal dpmatrix.h:447-486 arithmetic */
  ALN_DP_FAST = 2               /* force the O(n^2) kernel; ALN_E_NOT_INTEGRAL if the proof fails */
};

enum aln_enum_kind {
  ALN_ENUM_CW = 0,              /* ConstrainedNearOptimal, cw.h:68-284 */
  ALN_ENUM_UCW = 1,             /* UnconstrainedNearOptimal, ucw.h:64-236 */
  ALN_ENUM_KSCW = 2,            /* KSConstrainedNearOptimal, kscw.h:109-351 (parity unpinned: the reference header does not
                                   compile on LP64) */
  ALN_ENUM_CRCW = 3             /* CRConstrainedNearOptimal, crcw.h:134-594 (parity unpinned, same reason) */
};

enum aln_status {
  ALN_OK = 0,
  ALN_E_BOUNDS = -1,            /* "Illegal bounds building DPM"   dpmatrix.h:361,544,699,885 */
  ALN_E_GAPSTYLE = -2,          /* "Illegal gap style"             aasubalib.h:46,72 */
  ALN_E_STARTPAIR = -3,         /* "Illegal alignment start pair"  optimal.h:74 */
  ALN_E_RESIDUE = -4,           /* residue outside the substitution alphabet (UB in submatrix.h:36-38) */
  ALN_E_ARG = -5,               /* bad argument */
  ALN_E_HIP = -6,               /* HIP runtime error, see aln_last_error() */
  ALN_E_NOMEM = -7,
  ALN_E_TOO_LONG = -8,          /* sequence longer than this build's kernels handle */
  ALN_E_NOT_INTEGRAL = -9,      /* ALN_DP_FAST requested but scores/gaps are not small integers */
  ALN_E_STATE = -10,            /* call order: dp before optimal/enumerate/get_cells */
  ALN_E_OVERFLOW = -11          /* an output buffer or the enumeration pool is too small */
};

typedef struct aln_ctx aln_ctx;
typedef struct aln_batch aln_batch;

/* ---- plain descriptors ---------------------------------------------------------------- */

/* A pool of sequences; replaces Sequence<elem_t>/AASequence (sequence.h:41-64, aa_seq.h:10-25).
 * Sequence s is residues[offsets[s] .. offsets[s+1]) and INCLUDES '^' and '$'. */
typedef struct {
  int32_t n_seqs;
  const int64_t* offsets;       /* n_seqs + 1 */
  const char* residues;         /* one-letter codes (SequenceElem::olc) */
} aln_seqs;

/* SubstitutionMatrix / BlosumMatrix (submatrix.h:19-48): n x n row-major over `alphabet`. */
typedef struct {
  int32_t n;                    /* <= 30 */
  const char* alphabet;
  const float* table;
} aln_submatrix;

/* Per-position profile records for Hmap2Eval (HMAPElem, hmapalib_seq.h:28-99), one per residue of
 * the pool, sentinels included: aa[20] (aa_profile), sse[3] (sse_values), conf (sse_confid). */
typedef struct {
  const float* aa;              /* total_residues x 20 */
  const float* sse;             /* total_residues x 3  */
  const float* conf;            /* total_residues      */
} aln_profiles;

/* Gap model + AliParams (alib.h:28-46). */
typedef struct {
  int32_t model;                /* aln_gap_model */
  int32_t align_type;           /* aln_align_t */
  float gap_init, gap_extn;     /* AFFINE_CONST: AliParams::gap_init_penalty / gap_extn_penalty */
  const float* t_gap_init;      /* AFFINE_TPOS_MIN: per residue of the TEMPLATE pool (HMAPElem::gap_init()) */
  const float* t_gap_extn;
  int32_t dp_local;             /* the DPMatrix constructor's own `type == local` (dpmatrix.h:155) when it differs from the
                                   evaluator's align_type: 0 = same as align_type, 1 = not local, 2 = local */
  /* DEL_TABLE_INS_TPOS only.  t_gap_init / t_gap_extn / t_gap_cn are Gn2Eval's v_gi / v_ge / v_cn per residue of the TEMPLATE
   * pool (gn2_eval.cpp:113-130).  del_table: template sequence s (T residues) owns T*T floats at del_table[del_table_off[s]],
   * entry [t1*T + t2] = exactly what Evaluator::deletion(q,t,.,.,t1,t2) returns for t1 < t2 (end rules included). */
  const float* t_gap_cn;
  const float* del_table;       /* DEL_TABLE_INS_TPOS and TABLES */
  const int64_t* del_table_off; /* n template sequences */
  /* TABLES only: pair p (Q x T) owns three T x Q planes at ins_tables[ins_table_off[p]]: [0][t1*Q + d] = insertion(q1,q1+d,t1,t1+1)
   * for interior q1 and q1+d; [1][t1*Q + q2] = insertion(0,q2,t1,t1+1); [2][t1*Q + q1] = insertion(q1,Q-1,t1,t1+1).  No
   * end-gap rule is applied by the library in this model: the tables are the evaluator's own values. */
  const float* ins_tables;
  const int64_t* ins_table_off; /* n pairs */
} aln_gap;

/* Similarity source. */
typedef struct {
  int32_t kind;                 /* aln_sim_kind */
  aln_submatrix sub;            /* ALN_SIM_SUBMATRIX */
  const float* planes;          /* ALN_SIM_MATRIX: pair p's Q x T row-major plane starts at planes[plane_off[p]] */
  const int64_t* plane_off;
  aln_profiles q_prof, t_prof;  /* ALN_SIM_HMAP2 */
  float alpha;                  /* HMAPaliParams::alpha   (hmap_eval.cpp:4)  */
  float zero_shift;             /* HMAPaliParams::zero_shift (hmap_eval.cpp:7) */
  int32_t normalize;            /* run post_process (z-normalise + shift) */
} aln_sim;

/* NOaliParams subset used by cw.h / ucw.h (noalib.h:18-45). */
typedef struct {
  int32_t kind;                 /* aln_enum_kind */
  int32_t number_suboptimal;    /* NUM_SUBOPT; sortSet(max) */
  float delta_ratio;            /* DELTA_RATIO */
  uint32_t user_limit;          /* 0 = the reference's hard-coded 1000000 (cw.h:76) / 100000 (ucw.h:72) */
  int32_t n_existing;           /* < 0: seed the set with the pair's Optimal alignment like the drivers (aa_ali.cpp:83);
                                   >= 0: the caller's AlignmentSet already holds this many alignments (enumerate() appends) */
  const float* existing_scores; /* their scores (they take part in sortSet); such entries come back with n_pairs = -1,
                                   pair_off = their old index, uid -1, identity 0 and the caller's score.  NULL with
                                   n_existing > 0 is ALN_E_ARG.  The entries count for the brake `as.size() > user_limit`
                                   (cw.h:127) like the reference's own; KSCW / CRCW number what they create by its place
                                   in the WHOLE set (uid = index, kscw.h:262; the enumerator's seed has uid 1) */
  uint32_t k_limit;             /* KSCW / CRCW: operations a branch node keeps (NOaliParams::k_limit, default 16); their user_limit
                                   is NOaliParams::user_limit (0 = the default 100000, noalib.cpp:20) */
  uint32_t sort_limit;          /* CRCW: operations a branch node sorts and follows (NOaliParams::sort_limit; 0 = the default 100) */
  float max_overlap;            /* CRCW: share of an accepted sub-path a later one may repeat (NOaliParams::max_overlap, default 0.30) */
} aln_noa;

/* One alignment as the enumerators return it (AlignedPairList, alignment.h:52-113). */
typedef struct {
  float score;
  float identity;               /* calcIdentity, alignment.h:856-865 */
  int32_t uid;
  int32_t n_pairs;
  int64_t pair_off;             /* into the caller's pairs buffer, in (q,t) int32 units of 2 */
} aln_alignment;

/* ---- context ---------------------------------------------------------------------------- */
/* stream: a hipStream_t to launch on (e.g. torch.cuda.current_stream().cuda_stream) or NULL for a private stream. */
int aln_ctx_create(int device_id, void* stream, aln_ctx** out);
void aln_ctx_destroy(aln_ctx* ctx);
const char* aln_error_string(int status);
const char* aln_last_error(const aln_ctx* ctx);
int aln_ctx_synchronize(aln_ctx* ctx);
/* 1 if the shared object this function lives in carries a gfx950 code object (the offload-bundle id
 * "hipv4-amdgcn-amd-amdhsa--gfx950" is looked up in the file itself; needs no GPU), else 0. */
int aln_has_gfx950(void);
/* Tuning / kernel-selection hints of ONE context.  A context reads its defaults from the environment once, when it is created
 * (ALN_NO_TAG_KERNEL, ALN_NO_H16, ALN_NO_KEY16, ALN_TAG_ALT_PRIO, ALN_TAG_SEGMENTS, ALN_DP_VARIANT="NW,R[,X]", ALN_EXACT_NO_TILES,
 * ALN_EXACT_LITERAL, ALN_EXACT_ALT_PRIO, ALN_SCORE_NO_PACKED, ALN_ENUM_NODE_CAP, ALN_TAG_LAG, ALN_TAG_SOLO, ALN_TAG_BITS, ALN_TAG_OCCUPANCY, ALN_PLANE_ROW_ALIGN, ALN_ENUM_POOL_RETRIES, ALN_ENUM_WAVES, ALN_ENUM_DEBUG, ALN_ENUM_KEEP_POOLS, ALN_SEARCH_SLAB_ROWS, ALN_SEARCH_DEBUG, ALN_ZSCORE_CHUNK_ROWS, ALN_ALIGN_CHUNK_HITS); launches never read the environment.  Keys:
 *   "tag_kernel" "h16" "key16"     1/0: tagged-key kernel / uint16 score plane / 16-bit key layout allowed (results identical)
 *   "tag_alt_prio"                  1/0: row-alternating wave priority in the tagged kernel (a scheduling hint; pays when launches
 *                                   follow each other on one stream, loses when launches of several contexts overlap);
 *                                   2, 3 and 0x100 | four 2-bit levels: experimental schedules (dp_affine_tag.hip, row loop)
 *   "tag_segments"                  tagged kernel: 0 (default) one workgroup per pair; K in 2..8: long pairs are cut into K row
 *                                   segments handed out by a device queue when the batch alone fills the GPU; -K: whenever pairs are long
 *   "tag_occupancy"                 tagged kernel: 2 or 3 waves per SIMD (two builds of the 16-cells-per-lane instantiations); 0 (default):
 *                                   by the waves per SIMD the launch alone brings (rounds of 3 against rounds of 2).  A caller
 *                                   that overlaps launches of several contexts sets 3 (bench.py: -8 % per step).
 *   "tag_bits"                      12: the 12-tag-bit key layout (pointer dialect 2, sequences up to 4096) also for shorter sequences;
 *                                   0 (default): by length.  Results do not depend on it.
 *   "tag_solo"                      1: templates of up to 2048 columns run in the one-wave-per-pair kernel (dp_affine_solo.hip: no
 *                                   barriers; wants >= 2048 pairs in flight, i.e. two 1024-pair launches on two streams)
 *   "dp_variant_nw" "dp_variant_r" "dp_variant_x"   force a row-sweep instantiation (0 = automatic)
 *   "exact_tiles" "exact_literal" "score_packed" "enum_node_cap" "tag_lag"
 *   "exact_wavefront"               tiled exact-order kernel: 1 (default) = 64-column tiles, the four waves of a pair on four row
 *                                   blocks, no workgroup barrier; 0 = 256-column tiles with a barrier per row.  Same planes.
 *   "exact_alt_prio"                tiled exact-order kernel, wave priorities: 2 (default) = by progress (a wave ahead of the
 *                                   launch's average yields), 1 = rotation over the resident waves, 0 = none
 *   "exact_prune"                   1 (default): far candidate chunks that provably cannot matter are skipped (bit-exact); 0: off
 *   "exact_debug"                   1: aln_batch_last_exact_stats reports tested / skipped far chunks; 2: the waves' run times
 *   "enum_waves"                    ConstrainedNearOptimal / UnconstrainedNearOptimal / KSConstrainedNearOptimal search: waves per pair
 *                                   (2..16, enumerate_par.hip);
 *                                   1 = the one-wave kernel; 0 (default) = 16.  Same sets, same order.
 *   "enum_debug"                    1: aln_batch_enumerate_all reports every group of pairs it searches (pools, times, retries) on stderr
 *   "enum_keep_pools"               1 (default): aln_batch_enumerate_all keeps its device pools with the batch until the batch is destroyed
 *                                   (allocating tens of GB costs seconds); 0: frees them when it returns
 *   "enum_pool_retries"             aln_batch_enumerate_all: how often a pair whose pools overflowed is searched again with four
 *                                   times the capacity (default 2)
 *   "search_slab_rows"              aln_search_topk, aln_search_topk_profiles(_gaps): query rows whose scores are resident on the device at a time; 0 (default) = as many as
 *                                   keep the slab's scores (4 B x n_templates per row) and hits (16 B x K per row) below 1 GiB each
 *   "search_debug"                  1: aln_search_topk / aln_search_topk_profiles(_gaps) report their slabs and the device time of scoring / selection / end cells on stderr
 *   "zscore_chunk_rows"             aln_hits_zscores, aln_hits_zscores_profiles: query rows whose shuffled strings (profiles: shuffle
 *                                   orders) and accumulators are resident on the device at a time; 0 (default) = as many as keep the
 *                                   shuffled pool (n_shuffles x |q| bytes per row with a hit; profiles: n_shuffles x 2 B per profile
 *                                   row, padded) and the accumulators (16 B x K per row) below 1 GiB each; a larger value is cut to that
 *   "zscore_rows_per_chunk"         aln_hits_zscores_profiles: 0 (default) = the device rows of the profiles [q_begin, q_end) are
 *                                   uploaded once when they fit 1 GiB, else chunk by chunk; 1 = every chunk of query rows uploads
 *                                   the rows of its own profiles (environment default ALN_ZSCORE_ROWS_PER_CHUNK).  Same results.
 *   "align_chunk_hits"              aln_hits_align: hit slots whose 1 B/cell strips are resident on the device at a time; 0 (default) = as
 *                                   many as keep the strips, the lists and the lines below 1 GiB each; a value never lifts that budget
 *   "align_list_group_slots"        aln_hits_column_counts, aln_hits_pileup: batch-route slots whose pair lists are held on the host at a
 *                                   time; 0 (default) = as many as keep the lists below 256 MiB; a value never lifts that bound
 *                                   (environment default ALN_ALIGN_LIST_GROUP_SLOTS).  Same results.
 *   "weights_group_rows"            aln_hits_weights, aln_hits_weights_profiles: query rows whose letters rows (K x the block's longest
 *                                   Q-2 bytes per row) are resident on the device at a time; 0 (default) = as many as keep them below
 *                                   1 GiB; a value never lifts that budget (environment default ALN_WEIGHTS_GROUP_ROWS).  Same results.
 *                                   aln_hits_purge(_profiles) builds the same stack and reads the same hint.
 *   "align_fused_nonlocal"          aln_hits_align: 1 (default) = hits of the four non-local align types are aligned by the fused
 *                                   kernel where it applies; 0 = they all go through resident batches (environment default
 *                                   ALN_ALIGN_FUSED_NONLOCAL).  Same results.
 *   "align_rows_per_chunk"          aln_hits_align_profiles, aln_hits_align_multi_profiles: 0 (default) = the device rows of the profiles [q_begin, q_end) are
 *                                   uploaded once when they fit 1 GiB, else chunk by chunk; 1 = every chunk of hits uploads the
 *                                   rows of its own profiles (environment default ALN_ALIGN_ROWS_PER_CHUNK).  Same results.
 * Unknown key -> ALN_E_ARG.  No hint changes any result. */
int aln_ctx_set_hint(aln_ctx* ctx, const char* key, int64_t value);
int aln_ctx_get_hint(const aln_ctx* ctx, const char* key, int64_t* value);

/* ---- batch = many DPMatrix objects resident in HBM -------------------------------------- */
/* Replaces N x `DPMatrix(query, templ, ...)` construction up to initMtxMem (dpmatrix.h:250-259):
 * uploads both pools and the pair list (pair p aligns queries[q_idx[p]] with templates[t_idx[p]]).
 * score_only != 0 keeps no cell planes (all-vs-all scoring): only corner / best scores are produced. */
int aln_batch_create(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates,
                     int32_t n_pairs, const int32_t* q_idx, const int32_t* t_idx,
                     int32_t score_only, aln_batch** out);
void aln_batch_destroy(aln_batch* b);
int32_t aln_batch_n_pairs(const aln_batch* b);
/* bytes of HBM held by the batch (planes + sequences + results) */
int64_t aln_batch_device_bytes(const aln_batch* b);

/* DPMatrix::build (dpmatrix.h:291-317) for every pair: pre_calculate/SimilarityMatrix as `sim` says,
 * then the four builders (:356-1030) per direction and islocal = (align_type == local) (:155).
 * Asynchronous on the ctx stream.  bug_b4 != 0 reproduces dpmatrix.h:868 in reverse global builds. */
int aln_batch_dp(aln_batch* b, const aln_sim* sim, const aln_gap* gap,
                 int32_t direction, int32_t algo, int32_t bug_b4);
/* DPMatrix::reevaluate (dpmatrix.h:213-218): rebuild with the parameters of the last aln_batch_dp.
 * Lean rebuilds: when the build being replaced was used by the Optimal family (aln_batch_optimal, _enqueue, _strings*) and by
 * nothing that reads scores (aln_batch_get_cells, aln_batch_enumerate*), and the launch is the 2048-column local tagged kernel
 * (16-bit keys), the rebuild writes 2 B/cell: pointer words that also say "this cell scores 0" (the word the clip key leaves in
 * an interior cell, bit 15 in row 1 and column 1) and, of the score plane, only what the final cell needs.  The hints "tag_lag" and
 * "tag_alt_prio" values other than 1 are accepted and ignored by the lean kernel.  Optimal gives the same scores, lists and status on it.  The first other reader of the planes runs the full
 * build again on the batch's stream (one more DP launch, counted in aln_batch_dp_ms_history) and the reevaluate after it is
 * full; results already enqueued stay valid.  Context hint "lean_reevaluate" (ALN_LEAN_REEVALUATE): 0 never, 1 this rule
 * (default), 2 every eligible reevaluate.  aln_batch_dp and aln_batch_dp_sub are always full. */
int aln_batch_reevaluate(aln_batch* b);
/* Replace the gap description of the resident batch (constants, per-position arrays, deletion / insertion tables are uploaded
 * again; the similarity source stays resident); the next aln_batch_reevaluate builds with it.  The engine-side half of the
 * reference's refinement rounds — crcno.enumerate -> templ.updateCore -> dpm.reevaluate (gn2.cpp:146-185), where pre_calculate
 * derives new gap tables (gn2_eval.cpp:113-158) — for callers whose similarity does not change between rounds. */
int aln_batch_set_gap(aln_batch* b, const aln_gap* gap);
/* name of the DP kernel the last aln_batch_dp / _reevaluate launched ("dp_affine_tag_kernel<NW=2,R=2,X=8,local,h16,key16>",
 * "dp_affine_int_kernel<...>", "dp_exact_tiled_kernel<tpos,global,fwd>", "dp_exact_kernel<...>" ...) */
const char* aln_batch_dp_kernel_name(const aln_batch* b);

/* 7-argument DPMatrix ctor / build_subdpm (dpmatrix.h:169-189, :319-353) on one bounds rectangle per
 * pair: bounds[4*p..] = (q1_end, t1_end, q2_beg, t2_beg) in the order of the DEFINITION (B8). */
int aln_batch_dp_sub(aln_batch* b, const aln_sim* sim, const aln_gap* gap,
                     int32_t direction, const int32_t* bounds);

/* DPMatrix::getCell for a whole pair (dpmatrix.h:230-232): score, prev_query_idx, prev_template_idx
 * planes, Q x T row-major, untouched cells read 0 / -1 / -1 (dpmatrix.cpp:17-25).  Any pointer may be NULL.
 * After a lean aln_batch_reevaluate this first rebuilds the full planes (see there): the values are those of a full build. */
int aln_batch_get_cells(aln_batch* b, int32_t pair, float* score, int32_t* prev_q, int32_t* prev_t);
/* DPMatrix::getSim (dpmatrix.h:72-73) for a whole pair. */
int aln_batch_get_sim(aln_batch* b, int32_t pair, float* sim);
/* score of cell (Q-1,T-1) for forward, (0,0) for reverse builds, per pair (what global Optimal reports) */
int aln_batch_get_corner_scores(aln_batch* b, float* scores);

/* Optimal / Optimal_Rev ::enumerate (optimal.h:48-124, optimal_rev.h:44-131) for every pair:
 * find_max + pointer traceback on the device.  pairs: n_pairs x pair_stride x 2 int32, (q,t) in list
 * order; n[p] = list length; status[p] = 0 or ALN_E_STARTPAIR.  scores/n/status/pairs may be NULL. */
int aln_batch_optimal(aln_batch* b, float* scores, int32_t* n, int32_t* pairs, int32_t pair_stride,
                      int32_t* status);
/* The same, split so that a caller can keep the device busy: _enqueue launches find_max + traceback and the copy of the
 * per-pair results into a pinned host slot (two slots; ALN_E_STATE when both are waiting) and returns at once; _collect waits
 * for the OLDEST enqueued slot and hands out its scores / list lengths / status.  A loop `reevaluate; enqueue; collect(previous)`
 * overlaps the host's launch and copy latency of one step with the kernels of the next (bench.py). */
int aln_batch_optimal_enqueue(aln_batch* b);
int aln_batch_optimal_collect(aln_batch* b, float* scores, int32_t* n, int32_t* status);
/* Optimal + AlignmentSet::assignIdentity + SequenceGaps for every pair: what a driver prints for
 * `AlignmentSet as(dpm, optimal); as.assignIdentity(); cout << FastaOut(len) << as` (aa_ali.cpp:83-92, fastaio.h:51-76,
 * gstrings.h:84-164, alignment.h:856-865), without the FASTA framing.  Device: find_max + traceback, then one wave per pair lays
 * the template / query lines out and counts the identities (csrc/gapped_strings.hip); only the lines travel to the host.
 * tlines / qlines: n_pairs x stride chars, NUL-terminated (stride > T + Q covers any alignment); lengths[p] = line length
 * (0: status[p] != 0, or a list SequenceGaps cannot print).  scores/identity/status/lengths may be NULL.  Returns ALN_E_OVERFLOW when
 * a line does not fit the stride.  This is the end-to-end readout of config 2; aln_batch_optimal_enqueue/_collect is the score-only one. */
int aln_batch_optimal_strings(aln_batch* b, float* scores, float* identity, int32_t* status, char* tlines, char* qlines,
                              int32_t stride, int32_t* lengths);
/* The same, split like aln_batch_optimal_enqueue / _collect: _enqueue launches find_max + traceback + the string kernel on the
 * context's stream and the copy of the lines into one of two pinned slots on a separate copy stream, and returns at once
 * (ALN_E_STATE when both slots are waiting); _collect waits for the OLDEST slot and fills the caller's buffers (same `stride`).
 * `dp; strings_enqueue; strings_collect(previous)` overlaps step k's copy and host work with step k+1's kernels. */
int aln_batch_optimal_strings_enqueue(aln_batch* b, int32_t stride);
int aln_batch_optimal_strings_collect(aln_batch* b, float* scores, float* identity, int32_t* status, char* tlines, char* qlines,
                                      int32_t stride, int32_t* lengths);
/* Optimal_Subali::enumerate (optimal_subali.h:60-84) on the rectangles of the last aln_batch_dp_sub. */
int aln_batch_optimal_subali(aln_batch* b, float* scores, int32_t* n, int32_t* pairs,
                             int32_t pair_stride, int32_t* status);

/* ConstrainedNearOptimal / UnconstrainedNearOptimal ::enumerate (cw.h:68-92, ucw.h:64-85) for one pair
 * of the resident batch.  The set is seeded with the pair's Optimal alignment exactly like the drivers do
 * (aa_ali.cpp:83-89), the enumerator pushes its own uid-0 seed on top (B16), and the result is
 * sortSet(number_suboptimal)'ed.  flags: T bytes (SuboptFlags, sflags.h:23-37), ignored for UCW.
 * With noa->n_existing >= 0 the set is the caller's instead (see aln_noa): enumerate() appends to it, the seed included.
 * number_suboptimal 0 keeps everything in the order of creation (sortSet sorts nothing, alignment.h:925-931).
 * Outputs: up to max_alignments records + their pairs; *n_out = set size after sortSet.  ALN_E_OVERFLOW with max_alignments
 * smaller than that set *n_out to the size needed and writes no record; an argument or state error writes nothing at all. */
int aln_batch_enumerate(aln_batch* b, int32_t pair, const aln_noa* noa, const uint8_t* flags,
                        aln_alignment* out, int32_t max_alignments,
                        int32_t* pairs, int64_t pairs_capacity, int32_t* n_out);

/* The same enumeration for EVERY pair of the resident batch in one launch (BASELINE config 4: top-K near-optimal
 * tracebacks per pair from the GPU-resident matrices): one workgroup per pair runs its search (cw / ucw / kscw: 16 waves share
 * it, csrc/enumerate_par.hip; crcw: one wave), the host runs sortSet(number_suboptimal) per pair on (score,
 * index) keys in the reference's set order, survivors are unrolled on the device.  Every set is seeded with the pair's Optimal
 * alignment (noa->n_existing is ignored).
 *   flags: SuboptFlags rows, pair p's row at flags + p * flags_stride (flags_stride 0: one shared row of max T bytes);
 *   node_cap_per_pair / ali_cap_per_pair: trie nodes / alignments one pair's pools hold at first (0 = 1 Mi nodes / 64 Ki
 *   alignments).  A trie node is one aligned pair for the one-wave kernels and one diagonal run of up to 64 aligned pairs for
 *   the several-wave kernel, whose node pool is moreover shared by the pairs of a launch (n_pairs x node_cap_per_pair nodes in
 *   all: a 2000-residue homolog at DELTA_RATIO 0.01 needs 0.03-0.8 M of them).  Pairs that need more are searched again with 4 x larger pools, in groups sized to a device-memory budget,
 *   "enum_pool_retries" times (context hint, default 2), and only then report ALN_E_OVERFLOW;  K: slots per pair in the outputs (>= min(number_suboptimal, set size)).
 *   (Rounds continue past that count while the alignment pool is smaller than user_limit bounds, user_limit + 65536 + 16 (Q + T)
 *   slots, and every such round grows the node pool too.  The several-wave kernel hands its pool out in chunks of 65536 nodes,
 *   n_pairs x node_cap_per_pair nodes rounded down to chunks, at least one: below one chunk per pair some pairs get none and
 *   report ALN_E_OVERFLOW, and a few nodes per pair are still that one chunk after both 4 x retries.)
 *   A pair whose set after sortSet is larger than K reports ALN_E_OVERFLOW with n_out = K and its first K entries; an argument
 *   or state error (K <= 0, pair_stride < the batch's path stride, a REV or a sub-matrix build) writes no output.
 * Outputs (slot k of pair p at index p*K + k, set order): n_out[p] = set size after sortSet, scores, lengths,
 * pairs (NULL = not wanted) as (q,t) int32 at (p*K + k) * pair_stride * 2, status[p] = 0 / ALN_E_STARTPAIR /
 * ALN_E_OVERFLOW.  Returns the worst per-pair status. */
int aln_batch_enumerate_all(aln_batch* b, const aln_noa* noa, const uint8_t* flags, int32_t flags_stride,
                            uint32_t node_cap_per_pair, uint32_t ali_cap_per_pair, int32_t K,
                            int32_t* n_out, float* scores, int32_t* lengths, int32_t* pairs, int32_t pair_stride,
                            int32_t* status);
/* What the last aln_batch_enumerate_all used of every pair's pools: alignments created before sortSet (the reference's
 * as.size(), cw.h:91) and trie nodes (the several-wave kernel: runs, reserved 512 at a time by each wave) — also for pairs that reported ALN_E_OVERFLOW (the count at which they stopped), so that a
 * caller can size node_cap_per_pair / ali_cap_per_pair.  Either pointer may be NULL. */
int aln_batch_last_enum_usage(aln_batch* b, int32_t* alignments, int32_t* nodes);
/* Tickets the several-wave kernel handed out for every pair in the last aln_batch_enumerate_all (the search of that pair which
 * was run last: the final retry, or 0 when the one-wave kernel searched it, as it does for crcw, with enum_waves 1 and for a
 * pair that reached user_limit).  A pair's task ring has as many records as its alignment pool, so a count above the
 * ali_cap_per_pair of that search means the ring wrapped. */
int aln_batch_last_enum_tasks(aln_batch* b, int32_t* tasks);
/* Milliseconds the device spent in the search kernel / the unroll kernel of the last aln_batch_enumerate_all. */
int aln_batch_last_enum_ms(aln_batch* b, float* search_ms, float* unroll_ms);

/* ---- all-vs-all scoring without planes (BASELINE config 5) ------------------------------------ */
/* The score Optimal reports — find_max for local alignments (optimal.h:90-93,108-124), the final cell's score for the four
 * other align types (optimal.h:56-74) — for queries[q_begin..q_end) against EVERY template:
 * scores[(q - q_begin) * templates->n_seqs + t].  Replaces that many DPMatrix(q, t, AASubstitutionEval, fwd, align_type) +
 * Optimal constructions; nothing per cell is written to HBM.  A rank of a multi-GPU job calls it with its own block of query
 * rows.  ALN_GAP_AFFINE_CONST.  Integer table and gaps, templates up to 2046 residues: register-resident kernels
 * (local alignments whose values fit 15 bits run two queries per wave in packed 16-bit lanes).  Anything else the reference would
 * score — longer templates, fractional values — goes through resident batches of full builds (aln_batch_dp + Optimal) inside the
 * same call, ~12 GB of planes at a time; sequences beyond 65534 residues: ALN_E_TOO_LONG. */
int aln_score_all_vs_all(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                         const aln_gap* gap, int32_t q_begin, int32_t q_end, float* scores);

/* ---- all-vs-all search: the K best templates of every query, with end cells, selected on the device ---------------- */
/* One hit: template index, the score aln_score_all_vs_all reports for the pair (bit-identical), and the cell the optimal
 * alignment ends in, sentinels counted.  Unused slots hold { -1, 0.0f, -1, -1 }. */
typedef struct {
  int32_t t;        /* template index, -1 = unused slot */
  float   score;    /* bit-identical to aln_score_all_vs_all's value for (q, t) */
  int32_t q_end, t_end;
} aln_hit;
/* For every query of queries[q_begin..q_end): the K best templates among those with score >= min_score (-INFINITY: no
 * threshold), score descending, ties by template index ascending; n_hits[row] = min(K, candidates), hits[row * K + k].
 * Stands for (q_end - q_begin) x n_templates DPMatrix + Optimal constructions followed by a sort on the host (the reference has
 * no such driver); the dense score matrix never reaches the host, only hits and n_hits do.  Accepts what aln_score_all_vs_all
 * accepts, with its argument checks and status codes; K in 1..1024, else ALN_E_ARG.  q_begin == q_end: ALN_OK, nothing written.
 * (q_end, t_end): ALN_LOCAL — the cell Optimal::find_max returns (optimal.h:108-124: seeded at (Q-2, T-2), replaced only by a
 * strictly greater score, rows then columns ascending; a pair whose best score is 0 reports the seed), i.e. the entry before
 * the closing (Q-1, T-1) of aln_batch_optimal's pair list; the four other align types — (Q-1, T-1), where Optimal starts.
 * Query rows are scored a slab at a time (hint "search_slab_rows"); a rank of a multi-GPU job passes its own block of
 * rows and its hits are final (templates are replicated). */
int aln_search_topk(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                    const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K, float min_score,
                    aln_hit* hits /* (q_end-q_begin) x K */, int32_t* n_hits /* q_end-q_begin */);

/* ---- position-specific queries: all-vs-all scoring and search for profiles (PSSMs), no planes ---------------------- */
/* A pool of query profiles.  The reference builds a DPMatrix from any SimilarityMatrix, and a user Evaluator may return a
 * similarity that depends on the query POSITION, not on the query letter (evaluator.h:20-97): one score per template letter
 * for every query position — the second-round query of an iterative search, the query form of family databases.  Such a query
 * has no residue string to send through a substitution table.  Where such rows come from is the caller's business; the step
 * from a search round to the next one's rows is on the device too: aln_hits_column_counts (below, after
 * aln_hits_align_profiles) tallies the aligned template letters of a round's hits per query position, and
 * aln_amd.pssm_from_counts turns such counts into integer log-odds rows on the host; aln_hits_pssm (below, after
 * aln_hits_purge) goes from a round's hits to the next round's rows in one call, the log-odds made on the device by an exact
 * integer rule.  Rows may also carry their own gap penalties: aln_qgaps and aln_score_profiles_gaps_vs_all /
 * aln_search_topk_profiles_gaps (below, after aln_search_topk_profiles). */
typedef struct {
  int32_t n_seqs;
  const int64_t* offsets;       /* n_seqs + 1, in ROWS: profile s owns rows offsets[s] .. offsets[s+1); its first and last row stand
                                   for '^' and '$' (as aln_seqs INCLUDES them) and their values are never read; >= 2 rows each */
  const float* rows;            /* offsets[n_seqs] x n, row-major: rows[r * n + a] = similarity of position r and letter alphabet[a] */
  int32_t n;                    /* 1 .. 30 */
  const char* alphabet;         /* the TEMPLATES' alphabet */
} aln_qprofiles;
/* aln_score_all_vs_all and aln_search_topk for such queries.  For a profile of Q rows at row offset `off` and a template of T
 * residues (sentinels counted) S is the Q x T plane with S[i][j] = rows[(off + i) * n + index(t[j])] for 1 <= i <= Q-2 and
 * 1 <= j <= T-2, and 0 on the sentinel rows and columns; every reported value is what aln_batch_create over the pair (any
 * placeholder query of Q - 2 residues) + aln_batch_dp(ALN_SIM_MATRIX with that plane, gap, ALN_FWD, ALN_DP_AUTO) +
 * aln_batch_optimal give, bit for bit: find_max for local alignments, the final cell for the four other align types.
 * aln_score_profiles_vs_all replaces (q_end - q_begin) x n_templates such plane fills (4 B/cell) and full builds, and has
 * aln_score_all_vs_all's result layout; aln_search_topk_profiles replaces them and the host's sort of the dense result, and has
 * aln_search_topk's: the layout of hits / n_hits, the order (score descending, ties by template index, -0.0 = +0.0), min_score,
 * the padding { -1, 0, -1, -1 }, the end-cell rule with its (Q-2, T-2) seed, K in 1..1024, q_begin == q_end (ALN_OK, nothing
 * written), n_templates == 0, the slabs (hint "search_slab_rows") and "search_debug" are those of aln_search_topk, word for word.
 * Checks, in this order, nothing written when one fails: NULL arguments and (search) K; the row range; the gap model
 * (ALN_GAP_AFFINE_CONST) and align type; n outside 1..30, NULL alphabet / rows / offsets, a profile of fewer than 2 rows
 * (ALN_E_ARG); a template letter outside the alphabet (ALN_E_RESIDUE); more than 65534 rows or residues (ALN_E_TOO_LONG).
 * Routes: integer entries (of the interior rows of the whole pool) and gaps inside aln_score_all_vs_all's 2^23 bound, templates
 * of up to 2048 columns — register-resident kernels (csrc/score_only.hip): the device holds the rows of [q_begin, q_end) as
 * 32 x int32 each (the search uploads them slab by slab when they exceed 1 GiB) and nothing per cell touches HBM.  Everything
 * else — a fractional entry or gap, the bound exceeded, longer templates — goes through resident batches inside the call and so
 * accepts what aln_batch_dp accepts; the Q x T planes of a batch are expanded ON THE HOST for this fallback (it is the 4 B/cell
 * path the entries exist to avoid), and the ~12 GB budget of a batch counts them.
 * The hits of a profile search are aligned by aln_hits_align_profiles (below, after aln_hits_align), from the same device rows
 * and again with nothing per cell but the 1 B/cell strip; aln_hits_zscores still takes residue queries only: the hits of a
 * profile search go to aln_hits_zscores_profiles (below, after aln_hits_zscores), which permutes the rows of a profile. */
int aln_score_profiles_vs_all(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* templates, const aln_gap* gap,
                              int32_t q_begin, int32_t q_end, float* scores);
int aln_search_topk_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* templates, const aln_gap* gap,
                             int32_t q_begin, int32_t q_end, int32_t K, float min_score,
                             aln_hit* hits /* (q_end-q_begin) x K */, int32_t* n_hits /* q_end-q_begin */);

/* ---- position-specific GAP PENALTIES: scoring and search for profiles whose rows carry their own gap prices --------- */
/* A profile query is defined by where gaps are cheap (loops the hits disagree on) and where they are dear (conserved cores);
 * the reference's own evaluators (HMAP, Gn2) are built around position-dependent gaps.  No batch gap model can say this:
 * ALN_GAP_TABLES lets an insertion depend on (t1, q2 - q1), never on the query position. */
typedef struct {
  const float* del_init;   /* all four: one value per ROW of the profiles pool, indexed like aln_qprofiles.rows / n */
  const float* del_extn;
  const float* ins_init;
  const float* ins_extn;
} aln_qgaps;               /* 32 bytes */
/* aln_score_profiles_vs_all and aln_search_topk_profiles under such rows.  Take a profile of Q rows at row offset `off` and a
 * template of T residues, sentinels counted; S is the plane aln_score_profiles_vs_all defines.  Names follow the reference: a
 * DELETION skips template residues, an INSERTION skips profile positions.
 *   del(i, L), 0 <= i <= Q-2, L >= 1: the cost of L template residues skipped between profile positions i and i+1,
 *     del_init[off+i] + del_extn[off+i] * (L-1).  The gap is priced by the row it LEAVES; row 0, the '^' row, prices the head
 *     deletion and row Q-2 the tail deletion.
 *   ins(a, b), 1 <= a <= b <= Q-2: the cost of skipping profile positions a..b,
 *     ins_init[off+a] + sum_{p=a+1..b} ins_extn[off+p].  Every skipped position pays its own price.
 * Entries read: del_* at rows 0..Q-2 and ins_* at rows 1..Q-2.  The other sentinel entries are never read — del_* at row Q-1,
 * ins_* at rows 0 and Q-1: a NaN there changes nothing.
 * The recurrence is the one aln_score_profiles_vs_all pins (dpmatrix.h:375-689) with every gap cost replaced:
 *   D[i][j] = S[i][j] + max( D[i-1][j-1], max_{1<=k<j-1} D[i-1][k] - del(i-1, j-1-k), max_{1<=k<i-1} D[k][j-1] - ins(k+1, i-1) )
 * for interior cells, clipped at 0 under ALN_LOCAL; the head deletion into (1, j) costs del(0, j-1), the head insertion into
 * (i, 1) costs ins(1, i-1); into the final cell from (Q-2, k) the cost is del(Q-2, T-2-k), from (k, T-2) it is ins(k+1, Q-2);
 * each of these is 0 where the align type makes that end gap free (deletions: ALN_LOCAL, ALN_SEMI_LOCAL, ALN_LOCAL_GLOBAL;
 * insertions: ALN_LOCAL, ALN_SEMI_LOCAL, ALN_GLOBAL_LOCAL).  Degenerate shapes: Q = 2 costs del(0, T-2) and T = 2 costs
 * ins(1, Q-2), unless free.  The score is find_max for local alignments and the final cell for the four other align types.
 * THE ANCHOR: with all four arrays constant (del_init = ins_init = gi, del_extn = ins_extn = ge) every output of both entries
 * is byte-identical to aln_score_profiles_vs_all / aln_search_topk_profiles under { ALN_GAP_AFFINE_CONST, gi, ge, align_type },
 * for all five align types.
 * The result layouts, the hit order (score descending, ties by template index, -0.0 = +0.0), min_score and the padding
 * { -1, 0, -1, -1 }, K in 1..1024, the end-cell rule with its (Q-2, T-2) seed and strict-improvement order, q_begin == q_end,
 * n_templates == 0 and the slabs (hint "search_slab_rows") are aln_search_topk_profiles', word for word.
 * INTEGER SCORING ONLY, and there is no full-build fallback, because no batch gap model can express this: a fractional row
 * entry or gap value is refused with ALN_E_NOT_INTEGRAL, a gap value below 0 with ALN_E_ARG, a template of more than 2048
 * columns with ALN_E_TOO_LONG, and profiles->n above 26 with ALN_E_ARG (a row's four prices travel in words 26..29 of its
 * 128-byte device image).  The value bound is aln_score_all_vs_all's with the gaps' maximum in place of gi and ge: with G the
 * maximum of the entries read (of the whole pool), (maxs + G) * (maxQ + min(maxT, 2048)) + G + maxs < 2^23, else
 * ALN_E_NOT_INTEGRAL.
 * Order of the checks, nothing written when one fails: NULL arguments, and K for the search; the row range; align_type outside
 * 0..4; aln_score_profiles_vs_all's descriptor checks; n > 26, or a NULL array in aln_qgaps (all ALN_E_ARG); template letters
 * (ALN_E_RESIDUE); lengths (ALN_E_TOO_LONG, the 2048 columns included); a negative gap value (ALN_E_ARG); fractional values
 * and the bound (ALN_E_NOT_INTEGRAL).
 * Kernels: csrc/search_qgaps.hip over csrc/score_sweep_qgaps.h, register-resident like the constant-gap ones.  The hits of
 * such a search are aligned under the same rows by aln_hits_align_profiles_gaps and tallied by
 * aln_hits_column_counts_profiles_gaps (below, after aln_hits_column_counts_profiles), which start from the end cells reported
 * here.  They cannot yet be z-scored, piled up, weighted, purged, turned into the next round's rows or aligned into several
 * alignments under the same rows: those entries still take one gap_init / gap_extn.
 * THE ALIGNMENT under gap rows (what aln_hits_align_profiles_gaps reports).  The planes are those above.  The POINTER of a cell
 * is the reference's rule (dpmatrix.h:447-486 for an interior cell, 505-534 for the final cell, 607-649 under ALN_LOCAL) with
 * every cost replaced by del(.,.) / ins(.,.): the candidates of cell (i, j) are tried in the order
 *   match from (i-1, j-1); deletions from (i-1, k), k ascending; insertions from (k, j-1), k ascending,
 * and a later candidate wins only when it is STRICTLY greater than the best so far, so of equal candidates the first in that
 * order is the pointer.  A cell of row 1 or column 1 points at (0, 0).  The same order holds for the final cell (Q-1, T-1):
 * match from (Q-2, T-2), then (Q-2, k) with k ascending at del(Q-2, T-2-k), then (k, T-2) with k ascending at ins(k+1, Q-2); a
 * free end gap costs 0.  The LIST is Optimal's (optimal.h:56-74): (Q-1, T-1), then the pointers back to (0, 0), reported from
 * (0, 0) on.  Under ALN_LOCAL it is optimal.h:79-105: (Q-1, T-1), the end cell, then the pointers while the cell pointed at has
 * a score > 0 — the walk stops BEFORE a cell whose score is <= 0 — and (0, 0) in front when it stopped at a cell with both
 * indices > 0. */
int aln_score_profiles_gaps_vs_all(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_qgaps* gaps, const aln_seqs* templates,
                                   int32_t align_type, int32_t q_begin, int32_t q_end, float* scores);
int aln_search_topk_profiles_gaps(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_qgaps* gaps, const aln_seqs* templates,
                                  int32_t align_type, int32_t q_begin, int32_t q_end, int32_t K, float min_score,
                                  aln_hit* hits /* (q_end-q_begin) x K */, int32_t* n_hits /* q_end-q_begin */);

/* ---- shuffle z-scores of search hits: the background of every hit scored and reduced on the device ------------------- */
/* The reference has the hook (AlignedPairList::calcSignificance takes a Significance<Model> functor, significance.h) and ships
 * no model; this is the classic one.  The query of a hit is permuted n_shuffles times, every permutation is aligned to the
 * hit's template with the call's align type, table and gaps, and the hit's own score is placed against that sample. */
typedef struct {
  int64_t sum;     /* sum of the n shuffled-query scores (integer scoring, exact) */
  int64_t sumsq;   /* sum of their squares */
  int32_t n;       /* n_shuffles for a used slot, 0 for an unused one */
  float   z;       /* (score - mean) / sample standard deviation, see below; 0 when n < 2 or the sample has no spread */
} aln_hit_stats;   /* 24 bytes */
/* The layout is aln_search_topk's: row r is query q_begin + r, slots k < n_hits[r] of hits[r * K ..] are used, and only their
 * .t and .score are read — any list of (row, template) pairs will do, duplicates included.  stats[r * K + k] receives the
 * record of slot k; an unused slot gets { 0, 0, 0, 0.0f }.
 * Shuffle s (0 .. n_shuffles-1) of query q (its index in the POOL, not the row) with `seed`, all arithmetic uint32:
 *   fmix(x): x ^= x>>16; x *= 0x85EBCA6B; x ^= x>>13; x *= 0xC2B2AE35; x ^= x>>16
 *   key = fmix(fmix(fmix(seed ^ 0x9E3779B9) + q) + s)
 *   a = the interior residues (the sentinels stay), L = |q| - 2
 *   for i = L-1 down to 1:  r = fmix(key + i*0x9E3779B9);  j = (uint64(r) * (i+1)) >> 32;  swap(a[i], a[j])
 * so a shuffle depends on neither n_shuffles, the row block, K nor the chunking (hint "zscore_chunk_rows").
 * sum / sumsq run over the scores aln_score_all_vs_all reports for (shuffle s of the query, template t), all five align types.
 * With n = n_shuffles, N = n * (int64)score - sum and D = n * sumsq - sum * sum (exact, 128 bits):
 *   z = (float)((double)N * sqrt((double)(n-1) / ((double)n * (double)D))),   0.0f when n < 2 or D == 0.
 * INTEGER SCORING ONLY: the sums are exact integers, so a scoring system aln_score_all_vs_all would send through full builds
 * as a whole (fractional table or gaps, values beyond its 2^23 bound) is refused with ALN_E_NOT_INTEGRAL.  Templates beyond
 * 2048 columns are scored through full builds inside the call, like there.
 * Arguments: the checks and status codes of aln_score_all_vs_all; K in 1..1024, n_shuffles in 1..4096, every n_hits[r] in
 * 0..K and every used slot's t in [0, n_templates), else ALN_E_ARG — nothing is written when a check fails.
 * Order of the checks: NULL hits / n_hits / stats, K and n_shuffles first; then aln_score_all_vs_all's, in its order; then
 * n_hits and the used slots' t; ALN_E_NOT_INTEGRAL last.
 * q_begin == q_end: ALN_OK, nothing written.  Returns when stats is complete. */
int aln_hits_zscores(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                     const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                     const aln_hit* hits /* (q_end-q_begin) x K */, const int32_t* n_hits /* q_end-q_begin */,
                     int32_t n_shuffles, uint32_t seed, aln_hit_stats* stats /* (q_end-q_begin) x K */);

/* aln_hits_zscores for the hits of a profile search (aln_search_topk_profiles, or any list in its layout).  The hit layout and
 * the slots read, the aln_hit_stats record and its padding, the z formula with its exact 128-bit D, n_shuffles in 1..4096, K in
 * 1..1024, q_begin == q_end (ALN_OK, nothing written) and "returns when stats is complete" are aln_hits_zscores', word for word.
 * The shuffle permutes ROWS: with L = rows - 2 the interior rows of profile q (its index in the POOL, not the row block) and a =
 * the rule above applied to the list 0, 1, .., L-1 (same fmix, same key from seed, q, s, same descending swaps), shuffle s of
 * the profile keeps its two sentinel rows and has as interior row 1 + i the ORIGINAL row 1 + a[i].  sum / sumsq run over the
 * scores aln_score_profiles_vs_all reports for (shuffle s of profile q, template t), all five align types.  Consequence: for
 * profiles derived from residue queries under an integral table (row i = the table row of residue i) the result is
 * byte-identical to aln_hits_zscores on those residues with the same seed.
 * The permuted profiles are not materialised: the device keeps one copy of a profile's rows and reads it in permuted order
 * (csrc/search_zscore.hip), 2 B per row and shuffle; the chunking is aln_hits_zscores' (hints "zscore_chunk_rows",
 * "zscore_rows_per_chunk").  Templates beyond 2048 columns are scored through full builds inside the call.
 * INTEGER SCORING ONLY: a pool aln_score_profiles_vs_all would send through full builds as a whole (a fractional entry or gap,
 * its 2^23 bound exceeded) is refused with ALN_E_NOT_INTEGRAL.
 * Order of the checks, nothing written when one fails: NULL hits / n_hits / stats, K and n_shuffles (ALN_E_ARG);
 * aln_score_profiles_vs_all's, in its order; every n_hits[r] in 0..K and every used slot's t in [0, n_templates) (ALN_E_ARG);
 * ALN_E_NOT_INTEGRAL last. */
int aln_hits_zscores_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* templates, const aln_gap* gap,
                              int32_t q_begin, int32_t q_end, int32_t K,
                              const aln_hit* hits /* (q_end-q_begin) x K */, const int32_t* n_hits /* q_end-q_begin */,
                              int32_t n_shuffles, uint32_t seed, aln_hit_stats* stats /* (q_end-q_begin) x K */);

/* ---- the alignments of search hits, traced on the device from the end cells the search reported -------------------- */
/* One record per hit slot.  Unused slots hold { 0, 0, 0.0f, 0.0f }. */
typedef struct {
  int32_t n_pairs;          /* length of the pair list, 0 for an unused slot */
  int32_t status;           /* 0, ALN_E_STARTPAIR, ALN_E_OVERFLOW (list longer than pair_stride, line longer than line_stride), ALN_E_ARG (below) */
  float   score;            /* the score Optimal reports, bit-identical to aln_score_all_vs_all */
  float   identity;         /* calcIdentity, alignment.h:856-865, as aln_batch_optimal_strings reports it */
} aln_hit_alignment;        /* 16 bytes */
/* Optimal's alignment (optimal.h:48-105) of every used slot of a hit list in aln_search_topk's layout (row r is query
 * q_begin + r, slots k < n_hits[r] are used; duplicates allowed): out[r * K + k], the pair list in list order at
 * pairs + (r * K + k) * pair_stride * 2 (pairs == NULL: not wanted), the gapped template / query lines at
 * tlines / qlines + (r * K + k) * line_stride, NUL-terminated, and their length in lengths (the three line arguments all NULL:
 * not wanted; lengths alone may be NULL).  Every value is what aln_batch_create over the pair + aln_batch_dp(ALN_SIM_SUBMATRIX,
 * gap, ALN_FWD, ALN_DP_AUTO) + aln_batch_optimal / aln_batch_optimal_strings give, bit for bit.
 * ALN_LOCAL: the slot's (q_end, t_end) is TRUSTED as the cell the traceback starts from — it must be the cell aln_search_topk
 * reported (1 <= q_end <= Q-2, 1 <= t_end <= T-2 for pairs with Q >= 3 and T >= 3, else ALN_E_ARG before anything is written).
 * With an integer table and gaps and a template of up to 2048 columns one wave per hit sweeps rows 1 .. q_end with the state
 * in registers, writes 1 byte per cell into a transient strip and walks back through it (csrc/search_align.hip): no batch, no
 * planes, no find_max.  When the sweep's D[q_end][t_end] differs from the slot's .score the slot reports status ALN_E_ARG and
 * n_pairs 0 and the call goes on.
 * The four other align types ignore the slot's q_end, t_end and score: Optimal starts at (Q-1, T-1).  Under the same conditions
 * (integer table and gaps, template of up to 2048 columns, Q >= 3 and T >= 3) one wave per hit sweeps every row 1 .. Q-2,
 * writes 1 byte per cell into a transient strip of Q-3 rows, takes the final cell's pointer from the last row and the last
 * column and walks back to the origin; hint "align_fused_nonlocal" = 0 sends them through batches instead.
 * Longer templates, fractional scoring systems, pairs without an interior and, ALN_LOCAL, templates of 1793 .. 2048 columns go
 * through resident batches inside the call (~12 GB of planes at a time), so the call accepts what aln_search_topk accepts.
 * aln_hits_align_last_routes tells how many slots went which way.
 * Checks, in this order, nothing written when one fails: NULL hits / n_hits / out, K outside 1..1024, pairs with
 * pair_stride < 2, the line group given in part or line_stride < 1 (ALN_E_ARG); aln_score_all_vs_all's, in its order; every
 * n_hits[r] in 0..K, every used slot's t in [0, n_templates) and, local, its end cell in range (ALN_E_ARG).
 * q_begin == q_end: ALN_OK, nothing written.  A list longer than pair_stride (its first pair_stride entries are written) or a
 * line that does not fit line_stride (empty lines) gives the slot ALN_E_OVERFLOW.  Returns when every output is complete: the
 * lowest (most negative) per-slot status, ALN_OK when all are 0.  Hits are handled a chunk at a time (hint "align_chunk_hits"). */
int aln_hits_align(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                   const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                   const aln_hit* hits, const int32_t* n_hits,
                   aln_hit_alignment* out /* (q_end-q_begin) x K */,
                   int32_t* pairs, int32_t pair_stride /* NULL, or rows x K x pair_stride x 2 int32 */,
                   char* tlines, char* qlines, int32_t line_stride, int32_t* lengths /* all NULL, or as aln_batch_optimal_strings */);
/* aln_hits_align for the hits of a profile search (aln_search_topk_profiles).  The hit layout and which slots are used, out,
 * pairs, the line group and lengths, the per-slot statuses and the return value, the local rule (the slot's end cell is trusted;
 * a sweep score that differs from .score gives the slot ALN_E_ARG, n_pairs 0, and the call goes on), non-local slots ignoring
 * q_end / t_end / score, q_begin == q_end (ALN_OK, nothing written), the hints "align_chunk_hits" and "align_fused_nonlocal" and
 * aln_hits_align_last_routes are those of aln_hits_align.
 * Every value is what aln_batch_create over (the query letters of the row, the template) + aln_batch_dp(ALN_SIM_MATRIX with the
 * pair's plane as aln_score_profiles_vs_all defines it, gap, ALN_FWD, ALN_DP_AUTO) + aln_batch_optimal /
 * aln_batch_optimal_strings give, bit for bit.
 * Query letters: a profile has none, the query line and the identity need them.  `consensus` is an ordinary pool, sentinels
 * included, with n_seqs == profiles->n_seqs and offsets[s] == profiles->offsets[s] for every s; its letters are never scored
 * and are not checked against the alphabet.  NULL: the placeholder pool — the profiles' offsets, '^', alphabet[0] for every
 * interior position, '$'.  The identity counts equal CHARACTERS of the two pools over the list's entries (then - 2), as
 * aln_batch_optimal_strings does.
 * Routes: integer rows (of the interior rows of the whole pool) and gaps inside aln_score_all_vs_all's 2^23 bound, Q >= 3 and
 * T >= 3, a template of up to 2048 columns — one wave per hit, the rows staged from HBM into LDS 8 at a time, 1 byte per cell
 * into a transient strip (csrc/search_align.hip), for all five align types.  Everything else — fractional rows or gaps,
 * longer templates, pairs without an interior — goes through resident batches inside the call, whose planes are expanded on
 * the host and counted in the ~12 GB budget.  The device rows of [q_begin, q_end) are uploaded once when they fit 1 GiB, else
 * with every chunk of hits (hint "align_rows_per_chunk").
 * Checks, in this order, nothing written when one fails: NULL profiles / templates / gap / hits / n_hits / out; K outside
 * 1..1024; pairs with pair_stride < 2; the line group given in part or line_stride < 1 (ALN_E_ARG);
 * aln_score_profiles_vs_all's, in its order, with the consensus pool — a wrong n_seqs, a NULL member, any differing offset:
 * ALN_E_ARG — directly after the profile descriptor and before the templates' letters; every n_hits[r] in 0..K; every used
 * slot's t in [0, n_templates); local, its end cell in range (ALN_E_ARG). */
int aln_hits_align_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus /* may be NULL */,
                            const aln_seqs* templates, const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                            const aln_hit* hits, const int32_t* n_hits, aln_hit_alignment* out,
                            int32_t* pairs, int32_t pair_stride,
                            char* tlines, char* qlines, int32_t line_stride, int32_t* lengths);
/* ---- column counts of search hits: from one search round to the profile of the next, tallied on the device ----------- */
/* For every query of the row block, how often each template letter stands under each query position in the alignments of the
 * query's hits — what a position-specific query of the next round is made from — without an alignment leaving the device.
 * The hit layout and which slots are used are aln_hits_align's (duplicates allowed).  The alignment of a slot is the pair list
 * aln_hits_align reports for it: ALN_LOCAL trusts the slot's end cell (a sweep score that differs from .score gives the slot
 * ALN_E_ARG, n_pairs 0, and the call goes on), the four other align types start at (Q-1, T-1).  out[s] is, byte for byte, the
 * record aln_hits_align writes for the slot when called with pairs == NULL and no line group; unused slots hold { 0, 0, 0, 0 };
 * ALN_E_OVERFLOW cannot occur.
 * A slot contributes with weight w = weights[s] (weights == NULL: 1) when its status is 0, w > 0 and, ALN_LOCAL, its score is
 * > 0 (a score-0 local list is the seed cell's, not an alignment).  With off = offsets[q_begin], row(i) = offsets[query] - off +
 * i and n the alphabet's size, a contributing slot adds w to counts[row(i) * n + index(t[j])] for every list entry (i, j) with
 * 1 <= i <= Q-2 and 1 <= j <= T-2 (index: the letter's position in the call's alphabet), and, with i_lo / i_hi the smallest /
 * largest such i (when there is one), w to covered[row(i)] for every i_lo <= i <= i_hi: covered[r] - sum_a counts[r][a] is the
 * weighted number of alignments that pass query position r opposite a gap.  counts (and covered, which may be NULL) are
 * written in full by every successful call — zeros where nothing contributed, the sentinel rows included — and depend on
 * neither the chunking (hints "align_chunk_hits", "align_rows_per_chunk"), the launch order nor the route: every add is an
 * integer add.
 * Routes: those of aln_hits_align — one wave per hit sweeps as there, writes the 1 B/cell strip, walks back through it and
 * issues one integer atomic add per list entry into 32-wide int32 rows on the device (csrc/search_counts.hip), which are
 * zeroed once per call and downloaded once at its end; no list, no line and no per-hit download but the 16-byte record.
 * What those kernels do not take (longer templates, fractional scoring, pairs without an interior, ALN_LOCAL templates of
 * 1793 .. 2048 columns) goes through resident batches whose pair lists the host tallies into the same outputs.
 * aln_hits_align_last_routes reports this call's slots too.
 * Checks, in this order, nothing written when one fails: NULL hits / n_hits / out / counts, K outside 1..1024 (ALN_E_ARG);
 * aln_score_all_vs_all's, in its order; every n_hits[r] in 0..K, every used slot's t in [0, n_templates) and, local, its end
 * cell in range (ALN_E_ARG); every used slot's weight in 0..65535 (ALN_E_ARG: with K <= 1024 no count can leave int32).
 * q_begin == q_end: ALN_OK, nothing written.  Returns the lowest per-slot status, ALN_OK when all are 0. */
int aln_hits_column_counts(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                           const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                           const aln_hit* hits, const int32_t* n_hits,
                           const int32_t* weights /* rows x K, or NULL = every used slot 1 */,
                           aln_hit_alignment* out /* rows x K */,
                           int32_t* counts /* (offsets[q_end] - offsets[q_begin]) x sub->n */,
                           int32_t* covered /* offsets[q_end] - offsets[q_begin], may be NULL */);
/* The same for the hits of a profile search: the slots, records, routes and consensus pool are aln_hits_align_profiles', the
 * weights, counts (x profiles->n, in the order of profiles->alphabet) and covered are those above, and the checks are NULL
 * profiles / templates / gap / hits / n_hits / out / counts and K; aln_score_profiles_vs_all's, in its order, with the
 * consensus pool where aln_hits_align_profiles checks it; n_hits, t and the end cells; the weights.  For profiles derived from
 * residue queries under an integral table the outputs are byte-identical to aln_hits_column_counts' on those residues. */
int aln_hits_column_counts_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus /* may be NULL */,
                                    const aln_seqs* templates, const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                                    const aln_hit* hits, const int32_t* n_hits, const int32_t* weights,
                                    aln_hit_alignment* out, int32_t* counts /* ... x profiles->n */, int32_t* covered);
/* ---- the hits of a search under position-specific GAP PENALTIES (aln_qgaps), aligned and tallied under the same rows ---- */
/* aln_hits_align_profiles for the hits of aln_search_topk_profiles_gaps.  The alignment of a slot is the one defined with
 * aln_qgaps above (THE ALIGNMENT under gap rows): the planes of aln_score_profiles_gaps_vs_all, the pointer rule with its
 * order of candidates — match, deletions k ascending, insertions k ascending, a later one only when strictly greater —, the
 * final cell under the same order, Optimal's list.
 * Taken from aln_hits_align_profiles, word for word: the hit layout and which slots are used; out, pairs, the line group and
 * lengths; the consensus and placeholder pools; the identity counted over characters; the per-slot statuses and the return
 * value; q_begin == q_end (ALN_OK, nothing written); the local rule (the slot's end cell is trusted; a sweep score that differs
 * from .score gives the slot ALN_E_ARG, n_pairs 0, and the call goes on); non-local slots ignoring q_end / t_end / score; the
 * hints "align_chunk_hits" and "align_rows_per_chunk"; aln_hits_align_last_routes.
 * THE ANCHOR: with all four arrays constant (del_init = ins_init = gi, del_extn = ins_extn = ge) every output byte — records,
 * lists, lines, lengths — equals aln_hits_align_profiles under { ALN_GAP_AFFINE_CONST, gi, ge, align_type }, for all five
 * align types.
 * INTEGER SCORING ONLY: the descriptor and gap checks, their status codes, their order and the value bound are those of
 * aln_search_topk_profiles_gaps (n <= 26, a NULL array, a negative or fractional value, templates beyond 2048 columns ->
 * ALN_E_TOO_LONG).
 * Routes: there is no batch route, because no batch gap model prices a gap by the query position.  Every pair with an interior
 * (Q >= 3 and T >= 3; T <= 2048 by the checks) goes through one wave per hit over the gap-row sweeps
 * (csrc/search_align_qgaps.h: the 1 B/cell strip and the walk of aln_hits_align_profiles), for all eight length classes and all
 * five align types.  A pair without an interior (Q = 2 or T = 2) is filed on the host: its list is the one
 * aln_hits_align_profiles reports for such a pair, its score is the definition's — Q = 2: -del(0, T-2), T = 2: -ins(1, Q-2), 0
 * where that end gap is free or nothing is skipped, 0 under ALN_LOCAL.  aln_hits_align_last_routes counts the host-filed slots
 * in its second number.  Hint "align_fused_nonlocal" has nothing to switch to and is ignored.
 * Checks, in this order, nothing written when one fails: NULL profiles / gaps / templates / hits / n_hits / out; K outside
 * 1..1024; pairs with pair_stride < 2; the line group given in part or line_stride < 1 (ALN_E_ARG);
 * aln_search_topk_profiles_gaps', in its order, with the consensus pool — a wrong n_seqs, a NULL member, any differing offset:
 * ALN_E_ARG — directly after the profile descriptor, where aln_hits_align_profiles checks it; every n_hits[r] in 0..K; every
 * used slot's t in [0, n_templates); local, its end cell in range (ALN_E_ARG). */
int aln_hits_align_profiles_gaps(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_qgaps* gaps,
                                 const aln_seqs* consensus /* may be NULL */, const aln_seqs* templates, int32_t align_type,
                                 int32_t q_begin, int32_t q_end, int32_t K, const aln_hit* hits, const int32_t* n_hits,
                                 aln_hit_alignment* out, int32_t* pairs, int32_t pair_stride,
                                 char* tlines, char* qlines, int32_t line_stride, int32_t* lengths);
/* aln_hits_column_counts_profiles for the same hits: its arguments with `gaps` and `align_type` in place of `gap`.  The
 * alignment of a slot is the list aln_hits_align_profiles_gaps reports for it, and out[s] is, byte for byte, the record that
 * entry writes when called with pairs == NULL and no line group.  The weights (0..65535), counts (x profiles->n) and covered —
 * both written in full by every successful call —, the contribution rule and the independence of the chunking are
 * aln_hits_column_counts_profiles'.  A pair without an interior has no interior entry and contributes nothing.  With all four
 * arrays constant every output byte equals aln_hits_column_counts_profiles'.  Routes: those of aln_hits_align_profiles_gaps
 * (csrc/search_counts_qgaps.hip: the same kernels over the job that counts).  Checks: NULL profiles / gaps / templates / hits /
 * n_hits / out / counts and K; then those of aln_hits_align_profiles_gaps from aln_search_topk_profiles_gaps' on; the weights. */
int aln_hits_column_counts_profiles_gaps(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_qgaps* gaps,
                                         const aln_seqs* consensus /* may be NULL */, const aln_seqs* templates,
                                         int32_t align_type, int32_t q_begin, int32_t q_end, int32_t K,
                                         const aln_hit* hits, const int32_t* n_hits, const int32_t* weights,
                                         aln_hit_alignment* out, int32_t* counts /* ... x profiles->n */, int32_t* covered);
/* ---- the query-anchored pileup of search hits: one fixed-width row per hit, column = query position -------------------- */
/* The a3m / pileup form of a search round: for every used slot one row whose index is the query position and whose entry is
 * the template residue aligned to that position, or a gap — what per-hit weights, purging of near-identical hits, gap
 * statistics, a consensus and the MSA handed to another tool are read off — and the aligned range of every hit, without a pair
 * list leaving the device.
 * The hit layout and which slots are used are aln_hits_align's (duplicates allowed).  The alignment of a slot is the pair list
 * aln_hits_align reports for it: ALN_LOCAL trusts the slot's end cell (a sweep score that differs from .score gives the slot
 * ALN_E_ARG, n_pairs 0, and the call goes on), the four other align types start at (Q-1, T-1).  out[s] is, byte for byte, the
 * record aln_hits_align writes for the slot when called with pairs == NULL and no line group; unused slots hold { 0, 0, 0, 0 };
 * ALN_E_OVERFLOW cannot occur.
 * A slot CONTRIBUTES when its status is 0 and, ALN_LOCAL, its score is > 0 (aln_hits_column_counts' rule without the weights).
 * With Q the residues of the row's query and T those of the template (sentinels counted), query position i (1 <= i <= Q-2)
 * stands at index p = i - 1 of the slot's line: letters[s * line_stride + p], tpos[s * line_stride + p].  An INTERIOR ENTRY is
 * a list entry (i, j) with 1 <= i <= Q-2 and 1 <= j <= T-2; i_lo / i_hi are the smallest / largest i of the slot's interior
 * entries.  Then
 *   a contributing slot with interior entry (i, j):   tpos = j, letters = templates->residues[offsets[t] + j] — the pool's own
 *                                                     character, on both routes;
 *   a contributing slot, no entry at i, i_lo < i < i_hi:   tpos = 0, letters = '-';
 *   every other position p < Q-2 of a used slot:      tpos = 0, letters = '.' — outside [i_lo, i_hi], and every position of a
 *                                                     slot that does not contribute;
 *   indices Q-2 <= p < line_stride of a used slot and every index of an unused slot:   '\0' / 0.
 * ('.' and '-' are taken not to be letters of the templates.)  spans[s] = { i_lo, i_hi, the j of i_lo, the j of i_hi } for a
 * contributing slot with at least one interior entry, { 0, 0, 0, 0 } for every other slot; under ALN_LOCAL (q_lo, t_lo) is the
 * start cell of the hit whose end cell is (q_end, t_end).  j <= T-2 <= 65532, so uint16_t holds every position.
 * spans, letters and tpos are independent and each may be NULL; with all three NULL the call is aln_hits_align without lists
 * and lines.  line_stride is read only when letters or tpos is given.
 * The outputs are written in full by every successful call and depend on neither the chunking (hints "align_chunk_hits",
 * "align_rows_per_chunk"), the launch order, the route nor hint "align_fused_nonlocal".
 * Routes: those of aln_hits_align — one wave per hit sweeps as there, writes the 1 B/cell strip, walks back through it and per
 * list entry issues one 2-byte store into the hit's tpos row and one 1-byte store into its letters row on the device
 * (csrc/search_pileup.hip), then writes the span and the '-' of its range; per hit the 16-byte record, the span and Q-2 <=
 * stride entries of each row come down, no list.  What those kernels do not take (longer templates, fractional scoring, pairs
 * without an interior, ALN_LOCAL templates of 1793 .. 2048 columns, the non-local types under "align_fused_nonlocal" = 0) goes
 * through resident batches whose pair lists the host lays out into the same outputs.  aln_hits_align_last_routes reports
 * this call's slots too.
 * Checks, in this order, nothing written when one fails: NULL hits / n_hits / out, K outside 1..1024, line_stride < 1 when
 * letters or tpos is given (ALN_E_ARG); aln_score_all_vs_all's, in its order; line_stride < Q-2 for any query of
 * [q_begin, q_end) when letters or tpos is given (ALN_E_ARG); every n_hits[r] in 0..K, every used slot's t in
 * [0, n_templates) and, local, its end cell in range (ALN_E_ARG).
 * q_begin == q_end: ALN_OK, nothing written.  Returns the lowest per-slot status, ALN_OK when all are 0. */
typedef struct { int32_t q_lo, q_hi, t_lo, t_hi; } aln_hit_span;   /* 16 bytes; {0,0,0,0}: nothing aligned */
int aln_hits_pileup(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                    const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                    const aln_hit* hits, const int32_t* n_hits,
                    aln_hit_alignment* out /* rows x K */, aln_hit_span* spans /* rows x K, may be NULL */,
                    char* letters /* rows x K x line_stride, may be NULL */,
                    uint16_t* tpos /* rows x K x line_stride, may be NULL */, int32_t line_stride);
/* The same for the hits of a profile search: the slots, records, routes and consensus pool are aln_hits_align_profiles' — the
 * consensus only enters the records' identity —, spans, letters and tpos are those above, and the checks are NULL profiles /
 * templates / gap, then NULL hits / n_hits / out, K and line_stride < 1; aln_score_profiles_vs_all's, in its order, with the
 * consensus pool where aln_hits_align_profiles checks it; line_stride < Q-2; n_hits, t and the end cells.  For profiles derived
 * from residue queries under an integral table every output is byte-identical to aln_hits_pileup's on those residues. */
int aln_hits_pileup_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus /* may be NULL */,
                             const aln_seqs* templates, const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                             const aln_hit* hits, const int32_t* n_hits, aln_hit_alignment* out, aln_hit_span* spans,
                             char* letters, uint16_t* tpos, int32_t line_stride);
/* ---- position-based sequence weights of search hits: from a round's hits to weights and weighted counts, on the device ---- */
/* Before the hits of a round become the next round's profile, redundant hits are weighted down: forty near-copies of one
 * homolog must not out-vote five distant ones.  These are Henikoff's position-based weights, read off the pileup above without
 * the pileup leaving the device, and — when wanted — the column counts under those weights, every hit swept once.
 * Everything is exact integer arithmetic: the result depends on neither the launch order, the chunking nor the route.
 * For a query row r of the block take the pileup aln_hits_pileup defines for its slots k < n_hits[r]: the letters rows
 * L[k][p], p = 0 .. Q-3.  A slot CONTRIBUTES exactly when it does there: status 0 and, ALN_LOCAL, score > 0.  Only letters of
 * the call's alphabet count; '-', '.' and NUL never do.  Per position p:
 *   n_p[a]     the number of contributing slots with L[k][p] == alphabet[a];
 *   k_p        the number of letters a with n_p[a] > 0.
 * Per slot:
 *   raw[k]     the sum, over the positions p where L[k][p] is a letter a, of floor(2^24 / (k_p * n_p[a])), an int64; 0 for a
 *              slot that does not contribute or has no aligned letter;
 *   M          max_k raw[k] over the row;
 *   weight[k]  0 where raw[k] == 0, otherwise max(1, floor(w_max * raw[k] / M)) in 64-bit integers: the row's heaviest slot
 *              gets exactly w_max.
 * w_max is in 1..65535, the weights aln_hits_column_counts accepts.  (The denominator is at most 30 * 1024, raw is below 2^40
 * and w_max * raw below 2^56.)  The query itself is not a member of the stack: a caller who wants it counted lists it as a hit.
 * Slots, records, routes and statuses are aln_hits_pileup's: out[s] is, byte for byte, the record aln_hits_align writes for the
 * slot when called with pairs == NULL and no line group; a slot that fails (a falsified local score: ALN_E_ARG) does not
 * contribute and the call goes on.  weights (required) and raw (may be NULL) are rows x K; unused slots hold 0.
 * counts and covered (each may be NULL, independently) are, byte for byte, what aln_hits_column_counts returns for the same
 * hits with `weights` set to this call's weights, in its layout.
 * Device side (csrc/search_weights.hip): the letters rows of a group of consecutive queries stay on the device in slot order
 * (rows x K x the block's longest Q-2 bytes, at most 1 GiB per group; hint "weights_group_rows"); fused hits write them
 * through aln_hits_pileup's kernels, the slots of the batch route are laid out on the host and uploaded; then a column tally
 * (one wave per query and 64 positions, a 32-counter histogram per position in LDS), one wave per slot for raw, one wave per
 * query for the weights, and the tally once more under the weights.  Only weights, raw, the records and the count rows come down.
 * aln_hits_align_last_routes reports this call's slots too.
 * Checks, in this order, nothing written when one fails: NULL hits / n_hits / out, K outside 1..1024 (ALN_E_ARG);
 * aln_score_all_vs_all's, in its order; NULL weights, w_max outside 1..65535 (ALN_E_ARG); every n_hits[r] in 0..K, every used
 * slot's t in [0, n_templates) and, local, its end cell in range (ALN_E_ARG); last, an alphabet that holds '.' or '-'
 * (ALN_E_ARG: the pileup cannot show them as letters).
 * q_begin == q_end: ALN_OK, nothing written.  Returns the lowest per-slot status, ALN_OK when all are 0. */
int aln_hits_weights(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                     const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                     const aln_hit* hits, const int32_t* n_hits, int32_t w_max,
                     aln_hit_alignment* out /* rows x K */, int32_t* weights /* rows x K */,
                     int64_t* raw /* rows x K, may be NULL */,
                     int32_t* counts /* (offsets[q_end] - offsets[q_begin]) x sub->n, may be NULL */,
                     int32_t* covered /* offsets[q_end] - offsets[q_begin], may be NULL */);
/* The same for the hits of a profile search: the slots, records, routes and consensus pool are aln_hits_pileup_profiles', the
 * alphabet is profiles->alphabet, and the checks are NULL profiles / templates / gap, then NULL hits / n_hits / out and K;
 * aln_score_profiles_vs_all's, in its order, with the consensus pool where aln_hits_align_profiles checks it; weights and
 * w_max; n_hits, t and the end cells; the alphabet.  For profiles derived from residue queries under an integral table every
 * output is byte-identical to aln_hits_weights' on those residues. */
int aln_hits_weights_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus /* may be NULL */,
                              const aln_seqs* templates, const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                              const aln_hit* hits, const int32_t* n_hits, int32_t w_max, aln_hit_alignment* out,
                              int32_t* weights, int64_t* raw, int32_t* counts, int32_t* covered);
/* ---- purging of near-identical search hits: the purge decision and the survivors' weights, on the device ---------------- */
/* Before the weights of a round are made, near-identical hits are purged (PSI-BLAST at 94 % identity, hhfilter -id 90): weights
 * damp redundancy, they do not remove it.  These entries go from a round's hits to the purge decision and, when wanted, to the
 * weights and weighted counts of the survivors in one call: every hit is swept once and no pileup is downloaded.
 * All of it is exact integer arithmetic: the result depends on neither the chunking, the grouping, the route nor the launch order.
 * For a query row r of the block take the pileup aln_hits_pileup defines for its slots k < n_hits[r]: the letters rows
 * L[k][p], p = 0 .. Q-3.  A slot CONTRIBUTES exactly when it does there: status 0 and, ALN_LOCAL, score > 0.  A LETTER is a
 * character of the call's alphabet (sub->alphabet, or profiles->alphabet); '-', '.' and NUL never are letters, and the row of
 * a slot that does not contribute shows no letter.
 *   letters(k)     the number of positions where L[k][p] is a letter;
 *   overlap(j,k)   for j < k, the number of positions where both rows show a letter;
 *   same(j,k)      the number of those positions where the letters are equal.
 * Slot k is NEAR slot j (j < k) when overlap(j,k) >= 1, 100 * overlap(j,k) >= min_overlap * letters(k) and
 * 100 * same(j,k) >= max_identity * overlap(j,k).  (The products are at most 100 * 65532: int32 holds them.)
 * The greedy rule, slots in ascending order (the search's order: best score first): slot k is KEPT when letters(k) > 0 and it
 * is near no KEPT slot j < k; otherwise, if letters(k) > 0, it is PURGED and its keeper is the smallest kept j it is near.  A
 * purged slot purges nobody.
 * max_identity is in 1..101; 101 can never be met: then nothing is purged and every weight output is byte-identical to
 * aln_hits_weights'.  min_overlap is in 0..100; with 0 only overlap >= 1 is asked.
 * purge[s], per slot:   kept { k, 0, 0, letters(k) };   purged by j { j, same(j,k), overlap(j,k), letters(k) };
 *                       unused, not contributing, or without a letter { -1, 0, 0, 0 }.
 * weights may be NULL (purge only): then raw, counts and covered must be NULL too and w_max is not read.  With weights given,
 * w_max is in 1..65535, and weights, raw, counts and covered are exactly aln_hits_weights' definition applied to the pileup in
 * which every slot that is not kept shows '.' at every position: purged slots get weight 0 and raw 0, and counts and covered
 * are, byte for byte, what aln_hits_column_counts returns for the same hits under the returned weights.
 * out[s] is, byte for byte, the record aln_hits_align writes for the slot when called with pairs == NULL and no line group; a
 * slot with a falsified local score gets ALN_E_ARG, does not contribute, and the call goes on.
 * Device side (csrc/search_purge.hip): the stack is aln_hits_weights' (hint "weights_group_rows"; a group also keeps the pair
 * bits, K x ceil(K/64) x 8 bytes per query row, below 1 GiB); over a complete group a pair kernel (per query, tiles of 64 slots
 * k on the lanes x 32 slots j, rows staged through LDS and translated to letter codes, four positions per dword, one near bit
 * per pair), a greedy kernel (one wave per query), one wave per purged slot for its record, the rows of the slots that are not
 * kept rewritten to '.', then aln_hits_weights' four launches.  aln_hits_align_last_routes reports this call's slots too.
 * Checks, in this order, nothing written when one fails: NULL hits / n_hits / out, K outside 1..1024 (ALN_E_ARG);
 * aln_score_all_vs_all's, in its order; NULL purge; max_identity outside 1..101; min_overlap outside 0..100; weights == NULL
 * with any of raw / counts / covered given; w_max outside 1..65535 when weights is given (ALN_E_ARG); every n_hits[r] in 0..K,
 * every used slot's t in [0, n_templates) and, local, its end cell in range (ALN_E_ARG); last, an alphabet that holds '.' or
 * '-' (ALN_E_ARG).
 * q_begin == q_end: ALN_OK, nothing written.  Returns the lowest per-slot status, ALN_OK when all are 0. */
typedef struct { int32_t keeper, same, overlap, letters; } aln_hit_purge;   /* 16 bytes */
int aln_hits_purge(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                   const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                   const aln_hit* hits, const int32_t* n_hits,
                   int32_t max_identity, int32_t min_overlap, int32_t w_max,
                   aln_hit_alignment* out /* rows x K */, aln_hit_purge* purge /* rows x K */,
                   int32_t* weights /* rows x K, may be NULL = purge only */,
                   int64_t* raw /* rows x K, may be NULL */,
                   int32_t* counts /* (offsets[q_end] - offsets[q_begin]) x sub->n, may be NULL */,
                   int32_t* covered /* offsets[q_end] - offsets[q_begin], may be NULL */);
/* The same for the hits of a profile search: the slots, records, routes and consensus pool are aln_hits_pileup_profiles', the
 * alphabet is profiles->alphabet, and the checks are NULL profiles / templates / gap, then NULL hits / n_hits / out and K;
 * aln_score_profiles_vs_all's, in its order, with the consensus pool where aln_hits_align_profiles checks it; then purge,
 * max_identity, min_overlap, weights and w_max; n_hits, t and the end cells; the alphabet.  For profiles derived from residue
 * queries under an integral table every output is byte-identical to aln_hits_purge's on those residues. */
int aln_hits_purge_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus /* may be NULL */,
                            const aln_seqs* templates, const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                            const aln_hit* hits, const int32_t* n_hits, int32_t max_identity, int32_t min_overlap,
                            int32_t w_max, aln_hit_alignment* out, aln_hit_purge* purge, int32_t* weights, int64_t* raw,
                            int32_t* counts, int32_t* covered);
/* ---- next-round profile rows from search hits: purge, weights, counts and log-odds in one call, on the device ------------- */
/* The last step of a search round: the weighted counts become integer log-odds rows, the rows of the aln_qprofiles the next
 * round searches with.  These entries go from a round's hits to those rows in one call — purge, weights, counts and log-odds on
 * the device, no count row downloaded unless it is wanted.  The log-odds are defined in integers alone, so the rows are
 * reproducible bit for bit: they depend on neither chunking, grouping, route nor launch order, nor on any libm.
 * Parameters, n the call's alphabet size (sub->n, or profiles->n):
 *   bg[a]      integer background weights, each in 1..1024, B = sum_a bg[a] <= 1024;
 *   mix        n x n row-major, or NULL.  Every entry is >= 1 and every row sums to B.  mix[b][a] is the pseudo-count mass that
 *              letter a receives per observation of letter b: a target-frequency row of the substitution model scaled to B.
 *              NULL means mix[b][a] = bg[a], the background pseudo-counts of aln_amd.pssm_from_counts;
 *   beta       1..2^26, the pseudo-count mass in the units of the weights (a caller thinks of it relative to w_max);
 *   scale      one of 1, 2, 4, 8: scores are in 1/scale bits.
 * Per count row r take c[a] = counts[r][a], the weighted counts aln_hits_purge defines for the same hits, max_identity,
 * min_overlap and w_max, and N = sum_a c[a].  N is below 2^26: a slot adds at most one letter per position and the weights of
 * a row's 1024 slots sum to at most 1024 * 65535.
 * N == 0: row r of `rows` is the fallback row, copied bit for bit — sub->table[index(q[i]) * n + a] for position i of query q in
 * aln_hits_pssm, the profile's own row in aln_hits_pssm_profiles.
 * Otherwise, in unsigned 64-bit integers,
 *   g[a]   = sum_b c[b] * mix[b][a]                    (at most N * B)
 *   num[a] = c[a] * N * B + beta * g[a]
 *   den[a] = (N + beta) * N * bg[a]
 * Both are in [1, 2^63): c[a] * N * B < 2^26 * 2^26 * 2^10 and beta * g[a] <= 2^26 * 2^36, each at most 2^62; N + beta < 2^27,
 * so den[a] < 2^27 * 2^26 * 2^10; g[a] >= N >= 1 because every mix entry is >= 1.  num[a] / den[a] is the smoothed frequency
 * (c[a] + beta * g[a] / (N * B)) / (N + beta) over the background frequency bg[a] / B.
 * lg16(x, y) for x >= y >= 1:  e is the largest e >= 0 with y * 2^e <= x;  mant = floor(x * 2^32 / (y * 2^e)), which lies in
 * [2^32, 2^33);  lg16 = 16 * e + #{ m in 1..15 : T[m] <= mant }, with T[m] = floor(2^(32 + m/16)):
 *   0x10b5586cf 0x1172b83c7 0x12387a6e7 0x1306fe0a3 0x13dea64c1
 *   0x14bfdad53 0x15ab07dd4 0x16a09e667 0x17a11473e 0x18ace5422
 *   0x19c49182a 0x1ae89f995 0x1c199bdd8 0x1d5818dcf 0x1ea4afa2a
 * (four nested integer square roots of 2^(512 + m)).  lg16 is floor(16 * log2(x / y)) read off a 33-bit mantissa.
 * The score:  s = floor((lg16(num, den) * scale + 8) / 16) when num >= den,  s = -floor((lg16(den, num) * scale + 8) / 16)
 * otherwise; the row entry is (float)s.  |s| <= 8 * 37, so every derived row is integral.  This is rint(scale * log2(num / den))
 * wherever the ratio is further than 2^-32 (relative) from a rounding threshold; the thresholds are irrational, so the
 * real-valued rule has no ties.
 * The implementation uses neither 128-bit arithmetic nor a 64-bit division: mant - 2^32 is one subtraction (r = x - y * 2^e)
 * and 32 shift-and-subtract steps, in which 2r < 2 * y * 2^e <= 2x < 2^64 holds throughout (csrc/pssm_rule.h, one header for
 * host and device).
 * rows has the layout of counts with the entry's n: (offsets[q_end] - offsets[q_begin]) x n, the sentinel rows (first and last
 * row of every query) zeros; aln_hits_pssm_profiles' rows are the rows of an aln_qprofiles for the next round, unchanged.
 * out and rows are required.  purge, weights, raw, counts and covered may be NULL, each independently; every one that is given
 * is byte for byte what aln_hits_purge(_profiles) returns for the same arguments (max_identity = 101 purges nothing).  w_max is
 * always read.  A slot with a falsified local score gets ALN_E_ARG, does not contribute, and the call goes on.
 * Device side (csrc/search_pssm.hip): aln_hits_purge's stack and launches; the group's weighted count rows stay on the device
 * and one half-wave per count row (lane = letter) sums N by five xor-shuffles, makes g[a] from mix staged in LDS and the lanes'
 * c[b] broadcast across the half-wave, applies the rule per lane and stores the row coalesced.  Only the rows come down, and
 * the optional outputs that were asked for; the host copies the fallback rows in and zeroes the sentinel rows.
 * aln_hits_align_last_routes reports this call's slots as it does aln_hits_purge's.
 * Checks, in this order, nothing written when one fails: aln_hits_purge's up to and including w_max, without those on purge
 * and weights — NULL hits / n_hits / out, K outside 1..1024 (ALN_E_ARG); aln_score_all_vs_all's, in its order; max_identity
 * outside 1..101; min_overlap outside 0..100; w_max outside 1..65535 —; NULL par or rows; scale; beta; NULL bg, a bg[a] outside
 * 1..1024, B above 1024; a mix entry below 1, a mix row that does not sum to B (all ALN_E_ARG); every n_hits[r] in 0..K, every
 * used slot's t in [0, n_templates) and, local, its end cell in range; last, an alphabet that holds '.' or '-' (ALN_E_ARG).
 * q_begin == q_end: ALN_OK, nothing written.  Returns the lowest per-slot status, ALN_OK when all are 0. */
typedef struct { int32_t scale, beta; const int32_t* bg; const int32_t* mix; } aln_pssm_params;
int aln_hits_pssm(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                  const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                  const aln_hit* hits, const int32_t* n_hits,
                  int32_t max_identity, int32_t min_overlap, int32_t w_max, const aln_pssm_params* par,
                  aln_hit_alignment* out /* rows x K */,
                  float* rows /* (offsets[q_end] - offsets[q_begin]) x sub->n */,
                  aln_hit_purge* purge /* rows x K, may be NULL */, int32_t* weights /* rows x K, may be NULL */,
                  int64_t* raw /* rows x K, may be NULL */,
                  int32_t* counts /* (offsets[q_end] - offsets[q_begin]) x sub->n, may be NULL */,
                  int32_t* covered /* offsets[q_end] - offsets[q_begin], may be NULL */);
/* The same for the hits of a profile search: slots, records, routes, the consensus pool and the checks in front are
 * aln_hits_purge_profiles', n and the alphabet are profiles', and a row without counts keeps the profile's own row.  For
 * profiles derived from residue queries under an integral table every output is byte-identical to aln_hits_pssm's on those
 * residues. */
int aln_hits_pssm_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus /* may be NULL */,
                           const aln_seqs* templates, const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                           const aln_hit* hits, const int32_t* n_hits, int32_t max_identity, int32_t min_overlap,
                           int32_t w_max, const aln_pssm_params* par, aln_hit_alignment* out, float* rows,
                           aln_hit_purge* purge, int32_t* weights, int64_t* raw, int32_t* counts, int32_t* covered);
/* The score of the rule above for one (num, den): needs no GPU, like aln_gapped_strings.  0 for num == 0, den == 0, a value of
 * 2^63 or more, or a scale other than 1, 2, 4, 8. */
int32_t aln_pssm_entry(uint64_t num, uint64_t den, int32_t scale);
/* Several NON-INTERSECTING local alignments per hit (the second, third .. HSP of a hit; Waterman-Eggert's declumping restated on
 * the reference's recurrence).  ALN_LOCAL only.  For one pair — query of Q residues, template of T, sentinels counted — under a
 * table and constant affine gaps:
 *   round 0      is Optimal's alignment of the pair: exactly what aln_hits_align returns for the hit aln_search_topk reports.
 *   round a >= 1 is Optimal's alignment (find_max + the local walk, optimal.h:79-124) of the DPMatrix built from a CHANGED
 *                similarity plane: every aligned pair (i, j) of the rounds 0 .. a-1 holds a value so negative that the cell
 *                clips to 0.  An aligned pair is a list entry with 1 <= i <= Q-2 and 1 <= j <= T-2; the closing (Q-1, T-1) and the
 *                origin (0, 0) are none.  Any value <= -(score of round 0) does — masking only lowers cells, so no later cell
 *                exceeds that score — and the result does not depend on which is used.  Equivalently: D = 0 at those cells and
 *                everything else follows the reference's recurrence and candidate order.  A gap may jump over a forbidden
 *                cell; as a gap source a forbidden cell is an ordinary zero cell.
 *   reporting    a round is reported when its score is >= min_score (-INFINITY: no bound) and, for a >= 1, also > 0.  Round 0
 *                is reported even with score 0 (the seed-cell list), as aln_hits_align does.  The first round that is not
 *                reported ends the hit; at most max_alignments (N, 1..16) rounds are reported.
 * Consequences: the reported alignments of a hit share no aligned pair; their scores never increase from one round to the next;
 * every reported value is, bit for bit, what aln_batch_create over the pair + aln_batch_dp(ALN_SIM_MATRIX with the round's plane,
 * gap, ALN_FWD, ALN_DP_AUTO) + aln_batch_optimal / aln_batch_optimal_strings give.
 * The hit layout and which slots are used are aln_hits_align's, but only a slot's .t is read: end cell and score are recomputed,
 * so any (row, template) list will do.  Slot s = r * K + k, round a: the record is out[s * N + a], the pair list at
 * pairs + (s * N + a) * pair_stride * 2, the lines at tlines / qlines + (s * N + a) * line_stride, their length lengths[s * N + a];
 * "not wanted" (NULL pairs, the line group) as in aln_hits_align.  n_found[s] is the number of reported rounds (0 for an unused
 * slot); records >= n_found[s] hold { 0, 0, 0.0f, 0.0f }, empty lines and length 0.  A list longer than pair_stride or a line
 * that does not fit line_stride gives THAT alignment ALN_E_OVERFLOW as in aln_hits_align; an overflowing list still forbids all
 * of its cells — it is truncated for the caller only.
 * Routes: integer table and gaps inside aln_score_all_vs_all's 2^23 bound, Q >= 3, T >= 3 and a template of up to 1792 columns —
 * one wave per hit runs all rounds in one launch (csrc/search_align_multi.hip): per round one register-resident sweep of rows
 * 1 .. Q-2 that honours a 1-bit-per-cell plane of forbidden cells and yields both the end cell and the 1 B/cell strip, then the
 * walk back, which also sets the bits.  Everything else — longer templates, fractional tables or gaps, values beyond the bound,
 * pairs without an interior — goes through resident batches inside the call, round by round, on planes expanded and masked on
 * the host (~12 GB of planes at a time), so the call accepts what aln_search_topk accepts.  aln_hits_align_last_routes reports
 * this call's slots too.  No hint of its own: chunks obey "align_chunk_hits" and 1 GiB each of strips, masks, lists and lines.
 * Checks, in this order, nothing written when one fails: NULL n_found, max_alignments outside 1..16 and aln_hits_align's first
 * group (ALN_E_ARG); aln_score_all_vs_all's, in its order; an align type other than ALN_LOCAL (ALN_E_ARG); every n_hits[r] in
 * 0..K and every used slot's t in [0, n_templates) (ALN_E_ARG).  q_begin == q_end: ALN_OK, nothing written.  Returns when every
 * output is complete: the lowest per-alignment status, ALN_OK when all are 0. */
int aln_hits_align_multi(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub,
                         const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                         const aln_hit* hits, const int32_t* n_hits,
                         int32_t max_alignments /* N, 1..16 */, float min_score /* -INFINITY: none */,
                         int32_t* n_found /* rows x K */, aln_hit_alignment* out /* rows x K x N */,
                         int32_t* pairs, int32_t pair_stride, char* tlines, char* qlines, int32_t line_stride, int32_t* lengths);
/* aln_hits_align_multi for the hits of a profile search (aln_search_topk_profiles, or any (row, template) list in its layout).
 * The round rule and the reporting rule, that only a slot's .t is read, the s * N + a layout of out / pairs / lines / lengths,
 * n_found, the padding records, ALN_E_OVERFLOW per alignment (a truncated list still forbids all of its cells), the return value
 * and q_begin == q_end (ALN_OK, nothing written) are those of aln_hits_align_multi, word for word.  ALN_LOCAL only.
 * The pair's plane is the one aln_score_profiles_vs_all defines; every reported value is what aln_batch_create over (the query
 * letters of the row, the template) + aln_batch_dp(ALN_SIM_MATRIX with the round's masked plane, gap, ALN_FWD, ALN_DP_AUTO) +
 * aln_batch_optimal / aln_batch_optimal_strings give, bit for bit.
 * Query letters: `consensus` exactly as in aln_hits_align_profiles — an ordinary pool with the profiles' n_seqs and offsets,
 * never scored, not checked against the alphabet; NULL: the placeholder pool ('^', alphabet[0] .., '$').  The identity counts
 * equal CHARACTERS of the two pools over the list's entries (then - 2).
 * Routes: integer rows (of the interior rows of the whole pool) and gaps inside aln_score_all_vs_all's 2^23 bound, Q >= 3, T >= 3
 * and a template of up to 1792 columns — one wave per hit runs all rounds in one launch (csrc/search_align_multi.hip, the kernel
 * of aln_hits_align_multi instantiated for the profile side): the rows staged from HBM into LDS 8 at a time, per round one
 * sweep of rows 1 .. Q-2 over the 1-bit-per-cell plane of forbidden cells, the 1 B/cell strip, the walk.  Everything else —
 * fractional rows or gaps, values beyond the bound, longer templates, pairs without an interior — goes through resident batches
 * inside the call, round by round, EVERY round (round 0 included) on planes expanded on the host, later rounds masked there
 * (~12 GB of planes at a time).  The device rows of [q_begin, q_end) are uploaded once when they fit 1 GiB, else with every
 * chunk of hits (hint "align_rows_per_chunk"); chunks obey "align_chunk_hits" and 1 GiB each of strips, masks, lists and lines.
 * No hint of its own.  aln_hits_align_last_routes reports this call's slots too.
 * Checks, in this order, nothing written when one fails: NULL n_found, max_alignments outside 1..16 and
 * aln_hits_align_profiles' first group (ALN_E_ARG); aln_score_profiles_vs_all's, in its order, with the consensus pool where
 * aln_hits_align_profiles checks it; an align type other than ALN_LOCAL (ALN_E_ARG); every n_hits[r] in 0..K; every used slot's
 * t in [0, n_templates) (ALN_E_ARG). */
int aln_hits_align_multi_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus /* may be NULL */,
                                  const aln_seqs* templates, const aln_gap* gap, int32_t q_begin, int32_t q_end, int32_t K,
                                  const aln_hit* hits, const int32_t* n_hits,
                                  int32_t max_alignments /* N, 1..16 */, float min_score /* -INFINITY: none */,
                                  int32_t* n_found /* rows x K */, aln_hit_alignment* out /* rows x K x N */,
                                  int32_t* pairs, int32_t pair_stride, char* tlines, char* qlines, int32_t line_stride, int32_t* lengths);
/* out[0]: the used slots the last aln_hits_align / aln_hits_align_profiles / aln_hits_align_multi / aln_hits_align_multi_profiles / aln_hits_column_counts(_profiles) / aln_hits_purge(_profiles) / aln_hits_weights(_profiles) / aln_hits_pileup(_profiles) call on this context sent through a fused kernel,
 * out[1]: through resident batches; { 0, 0 } before any call and after a call that failed its checks.  NULL argument: ALN_E_ARG.
 * aln_hits_align_profiles_gaps and aln_hits_column_counts_profiles_gaps report here too: out[1] counts the slots the host filed
 * (pairs without an interior; those entries have no batch route). */
int aln_hits_align_last_routes(const aln_ctx* ctx, int64_t out[2]);

/* ---- multi-GPU: a length-sorted deal of independent units + ONE collective (RCCL all-gather of scores) ----------- */
/* The reference is one thread, one DPMatrix at a time; pairs are independent (dpmatrix.h:104-111), so ranks own disjoint pair
 * lists and the only exchange is the final gather of the per-pair scores (BASELINE north_star). */
typedef struct aln_comm aln_comm;
#define ALN_COMM_ID_BYTES 128   /* sizeof(ncclUniqueId) */
/* Length-sorted deal: units sorted by work[u] (= Q*T of a pair, or the residues of a query row) descending, ties by index, dealt
 * over n_ranks in boustrophedon order (0..n-1, n-1..0, ...).  owner[u] = rank; slot[u] (may be NULL) = position of u in that
 * rank's local list, which keeps the sorted order (long units first).  Host arithmetic only. */
int aln_deal_units(const int64_t* work, int64_t n_units, int32_t n_ranks, int32_t* owner, int32_t* slot);
/* One process per GPU: rank 0 obtains an id, ships its ALN_COMM_ID_BYTES bytes to the other processes by the job's own
 * transport, and every process calls aln_comm_create(&its_ctx, 1, id, n_ranks, its_rank, ...).
 * One process driving n GPUs: aln_comm_create(ctxs, n, NULL, n, 0, ...) — or aln_ctx_create_multi, which also makes the contexts.
 * librccl.so is dlopen()ed on first use.  Collective calls run on each context's stream. */
int aln_comm_unique_id(void* id_out);
int aln_comm_create(aln_ctx* const* ctxs, int32_t n_local, const void* id, int32_t n_ranks, int32_t first_rank, aln_comm** out);
int aln_ctx_create_multi(const int32_t* device_ids, int32_t n, aln_ctx** ctxs_out, aln_comm** comm_out);
void aln_comm_destroy(aln_comm* comm);
int32_t aln_comm_n_ranks(const aln_comm* comm);
const char* aln_comm_last_error(const aln_comm* comm);
/* All ranks call it together.  Local rank k of this process contributes n_local[k] (<= n_max, the same n_max on every rank)
 * scores; global_index[k][e] is the position of local score e in the job's pair list.  On return global_out[0..n_total) holds
 * every contributed score on every rank.  One ncclAllGather of (index, score) records over xGMI. */
int aln_gather_scores(aln_comm* comm, const float* const* local_scores, const int32_t* const* global_index,
                      const int32_t* n_local, int32_t n_max, float* global_out, int64_t n_total);
/* The same collective for scores that are still on the device, split like aln_batch_optimal_enqueue / _collect.  Local rank k
 * contributes the Optimal scores of the first n_local[k] pairs of batches[k] (a batch of context k of `comm`; NULL when
 * n_local[k] == 0), whose current build must have had Optimal launched (aln_batch_optimal*, ..._enqueue; else ALN_E_STATE).
 * _enqueue launches, on each context's stream, a pack kernel over the resident results, the ncclAllGather, a scatter kernel and
 * the copy of the dense result into one of two pinned slots (ALN_E_STATE when both are waiting), and returns at once: it never
 * waits for the device.  global_index is read during the call (an index outside [0, n_total) is ALN_E_ARG, nothing enqueued).
 * _collect waits for the OLDEST slot only and writes global_out[i] for every contributed i (the others keep their value);
 * ALN_E_ARG if another process's rank sent an index >= n_total, ALN_E_STATE if n_total is not that slot's or nothing is pending.
 * `reevaluate; optimal_enqueue; gather_resident_enqueue; collect(previous)` keeps the cross-rank wait off the launching thread. */
int aln_gather_resident_enqueue(aln_comm* comm, aln_batch* const* batches, const int32_t* const* global_index,
                                const int32_t* n_local, int32_t n_max, int64_t n_total);
int aln_gather_resident_collect(aln_comm* comm, float* global_out, int64_t n_total);

/* ---- host-side helpers with no device work (alignment.h / gstrings.h) -------------------- */
/* AlignedPairList::calcIdentity (alignment.h:856-865). qstr/tstr include sentinels. */
float aln_identity(const char* qstr, int32_t Q, const char* tstr, int32_t T,
                   const int32_t* pairs, int32_t n_pairs);
/* SequenceGaps (gstrings.h:84-164, gstrings.cpp:17-29): gapped template line and one gapped query line
 * per alignment.  aln_gapped_length() gives the length of every line (without NUL).  qlines may be NULL
 * (template line only); tline may be NULL. */
int32_t aln_gapped_length(int32_t T, const aln_alignment* alis, int32_t n_alis, const int32_t* pairs);
int aln_gapped_strings(const char* qstr, int32_t Q, const char* tstr, int32_t T,
                       const aln_alignment* alis, int32_t n_alis, const int32_t* pairs,
                       char* tline, char* qlines, int32_t stride);

/* Hmap2Eval::pre_calculate (hmap2_eval.cpp:17-25): per template residue gap coefficients
 * t_gap_init = gap_init * Pi, t_gap_extn = gap_extn * Pi, Pi = exp(beta * (1 - 1.25 * p_coil)), p_coil = sse[3*i+2].
 * Host arithmetic with the host libm, like the reference; feeds aln_gap.t_gap_init / t_gap_extn. */
int aln_hmap2_gap_arrays(const float* t_sse, int64_t n, float gap_init, float gap_extn, float beta,
                         float* t_gap_init, float* t_gap_extn);

/* ---- measurement hooks ---------------------------------------------------------------------- */
/* Context hint "exact_debug" = 1: the exact-order tiled kernel (config 3) counts, per wave, the far candidate chunks it tested
 * against their bounds and the ones it could skip: out4 = {deletion chunks tested, skipped, insertion chunks tested, skipped}.
 * "exact_debug" = 2: the same four words hold how long the kernel's waves ran instead — {sum, longest, bitwise NOT of the
 * shortest, number of waves}, in units of 1024 s_memtime ticks — and the library lists the slowest pairs on stderr (that is how
 * a degenerate all-NaN pair was found to bound a 1024-pair launch).
 * (No reference counterpart: the reference scans every candidate, dpmatrix.h:453-480.) */
int aln_batch_last_exact_stats(const aln_batch* b, uint64_t* out4);
/* Milliseconds the device spent in the DP kernel(s) of the last aln_batch_dp, from HIP events recorded on
 * the ctx stream around those launches; synchronises the stream. */
int aln_batch_last_dp_ms(aln_batch* b, float* ms);
/* The same for up to max_n of the latest builds (ms[0] = the latest; the library keeps 64 event pairs), so that a pipelined
 * caller can read the kernel times after its loop instead of synchronising inside it.  Returns how many it wrote, -1 on error. */
int aln_batch_dp_ms_history(aln_batch* b, float* ms, int32_t max_n);
/* Bytes one DP launch MUST write to HBM with the plane layout the last aln_batch_dp chose: per cell of the Q x T matrices
 * the score element (fp32, or uint16 in local tagged builds) + the pointer element (32-bit, or 16-bit tagged words):
 * 8, 6 or 4 B/cell.  This is what a roofline fraction is computed from.  _contract_bytes is SURVEY.md 8(d)'s figure for the
 * reference's layout, 8 B per cell (fp32 score + 32-bit packed pointer), whatever was chosen; _plane_bytes_per_cell the factor.
 * While the resident planes are those of a lean aln_batch_reevaluate the factor is 2 (marked pointer words only). */
int64_t aln_batch_dp_algorithmic_bytes(const aln_batch* b);
int64_t aln_batch_dp_contract_bytes(const aln_batch* b);
int32_t aln_batch_plane_bytes_per_cell(const aln_batch* b);
int64_t aln_batch_cells(const aln_batch* b);      /* sum over pairs of |q|*|t| = (Q-2)(T-2) */

#ifdef __cplusplus
}
#endif
#endif /* ALN_HIP_H */
