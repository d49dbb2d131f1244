"""aln_amd — thin ctypes binding of libalnhip.so (include/aln_hip.h), used by tests/ and bench.py.

The product is the C-ABI shared library built from csrc/*.hip for gfx950; this module only loads it
and marshals numpy arrays.  There is NO CPU fallback: if the library is missing or there is no GPU the
calls fail loudly.
"""
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_DIR, "libalnhip.so")

GLOBAL_LOCAL, GLOBAL, LOCAL_GLOBAL, LOCAL, SEMI_LOCAL = 0, 1, 2, 3, 4
FWD, REV = 1, 2
GAP_AFFINE_CONST, GAP_AFFINE_TPOS_MIN, GAP_DEL_TABLE_INS_TPOS, GAP_TABLES = 0, 1, 2, 3
SIM_SUBMATRIX, SIM_MATRIX, SIM_HMAP2 = 0, 1, 2
DP_AUTO, DP_EXACT, DP_FAST = 0, 1, 2
ENUM_CW, ENUM_UCW, ENUM_KSCW, ENUM_CRCW = 0, 1, 2, 3
_ENUM = {"cw": ENUM_CW, "ucw": ENUM_UCW, "kscw": ENUM_KSCW, "crcw": ENUM_CRCW}

E_BOUNDS, E_GAPSTYLE, E_STARTPAIR, E_RESIDUE, E_ARG, E_HIP, E_NOMEM, E_TOO_LONG, E_NOT_INTEGRAL, E_STATE, E_OVERFLOW = range(-1, -12, -1)

_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)


class AlnSeqs(C.Structure):
    _fields_ = [("n_seqs", C.c_int32), ("offsets", _lp), ("residues", C.c_char_p)]


class AlnSubmatrix(C.Structure):
    _fields_ = [("n", C.c_int32), ("alphabet", C.c_char_p), ("table", _fp)]


class AlnQProfiles(C.Structure):
    _fields_ = [("n_seqs", C.c_int32), ("offsets", _lp), ("rows", _fp), ("n", C.c_int32), ("alphabet", C.c_char_p)]


class AlnQGaps(C.Structure):
    _fields_ = [("del_init", _fp), ("del_extn", _fp), ("ins_init", _fp), ("ins_extn", _fp)]


class AlnProfiles(C.Structure):
    _fields_ = [("aa", _fp), ("sse", _fp), ("conf", _fp)]


class AlnGap(C.Structure):
    _fields_ = [("model", C.c_int32), ("align_type", C.c_int32), ("gap_init", C.c_float), ("gap_extn", C.c_float),
                ("t_gap_init", _fp), ("t_gap_extn", _fp), ("dp_local", C.c_int32), ("t_gap_cn", _fp), ("del_table", _fp),
                ("del_table_off", _lp), ("ins_tables", _fp), ("ins_table_off", _lp)]


class AlnSim(C.Structure):
    _fields_ = [("kind", C.c_int32), ("sub", AlnSubmatrix), ("planes", _fp), ("plane_off", _lp),
                ("q_prof", AlnProfiles), ("t_prof", AlnProfiles), ("alpha", C.c_float), ("zero_shift", C.c_float),
                ("normalize", C.c_int32)]


class AlnNoa(C.Structure):
    _fields_ = [("kind", C.c_int32), ("number_suboptimal", C.c_int32), ("delta_ratio", C.c_float), ("user_limit", C.c_uint32),
                ("n_existing", C.c_int32), ("existing_scores", _fp), ("k_limit", C.c_uint32), ("sort_limit", C.c_uint32),
                ("max_overlap", C.c_float)]


class AlnAlignment(C.Structure):
    _fields_ = [("score", C.c_float), ("identity", C.c_float), ("uid", C.c_int32), ("n_pairs", C.c_int32), ("pair_off", C.c_int64)]


class AlnHit(C.Structure):
    _fields_ = [("t", C.c_int32), ("score", C.c_float), ("q_end", C.c_int32), ("t_end", C.c_int32)]


HIT_DTYPE = np.dtype([("t", np.int32), ("score", np.float32), ("q_end", np.int32), ("t_end", np.int32)])


class AlnHitStats(C.Structure):
    _fields_ = [("sum", C.c_int64), ("sumsq", C.c_int64), ("n", C.c_int32), ("z", C.c_float)]


HIT_STATS_DTYPE = np.dtype([("sum", np.int64), ("sumsq", np.int64), ("n", np.int32), ("z", np.float32)])

class AlnHitAlignment(C.Structure):
    _fields_ = [("n_pairs", C.c_int32), ("status", C.c_int32), ("score", C.c_float), ("identity", C.c_float)]


HIT_ALIGNMENT_DTYPE = np.dtype([("n_pairs", np.int32), ("status", np.int32), ("score", np.float32), ("identity", np.float32)])


class AlnHitSpan(C.Structure):
    _fields_ = [("q_lo", C.c_int32), ("q_hi", C.c_int32), ("t_lo", C.c_int32), ("t_hi", C.c_int32)]


HIT_SPAN_DTYPE = np.dtype([("q_lo", np.int32), ("q_hi", np.int32), ("t_lo", np.int32), ("t_hi", np.int32)])


class AlnHitPurge(C.Structure):
    _fields_ = [("keeper", C.c_int32), ("same", C.c_int32), ("overlap", C.c_int32), ("letters", C.c_int32)]


HIT_PURGE_DTYPE = np.dtype([("keeper", np.int32), ("same", np.int32), ("overlap", np.int32), ("letters", np.int32)])


class AlnPssmParams(C.Structure):
    """aln_pssm_params.  make() builds one from Python values and keeps the arrays its pointers were made from."""
    _fields_ = [("scale", C.c_int32), ("beta", C.c_int32), ("bg", _ip), ("mix", _ip)]

    @classmethod
    def make(cls, bg, beta, scale=2, mix=None):
        """bg: n integer background weights (1..1024 each, sum B <= 1024); beta: 1..2^26; scale: 1, 2, 4 or 8; mix: None
        (background pseudo-counts) or n x n integers >= 1 whose rows sum to B"""
        p = cls()
        p.scale, p.beta = int(scale), int(beta)
        p.bg_array = np.ascontiguousarray(bg, dtype=np.int32).reshape(-1)
        p.bg = p.bg_array.ctypes.data_as(_ip)
        p.mix_array = None
        if mix is not None:
            p.mix_array = np.ascontiguousarray(mix, dtype=np.int32).reshape(len(p.bg_array), len(p.bg_array))
            p.mix = p.mix_array.ctypes.data_as(_ip)
        return p

EXPORTS = [
    "aln_ctx_create", "aln_ctx_destroy", "aln_error_string", "aln_last_error", "aln_ctx_synchronize", "aln_has_gfx950",
    "aln_batch_create", "aln_batch_destroy", "aln_batch_n_pairs", "aln_batch_device_bytes", "aln_batch_dp",
    "aln_batch_reevaluate", "aln_batch_dp_kernel_name", "aln_batch_dp_sub", "aln_batch_get_cells", "aln_batch_get_sim",
    "aln_batch_get_corner_scores", "aln_batch_optimal", "aln_batch_optimal_enqueue", "aln_batch_optimal_collect", "aln_batch_optimal_subali", "aln_batch_enumerate", "aln_batch_enumerate_all", "aln_batch_last_enum_ms", "aln_batch_last_enum_usage", "aln_batch_last_enum_tasks", "aln_identity",
    "aln_gapped_length", "aln_gapped_strings", "aln_hmap2_gap_arrays", "aln_score_all_vs_all", "aln_batch_last_dp_ms", "aln_batch_dp_ms_history", "aln_batch_dp_algorithmic_bytes", "aln_batch_cells",
    "aln_batch_optimal_strings", "aln_batch_optimal_strings_enqueue", "aln_batch_optimal_strings_collect", "aln_batch_last_exact_stats", "aln_batch_set_gap", "aln_ctx_set_hint", "aln_ctx_get_hint", "aln_batch_dp_contract_bytes", "aln_batch_plane_bytes_per_cell",
    "aln_deal_units", "aln_comm_unique_id", "aln_comm_create", "aln_ctx_create_multi", "aln_comm_destroy", "aln_comm_n_ranks",
    "aln_comm_last_error", "aln_gather_scores", "aln_gather_resident_enqueue", "aln_gather_resident_collect", "aln_search_topk",
    "aln_hits_zscores", "aln_hits_align", "aln_hits_align_last_routes", "aln_score_profiles_vs_all", "aln_search_topk_profiles",
    "aln_hits_align_profiles", "aln_hits_zscores_profiles", "aln_hits_align_multi",
    "aln_hits_align_multi_profiles", "aln_hits_column_counts", "aln_hits_column_counts_profiles",
    "aln_hits_pileup", "aln_hits_pileup_profiles", "aln_hits_weights", "aln_hits_weights_profiles",
    "aln_hits_purge", "aln_hits_purge_profiles", "aln_hits_pssm", "aln_hits_pssm_profiles", "aln_pssm_entry",
    "aln_score_profiles_gaps_vs_all", "aln_search_topk_profiles_gaps",
    "aln_hits_align_profiles_gaps", "aln_hits_column_counts_profiles_gaps",
]
COMM_ID_BYTES = 128

_LIB = None


class AlnError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "%s (aln status %d)" % (msg, code))
        self.code = code


def build_library():
    subprocess.check_call(["make", "-s", "-C", PKG_DIR, "-j8"])


def lib():
    """Load libalnhip.so (never a fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libalnhip.so not built: run `make -C alignment-algos_amd` (hipcc --offload-arch=gfx950)")
        L = C.CDLL(LIB_PATH)
        L.aln_error_string.restype = C.c_char_p
        L.aln_last_error.restype = C.c_char_p
        L.aln_last_error.argtypes = [C.c_void_p]
        L.aln_batch_dp_kernel_name.restype = C.c_char_p
        L.aln_batch_dp_kernel_name.argtypes = [C.c_void_p]
        L.aln_identity.restype = C.c_float
        for f in ("aln_batch_device_bytes", "aln_batch_dp_algorithmic_bytes", "aln_batch_dp_contract_bytes", "aln_batch_cells"):
            getattr(L, f).restype = C.c_int64
            getattr(L, f).argtypes = [C.c_void_p]
        L.aln_ctx_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        L.aln_ctx_destroy.argtypes = [C.c_void_p]
        L.aln_ctx_synchronize.argtypes = [C.c_void_p]
        L.aln_batch_create.argtypes = [C.c_void_p, C.POINTER(AlnSeqs), C.POINTER(AlnSeqs), C.c_int32, _ip, _ip, C.c_int32, C.POINTER(C.c_void_p)]
        L.aln_batch_destroy.argtypes = [C.c_void_p]
        L.aln_batch_n_pairs.argtypes = [C.c_void_p]
        L.aln_batch_dp.argtypes = [C.c_void_p, C.POINTER(AlnSim), C.POINTER(AlnGap), C.c_int32, C.c_int32, C.c_int32]
        L.aln_batch_reevaluate.argtypes = [C.c_void_p]
        L.aln_batch_set_gap.argtypes = [C.c_void_p, C.POINTER(AlnGap)]
        L.aln_batch_dp_sub.argtypes = [C.c_void_p, C.POINTER(AlnSim), C.POINTER(AlnGap), C.c_int32, _ip]
        L.aln_batch_get_cells.argtypes = [C.c_void_p, C.c_int32, _fp, _ip, _ip]
        L.aln_batch_get_sim.argtypes = [C.c_void_p, C.c_int32, _fp]
        L.aln_batch_get_corner_scores.argtypes = [C.c_void_p, _fp]
        L.aln_batch_optimal.argtypes = [C.c_void_p, _fp, _ip, _ip, C.c_int32, _ip]
        L.aln_batch_optimal_enqueue.argtypes = [C.c_void_p]
        L.aln_batch_optimal_collect.argtypes = [C.c_void_p, _fp, _ip, _ip]
        L.aln_batch_optimal_subali.argtypes = [C.c_void_p, _fp, _ip, _ip, C.c_int32, _ip]
        L.aln_batch_enumerate.argtypes = [C.c_void_p, C.c_int32, C.POINTER(AlnNoa), C.POINTER(C.c_uint8), C.POINTER(AlnAlignment),
                                          C.c_int32, _ip, C.c_int64, _ip]
        L.aln_batch_enumerate_all.argtypes = [C.c_void_p, C.POINTER(AlnNoa), C.POINTER(C.c_uint8), C.c_int32, C.c_uint32, C.c_uint32,
                                              C.c_int32, _ip, _fp, _ip, _ip, C.c_int32, _ip]
        L.aln_batch_last_enum_ms.argtypes = [C.c_void_p, _fp, _fp]
        L.aln_batch_last_enum_usage.argtypes = [C.c_void_p, _ip, _ip]
        L.aln_batch_last_enum_tasks.argtypes = [C.c_void_p, _ip]
        L.aln_identity.argtypes = [C.c_char_p, C.c_int32, C.c_char_p, C.c_int32, _ip, C.c_int32]
        L.aln_gapped_length.argtypes = [C.c_int32, C.POINTER(AlnAlignment), C.c_int32, _ip]
        L.aln_gapped_strings.argtypes = [C.c_char_p, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(AlnAlignment), C.c_int32, _ip,
                                         C.c_char_p, C.c_char_p, C.c_int32]
        L.aln_batch_last_dp_ms.argtypes = [C.c_void_p, _fp]
        L.aln_batch_dp_ms_history.argtypes = [C.c_void_p, _fp, C.c_int32]
        L.aln_score_all_vs_all.argtypes = [C.c_void_p, C.POINTER(AlnSeqs), C.POINTER(AlnSeqs), C.POINTER(AlnSubmatrix), C.POINTER(AlnGap),
                                           C.c_int32, C.c_int32, _fp]
        L.aln_search_topk.argtypes = [C.c_void_p, C.POINTER(AlnSeqs), C.POINTER(AlnSeqs), C.POINTER(AlnSubmatrix), C.POINTER(AlnGap),
                                      C.c_int32, C.c_int32, C.c_int32, C.c_float, C.POINTER(AlnHit), _ip]
        L.aln_score_profiles_vs_all.argtypes = [C.c_void_p, C.POINTER(AlnQProfiles), C.POINTER(AlnSeqs), C.POINTER(AlnGap), C.c_int32, C.c_int32,
                                                _fp]
        L.aln_search_topk_profiles.argtypes = [C.c_void_p, C.POINTER(AlnQProfiles), C.POINTER(AlnSeqs), C.POINTER(AlnGap), C.c_int32, C.c_int32,
                                               C.c_int32, C.c_float, C.POINTER(AlnHit), _ip]
        L.aln_score_profiles_gaps_vs_all.argtypes = [C.c_void_p, C.POINTER(AlnQProfiles), C.POINTER(AlnQGaps), C.POINTER(AlnSeqs), C.c_int32,
                                                     C.c_int32, C.c_int32, _fp]
        L.aln_search_topk_profiles_gaps.argtypes = [C.c_void_p, C.POINTER(AlnQProfiles), C.POINTER(AlnQGaps), C.POINTER(AlnSeqs), C.c_int32,
                                                    C.c_int32, C.c_int32, C.c_int32, C.c_float, C.POINTER(AlnHit), _ip]
        L.aln_hits_zscores.argtypes = [C.c_void_p, C.POINTER(AlnSeqs), C.POINTER(AlnSeqs), C.POINTER(AlnSubmatrix), C.POINTER(AlnGap),
                                       C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlnHit), _ip, C.c_int32, C.c_uint32,
                                       C.POINTER(AlnHitStats)]
        L.aln_hits_zscores_profiles.argtypes = [C.c_void_p, C.POINTER(AlnQProfiles), C.POINTER(AlnSeqs), C.POINTER(AlnGap), C.c_int32,
                                                C.c_int32, C.c_int32, C.POINTER(AlnHit), _ip, C.c_int32, C.c_uint32,
                                                C.POINTER(AlnHitStats)]
        L.aln_hits_align.argtypes = [C.c_void_p, C.POINTER(AlnSeqs), C.POINTER(AlnSeqs), C.POINTER(AlnSubmatrix), C.POINTER(AlnGap),
                                     C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlnHit), _ip, C.POINTER(AlnHitAlignment), _ip, C.c_int32,
                                     C.c_char_p, C.c_char_p, C.c_int32, _ip]
        L.aln_hits_align_profiles.argtypes = [C.c_void_p, C.POINTER(AlnQProfiles), C.POINTER(AlnSeqs), C.POINTER(AlnSeqs), C.POINTER(AlnGap),
                                              C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlnHit), _ip, C.POINTER(AlnHitAlignment), _ip,
                                              C.c_int32, C.c_char_p, C.c_char_p, C.c_int32, _ip]
        L.aln_hits_align_multi.argtypes = [C.c_void_p, C.POINTER(AlnSeqs), C.POINTER(AlnSeqs), C.POINTER(AlnSubmatrix), C.POINTER(AlnGap),
                                           C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlnHit), _ip, C.c_int32, C.c_float, _ip,
                                           C.POINTER(AlnHitAlignment), _ip, C.c_int32, C.c_char_p, C.c_char_p, C.c_int32, _ip]
        L.aln_hits_align_multi_profiles.argtypes = [C.c_void_p, C.POINTER(AlnQProfiles), C.POINTER(AlnSeqs), C.POINTER(AlnSeqs),
                                                    C.POINTER(AlnGap), C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlnHit), _ip, C.c_int32,
                                                    C.c_float, _ip, C.POINTER(AlnHitAlignment), _ip, C.c_int32, C.c_char_p, C.c_char_p,
                                                    C.c_int32, _ip]
        L.aln_hits_column_counts.argtypes = [C.c_void_p, C.POINTER(AlnSeqs), C.POINTER(AlnSeqs), C.POINTER(AlnSubmatrix), C.POINTER(AlnGap),
                                             C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlnHit), _ip, _ip, C.POINTER(AlnHitAlignment), _ip,
                                             _ip]
        L.aln_hits_column_counts_profiles.argtypes = [C.c_void_p, C.POINTER(AlnQProfiles), C.POINTER(AlnSeqs), C.POINTER(AlnSeqs),
                                                      C.POINTER(AlnGap), C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlnHit), _ip, _ip,
                                                      C.POINTER(AlnHitAlignment), _ip, _ip]
        L.aln_hits_align_profiles_gaps.argtypes = [C.c_void_p, C.POINTER(AlnQProfiles), C.POINTER(AlnQGaps), C.POINTER(AlnSeqs),
                                                   C.POINTER(AlnSeqs), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlnHit), _ip,
                                                   C.POINTER(AlnHitAlignment), _ip, C.c_int32, C.c_char_p, C.c_char_p, C.c_int32, _ip]
        L.aln_hits_column_counts_profiles_gaps.argtypes = [C.c_void_p, C.POINTER(AlnQProfiles), C.POINTER(AlnQGaps), C.POINTER(AlnSeqs),
                                                           C.POINTER(AlnSeqs), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                           C.POINTER(AlnHit), _ip, _ip, C.POINTER(AlnHitAlignment), _ip, _ip]
        L.aln_hits_pileup.argtypes = [C.c_void_p, C.POINTER(AlnSeqs), C.POINTER(AlnSeqs), C.POINTER(AlnSubmatrix), C.POINTER(AlnGap),
                                      C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlnHit), _ip, C.POINTER(AlnHitAlignment),
                                      C.POINTER(AlnHitSpan), C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.c_int32]
        L.aln_hits_pileup_profiles.argtypes = [C.c_void_p, C.POINTER(AlnQProfiles), C.POINTER(AlnSeqs), C.POINTER(AlnSeqs),
                                               C.POINTER(AlnGap), C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlnHit), _ip,
                                               C.POINTER(AlnHitAlignment), C.POINTER(AlnHitSpan), C.POINTER(C.c_uint8),
                                               C.POINTER(C.c_uint16), C.c_int32]
        L.aln_hits_weights.argtypes = [C.c_void_p, C.POINTER(AlnSeqs), C.POINTER(AlnSeqs), C.POINTER(AlnSubmatrix), C.POINTER(AlnGap),
                                       C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlnHit), _ip, C.c_int32, C.POINTER(AlnHitAlignment),
                                       _ip, _lp, _ip, _ip]
        L.aln_hits_weights_profiles.argtypes = [C.c_void_p, C.POINTER(AlnQProfiles), C.POINTER(AlnSeqs), C.POINTER(AlnSeqs),
                                                C.POINTER(AlnGap), C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlnHit), _ip, C.c_int32,
                                                C.POINTER(AlnHitAlignment), _ip, _lp, _ip, _ip]
        L.aln_hits_purge.argtypes = [C.c_void_p, C.POINTER(AlnSeqs), C.POINTER(AlnSeqs), C.POINTER(AlnSubmatrix), C.POINTER(AlnGap),
                                     C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlnHit), _ip, C.c_int32, C.c_int32, C.c_int32,
                                     C.POINTER(AlnHitAlignment), C.POINTER(AlnHitPurge), _ip, _lp, _ip, _ip]
        L.aln_hits_purge_profiles.argtypes = [C.c_void_p, C.POINTER(AlnQProfiles), C.POINTER(AlnSeqs), C.POINTER(AlnSeqs),
                                              C.POINTER(AlnGap), C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlnHit), _ip, C.c_int32,
                                              C.c_int32, C.c_int32, C.POINTER(AlnHitAlignment), C.POINTER(AlnHitPurge), _ip, _lp, _ip,
                                              _ip]
        L.aln_hits_pssm.argtypes = [C.c_void_p, C.POINTER(AlnSeqs), C.POINTER(AlnSeqs), C.POINTER(AlnSubmatrix), C.POINTER(AlnGap),
                                    C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlnHit), _ip, C.c_int32, C.c_int32, C.c_int32,
                                    C.POINTER(AlnPssmParams), C.POINTER(AlnHitAlignment), _fp, C.POINTER(AlnHitPurge), _ip, _lp, _ip,
                                    _ip]
        L.aln_hits_pssm_profiles.argtypes = [C.c_void_p, C.POINTER(AlnQProfiles), C.POINTER(AlnSeqs), C.POINTER(AlnSeqs),
                                             C.POINTER(AlnGap), C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlnHit), _ip, C.c_int32,
                                             C.c_int32, C.c_int32, C.POINTER(AlnPssmParams), C.POINTER(AlnHitAlignment), _fp,
                                             C.POINTER(AlnHitPurge), _ip, _lp, _ip, _ip]
        L.aln_pssm_entry.argtypes = [C.c_uint64, C.c_uint64, C.c_int32]
        L.aln_pssm_entry.restype = C.c_int32
        L.aln_hits_align_last_routes.argtypes = [C.c_void_p, _lp]
        L.aln_hmap2_gap_arrays.argtypes = [_fp, C.c_int64, C.c_float, C.c_float, C.c_float, _fp, _fp]
        L.aln_batch_plane_bytes_per_cell.argtypes = [C.c_void_p]
        L.aln_batch_optimal_strings.argtypes = [C.c_void_p, _fp, _fp, _ip, C.c_char_p, C.c_char_p, C.c_int32, _ip]
        L.aln_batch_last_exact_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.aln_batch_optimal_strings_enqueue.argtypes = [C.c_void_p, C.c_int32]
        L.aln_batch_optimal_strings_collect.argtypes = [C.c_void_p, _fp, _fp, _ip, C.c_char_p, C.c_char_p, C.c_int32, _ip]
        L.aln_ctx_set_hint.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.aln_ctx_get_hint.argtypes = [C.c_void_p, C.c_char_p, _lp]
        L.aln_deal_units.argtypes = [_lp, C.c_int64, C.c_int32, _ip, _ip]
        L.aln_comm_unique_id.argtypes = [C.c_void_p]
        L.aln_comm_create.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.aln_ctx_create_multi.argtypes = [_ip, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.aln_comm_destroy.argtypes = [C.c_void_p]
        L.aln_comm_n_ranks.argtypes = [C.c_void_p]
        L.aln_comm_last_error.argtypes = [C.c_void_p]
        L.aln_comm_last_error.restype = C.c_char_p
        L.aln_gather_scores.argtypes = [C.c_void_p, C.POINTER(_fp), C.POINTER(_ip), _ip, C.c_int32, _fp, C.c_int64]
        L.aln_gather_resident_enqueue.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(_ip), _ip, C.c_int32, C.c_int64]
        L.aln_gather_resident_collect.argtypes = [C.c_void_p, _fp, C.c_int64]
        _LIB = L
    return _LIB


def _check(rc, ctx=None):
    if rc != 0:
        msg = lib().aln_error_string(rc).decode()
        if ctx is not None and rc == E_HIP:
            msg += ": " + lib().aln_last_error(ctx).decode()
        raise AlnError(rc, msg)


def _f(a):
    return a.ctypes.data_as(_fp)


def _i(a):
    return a.ctypes.data_as(_ip)


class SeqPool:
    """A pool of sequences; each entry is given WITHOUT sentinels and stored as '^' + s + '$'."""

    def __init__(self, seqs):
        self.seqs = ["^" + s + "$" for s in seqs]
        self.offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
        np.cumsum([len(s) for s in self.seqs], out=self.offsets[1:])
        self.blob = "".join(self.seqs).encode()
        self.c = AlnSeqs(len(seqs), self.offsets.ctypes.data_as(_lp), self.blob)


class Context:
    def __init__(self, device=0, stream=None):
        self.h = C.c_void_p()
        self.device = device
        _check(lib().aln_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(self.h)))

    def synchronize(self):
        _check(lib().aln_ctx_synchronize(self.h), self.h)

    def set_hint(self, key, value):
        """aln_ctx_set_hint: a tuning / kernel-selection switch of this context (never changes a result)."""
        _check(lib().aln_ctx_set_hint(self.h, key.encode(), int(value)), self.h)

    def get_hint(self, key):
        v = C.c_int64(0)
        _check(lib().aln_ctx_get_hint(self.h, key.encode(), C.byref(v)), self.h)
        return v.value

    def hints(self, **kv):
        """Context manager: set hints, restore the previous values on exit."""
        ctx = self

        class _H:
            def __enter__(self_):
                self_.old = {k: ctx.get_hint(k) for k in kv}
                for k, v in kv.items():
                    ctx.set_hint(k, v)

            def __exit__(self_, *a):
                for k, v in self_.old.items():
                    ctx.set_hint(k, v)
        return _H()

    def close(self):
        if self.h:
            lib().aln_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def score_all_vs_all(ctx, queries, templates, alphabet, table, gi, ge, q_begin=0, q_end=None, align_type=LOCAL):
    """The score Optimal(align_type) reports for queries[q_begin:q_end] against every template, no planes (aln_score_all_vs_all)."""
    return _score(ctx, _ResidueSide("aln_score_all_vs_all", queries, templates, alphabet, table), gi, ge, q_begin, q_end, align_type)


def search_topk(ctx, queries, templates, alphabet, table, gi, ge, K, min_score=-np.inf, q_begin=0, q_end=None, align_type=LOCAL):
    """aln_search_topk: for queries[q_begin:q_end] the K best templates with score >= min_score (score descending, ties by
    template index), selected on the device.  -> hits[rows, K] (fields t, score, q_end, t_end; unused slots -1, 0, -1, -1),
    n_hits[rows]."""
    return _search(ctx, _ResidueSide("aln_search_topk", queries, templates, alphabet, table), gi, ge, K, min_score, q_begin, q_end,
                   align_type)


class QueryProfiles:
    """A pool of position-specific queries (aln_qprofiles).  Each entry is an L x n array — row i holds the similarity of query
    position i and every letter of `alphabet`, the TEMPLATES' alphabet — given WITHOUT sentinels and stored with a zero row in
    front and behind, as SeqPool stores '^' + s + '$'."""

    def __init__(self, profiles, alphabet):
        n = len(alphabet)
        self.alphabet = alphabet
        self.profiles = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1, n) for p in profiles]
        self.offsets = np.zeros(len(self.profiles) + 1, dtype=np.int64)
        np.cumsum([len(p) + 2 for p in self.profiles], out=self.offsets[1:])
        self.rows = np.zeros((int(self.offsets[-1]), n), dtype=np.float32)
        for k, p in enumerate(self.profiles):
            self.rows[self.offsets[k] + 1:self.offsets[k + 1] - 1] = p
        self._ab = alphabet.encode()
        self.c = AlnQProfiles(len(self.profiles), self.offsets.ctypes.data_as(_lp), _f(self.rows), n, self._ab)

    def __len__(self):
        return len(self.profiles)


def profiles_from_sequences(seqs, alphabet, table):
    """The profiles that score like the residue strings `seqs` under `table`: row i is the table row of residue i."""
    tab = np.asarray(table, dtype=np.float32).reshape(len(alphabet), len(alphabet))
    idx = {ch: k for k, ch in enumerate(alphabet)}
    return QueryProfiles([tab[[idx[ch] for ch in s]].reshape(len(s), len(alphabet)) for s in seqs], alphabet)


def profile_planes(profile, template, alphabet):
    """The (L + 2) x (T + 2) float32 similarity plane of one profile (L x n, no sentinel rows) against one template (a string,
    no sentinels): what Batch.dp_simmatrix takes for the pair.  hits_align_profiles aligns the hits of a profile search without
    it; a resident batch over such planes (query residues: any string of L letters) is what that call is defined by."""
    prof = np.asarray(profile, dtype=np.float32).reshape(-1, len(alphabet))
    idx = {ch: k for k, ch in enumerate(alphabet)}
    S = np.zeros((len(prof) + 2, len(template) + 2), dtype=np.float32)
    if len(prof) and len(template):
        S[1:-1, 1:-1] = prof[:, [idx[ch] for ch in template]]
    return S


def _const_gap(align_type, gi, ge):
    g = AlnGap()
    g.model = GAP_AFFINE_CONST
    g.align_type = int(align_type)
    g.gap_init = float(np.float32(gi))
    g.gap_extn = float(np.float32(ge))
    return g


def score_profiles_vs_all(ctx, profiles, templates, gi, ge, q_begin=0, q_end=None, align_type=LOCAL):
    """aln_score_profiles_vs_all: the score Optimal(align_type) reports for profiles[q_begin:q_end] (a QueryProfiles) against
    every template, no planes -> float32 [rows, n_templates]."""
    return _score(ctx, _ProfileSide("aln_score_profiles_vs_all", profiles, templates), gi, ge, q_begin, q_end, align_type)


def search_topk_profiles(ctx, profiles, templates, gi, ge, K, min_score=-np.inf, q_begin=0, q_end=None, align_type=LOCAL):
    """aln_search_topk_profiles: search_topk for position-specific queries (a QueryProfiles) -> hits[rows, K], n_hits[rows]."""
    return _search(ctx, _ProfileSide("aln_search_topk_profiles", profiles, templates), gi, ge, K, min_score, q_begin, q_end, align_type)


class QueryGaps:
    """Position-specific gap penalties for a QueryProfiles pool (aln_qgaps).  Each of the four arguments is a list with one entry
    per profile: L + 1 values for a profile of L interior rows — row 0 (the '^' row, whose del_* price the head deletion; its
    ins_* are never read) followed by the interior rows 1 .. L.  They become four float32 pool arrays indexed like
    QueryProfiles.rows (the '$' rows hold 0), which this object keeps alive."""

    def __init__(self, del_init, del_extn, ins_init, ins_extn):
        lists = [[np.asarray(v, dtype=np.float32).reshape(-1) for v in per_profile] for per_profile in (del_init, del_extn, ins_init, ins_extn)]
        lengths = [len(v) for v in lists[0]]
        assert all([len(v) for v in l] == lengths for l in lists) and all(n >= 1 for n in lengths), "L + 1 values per profile, in all four"
        self.offsets = np.zeros(len(lengths) + 1, dtype=np.int64)
        np.cumsum([n + 1 for n in lengths], out=self.offsets[1:])
        pools = [np.zeros(int(self.offsets[-1]), dtype=np.float32) for _ in range(4)]
        for a, l in zip(pools, lists):
            for k, v in enumerate(l):
                a[self.offsets[k]:self.offsets[k + 1] - 1] = v
        self.del_init, self.del_extn, self.ins_init, self.ins_extn = pools
        self.c = AlnQGaps(_f(self.del_init), _f(self.del_extn), _f(self.ins_init), _f(self.ins_extn))

    @classmethod
    def constant(cls, profiles, gi, ge):
        """every row of the QueryProfiles priced gi / ge: what the constant-gap entries compute (the anchor of include/aln_hip.h)"""
        i = [np.full(len(p) + 1, gi, np.float32) for p in profiles.profiles]
        e = [np.full(len(p) + 1, ge, np.float32) for p in profiles.profiles]
        return cls(i, e, i, e)


def score_profiles_gaps_vs_all(ctx, profiles, gaps, templates, q_begin=0, q_end=None, align_type=LOCAL):
    """aln_score_profiles_gaps_vs_all: score_profiles_vs_all with the gap penalties of `gaps` (a QueryGaps over `profiles`), which
    every profile row carries for itself -> float32 [rows, n_templates]."""
    tpool = _pool(templates)
    if q_end is None:
        q_end = len(profiles)
    out = np.empty((max(q_end - q_begin, 0), len(tpool.seqs)), dtype=np.float32)
    _check(lib().aln_score_profiles_gaps_vs_all(ctx.h, C.byref(profiles.c), C.byref(gaps.c), C.byref(tpool.c), int(align_type), q_begin,
                                                q_end, _f(out)), ctx.h)
    return out


def search_topk_profiles_gaps(ctx, profiles, gaps, templates, K, min_score=-np.inf, q_begin=0, q_end=None, align_type=LOCAL):
    """aln_search_topk_profiles_gaps: search_topk_profiles under the rows' own gap penalties -> hits[rows, K], n_hits[rows]."""
    tpool = _pool(templates)
    if q_end is None:
        q_end = len(profiles)
    rows = max(q_end - q_begin, 0)
    hits = np.zeros((rows, max(int(K), 0)), dtype=HIT_DTYPE)
    n_hits = np.zeros(rows, dtype=np.int32)
    _check(lib().aln_search_topk_profiles_gaps(ctx.h, C.byref(profiles.c), C.byref(gaps.c), C.byref(tpool.c), int(align_type), q_begin,
                                               q_end, int(K), float(min_score), _as(hits, AlnHit), _i(n_hits)), ctx.h)
    return hits, n_hits


# ---- what the search family's entries share ---------------------------------------------------------------------------------
# A residue entry and its profile twin differ in the leading ctypes arguments, in where query lengths and offsets come from and
# in the entry called: that is a side.  Everything else of a pair is one body (_score, _search, _zscores, _align, _counts).
def _pool(seqs):
    return seqs if isinstance(seqs, SeqPool) else SeqPool(seqs)


def _submatrix(alphabet, table):
    """The aln_submatrix of a call.  A ctypes struct keeps the object behind a c_char_p field (the alphabet's bytes are in its
    _objects) but NOT the array a pointer field was made from — storing the pointer copies the address only — so the table
    rides along as an attribute and lives as long as the struct."""
    tab = np.ascontiguousarray(table, dtype=np.float32)
    sub = AlnSubmatrix(len(alphabet), alphabet.encode(), _f(tab))
    sub.table_array = tab
    return sub


class _Side:
    """lead: the arguments between the context and the gap (byref keeps its struct, the side keeps what the structs point to);
    offsets: the query pool's, sentinels included, which give the queries' number and lengths; n_letters: columns of a count row."""

    def call(self, ctx, gap, *tail):
        return getattr(lib(), self.entry)(ctx.h, *(self.lead + (C.byref(gap),) + tail))


class _ResidueSide(_Side):
    def __init__(self, entry, queries, templates, alphabet, table):
        self.entry, self.qpool, self.tpool, self.sub = entry, _pool(queries), _pool(templates), _submatrix(alphabet, table)
        self.lead = (C.byref(self.qpool.c), C.byref(self.tpool.c), C.byref(self.sub))
        self.offsets, self.n_letters = self.qpool.offsets, len(alphabet)


class _ProfileSide(_Side):
    def __init__(self, entry, profiles, templates, consensus=False):
        """consensus: False for an entry without the argument, else the caller's (None: NULL)"""
        self.entry, self.profiles, self.tpool = entry, profiles, _pool(templates)
        self.cpool = None if consensus is None or consensus is False else _pool(consensus)
        cons = () if consensus is False else (C.byref(self.cpool.c) if self.cpool is not None else None,)
        self.lead = (C.byref(profiles.c),) + cons + (C.byref(self.tpool.c),)
        self.offsets, self.n_letters = profiles.offsets, len(profiles.alphabet)


class _GapRowSide(_ProfileSide):
    """a profile side whose rows carry their own gap penalties (gaps: a QueryGaps over `profiles`): the entry takes the gap rows
    after the profiles and, where its twin takes the gap, the align type alone"""

    def __init__(self, entry, profiles, gaps, templates, consensus):
        _ProfileSide.__init__(self, entry, profiles, templates, consensus)
        self.gaps = gaps
        self.lead = self.lead[:1] + (C.byref(gaps.c),) + self.lead[1:]

    def call(self, ctx, gap, *tail):
        return getattr(lib(), self.entry)(ctx.h, *(self.lead + (int(gap.align_type),) + tail))


def _as(a, struct):
    return a.ctypes.data_as(C.POINTER(struct))


def _score(ctx, side, gi, ge, q_begin, q_end, align_type):
    if q_end is None:
        q_end = len(side.offsets) - 1
    out = np.empty((q_end - q_begin, len(side.tpool.seqs)), dtype=np.float32)
    _check(side.call(ctx, _const_gap(align_type, gi, ge), q_begin, q_end, _f(out)), ctx.h)
    return out


def _search(ctx, side, gi, ge, K, min_score, q_begin, q_end, align_type):
    if q_end is None:
        q_end = len(side.offsets) - 1
    rows = max(q_end - q_begin, 0)
    hits = np.zeros((rows, max(int(K), 0)), dtype=HIT_DTYPE)
    n_hits = np.zeros(rows, dtype=np.int32)
    _check(side.call(ctx, _const_gap(align_type, gi, ge), q_begin, q_end, int(K), float(min_score), _as(hits, AlnHit), _i(n_hits)), ctx.h)
    return hits, n_hits


def _hit_list(hits, n_hits):
    """a search's result as the entries take it -> hits, n_hits, rows, K"""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    n_hits = np.ascontiguousarray(n_hits, dtype=np.int32)
    rows, K = hits.shape
    assert n_hits.shape == (rows,)
    return hits, n_hits, rows, K


def _strides(side, q_begin, rows, pair_stride, line_stride):
    """the defaults: the longest list and line a pair of the block can have"""
    maxq = int(np.diff(side.offsets[q_begin:q_begin + rows + 1]).max(initial=2))
    maxt = int(np.diff(side.tpool.offsets).max(initial=2))
    return (min(maxq, maxt) + 3 if pair_stride is None else pair_stride), (maxq + maxt + 2 if line_stride is None else line_stride)


def _fmix32(x):
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    return x ^ (x >> 16)


def shuffle_order(seed, q_index, s, n):
    """The order shuffle s of query q_index (its index in the pool) under `seed` puts n interior positions in (include/aln_hip.h:
    the rule applied to the list 0 .. n-1): position i of the shuffle holds the original position a[i].  aln_hits_zscores
    permutes residues by it, aln_hits_zscores_profiles the interior rows of a profile.  Pure Python.  -> the list a"""
    key = _fmix32((_fmix32((_fmix32((seed ^ 0x9E3779B9) & 0xFFFFFFFF) + q_index) & 0xFFFFFFFF) + s) & 0xFFFFFFFF)
    a = list(range(n))
    for i in range(n - 1, 0, -1):
        j = (_fmix32((key + i * 0x9E3779B9) & 0xFFFFFFFF) * (i + 1)) >> 32
        a[i], a[j] = a[j], a[i]
    return a


def shuffle_query(seed, q_index, s, residues):
    """Shuffle s of query q_index (its index in the pool) under `seed`, as aln_hits_zscores permutes it (include/aln_hip.h):
    pure Python over the interior residues — `residues` comes WITHOUT sentinels.  Reproduces a background sample."""
    return "".join(residues[i] for i in shuffle_order(seed, q_index, s, len(residues)))


def hits_zscores(ctx, queries, templates, hits, n_hits, alphabet, table, gi, ge, n_shuffles, seed=0, q_begin=0, align_type=LOCAL):
    """aln_hits_zscores: for the used slots of hits[rows, K] (search_topk's layout; row r is query q_begin + r) the sum and the
    sum of squares of the scores of n_shuffles permutations of the query against the hit's template, scored and reduced on
    the device, and the z-score of the hit's own score against that sample.  Integer scoring only.
    -> stats[rows, K] (fields sum, sumsq, n, z; unused slots 0)."""
    return _zscores(ctx, _ResidueSide("aln_hits_zscores", queries, templates, alphabet, table), hits, n_hits, gi, ge, n_shuffles, seed,
                    q_begin, align_type)


def _zscores(ctx, side, hits, n_hits, gi, ge, n_shuffles, seed, q_begin, align_type):
    hits, n_hits, rows, K = _hit_list(hits, n_hits)
    stats = np.zeros((rows, K), dtype=HIT_STATS_DTYPE)
    _check(side.call(ctx, _const_gap(align_type, gi, ge), q_begin, q_begin + rows, int(K), _as(hits, AlnHit), _i(n_hits),
                     int(n_shuffles), int(seed) & 0xFFFFFFFF, _as(stats, AlnHitStats)), ctx.h)
    return stats


def hits_zscores_profiles(ctx, profiles, templates, hits, n_hits, gi, ge, n_shuffles, seed=0, q_begin=0, align_type=LOCAL):
    """aln_hits_zscores_profiles: hits_zscores for the hits of a profile search (profiles: a QueryProfiles; hits / n_hits in
    search_topk_profiles' layout, row r is profile q_begin + r).  Shuffle s of a profile is the profile with its interior rows in
    the order shuffle_order gives; the device reads one resident copy of the rows in that order.  Integer scoring only.
    -> stats[rows, K] (fields sum, sumsq, n, z; unused slots 0)."""
    return _zscores(ctx, _ProfileSide("aln_hits_zscores_profiles", profiles, templates), hits, n_hits, gi, ge, n_shuffles, seed,
                    q_begin, align_type)


def hits_align(ctx, queries, templates, hits, n_hits, alphabet, table, gi, ge, q_begin=0, align_type=LOCAL, want_pairs=True,
               want_lines=True, pair_stride=None, line_stride=None):
    """aln_hits_align: Optimal's alignment of every used slot of hits[rows, K] (search_topk's layout; row r is query q_begin + r),
    traced on the device from the end cell the search reported.  -> rec[rows, K] (fields n_pairs, status, score, identity;
    unused slots 0), lists (rows x K pair arrays in list order, or None), tlines, qlines (rows x K str, or None), lengths[rows, K]
    (or None), rc (the call's status: 0, or the lowest per-slot status).  Raises only when the call wrote nothing."""
    return _align(ctx, _ResidueSide("aln_hits_align", queries, templates, alphabet, table), hits, n_hits, gi, ge, q_begin, align_type,
                  want_pairs, want_lines, pair_stride, line_stride)


def _hit_outputs(rows, K, pair_stride, line_stride, want_pairs, want_lines):
    rec = np.zeros((rows, K), dtype=HIT_ALIGNMENT_DTYPE)
    pairs = np.zeros((rows, K, pair_stride, 2), dtype=np.int32) if want_pairs else None
    tl = C.create_string_buffer(max(rows * K * line_stride, 1)) if want_lines else None
    ql = C.create_string_buffer(max(rows * K * line_stride, 1)) if want_lines else None
    lengths = np.zeros((rows, K), dtype=np.int32) if want_lines else None
    return rec, pairs, tl, ql, lengths


def _nest(flat, shape):
    """a flat list as nested lists of `shape`"""
    a = np.empty(len(flat), dtype=object)
    for i, v in enumerate(flat):
        a[i] = v
    return a.reshape(shape).tolist()


def _cut(buf, lengths, line_stride):
    """a line buffer, one slot of line_stride bytes per entry of `lengths` ([r][k] or [r][k][a]) -> str, nested like `lengths`"""
    raw = buf.raw
    return _nest([raw[i * line_stride:i * line_stride + int(n)].decode() for i, n in enumerate(lengths.reshape(-1))], lengths.shape)


def _align(ctx, side, hits, n_hits, gi, ge, q_begin, align_type, want_pairs, want_lines, pair_stride, line_stride, multi=None):
    """hits_align's body and, with multi = (max_alignments, min_score), hits_align_multi's: M = max(N, 1) alignments per slot,
    outputs [r][k][a] instead of [r][k], and n_found in front of rc"""
    hits, n_hits, rows, K = _hit_list(hits, n_hits)
    pair_stride, line_stride = _strides(side, q_begin, rows, pair_stride, line_stride)
    shape, more = (rows, K), ()
    if multi is not None:
        n_found = np.zeros((rows, K), dtype=np.int32)
        shape, more = (rows, K, max(int(multi[0]), 1)), (int(multi[0]), float(multi[1]), _i(n_found))
    rec, pairs, tl, ql, lengths = _hit_outputs(rows, int(np.prod(shape[1:])), pair_stride, line_stride, want_pairs, want_lines)
    rc = side.call(ctx, _const_gap(align_type, gi, ge), q_begin, q_begin + rows, int(K), _as(hits, AlnHit), _i(n_hits), *more,
                   _as(rec, AlnHitAlignment), _i(pairs) if want_pairs else None, int(pair_stride) if want_pairs else 0, tl, ql,
                   int(line_stride) if want_lines else 0, _i(lengths) if want_lines else None)
    if rc != 0 and not (rec["status"] == rc).any():
        _check(rc, ctx.h)
    rec = rec.reshape(shape)
    lists = tlines = qlines = None
    if want_pairs:
        flat = pairs.reshape(rec.size, pair_stride, 2)
        lists = _nest([flat[i, :min(int(n), pair_stride)].copy() for i, n in enumerate(rec["n_pairs"].reshape(-1))], shape)
    if want_lines:
        lengths = lengths.reshape(shape)
        tlines, qlines = _cut(tl, lengths, line_stride), _cut(ql, lengths, line_stride)
    return (rec, lists, tlines, qlines, lengths) + (() if multi is None else (n_found,)) + (rc,)


def hits_align_profiles(ctx, profiles, templates, hits, n_hits, gi, ge, consensus=None, q_begin=0, align_type=LOCAL, want_pairs=True,
                        want_lines=True, pair_stride=None, line_stride=None):
    """aln_hits_align_profiles: hits_align for the hits of a profile search (profiles: a QueryProfiles; hits / n_hits in
    search_topk_profiles' layout, row r is profile q_begin + r).  consensus: the query letters the lines and the identity are made
    of — one string per profile of the POOL, without sentinels and of the profile's length (or a SeqPool of such) — or None for
    the placeholder alphabet[0].  -> the 6-tuple of hits_align."""
    return _align(ctx, _ProfileSide("aln_hits_align_profiles", profiles, templates, consensus), hits, n_hits, gi, ge, q_begin, align_type,
                  want_pairs, want_lines, pair_stride, line_stride)


def hits_align_profiles_gaps(ctx, profiles, gaps, templates, hits, n_hits, consensus=None, q_begin=0, align_type=LOCAL, want_pairs=True,
                             want_lines=True, pair_stride=None, line_stride=None):
    """aln_hits_align_profiles_gaps: hits_align_profiles for the hits of search_topk_profiles_gaps, aligned under the rows' own
    gap penalties (gaps: the QueryGaps of the search).  -> the 6-tuple of hits_align."""
    return _align(ctx, _GapRowSide("aln_hits_align_profiles_gaps", profiles, gaps, templates, consensus), hits, n_hits, 0, 0, q_begin,
                  align_type, want_pairs, want_lines, pair_stride, line_stride)


def hits_align_multi(ctx, queries, templates, hits, n_hits, alphabet, table, gi, ge, max_alignments, min_score=-np.inf, q_begin=0,
                     align_type=LOCAL, want_pairs=True, want_lines=True, pair_stride=None, line_stride=None):
    """aln_hits_align_multi: up to N = max_alignments non-intersecting local alignments of every used slot of hits[rows, K]
    (only the slots' t is read): round 0 is Optimal's alignment, round a >= 1 Optimal's alignment with every aligned pair of
    the earlier rounds forbidden.  -> rec[rows, K, N] (unreported rounds 0), lists (rows x K x N pair arrays in list order, or
    None), tlines, qlines (rows x K x N str, or None), lengths[rows, K, N] (or None), n_found[rows, K], rc (0, or the lowest
    per-alignment status).  Raises only when the call wrote nothing."""
    return _align(ctx, _ResidueSide("aln_hits_align_multi", queries, templates, alphabet, table), hits, n_hits, gi, ge, q_begin,
                  align_type, want_pairs, want_lines, pair_stride, line_stride, multi=(max_alignments, min_score))


def hits_align_multi_profiles(ctx, profiles, templates, hits, n_hits, gi, ge, max_alignments, min_score=-np.inf, consensus=None,
                              q_begin=0, align_type=LOCAL, want_pairs=True, want_lines=True, pair_stride=None, line_stride=None):
    """aln_hits_align_multi_profiles: hits_align_multi for the hits of a profile search (profiles: a QueryProfiles; row r is
    profile q_begin + r; only the slots' t is read).  consensus: the query letters of the lines and the identity, as in
    hits_align_profiles, or None for the placeholder alphabet[0].  -> the 7-tuple of hits_align_multi."""
    return _align(ctx, _ProfileSide("aln_hits_align_multi_profiles", profiles, templates, consensus), hits, n_hits, gi, ge, q_begin,
                  align_type, want_pairs, want_lines, pair_stride, line_stride, multi=(max_alignments, min_score))


def masked_plane(q, t, alphabet, table, forbidden, value):
    """The Q x T float32 similarity plane of '^'+q+'$' against '^'+t+'$' (sentinel rows and columns 0) with `value` at every
    cell of `forbidden` (pairs (i, j)): what a round of hits_align_multi is defined on."""
    tab = np.asarray(table, dtype=np.float32)
    idx = {ch: k for k, ch in enumerate(alphabet)}
    S = np.zeros((len(q) + 2, len(t) + 2), dtype=np.float32)
    if len(q) and len(t):
        qi = np.array([idx[c] for c in q], dtype=np.int64)
        tj = np.array([idx[c] for c in t], dtype=np.int64)
        S[1:-1, 1:-1] = tab[qi[:, None], tj[None, :]]
    for i, j in forbidden:
        S[i, j] = value
    return S


def hits_align_multi_detour(ctx, queries, templates, pairs_qt, alphabet, table, gi, ge, max_alignments, min_score=-np.inf,
                            group=512):
    """What hits_align_multi replaces, spelled out with resident batches (host glue only; the comparator of the tests and of
    tools/bench_align_multi.py): per round one Batch over the (query index, template index) pairs still alive, built by
    dp_simmatrix from planes expanded and masked on the host, then optimal + optimal_strings (`group` pairs per Batch, so that the
    host planes stay small).
    -> per pair the list of its reported rounds, each (score, pair list, identity, tline, qline, status)."""
    queries, templates = _pool(queries), _pool(templates)
    return _multi_detour(ctx, queries, templates, pairs_qt, gi, ge, max_alignments, min_score, group,
                         lambda q, t: masked_plane(queries.seqs[q][1:-1], templates.seqs[t][1:-1], alphabet, table, (), 0.0))


def _multi_detour(ctx, letters, templates, pairs_qt, gi, ge, max_alignments, min_score, group, plane):
    """The rounds of both detours.  letters: the pool the batches take their query letters from; plane(q, t): the pair's
    similarity plane before any cell is forbidden."""
    out = [[] for _ in pairs_qt]
    forb = [[] for _ in pairs_qt]
    neg = [0.0] * len(pairs_qt)
    alive = list(range(len(pairs_qt)))
    for a in range(int(max_alignments)):
        if not alive:
            break
        nxt = []
        for g0 in range(0, len(alive), group):
            part = alive[g0:g0 + group]
            planes = []
            for p in part:
                S = plane(*pairs_qt[p])
                for i, j in forb[p]:
                    S[i, j] = neg[p]
                planes.append(S)
            b = Batch(ctx, letters, templates, [pairs_qt[p][0] for p in part], [pairs_qt[p][1] for p in part])
            try:
                b.dp_simmatrix(planes, LOCAL, gi, ge)
                scores, lists, status = b.optimal()
                s2, ident, st2, tl, ql = b.optimal_strings()
            finally:
                b.close()
            for k, p in enumerate(part):
                sc = scores[k]
                if not (sc >= min_score and (a == 0 or sc > 0)):
                    continue
                out[p].append((sc, lists[k], ident[k], tl[k], ql[k], int(status[k])))
                if status[k] != 0:
                    continue
                Q, T = planes[k].shape
                if a == 0:
                    neg[p] = -(float(sc) + 1.0)
                forb[p] += [(int(i), int(j)) for i, j in lists[k] if 1 <= i <= Q - 2 and 1 <= j <= T - 2]
                nxt.append(p)
        alive = nxt
    return out


def hits_align_multi_profiles_detour(ctx, profiles, templates, pairs_qt, gi, ge, max_alignments, min_score=-np.inf, consensus=None,
                                     group=512):
    """What hits_align_multi_profiles replaces (host glue only; the comparator of the tests and of
    tools/bench_align_multi_profiles.py): hits_align_multi_detour with every round's plane — round 0's included — expanded from
    the profile by profile_planes and masked on the host; the query letters of the batches are `consensus` (one string per
    profile of the pool, no sentinels) or the placeholder alphabet[0].
    -> per pair the list of its reported rounds, each (score, pair list, identity, tline, qline, status)."""
    alphabet, templates = profiles.alphabet, _pool(templates)
    letters = _pool(consensus if consensus is not None else [alphabet[0] * len(p) for p in profiles.profiles])
    return _multi_detour(ctx, letters, templates, pairs_qt, gi, ge, max_alignments, min_score, group,
                         lambda q, t: profile_planes(profiles.profiles[q], templates.seqs[t][1:-1], alphabet))


def _counts(ctx, side, hits, n_hits, gi, ge, weights, q_begin, align_type, want_covered):
    hits, n_hits, rows, K = _hit_list(hits, n_hits)
    cut = [int(side.offsets[q_begin + r] - side.offsets[q_begin]) for r in range(rows + 1)]
    rec = np.zeros((rows, K), dtype=HIT_ALIGNMENT_DTYPE)
    counts = np.zeros((cut[rows], side.n_letters), dtype=np.int32)
    covered = np.zeros(cut[rows], dtype=np.int32) if want_covered else None
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.int32)
        assert weights.shape == (rows, K)
    rc = side.call(ctx, _const_gap(align_type, gi, ge), q_begin, q_begin + rows, int(K), _as(hits, AlnHit), _i(n_hits),
                   _i(weights) if weights is not None else None, _as(rec, AlnHitAlignment), _i(counts),
                   _i(covered) if want_covered else None)
    if rc != 0 and not (rec["status"] == rc).any():
        _check(rc, ctx.h)
    return rec, [counts[cut[r]:cut[r + 1]] for r in range(rows)], covered, rc


def hits_column_counts(ctx, queries, templates, hits, n_hits, alphabet, table, gi, ge, weights=None, q_begin=0, align_type=LOCAL,
                       want_covered=True):
    """aln_hits_column_counts: per query of the row block, how often each letter of `alphabet` stands under each query position
    in the alignments hits_align reports for the used slots of hits[rows, K], tallied on the device — no alignment is downloaded.
    weights: None (every used slot counts 1) or int32 [rows, K] in 0..65535.  -> rec[rows, K] (hits_align's records without
    lists), counts (per row an int32 (Q, n) array, sentinel rows included and zero; views of one block), covered (int32, one
    entry per row of the block's queries: the weighted alignments that span the position, aligned or opposite a gap; None when
    not wanted), rc (0, or the lowest per-slot status).  Raises only when the call wrote nothing."""
    return _counts(ctx, _ResidueSide("aln_hits_column_counts", queries, templates, alphabet, table), hits, n_hits, gi, ge, weights,
                   q_begin, align_type, want_covered)


def hits_column_counts_profiles(ctx, profiles, templates, hits, n_hits, gi, ge, consensus=None, weights=None, q_begin=0,
                                align_type=LOCAL, want_covered=True):
    """aln_hits_column_counts_profiles: hits_column_counts for the hits of a profile search (profiles: a QueryProfiles, whose
    alphabet the counts' columns follow; consensus as in hits_align_profiles — it only enters the records' identity).
    -> the 4-tuple of hits_column_counts."""
    return _counts(ctx, _ProfileSide("aln_hits_column_counts_profiles", profiles, templates, consensus), hits, n_hits, gi, ge, weights,
                   q_begin, align_type, want_covered)


def hits_column_counts_profiles_gaps(ctx, profiles, gaps, templates, hits, n_hits, consensus=None, weights=None, q_begin=0,
                                     align_type=LOCAL, want_covered=True):
    """aln_hits_column_counts_profiles_gaps: hits_column_counts_profiles over the alignments hits_align_profiles_gaps reports
    (gaps: the QueryGaps of the search).  -> the 4-tuple of hits_column_counts."""
    return _counts(ctx, _GapRowSide("aln_hits_column_counts_profiles_gaps", profiles, gaps, templates, consensus), hits, n_hits, 0, 0,
                   weights, q_begin, align_type, want_covered)


def _pileup(ctx, side, hits, n_hits, gi, ge, q_begin, align_type, want_letters, want_tpos, want_spans, line_stride):
    hits, n_hits, rows, K = _hit_list(hits, n_hits)
    if line_stride is None:
        line_stride = max(int(np.diff(side.offsets[q_begin:q_begin + rows + 1]).max(initial=2)) - 2, 1)
    stride = max(int(line_stride), 0)
    rec = np.zeros((rows, K), dtype=HIT_ALIGNMENT_DTYPE)
    spans = np.zeros((rows, K), dtype=HIT_SPAN_DTYPE) if want_spans else None
    letters = np.zeros((rows, K, stride), dtype=np.uint8) if want_letters else None
    tpos = np.zeros((rows, K, stride), dtype=np.uint16) if want_tpos else None
    rc = side.call(ctx, _const_gap(align_type, gi, ge), q_begin, q_begin + rows, int(K), _as(hits, AlnHit), _i(n_hits),
                   _as(rec, AlnHitAlignment), _as(spans, AlnHitSpan) if want_spans else None,
                   letters.ctypes.data_as(C.POINTER(C.c_uint8)) if want_letters else None,
                   tpos.ctypes.data_as(C.POINTER(C.c_uint16)) if want_tpos else None, int(line_stride))
    if rc != 0 and not (rec["status"] == rc).any():
        _check(rc, ctx.h)
    return rec, spans, letters, tpos, rc


def hits_pileup(ctx, queries, templates, hits, n_hits, alphabet, table, gi, ge, q_begin=0, align_type=LOCAL, want_letters=True,
                want_tpos=True, want_spans=True, line_stride=None):
    """aln_hits_pileup: the query-anchored stack of the alignments hits_align reports for the used slots of hits[rows, K], laid
    out on the device — one row per slot whose index p is query position p + 1: the template's letter aligned to it, '-' where
    the alignment passes the position opposite a gap, '.' outside the aligned range and in slots that do not contribute (status
    != 0; local score <= 0), NUL beyond the query and in unused slots; tpos holds the template position (0: none).
    line_stride: None = the longest query of the block (at least 1).  -> rec[rows, K] (hits_align's records without lists),
    spans[rows, K] (fields q_lo, q_hi, t_lo, t_hi; zero where nothing is aligned; or None), letters uint8 [rows, K, stride] (or
    None), tpos uint16 [rows, K, stride] (or None), rc (0, or the lowest per-slot status).  Raises only when the call wrote
    nothing."""
    return _pileup(ctx, _ResidueSide("aln_hits_pileup", queries, templates, alphabet, table), hits, n_hits, gi, ge, q_begin, align_type,
                   want_letters, want_tpos, want_spans, line_stride)


def hits_pileup_profiles(ctx, profiles, templates, hits, n_hits, gi, ge, consensus=None, q_begin=0, align_type=LOCAL,
                         want_letters=True, want_tpos=True, want_spans=True, line_stride=None):
    """aln_hits_pileup_profiles: hits_pileup for the hits of a profile search (profiles: a QueryProfiles; consensus as in
    hits_align_profiles — it only enters the records' identity).  -> the 5-tuple of hits_pileup."""
    return _pileup(ctx, _ProfileSide("aln_hits_pileup_profiles", profiles, templates, consensus), hits, n_hits, gi, ge, q_begin,
                   align_type, want_letters, want_tpos, want_spans, line_stride)


def _weights(ctx, side, hits, n_hits, gi, ge, w_max, q_begin, align_type, want_raw, want_counts, want_covered):
    hits, n_hits, rows, K = _hit_list(hits, n_hits)
    cut = [int(side.offsets[q_begin + r] - side.offsets[q_begin]) for r in range(rows + 1)]
    rec = np.zeros((rows, K), dtype=HIT_ALIGNMENT_DTYPE)
    weights = np.zeros((rows, K), dtype=np.int32)
    raw = np.zeros((rows, K), dtype=np.int64) if want_raw else None
    counts = np.zeros((cut[rows], side.n_letters), dtype=np.int32) if want_counts else None
    covered = np.zeros(cut[rows], dtype=np.int32) if want_covered else None
    rc = side.call(ctx, _const_gap(align_type, gi, ge), q_begin, q_begin + rows, int(K), _as(hits, AlnHit), _i(n_hits), int(w_max),
                   _as(rec, AlnHitAlignment), _i(weights), raw.ctypes.data_as(_lp) if want_raw else None,
                   _i(counts) if want_counts else None, _i(covered) if want_covered else None)
    if rc != 0 and not (rec["status"] == rc).any():
        _check(rc, ctx.h)
    return rec, weights, raw, ([counts[cut[r]:cut[r + 1]] for r in range(rows)] if want_counts else None), covered, rc


def hits_weights(ctx, queries, templates, hits, n_hits, alphabet, table, gi, ge, w_max=1000, q_begin=0, align_type=LOCAL, want_raw=True,
                 want_counts=True, want_covered=True):
    """aln_hits_weights: Henikoff position-based weights of the used slots of hits[rows, K], read off the query-anchored pileup
    (hits_pileup's letters) on the device, and the column counts under those weights — no pileup is downloaded and every hit is
    swept once.  Per query position p: n_p[a] slots show letter a, k_p letters occur; raw[k] = sum over the slot's letters of
    floor(2^24 / (k_p n_p[a])); weight[k] = 0 where raw[k] == 0, else max(1, floor(w_max raw[k] / max raw of the row)), w_max in
    1..65535.  -> rec[rows, K] (hits_align's records without lists), weights int32 [rows, K], raw int64 [rows, K] (or None),
    counts and covered as hits_column_counts(..., weights=weights) returns them (or None), rc (0, or the lowest per-slot status).
    Raises only when the call wrote nothing."""
    return _weights(ctx, _ResidueSide("aln_hits_weights", queries, templates, alphabet, table), hits, n_hits, gi, ge, w_max, q_begin,
                    align_type, want_raw, want_counts, want_covered)


def hits_weights_profiles(ctx, profiles, templates, hits, n_hits, gi, ge, consensus=None, w_max=1000, q_begin=0, align_type=LOCAL,
                          want_raw=True, want_counts=True, want_covered=True):
    """aln_hits_weights_profiles: hits_weights for the hits of a profile search (profiles: a QueryProfiles, whose alphabet the
    letters are counted in; consensus as in hits_align_profiles — it only enters the records' identity).
    -> the 6-tuple of hits_weights."""
    return _weights(ctx, _ProfileSide("aln_hits_weights_profiles", profiles, templates, consensus), hits, n_hits, gi, ge, w_max,
                    q_begin, align_type, want_raw, want_counts, want_covered)


def weights_from_pileup(letters_row, alphabet, w_max):
    """The weights of hits_weights restated over a pileup, pure numpy, int64 throughout.  letters_row: [K, L] letters of one
    query (one row of hits_pileup's letters; L = its residues or more); w_max: 1..65535.  -> (weights int64 [K], raw int64 [K])."""
    rows = np.asarray(letters_row, dtype=np.uint8)
    assert rows.ndim == 2 and 1 <= int(w_max) <= 65535
    is_a = np.stack([rows == ord(ch) for ch in alphabet], axis=0) if len(alphabet) else np.zeros((0,) + rows.shape, bool)
    n = is_a.sum(axis=1, dtype=np.int64)                              # [n letters, L]
    k = (n > 0).sum(axis=0, dtype=np.int64)                           # [L]
    term = np.int64(1 << 24) // np.maximum(k[None, :] * n, 1)         # [n letters, L]; read only where n > 0
    raw = (is_a * term[:, None, :]).sum(axis=(0, 2), dtype=np.int64)
    M = int(raw.max(initial=0))
    weights = np.zeros(rows.shape[0], np.int64)
    if M > 0:
        weights = np.where(raw > 0, np.maximum(np.int64(w_max) * raw // np.int64(M), 1), 0).astype(np.int64)
    return weights, raw


def _purge(ctx, side, hits, n_hits, gi, ge, max_identity, min_overlap, w_max, q_begin, align_type, want_weights, want_raw, want_counts,
           want_covered):
    hits, n_hits, rows, K = _hit_list(hits, n_hits)
    cut = [int(side.offsets[q_begin + r] - side.offsets[q_begin]) for r in range(rows + 1)]
    rec = np.zeros((rows, K), dtype=HIT_ALIGNMENT_DTYPE)
    purge = np.zeros((rows, K), dtype=HIT_PURGE_DTYPE)
    weights = np.zeros((rows, K), dtype=np.int32) if want_weights else None
    raw = np.zeros((rows, K), dtype=np.int64) if want_weights and want_raw else None
    counts = np.zeros((cut[rows], side.n_letters), dtype=np.int32) if want_weights and want_counts else None
    covered = np.zeros(cut[rows], dtype=np.int32) if want_weights and want_covered else None
    rc = side.call(ctx, _const_gap(align_type, gi, ge), q_begin, q_begin + rows, int(K), _as(hits, AlnHit), _i(n_hits),
                   int(max_identity), int(min_overlap), int(w_max), _as(rec, AlnHitAlignment), _as(purge, AlnHitPurge),
                   _i(weights) if weights is not None else None, raw.ctypes.data_as(_lp) if raw is not None else None,
                   _i(counts) if counts is not None else None, _i(covered) if covered is not None else None)
    if rc != 0 and not (rec["status"] == rc).any():
        _check(rc, ctx.h)
    return (rec, purge, weights, raw, ([counts[cut[r]:cut[r + 1]] for r in range(rows)] if counts is not None else None), covered, rc)


def hits_purge(ctx, queries, templates, hits, n_hits, alphabet, table, gi, ge, max_identity=90, min_overlap=50, w_max=1000, q_begin=0,
               align_type=LOCAL, want_weights=True, want_raw=True, want_counts=True, want_covered=True):
    """aln_hits_purge: near-identical hits purged on the device, and the weights of the survivors.  Over the query-anchored
    pileup of the used slots of hits[rows, K] (hits_pileup's letters, which stay on the device): slot k is NEAR an earlier slot
    j when their rows overlap in at least one letter position, 100 overlap >= min_overlap letters(k) and 100 same >=
    max_identity overlap; in ascending order a slot with a letter is kept unless it is near a KEPT earlier slot, whose smallest
    is then its keeper.  max_identity: 1..101 (101: nothing is purged); min_overlap: 0..100.  The weights, raw, counts and
    covered are hits_weights' over the pileup whose slots that are not kept show '.' everywhere (want_weights=False: purge only).
    -> rec[rows, K] (hits_align's records without lists), purge[rows, K] (fields keeper, same, overlap, letters: kept
    {k, 0, 0, letters}; purged by j {j, same, overlap, letters}; every other slot {-1, 0, 0, 0}), weights, raw, counts, covered
    (as hits_weights returns them; None for what was not asked), rc (0, or the lowest per-slot status).  Raises only when the
    call wrote nothing."""
    return _purge(ctx, _ResidueSide("aln_hits_purge", queries, templates, alphabet, table), hits, n_hits, gi, ge, max_identity,
                  min_overlap, w_max, q_begin, align_type, want_weights, want_raw, want_counts, want_covered)


def hits_purge_profiles(ctx, profiles, templates, hits, n_hits, gi, ge, consensus=None, max_identity=90, min_overlap=50, w_max=1000,
                        q_begin=0, align_type=LOCAL, want_weights=True, want_raw=True, want_counts=True, want_covered=True):
    """aln_hits_purge_profiles: hits_purge for the hits of a profile search (profiles: a QueryProfiles, whose alphabet the
    letters are; consensus as in hits_align_profiles — it only enters the records' identity).  -> the 7-tuple of hits_purge."""
    return _purge(ctx, _ProfileSide("aln_hits_purge_profiles", profiles, templates, consensus), hits, n_hits, gi, ge, max_identity,
                  min_overlap, w_max, q_begin, align_type, want_weights, want_raw, want_counts, want_covered)


def purge_from_pileup(letters_row, alphabet, max_identity, min_overlap):
    """The purge of hits_purge restated over a pileup, pure numpy, int64 throughout.  letters_row: [K, L] letters of one query
    (one row of hits_pileup's letters; L = its residues or more); max_identity: 1..101; min_overlap: 0..100.
    -> (keeper, same, overlap, letters), four int64 [K] arrays: hits_purge's record per slot."""
    rows = np.asarray(letters_row, dtype=np.uint8)
    assert rows.ndim == 2 and 1 <= int(max_identity) <= 101 and 0 <= int(min_overlap) <= 100
    K = rows.shape[0]
    is_letter = np.isin(rows, np.frombuffer(alphabet.encode(), np.uint8))
    letters = is_letter.sum(axis=1, dtype=np.int64)
    keeper = np.full(K, -1, np.int64)
    same = np.zeros(K, np.int64)
    overlap = np.zeros(K, np.int64)
    kept = []
    for k in range(K):
        if letters[k] == 0:
            continue
        keeper[k] = k
        if kept:
            both = is_letter[kept] & is_letter[k][None, :]
            ov = both.sum(axis=1, dtype=np.int64)
            sm = (both & (rows[kept] == rows[k][None, :])).sum(axis=1, dtype=np.int64)
            near = (ov >= 1) & (100 * ov >= np.int64(min_overlap) * letters[k]) & (100 * sm >= np.int64(max_identity) * ov)
            if near.any():
                first = int(np.argmax(near))
                keeper[k], same[k], overlap[k] = kept[first], sm[first], ov[first]
                continue
        kept.append(k)
    letters = np.where(keeper >= 0, letters, 0)
    return keeper, same, overlap, letters


def counts_from_pileup(letters_row, alphabet, weights=None):
    """The tally of hits_column_counts restated over a pileup, pure numpy.  letters_row: [K, L] letters of one query (one row of
    hits_pileup's letters; L = its residues or more); weights: None (every slot 1) or K integers.
    -> (counts int64 [L, n]: per position how often each letter of `alphabet` stands there, covered int64 [L]: the weighted
    slots whose aligned range spans the position, aligned or '-')."""
    rows = np.asarray(letters_row, dtype=np.uint8)
    assert rows.ndim == 2
    w = np.ones(rows.shape[0], np.int64) if weights is None else np.asarray(weights, np.int64).reshape(rows.shape[0])
    counts = np.zeros((rows.shape[1], len(alphabet)), np.int64)
    for a, ch in enumerate(alphabet):
        counts[:, a] = ((rows == ord(ch)) * w[:, None]).sum(axis=0)
    covered = (((rows != ord(".")) & (rows != 0)) * w[:, None]).sum(axis=0)
    return counts, covered


def a3m_from_pileup(template, letters_line, tpos_line):
    """One a3m row of a slot, pure numpy.  template: the hit's residues WITHOUT sentinels (position j is template[j - 1]);
    letters_line / tpos_line: the slot's L = Q - 2 entries of hits_pileup's letters and tpos.  Per query position the letter
    ('.' written as '-'); after an aligned position (i, j) whose next aligned position is (i', j') with j' > j + 1 the template
    residues j + 1 .. j' - 1 in lower case.  Template residues before t_lo and after t_hi do not appear.  -> str"""
    letters = np.asarray(letters_line, dtype=np.uint8)
    tpos = np.asarray(tpos_line, dtype=np.int64)
    aligned = np.nonzero(tpos > 0)[0]
    nxt = {int(p): int(tpos[n]) for p, n in zip(aligned[:-1], aligned[1:])}
    out = []
    for p in range(len(letters)):
        ch = chr(int(letters[p]))
        out.append("-" if ch == "." else ch)
        j = int(tpos[p])
        if p in nxt and nxt[p] > j + 1:
            out.append(template[j:nxt[p] - 1].lower())
    return "".join(out)


def pssm_from_counts(counts, background, fallback_rows, pseudo=1.0, scale=2.0):
    """Column counts -> the rows of a position-specific query (one entry of QueryProfiles), float64 numpy throughout.
    counts: (L, n) — the INTERIOR rows of one entry of hits_column_counts' list (entry[1:-1]); background: n letter
    frequencies, each > 0 (they need not sum to 1: only ratios to them enter); fallback_rows: (L, n), what a position nothing
    was aligned to keeps — the round's own query rows, e.g. profiles_from_sequences(...).profiles[q].
    With N_i = sum_a counts[i][a], a row with N_i > 0 becomes
        rint(scale * log2((counts[i][a] + pseudo * bg[a]) / ((N_i + pseudo) * bg[a])))
    — the log-odds, in 1/scale bits, of the observed frequencies smoothed by `pseudo` background-distributed pseudo-counts
    (pseudo > 0, so no logarithm of 0) — and a row with N_i == 0 is fallback_rows[i].  -> float32 (L, n) with integer values
    wherever the fallback's are: a profile made this way stays on the register-resident route."""
    c = np.asarray(counts, dtype=np.float64)
    bg = np.asarray(background, dtype=np.float64).reshape(1, -1)
    fb = np.asarray(fallback_rows, dtype=np.float64)
    assert c.ndim == 2 and c.shape == fb.shape and bg.shape[1] == c.shape[1] and (bg > 0).all() and pseudo > 0
    N = c.sum(axis=1, keepdims=True)
    odds = (c + pseudo * bg) / ((N + pseudo) * bg)
    return np.where(N > 0, np.rint(scale * np.log2(odds)), fb).astype(np.float32)


# T[m] = floor(2^(32 + m/16)), m = 1 .. 15 (include/aln_hip.h): four nested integer square roots of 2^(512 + m)
PSSM_T = (0x10b5586cf, 0x1172b83c7, 0x12387a6e7, 0x1306fe0a3, 0x13dea64c1, 0x14bfdad53, 0x15ab07dd4, 0x16a09e667, 0x17a11473e,
          0x18ace5422, 0x19c49182a, 0x1ae89f995, 0x1c199bdd8, 0x1d5818dcf, 0x1ea4afa2a)


def _lg16(x, y):
    """lg16 of include/aln_hip.h for Python integers x >= y >= 1: floor(16 log2(x / y)) read off a 33-bit mantissa"""
    e = x.bit_length() - y.bit_length()
    if (y << e) > x:
        e -= 1
    mant = (x << 32) // (y << e)
    return 16 * e + sum(1 for t in PSSM_T if t <= mant)


def pssm_score(num, den, scale):
    """The score of aln_hits_pssm's rule for Python integers num, den >= 1 (any size) and scale in 1, 2, 4, 8, no float anywhere:
    floor((lg16(num, den) scale + 8) / 16), or minus that of (den, num) when num < den."""
    num, den, scale = int(num), int(den), int(scale)
    assert num >= 1 and den >= 1 and scale in (1, 2, 4, 8)
    return (_lg16(num, den) * scale + 8) // 16 if num >= den else -((_lg16(den, num) * scale + 8) // 16)


def pssm_entry(num, den, scale):
    """aln_pssm_entry: the same score from the library's host helper (no GPU); 0 for num or den of 0 or >= 2^63 or a scale other
    than 1, 2, 4, 8."""
    return int(lib().aln_pssm_entry(int(num), int(den), int(scale)))


def pssm_rows_from_counts(counts, bg, beta, scale, fallback_rows, mix=None):
    """The rule of hits_pssm restated with Python integers (arbitrary precision, no floats).  counts: (L, n) integers — the
    INTERIOR rows of one entry of hits_purge's counts (entry[1:-1]); bg: n integers >= 1, B their sum; beta: the pseudo-count
    mass in the units of the weights; scale: 1, 2, 4 or 8; fallback_rows: (L, n), what a row without counts keeps, bit for bit;
    mix: None (mix[b][a] = bg[a]) or n x n integers, mix[b][a] the pseudo-count mass letter a receives per observation of b.
    With N = sum_a c[a] > 0:  g[a] = sum_b c[b] mix[b][a],  num = c[a] N B + beta g[a],  den = (N + beta) N bg[a],  entry =
    pssm_score(num, den, scale).  -> float32 (L, n)"""
    fb = np.asarray(fallback_rows, dtype=np.float32)
    rows = [[int(v) for v in row] for row in np.asarray(counts).reshape(fb.shape).tolist()]
    bg = [int(v) for v in np.asarray(bg).reshape(-1).tolist()]
    n, B, beta = len(bg), sum(bg), int(beta)
    assert fb.ndim == 2 and fb.shape[1] == n
    mix = [bg] * n if mix is None else [[int(v) for v in row] for row in np.asarray(mix).reshape(n, n).tolist()]
    out = fb.copy()
    for i, c in enumerate(rows):
        N = sum(c)
        if N == 0:
            continue
        for a in range(n):
            g = sum(c[b] * mix[b][a] for b in range(n))
            out[i, a] = pssm_score(c[a] * N * B + beta * g, (N + beta) * N * bg[a], scale)
    return out


def _pssm(ctx, side, hits, n_hits, gi, ge, params, max_identity, min_overlap, w_max, q_begin, align_type, want_purge, want_weights,
          want_raw, want_counts, want_covered):
    hits, n_hits, rows, K = _hit_list(hits, n_hits)
    cut = [int(side.offsets[q_begin + r] - side.offsets[q_begin]) for r in range(rows + 1)]
    rec = np.zeros((rows, K), dtype=HIT_ALIGNMENT_DTYPE)
    prows = np.zeros((cut[rows], side.n_letters), dtype=np.float32)
    purge = np.zeros((rows, K), dtype=HIT_PURGE_DTYPE) if want_purge else None
    weights = np.zeros((rows, K), dtype=np.int32) if want_weights else None
    raw = np.zeros((rows, K), dtype=np.int64) if want_raw else None
    counts = np.zeros((cut[rows], side.n_letters), dtype=np.int32) if want_counts else None
    covered = np.zeros(cut[rows], dtype=np.int32) if want_covered else None
    rc = side.call(ctx, _const_gap(align_type, gi, ge), q_begin, q_begin + rows, int(K), _as(hits, AlnHit), _i(n_hits),
                   int(max_identity), int(min_overlap), int(w_max), C.byref(params) if params is not None else None,
                   _as(rec, AlnHitAlignment), _f(prows), _as(purge, AlnHitPurge) if want_purge else None,
                   _i(weights) if want_weights else None, raw.ctypes.data_as(_lp) if want_raw else None,
                   _i(counts) if want_counts else None, _i(covered) if want_covered else None)
    if rc != 0 and not (rec["status"] == rc).any():
        _check(rc, ctx.h)
    per_query = lambda x: [x[cut[r]:cut[r + 1]] for r in range(rows)]
    return rec, per_query(prows), purge, weights, raw, (per_query(counts) if want_counts else None), covered, rc


def hits_pssm(ctx, queries, templates, hits, n_hits, alphabet, table, gi, ge, params, max_identity=90, min_overlap=50, w_max=1000,
              q_begin=0, align_type=LOCAL, want_purge=True, want_weights=True, want_raw=True, want_counts=True, want_covered=True):
    """aln_hits_pssm: from a round's hits to the next round's profile rows in one call, on the device — hits_purge's purge,
    weights and weighted counts, then per count row with N = sum of its counts > 0 the integer log-odds
    pssm_rows_from_counts restates (params: an AlnPssmParams, e.g. AlnPssmParams.make(bg, beta, scale, mix)); a row without
    counts keeps the table row of the query's residue, bit for bit.  No count row is downloaded unless asked for.
    -> rec[rows, K] (hits_align's records without lists), rows (per query a float32 (Q, n) array, the sentinel rows included
    and zero; views of one block — entry[1:-1] is an entry of QueryProfiles), then purge, weights, raw, counts, covered exactly
    as hits_purge returns them for the same arguments (None for what was not asked), rc (0, or the lowest per-slot status).
    Raises only when the call wrote nothing."""
    return _pssm(ctx, _ResidueSide("aln_hits_pssm", queries, templates, alphabet, table), hits, n_hits, gi, ge, params, max_identity,
                 min_overlap, w_max, q_begin, align_type, want_purge, want_weights, want_raw, want_counts, want_covered)


def hits_pssm_profiles(ctx, profiles, templates, hits, n_hits, gi, ge, params, consensus=None, max_identity=90, min_overlap=50,
                       w_max=1000, q_begin=0, align_type=LOCAL, want_purge=True, want_weights=True, want_raw=True, want_counts=True,
                       want_covered=True):
    """aln_hits_pssm_profiles: hits_pssm for the hits of a profile search (profiles: a QueryProfiles, whose alphabet the letters
    are; consensus as in hits_align_profiles — it only enters the records' identity); a row without counts keeps the profile's
    own row.  -> the 8-tuple of hits_pssm."""
    return _pssm(ctx, _ProfileSide("aln_hits_pssm_profiles", profiles, templates, consensus), hits, n_hits, gi, ge, params,
                 max_identity, min_overlap, w_max, q_begin, align_type, want_purge, want_weights, want_raw, want_counts, want_covered)


def iterate_search(ctx, queries, templates, alphabet, table, gi, ge, K, rounds, params, max_identity=90, min_overlap=50, w_max=1000,
                   min_score=-np.inf, align_type=LOCAL):
    """An iterative profile search, every step on the device.  Round 1: search_topk, then hits_pssm makes the profiles; every
    later round: search_topk_profiles with the profiles, then hits_pssm_profiles (the queries as consensus) makes the next ones.
    Stops after `rounds` rounds, or after the first round in which every row's template list equals the previous round's (that
    round's hits are reported, no profiles are made from them).  queries: a list of strings.
    -> (per round (hits, n_hits), the last profiles made: a QueryProfiles)"""
    assert rounds >= 1
    quiet = dict(max_identity=max_identity, min_overlap=min_overlap, w_max=w_max, align_type=align_type, want_purge=False,
                 want_weights=False, want_raw=False, want_counts=False, want_covered=False)
    found, profiles, previous = [], None, None
    for _ in range(int(rounds)):
        if profiles is None:
            hits, n_hits = search_topk(ctx, queries, templates, alphabet, table, gi, ge, K, min_score, align_type=align_type)
        else:
            hits, n_hits = search_topk_profiles(ctx, profiles, templates, gi, ge, K, min_score, align_type=align_type)
        lists = [hits["t"][r, :n_hits[r]].tolist() for r in range(len(n_hits))]
        found.append((hits, n_hits))
        if lists == previous:
            break
        previous = lists
        if profiles is None:
            res = hits_pssm(ctx, queries, templates, hits, n_hits, alphabet, table, gi, ge, params, **quiet)
        else:
            res = hits_pssm_profiles(ctx, profiles, templates, hits, n_hits, gi, ge, params, consensus=queries, **quiet)
        if res[7] != 0:
            _check(res[7], ctx.h)
        profiles = QueryProfiles([rows[1:-1] for rows in res[1]], alphabet)
    return found, profiles


def hits_align_routes(ctx):
    """aln_hits_align_last_routes: the used slots the context's last hits_align / hits_align_profiles call sent through a fused
    kernel and through resident batches -> (fused, batched); (0, 0) before any call."""
    out = np.zeros(2, dtype=np.int64)
    _check(lib().aln_hits_align_last_routes(ctx.h, out.ctypes.data_as(_lp)), ctx.h)
    return int(out[0]), int(out[1])


def align_hits(ctx, queries, templates, hits, n_hits, alphabet, table, gi, ge, q_begin=0, align_type=LOCAL):
    """The "align what matters" half of a search: one resident Batch over the valid hits of search_topk (row-major hit order),
    full builds + Optimal.  Host glue only.  -> scores[n], list of n pair arrays."""
    rows, slots = np.nonzero(np.arange(hits.shape[1])[None, :] < np.asarray(n_hits)[:, None])
    if len(rows) == 0:
        return np.empty(0, dtype=np.float32), []
    b = Batch(ctx, queries, templates, rows + q_begin, hits["t"][rows, slots])
    try:
        b.dp_submatrix(alphabet, table, align_type, gi, ge)
        scores, lists, status = b.optimal()
    finally:
        b.close()
    bad = np.nonzero(status)[0]
    if len(bad):
        _check(int(status[bad[0]]), ctx.h)
    return scores, lists


class Batch:
    """Many DPMatrix objects resident in HBM (aln_batch)."""

    def __init__(self, ctx, queries, templates, q_idx=None, t_idx=None, score_only=False):
        self.ctx = ctx
        self.qpool = queries if isinstance(queries, SeqPool) else SeqPool(queries)
        self.tpool = templates if isinstance(templates, SeqPool) else SeqPool(templates)
        if q_idx is None:
            q_idx = np.arange(len(self.qpool.seqs))
            t_idx = np.arange(len(self.tpool.seqs))
        self.q_idx = np.ascontiguousarray(q_idx, dtype=np.int32)
        self.t_idx = np.ascontiguousarray(t_idx, dtype=np.int32)
        self.n = len(self.q_idx)
        self.h = C.c_void_p()
        _check(lib().aln_batch_create(ctx.h, C.byref(self.qpool.c), C.byref(self.tpool.c), self.n, _i(self.q_idx), _i(self.t_idx),
                                      int(score_only), C.byref(self.h)), ctx.h)
        self._keep = []

    def close(self):
        if self.h:
            lib().aln_batch_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def dims(self, p):
        return len(self.qpool.seqs[self.q_idx[p]]), len(self.tpool.seqs[self.t_idx[p]])

    # --- DP ---------------------------------------------------------------------------------
    def _gap(self, align_type, gi, ge, tgi=None, tge=None, tcn=None, del_tables=None, ins_tables=None):
        g = _const_gap(align_type, gi, ge)                      # the model unless one of the following replaces it
        if ins_tables is not None:
            # fully tabulated gap functions: one T x T deletion table per template sequence, three T x Q insertion planes per pair
            g.model = GAP_TABLES
            dflat = [np.ascontiguousarray(t, dtype=np.float32).reshape(-1) for t in del_tables]
            doff = np.zeros(len(dflat), dtype=np.int64)
            doff[1:] = np.cumsum([len(t) for t in dflat])[:-1]
            iflat = [np.ascontiguousarray(t, dtype=np.float32).reshape(-1) for t in ins_tables]
            ioff = np.zeros(len(iflat), dtype=np.int64)
            ioff[1:] = np.cumsum([len(t) for t in iflat])[:-1]
            dblob, iblob = np.concatenate(dflat), np.concatenate(iflat)
            self._keep += [dblob, doff, iblob, ioff]
            g.del_table, g.del_table_off = _f(dblob), doff.ctypes.data_as(_lp)
            g.ins_tables, g.ins_table_off = _f(iblob), ioff.ctypes.data_as(_lp)
        elif del_tables is not None:
            # Gn2Eval model: v_gi / v_ge / v_cn over the template pool + one T x T deletion table per template sequence
            g.model = GAP_DEL_TABLE_INS_TPOS
            a, b, c = (np.ascontiguousarray(x, dtype=np.float32) for x in (tgi, tge, tcn))
            flat = [np.ascontiguousarray(t, dtype=np.float32).reshape(-1) for t in del_tables]
            off = np.zeros(len(flat), dtype=np.int64)
            off[1:] = np.cumsum([len(t) for t in flat])[:-1]
            blob = np.concatenate(flat)
            self._keep += [a, b, c, blob, off]
            g.t_gap_init, g.t_gap_extn, g.t_gap_cn = _f(a), _f(b), _f(c)
            g.del_table, g.del_table_off = _f(blob), off.ctypes.data_as(_lp)
        elif tgi is not None:
            g.model = GAP_AFFINE_TPOS_MIN
            a = np.ascontiguousarray(tgi, dtype=np.float32)
            b = np.ascontiguousarray(tge, dtype=np.float32)
            self._keep += [a, b]
            g.t_gap_init, g.t_gap_extn = _f(a), _f(b)
        return g

    def dp_submatrix(self, alphabet, table, align_type, gi, ge, direction=FWD, algo=DP_AUTO, bug_b4=False, tgi=None, tge=None):
        s = AlnSim()
        s.kind = SIM_SUBMATRIX
        tab = np.ascontiguousarray(table, dtype=np.float32)
        ab = alphabet.encode()
        s.sub = AlnSubmatrix(len(alphabet), ab, _f(tab))
        g = self._gap(align_type, gi, ge, tgi, tge)
        _check(lib().aln_batch_dp(self.h, C.byref(s), C.byref(g), direction, algo, int(bug_b4)), self.ctx.h)

    def dp_simmatrix(self, planes, align_type, gi, ge, direction=FWD, algo=DP_AUTO, bug_b4=False, tgi=None, tge=None, tcn=None,
                     del_tables=None, ins_tables=None):
        """planes: list of Q x T float32 arrays, one per pair."""
        flat = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in planes]
        off = np.zeros(len(flat) + 1, dtype=np.int64)
        np.cumsum([len(p) for p in flat], out=off[1:])
        blob = np.concatenate(flat) if flat else np.zeros(1, np.float32)
        s = AlnSim()
        s.kind = SIM_MATRIX
        s.planes = _f(blob)
        s.plane_off = off.ctypes.data_as(_lp)
        g = self._gap(align_type, gi, ge, tgi, tge, tcn, del_tables, ins_tables)
        _check(lib().aln_batch_dp(self.h, C.byref(s), C.byref(g), direction, algo, int(bug_b4)), self.ctx.h)

    def dp_sub_submatrix(self, alphabet, table, align_type, gi, ge, direction, bounds):
        """7-argument DPMatrix ctor: bounds[p] = (q1_end, t1_end, q2_beg, t2_beg)."""
        s = AlnSim()
        s.kind = SIM_SUBMATRIX
        tab = np.ascontiguousarray(table, dtype=np.float32)
        ab = alphabet.encode()
        s.sub = AlnSubmatrix(len(alphabet), ab, _f(tab))
        g = self._gap(align_type, gi, ge)
        bd = np.ascontiguousarray(bounds, dtype=np.int32).reshape(-1)
        _check(lib().aln_batch_dp_sub(self.h, C.byref(s), C.byref(g), direction, _i(bd)), self.ctx.h)

    def dp_hmap2(self, qprof, tprof, align_type, gi, ge, alpha=0.5, beta=1.0, zero_shift=0.12, normalize=True, direction=FWD,
                 algo=DP_AUTO):
        """Hmap2Eval on the device.  qprof/tprof: dicts aa[n,20], sse[n,3], conf[n] over the POOLS (sentinels included).
        pre_calculate (gap arrays from p_coil) runs on the host through aln_hmap2_gap_arrays."""
        arrs = [np.ascontiguousarray(x, dtype=np.float32) for x in (qprof["aa"], qprof["sse"], qprof["conf"], tprof["aa"], tprof["sse"], tprof["conf"])]
        nt = len(arrs[5])
        tgi = np.zeros(nt, dtype=np.float32)
        tge = np.zeros(nt, dtype=np.float32)
        _check(lib().aln_hmap2_gap_arrays(_f(arrs[4]), nt, float(np.float32(gi)), float(np.float32(ge)), float(np.float32(beta)), _f(tgi), _f(tge)))
        s = AlnSim()
        s.kind = SIM_HMAP2
        s.q_prof = AlnProfiles(_f(arrs[0]), _f(arrs[1]), _f(arrs[2]))
        s.t_prof = AlnProfiles(_f(arrs[3]), _f(arrs[4]), _f(arrs[5]))
        s.alpha = float(np.float32(alpha))
        s.zero_shift = float(np.float32(zero_shift))
        s.normalize = int(bool(normalize))
        g = self._gap(align_type, 0, 0, tgi, tge)
        _check(lib().aln_batch_dp(self.h, C.byref(s), C.byref(g), direction, algo, 0), self.ctx.h)
        return tgi, tge

    def set_gap(self, align_type, gi=0, ge=0, tgi=None, tge=None, tcn=None, del_tables=None, ins_tables=None):
        """aln_batch_set_gap: new gap parameters for the resident batch (similarity untouched); follow with reevaluate()."""
        g = self._gap(align_type, gi, ge, tgi, tge, tcn, del_tables, ins_tables)
        _check(lib().aln_batch_set_gap(self.h, C.byref(g)), self.ctx.h)

    def reevaluate(self):
        _check(lib().aln_batch_reevaluate(self.h), self.ctx.h)

    def kernel_name(self):
        return lib().aln_batch_dp_kernel_name(self.h).decode()

    def last_exact_stats(self):
        """hint exact_debug: far chunks (tested, skipped) of the deletion and the insertion scans of the last tiled exact build"""
        out = (C.c_uint64 * 4)()
        _check(lib().aln_batch_last_exact_stats(self.h, out), self.ctx.h)
        return [int(x) for x in out]

    def last_dp_ms(self):
        ms = C.c_float(0)
        _check(lib().aln_batch_last_dp_ms(self.h, C.byref(ms)), self.ctx.h)
        return ms.value

    def dp_ms_history(self, n):
        ms = np.zeros(n, dtype=np.float32)
        got = lib().aln_batch_dp_ms_history(self.h, _f(ms), n)
        if got < 0:
            raise AlnError(E_HIP, "aln_batch_dp_ms_history")
        return ms[:got]

    def cells(self):
        return lib().aln_batch_cells(self.h)

    def algorithmic_bytes(self):
        """bytes one DP launch must write with the chosen plane layout (4, 6 or 8 B per matrix cell)"""
        return lib().aln_batch_dp_algorithmic_bytes(self.h)

    def contract_bytes(self):
        """SURVEY 8(d)'s figure: 8 B per matrix cell (fp32 score + 32-bit pointer), whatever layout was chosen"""
        return lib().aln_batch_dp_contract_bytes(self.h)

    def plane_bytes_per_cell(self):
        return lib().aln_batch_plane_bytes_per_cell(self.h)

    def device_bytes(self):
        return lib().aln_batch_device_bytes(self.h)

    # --- results -----------------------------------------------------------------------------
    def get_cells(self, p):
        Q, T = self.dims(p)
        D = np.empty((Q, T), dtype=np.float32)
        PQ = np.empty((Q, T), dtype=np.int32)
        PT = np.empty((Q, T), dtype=np.int32)
        _check(lib().aln_batch_get_cells(self.h, p, _f(D), _i(PQ), _i(PT)), self.ctx.h)
        return D, PQ, PT

    def get_sim(self, p):
        Q, T = self.dims(p)
        S = np.empty((Q, T), dtype=np.float32)
        _check(lib().aln_batch_get_sim(self.h, p, _f(S)), self.ctx.h)
        return S

    def corner_scores(self):
        s = np.empty(self.n, dtype=np.float32)
        _check(lib().aln_batch_get_corner_scores(self.h, _f(s)), self.ctx.h)
        return s

    def enumerate(self, p, kind, number_suboptimal, delta_ratio, flags=None, user_limit=0, max_alignments=None, pairs_capacity=None,
                  k_limit=0, sort_limit=0, max_overlap=0.30, existing_scores=None):
        """ConstrainedNearOptimal ("cw") / UnconstrainedNearOptimal ("ucw") / KSConstrainedNearOptimal ("kscw") /
        CRConstrainedNearOptimal ("crcw") for pair p -> list of dicts in set order.  existing_scores: None seeds the set with the
        pair's Optimal alignment; a sequence (possibly empty) is the scores of the set the caller already holds, and those
        entries come back as dict(score=..., existing=their old index)."""
        Q, T = self.dims(p)
        ex, n_ex = None, -1
        if existing_scores is not None:
            ex = np.ascontiguousarray(existing_scores, dtype=np.float32)
            n_ex = len(ex)
        noa = AlnNoa(_ENUM[kind], int(number_suboptimal), float(np.float32(delta_ratio)),
                     int(user_limit), n_ex, _f(ex) if n_ex > 0 else None, int(k_limit), int(sort_limit), float(np.float32(max_overlap)))
        if max_alignments is None:
            max_alignments = max(int(number_suboptimal), 1) + 2
        if pairs_capacity is None:
            pairs_capacity = max_alignments * (min(Q, T) + 3)
        out = (AlnAlignment * max_alignments)()
        pairs = np.zeros((pairs_capacity, 2), dtype=np.int32)
        n = C.c_int32(0)
        fl = None
        if flags is not None:
            fl = np.ascontiguousarray(flags, dtype=np.uint8)
            assert len(fl) == T
        _check(lib().aln_batch_enumerate(self.h, p, C.byref(noa), fl.ctypes.data_as(C.POINTER(C.c_uint8)) if fl is not None else None,
                                         out, max_alignments, _i(pairs), pairs_capacity, C.byref(n)), self.ctx.h)
        res = []
        for k in range(n.value):
            a = out[k]
            if a.n_pairs == -1:
                res.append({"score": np.float32(a.score), "existing": a.pair_off})
                continue
            res.append({"score": np.float32(a.score), "identity": np.float32(a.identity), "uid": a.uid,
                        "pairs": pairs[a.pair_off:a.pair_off + a.n_pairs].copy()})
        return res

    def enumerate_all(self, kind, number_suboptimal, delta_ratio, flags=None, K=None, user_limit=0, node_cap=0, ali_cap=0,
                      want_pairs=True, raise_on_overflow=True, k_limit=0, sort_limit=0, max_overlap=0.30):
        """aln_batch_enumerate_all: every pair of the batch in one launch.  flags: None, one shared row, or an
        [n, stride] uint8 array.  -> n_out[n], scores[n,K], lengths[n,K], pairs[n,K,stride,2] or None, status[n]"""
        noa = AlnNoa(_ENUM[kind], int(number_suboptimal), float(np.float32(delta_ratio)),
                     int(user_limit), -1, None, int(k_limit), int(sort_limit), float(np.float32(max_overlap)))
        if K is None:
            K = max(int(number_suboptimal), 1) + 2
        fl, fstride = None, 0
        if flags is not None:
            fl = np.ascontiguousarray(flags, dtype=np.uint8)
            fstride = fl.shape[1] if fl.ndim == 2 else 0
        if not hasattr(self, "_stride"):
            self._stride = max(min(max(self.dims(p)[0] for p in range(self.n)), max(self.dims(p)[1] for p in range(self.n))) + 3, 4) if self.n else 4
        stride = self._stride
        n_out = np.zeros(self.n, dtype=np.int32)
        scores = np.zeros((self.n, K), dtype=np.float32)
        lengths = np.zeros((self.n, K), dtype=np.int32)
        status = np.zeros(self.n, dtype=np.int32)
        pairs = np.zeros((self.n, K, stride, 2), dtype=np.int32) if want_pairs else None
        rc = lib().aln_batch_enumerate_all(self.h, C.byref(noa), fl.ctypes.data_as(C.POINTER(C.c_uint8)) if fl is not None else None, fstride,
                                           int(node_cap), int(ali_cap), K, _i(n_out), _f(scores), _i(lengths),
                                           _i(pairs) if want_pairs else None, stride, _i(status))
        if rc != 0 and (raise_on_overflow or rc != E_OVERFLOW):
            _check(rc, self.ctx.h)
        return n_out, scores, lengths, pairs, status

    def last_enum_usage(self):
        """-> alignments created, trie nodes used, per pair, by the last enumerate_all (also for overflowed pairs)"""
        a = np.zeros(self.n, dtype=np.int32)
        nd = np.zeros(self.n, dtype=np.int32)
        _check(lib().aln_batch_last_enum_usage(self.h, _i(a), _i(nd)), self.ctx.h)
        return a, nd

    def last_enum_tasks(self):
        """-> tickets the several-wave kernel handed out per pair in the last enumerate_all (0: the one-wave kernel searched it)"""
        t = np.zeros(self.n, dtype=np.int32)
        _check(lib().aln_batch_last_enum_tasks(self.h, _i(t)), self.ctx.h)
        return t

    def last_enum_ms(self):
        a, b = C.c_float(0), C.c_float(0)
        _check(lib().aln_batch_last_enum_ms(self.h, C.byref(a), C.byref(b)), self.ctx.h)
        return a.value, b.value

    def optimal_enqueue(self):
        """Launch find_max + traceback + the copy of the results into a pinned slot; returns at once (two slots)."""
        _check(lib().aln_batch_optimal_enqueue(self.h), self.ctx.h)

    def optimal_collect(self):
        """Wait for the oldest enqueued slot -> scores[n], list lengths[n], status[n]."""
        scores = np.empty(self.n, dtype=np.float32)
        cnt = np.zeros(self.n, dtype=np.int32)
        status = np.zeros(self.n, dtype=np.int32)
        _check(lib().aln_batch_optimal_collect(self.h, _f(scores), _i(cnt), _i(status)), self.ctx.h)
        return scores, cnt, status

    def _string_buffers(self):
        stride = max(sum(self.dims(p)) for p in range(self.n)) + 2 if self.n else 4
        if not hasattr(self, "_tl") or len(self._tl) < self.n * stride:
            self._tl = C.create_string_buffer(max(self.n * stride, 1))
            self._ql = C.create_string_buffer(max(self.n * stride, 1))
        return stride

    def optimal_strings_enqueue(self):
        """Launch find_max + traceback + the string kernel and the copy of the lines into a pinned slot; returns at once (two slots)."""
        _check(lib().aln_batch_optimal_strings_enqueue(self.h, self._string_buffers()), self.ctx.h)

    def optimal_strings_collect(self, decode=True):
        """Wait for the oldest enqueued slot -> like optimal_strings."""
        return self._strings(lib().aln_batch_optimal_strings_collect, decode)

    def optimal_strings(self, decode=True):
        """aln_batch_optimal_strings -> scores[n], identity[n], status[n], template lines, query lines (lists of str, or the
        raw buffers + lengths when decode is False)."""
        return self._strings(lib().aln_batch_optimal_strings, decode)

    def _strings(self, fn, decode):
        scores = np.empty(self.n, dtype=np.float32)
        ident = np.zeros(self.n, dtype=np.float32)
        status = np.zeros(self.n, dtype=np.int32)
        lengths = np.zeros(self.n, dtype=np.int32)
        stride = self._string_buffers()
        rc = fn(self.h, _f(scores), _f(ident), _i(status), self._tl, self._ql, stride, _i(lengths))
        if rc != 0 and rc != E_STARTPAIR:
            _check(rc, self.ctx.h)
        if not decode:
            return scores, ident, status, self._tl, self._ql, lengths, stride
        tl = [self._tl.raw[p * stride:p * stride + lengths[p]].decode() for p in range(self.n)]
        ql = [self._ql.raw[p * stride:p * stride + lengths[p]].decode() for p in range(self.n)]
        return scores, ident, status, tl, ql

    def optimal(self, want_pairs=True, subali=False):
        """-> scores[n], list of pair arrays (list order), status[n]"""
        scores = np.empty(self.n, dtype=np.float32)
        cnt = np.zeros(self.n, dtype=np.int32)
        status = np.zeros(self.n, dtype=np.int32)
        if not hasattr(self, "_stride"):
            self._stride = max(min(max(self.dims(p)[0] for p in range(self.n)), max(self.dims(p)[1] for p in range(self.n))) + 3, 4) if self.n else 4
        stride = self._stride
        pairs = np.zeros((self.n, stride, 2), dtype=np.int32) if want_pairs else None
        fn = lib().aln_batch_optimal_subali if subali else lib().aln_batch_optimal
        _check(fn(self.h, _f(scores), _i(cnt), _i(pairs) if want_pairs else None, stride, _i(status)), self.ctx.h)
        lists = [pairs[p, :cnt[p]].copy() for p in range(self.n)] if want_pairs else None
        return scores, lists, status
