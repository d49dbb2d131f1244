"""CPU-only: aln_amd.shuffle_order (the Python statement of the order aln_hits_zscores_profiles reads a profile's rows in), the
int64 reference of the profile z-scores (profile_zscore_cases) against the residue one (search_cases), and
aln_hits_zscores_profiles at the ABI boundary: exported and bound, named in the header with its hint, a NULL context refused
before anything is touched."""
import ctypes as C
import inspect
import os

import numpy as np

import aln_amd
import profile_cases as pc
import profile_zscore_cases as pz
import range_cases as rc
import search_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AA = "ACDEFGHIKLMNPQRSTVWY"
MODES = (rc.LOCAL, rc.GLOBAL, rc.GLOBAL_LOCAL, rc.LOCAL_GLOBAL, rc.SEMI_LOCAL)


# ---- the order -----------------------------------------------------------------------------------------------------------
def test_pinned_orders():
    """the pinned strings of tests/test_zscore_shuffle.py, read through the order"""
    for (seed, q, s), want in [((12345, 3, 7), "YVHTLMIKSNCEARDPGQFW"), ((12345, 3, 8), "IETGNQYHFSCPRMAVDWLK"),
                               ((0, 0, 0), "NQEMWKLRICHFDATSPYVG"), ((0xFFFFFFFF, 70000, 4095), "EHKTIGSYMDACVQWLRNFP")]:
        assert "".join(AA[k] for k in aln_amd.shuffle_order(seed, q, s, 20)) == want, (seed, q, s)


def test_order_is_a_permutation():
    for n in (2, 3, 20, 257):
        for s in range(5):
            a = aln_amd.shuffle_order(77, 4, s, n)
            assert sorted(a) == list(range(n))
    for s in range(4):
        assert aln_amd.shuffle_order(9, 1, s, 0) == []
        assert aln_amd.shuffle_order(9, 1, s, 1) == [0]


def test_shuffle_query_is_the_order_applied():
    for x in ("", "W", "AC", (AA * 13)[:257], AA):
        for seed, q, s in ((77, 4, 0), (77, 4, 3), (0xFFFFFFFF, 70000, 4095)):
            assert aln_amd.shuffle_query(seed, q, s, x) == "".join(x[k] for k in aln_amd.shuffle_order(seed, q, s, len(x)))


# ---- the reference -------------------------------------------------------------------------------------------------------
def test_shuffled_permutes_rows():
    prof = np.arange(7 * pc.N).reshape(7, pc.N)
    out = pz.shuffled(5, 2, 1, prof)
    a = aln_amd.shuffle_order(5, 2, 1, 7)
    assert a != list(range(7)) and out.shape == prof.shape
    for i in range(7):
        assert (out[i] == prof[a[i]]).all()
    assert pz.shuffled(5, 2, 1, np.zeros((0, pc.N), np.int64)).shape == (0, pc.N)


def test_derived_profiles_have_the_residue_statistics():
    """row i = the table row of residue i: permuting rows is permuting residues"""
    q, t = rc.random_seq(pc.ALPHA, 610, 20), rc.random_seq(pc.ALPHA, 611, 30)
    prof = pc.derived([q], sc.TABLES["blosum62"])[0]
    spread = 0
    for mode in MODES:
        got = pz.zstats_reference(2024, 3, prof, t, mode, 11, 1, 4)
        want = sc.zstats_reference(2024, 3, q, t, "blosum62", mode, 11, 1, 4)
        assert got == want, mode
        spread += len(set(got[2])) > 1
    assert spread >= 3                                       # the shuffles do score differently


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def test_hits_zscores_profiles_is_exported_and_bound():
    if not os.path.exists(aln_amd.LIB_PATH):
        aln_amd.build_library()
    L = C.CDLL(aln_amd.LIB_PATH)
    assert hasattr(L, "aln_hits_zscores_profiles")
    assert "aln_hits_zscores_profiles" in aln_amd.EXPORTS
    argtypes = aln_amd.lib().aln_hits_zscores_profiles.argtypes
    assert len(argtypes) == 12
    assert argtypes[1:4] == [C.POINTER(aln_amd.AlnQProfiles), C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnGap)]
    assert argtypes[10] == C.c_uint32 and argtypes[11] == C.POINTER(aln_amd.AlnHitStats)


def test_the_wrappers_exist():
    assert callable(aln_amd.shuffle_order)
    assert list(inspect.signature(aln_amd.shuffle_order).parameters) == ["seed", "q_index", "s", "n"]
    names = list(inspect.signature(aln_amd.hits_zscores_profiles).parameters)
    assert names == ["ctx", "profiles", "templates", "hits", "n_hits", "gi", "ge", "n_shuffles", "seed", "q_begin", "align_type"]


def test_the_header_names_the_entry_and_the_hint():
    header = open(os.path.join(ROOT, "include", "aln_hip.h")).read()
    assert "int aln_hits_zscores_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* templates, const aln_gap* gap," in header
    assert "aln_hits_zscores still takes residue queries only" in header
    assert '"zscore_rows_per_chunk"' in header and "ALN_ZSCORE_ROWS_PER_CHUNK" in header
    hints = open(os.path.join(ROOT, "alignment-algos_amd", "csrc", "aln_hints.hip")).read()
    assert '"zscore_rows_per_chunk", "ALN_ZSCORE_ROWS_PER_CHUNK"' in hints


def test_a_null_context_is_refused():
    qp = aln_amd.QueryProfiles([np.ones((3, 2), np.float32)], "AC")
    tp = aln_amd.SeqPool(["ACA"])
    g = aln_amd.AlnGap()
    g.model, g.align_type, g.gap_init, g.gap_extn = aln_amd.GAP_AFFINE_CONST, aln_amd.LOCAL, 11.0, 1.0
    hits = np.zeros((1, 1), dtype=aln_amd.HIT_DTYPE)
    n_hits = np.ones(1, np.int32)
    stats = np.full(24, 0x5A, dtype=np.uint8)
    rc_ = aln_amd.lib().aln_hits_zscores_profiles(None, C.byref(qp.c), C.byref(tp.c), C.byref(g), 0, 1, 1,
                                                  hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)),
                                                  n_hits.ctypes.data_as(C.POINTER(C.c_int32)), 4, 7,
                                                  stats.ctypes.data_as(C.POINTER(aln_amd.AlnHitStats)))
    assert rc_ == aln_amd.E_ARG and stats.tobytes() == bytes([0x5A]) * 24
