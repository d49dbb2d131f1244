"""aln_hits_align_profiles at the ABI boundary (no GPU): the symbol is exported and bound, the Python wrapper exists, the header
names the entry and its hint, and a NULL context is refused before anything is touched."""
import ctypes as C
import os

import numpy as np

import aln_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hits_align_profiles_is_exported_and_bound():
    if not os.path.exists(aln_amd.LIB_PATH):
        aln_amd.build_library()
    L = C.CDLL(aln_amd.LIB_PATH)
    assert hasattr(L, "aln_hits_align_profiles")
    assert "aln_hits_align_profiles" in aln_amd.EXPORTS
    argtypes = aln_amd.lib().aln_hits_align_profiles.argtypes
    assert len(argtypes) == 17
    assert argtypes[1:4] == [C.POINTER(aln_amd.AlnQProfiles), C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnSeqs)]
    assert argtypes[10] == C.POINTER(aln_amd.AlnHitAlignment)


def test_the_wrapper_is_callable():
    assert callable(aln_amd.hits_align_profiles)
    import inspect
    names = list(inspect.signature(aln_amd.hits_align_profiles).parameters)
    assert names[:7] == ["ctx", "profiles", "templates", "hits", "n_hits", "gi", "ge"]
    for name in ("consensus", "q_begin", "align_type", "want_pairs", "want_lines", "pair_stride", "line_stride"):
        assert name in names


def test_the_header_names_the_entry_and_the_hint():
    header = open(os.path.join(ROOT, "include", "aln_hip.h")).read()
    assert "int aln_hits_align_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus" in header
    assert '"align_rows_per_chunk"' in header and "ALN_ALIGN_ROWS_PER_CHUNK" in header
    assert "aln_amd.profile_planes" not in header                    # the paragraph that sent profile hits through planes is gone
    assert "aln_hits_zscores still takes residue queries only" in header
    hints = open(os.path.join(ROOT, "alignment-algos_amd", "csrc", "aln_hints.hip")).read()
    assert '"align_rows_per_chunk", "ALN_ALIGN_ROWS_PER_CHUNK"' in hints


def test_a_null_context_is_refused():
    qp = aln_amd.QueryProfiles([np.ones((3, 2), np.float32)], "AC")
    tp = aln_amd.SeqPool(["ACA"])
    g = aln_amd.AlnGap()
    g.model, g.align_type, g.gap_init, g.gap_extn = aln_amd.GAP_AFFINE_CONST, aln_amd.LOCAL, 11.0, 1.0
    hits = np.zeros((1, 1), dtype=aln_amd.HIT_DTYPE)
    n_hits = np.ones(1, np.int32)
    rec = np.frombuffer(bytearray([0x5A]) * 16, dtype=aln_amd.HIT_ALIGNMENT_DTYPE).copy()
    rc = aln_amd.lib().aln_hits_align_profiles(None, C.byref(qp.c), None, C.byref(tp.c), C.byref(g), 0, 1, 1,
                                               hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits.ctypes.data_as(C.POINTER(C.c_int32)),
                                               rec.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)), None, 0, None, None, 0, None)
    assert rc == aln_amd.E_ARG and rec.tobytes() == bytes([0x5A]) * 16
