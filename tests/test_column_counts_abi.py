"""aln_hits_column_counts / aln_hits_column_counts_profiles at the ABI boundary (no GPU): both symbols are exported and bound,
the Python wrappers exist, the header names the entries, and a NULL context is refused before anything is touched."""
import ctypes as C
import inspect
import os

import numpy as np

import aln_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ip = C.POINTER(C.c_int32)


def test_both_entries_are_exported_and_bound():
    if not os.path.exists(aln_amd.LIB_PATH):
        aln_amd.build_library()
    L = C.CDLL(aln_amd.LIB_PATH)
    for name in ("aln_hits_column_counts", "aln_hits_column_counts_profiles"):
        assert hasattr(L, name)
        assert name in aln_amd.EXPORTS
    a = aln_amd.lib().aln_hits_column_counts.argtypes
    assert len(a) == 14
    assert a[1:4] == [C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnSubmatrix)]
    assert a[8] == C.POINTER(aln_amd.AlnHit) and a[11] == C.POINTER(aln_amd.AlnHitAlignment) and a[10] == a[12] == a[13] == _ip
    p = aln_amd.lib().aln_hits_column_counts_profiles.argtypes
    assert len(p) == 14
    assert p[1:4] == [C.POINTER(aln_amd.AlnQProfiles), C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnSeqs)]
    assert p[11] == C.POINTER(aln_amd.AlnHitAlignment) and p[10] == p[12] == p[13] == _ip


def test_the_wrappers_are_callable():
    names = list(inspect.signature(aln_amd.hits_column_counts).parameters)
    assert names[:9] == ["ctx", "queries", "templates", "hits", "n_hits", "alphabet", "table", "gi", "ge"]
    for name in ("weights", "q_begin", "align_type", "want_covered"):
        assert name in names
    names = list(inspect.signature(aln_amd.hits_column_counts_profiles).parameters)
    assert names[:7] == ["ctx", "profiles", "templates", "hits", "n_hits", "gi", "ge"]
    for name in ("consensus", "weights", "q_begin", "align_type", "want_covered"):
        assert name in names
    assert callable(aln_amd.pssm_from_counts) and aln_amd.pssm_from_counts.__doc__


def test_the_header_names_the_entries():
    header = open(os.path.join(ROOT, "include", "aln_hip.h")).read()
    assert "int aln_hits_column_counts(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates" in header
    assert "int aln_hits_column_counts_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus" in header
    assert header.index("int aln_hits_align_profiles(") < header.index("int aln_hits_column_counts(") < header.index(
        "int aln_hits_align_multi(")
    assert "every used slot's weight in 0..65535" in header
    assert "aln_amd.pssm_from_counts" in header                      # the profile paragraph says where profiles can come from


def test_align_list_group_slots_is_a_declared_hint():
    assert '"align_list_group_slots"' in open(os.path.join(ROOT, "include", "aln_hip.h")).read()
    hints = open(os.path.join(ROOT, "alignment-algos_amd", "csrc", "aln_hints.hip")).read()
    assert '"align_list_group_slots", "ALN_ALIGN_LIST_GROUP_SLOTS"' in hints
    assert "`align_list_group_slots`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _gap():
    g = aln_amd.AlnGap()
    g.model, g.align_type, g.gap_init, g.gap_extn = aln_amd.GAP_AFFINE_CONST, aln_amd.LOCAL, 11.0, 1.0
    return g


def test_a_null_context_is_refused():
    qp = aln_amd.SeqPool(["AC"])
    tp = aln_amd.SeqPool(["ACA"])
    tab = np.ones((2, 2), np.float32)
    sub = aln_amd.AlnSubmatrix(2, b"AC", tab.ctypes.data_as(C.POINTER(C.c_float)))
    g = _gap()
    hits = np.zeros((1, 1), dtype=aln_amd.HIT_DTYPE)
    n_hits = np.ones(1, np.int32)
    rec = np.frombuffer(bytearray([0x5A]) * 16, dtype=aln_amd.HIT_ALIGNMENT_DTYPE).copy()
    counts = np.full((4, 2), 0x5A5A5A5A, np.int32)
    covered = np.full(4, 0x5A5A5A5A, np.int32)
    rc = aln_amd.lib().aln_hits_column_counts(None, C.byref(qp.c), C.byref(tp.c), C.byref(sub), C.byref(g), 0, 1, 1,
                                              hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits.ctypes.data_as(_ip), None,
                                              rec.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)), counts.ctypes.data_as(_ip),
                                              covered.ctypes.data_as(_ip))
    assert rc == aln_amd.E_ARG
    assert rec.tobytes() == bytes([0x5A]) * 16 and (counts == 0x5A5A5A5A).all() and (covered == 0x5A5A5A5A).all()


def test_a_null_context_is_refused_by_the_profile_entry():
    qp = aln_amd.QueryProfiles([np.ones((2, 2), np.float32)], "AC")
    tp = aln_amd.SeqPool(["ACA"])
    g = _gap()
    hits = np.zeros((1, 1), dtype=aln_amd.HIT_DTYPE)
    n_hits = np.ones(1, np.int32)
    rec = np.frombuffer(bytearray([0x5A]) * 16, dtype=aln_amd.HIT_ALIGNMENT_DTYPE).copy()
    counts = np.full((4, 2), 0x5A5A5A5A, np.int32)
    rc = aln_amd.lib().aln_hits_column_counts_profiles(None, C.byref(qp.c), None, C.byref(tp.c), C.byref(g), 0, 1, 1,
                                                       hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits.ctypes.data_as(_ip),
                                                       None, rec.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)),
                                                       counts.ctypes.data_as(_ip), None)
    assert rc == aln_amd.E_ARG and rec.tobytes() == bytes([0x5A]) * 16 and (counts == 0x5A5A5A5A).all()
