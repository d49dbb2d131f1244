"""aln_hits_purge / aln_hits_purge_profiles at the ABI boundary (no GPU): both symbols are exported and bound, the record is 16
bytes, the Python wrappers exist, the header carries the definition in its place, and a NULL context is refused before
anything is touched."""
import ctypes as C
import inspect
import os

import numpy as np

import aln_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)


def test_both_entries_are_exported_and_bound():
    if not os.path.exists(aln_amd.LIB_PATH):
        aln_amd.build_library()
    L = C.CDLL(aln_amd.LIB_PATH)
    for name in ("aln_hits_purge", "aln_hits_purge_profiles"):
        assert hasattr(L, name)
        assert name in aln_amd.EXPORTS
    assert C.sizeof(aln_amd.AlnHitPurge) == 16 and aln_amd.HIT_PURGE_DTYPE.itemsize == 16
    assert [f[0] for f in aln_amd.AlnHitPurge._fields_] == ["keeper", "same", "overlap", "letters"] == list(aln_amd.HIT_PURGE_DTYPE.names)
    tail = [C.POINTER(aln_amd.AlnHit), _ip, C.c_int32, C.c_int32, C.c_int32, C.POINTER(aln_amd.AlnHitAlignment),
            C.POINTER(aln_amd.AlnHitPurge), _ip, _lp, _ip, _ip]
    a = aln_amd.lib().aln_hits_purge.argtypes
    assert len(a) == 19
    assert a[1:5] == [C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnSubmatrix), C.POINTER(aln_amd.AlnGap)]
    assert a[5:8] == [C.c_int32] * 3 and a[8:] == tail
    p = aln_amd.lib().aln_hits_purge_profiles.argtypes
    assert len(p) == 19
    assert p[1:5] == [C.POINTER(aln_amd.AlnQProfiles), C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnGap)]
    assert p[5:8] == [C.c_int32] * 3 and p[8:] == tail


def test_the_wrappers_are_callable():
    tail = ["max_identity", "min_overlap", "w_max", "q_begin", "align_type", "want_weights", "want_raw", "want_counts", "want_covered"]
    names = list(inspect.signature(aln_amd.hits_purge).parameters)
    assert names[:9] == ["ctx", "queries", "templates", "hits", "n_hits", "alphabet", "table", "gi", "ge"] and names[9:] == tail
    names = list(inspect.signature(aln_amd.hits_purge_profiles).parameters)
    assert names[:8] == ["ctx", "profiles", "templates", "hits", "n_hits", "gi", "ge", "consensus"] and names[8:] == tail
    assert list(inspect.signature(aln_amd.purge_from_pileup).parameters) == ["letters_row", "alphabet", "max_identity", "min_overlap"]
    for f in (aln_amd.hits_purge, aln_amd.hits_purge_profiles, aln_amd.purge_from_pileup):
        assert callable(f) and f.__doc__


def test_the_header_carries_the_definition_in_its_place():
    header = open(os.path.join(ROOT, "include", "aln_hip.h")).read()
    assert "typedef struct { int32_t keeper, same, overlap, letters; } aln_hit_purge;" in header
    assert "int aln_hits_purge(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub," in header
    assert "int aln_hits_purge_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus" in header
    assert header.index("int aln_hits_weights_profiles(") < header.index("} aln_hit_purge;") < header.index("int aln_hits_purge(") < \
        header.index("int aln_hits_purge_profiles(") < header.index("int aln_hits_align_multi(")
    for sentence in ("All of it is exact integer arithmetic",
                     "A slot CONTRIBUTES exactly when it does there: status 0 and, ALN_LOCAL, score > 0",
                     "'-', '.' and NUL never are letters",
                     "the number of positions where L[k][p] is a letter",
                     "for j < k, the number of positions where both rows show a letter",
                     "the number of those positions where the letters are equal",
                     "100 * overlap(j,k) >= min_overlap * letters(k)",
                     "100 * same(j,k) >= max_identity * overlap(j,k)",
                     "The products are at most 100 * 65532",
                     "slot k is KEPT when letters(k) > 0 and it\n * is near no KEPT slot j < k",
                     "its keeper is the smallest kept j it is near",
                     "purged slot purges nobody",
                     "max_identity is in 1..101; 101 can never be met",
                     "min_overlap is in 0..100; with 0 only overlap >= 1 is asked",
                     "kept { k, 0, 0, letters(k) }",
                     "purged by j { j, same(j,k), overlap(j,k), letters(k) }",
                     "unused, not contributing, or without a letter { -1, 0, 0, 0 }",
                     "weights may be NULL (purge only): then raw, counts and covered must be NULL too and w_max is not read",
                     "every slot that is not kept shows '.' at every position",
                     "what aln_hits_column_counts returns for the same hits under the returned weights",
                     "NULL purge; max_identity outside 1..101; min_overlap outside 0..100; weights == NULL\n * with any of raw / counts / covered given; w_max outside 1..65535 when weights is given",
                     "last, an alphabet that holds '.' or\n * '-'",
                     "every output is byte-identical to aln_hits_purge's on those residues",
                     "aln_hits_purge(_profiles) / aln_hits_weights(_profiles) / aln_hits_pileup(_profiles) call on this context"):
        assert sentence in header, sentence


def _gap():
    g = aln_amd.AlnGap()
    g.model, g.align_type, g.gap_init, g.gap_extn = aln_amd.GAP_AFFINE_CONST, aln_amd.LOCAL, 11.0, 1.0
    return g


class _Outputs:
    def __init__(self):
        self.rec = np.full(16, 0x5A, np.uint8)
        self.purge = np.full(16, 0x5A, np.uint8)
        self.weights = np.full(1, 0x5A5A5A5A, np.int32)
        self.raw = np.full(1, 0x5A5A5A5A5A5A5A5A, np.int64)
        self.counts = np.full(5 * 2, 0x5A5A5A5A, np.int32)
        self.covered = np.full(5, 0x5A5A5A5A, np.int32)

    def tail(self):
        return (90, 50, 1000, self.rec.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)),
                self.purge.ctypes.data_as(C.POINTER(aln_amd.AlnHitPurge)), self.weights.ctypes.data_as(_ip),
                self.raw.ctypes.data_as(_lp), self.counts.ctypes.data_as(_ip), self.covered.ctypes.data_as(_ip))

    def untouched(self):
        return bool((self.rec == 0x5A).all() and (self.purge == 0x5A).all() and (self.weights == 0x5A5A5A5A).all() and
                    (self.raw == 0x5A5A5A5A5A5A5A5A).all() and (self.counts == 0x5A5A5A5A).all() and (self.covered == 0x5A5A5A5A).all())


def test_a_null_context_is_refused():
    qp = aln_amd.SeqPool(["ACA"])
    tp = aln_amd.SeqPool(["ACA"])
    tab = np.ones((2, 2), np.float32)
    sub = aln_amd.AlnSubmatrix(2, b"AC", tab.ctypes.data_as(C.POINTER(C.c_float)))
    g = _gap()
    hits = np.zeros((1, 1), dtype=aln_amd.HIT_DTYPE)
    n_hits = np.ones(1, np.int32)
    o = _Outputs()
    rc = aln_amd.lib().aln_hits_purge(None, C.byref(qp.c), C.byref(tp.c), C.byref(sub), C.byref(g), 0, 1, 1,
                                      hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits.ctypes.data_as(_ip), *o.tail())
    assert rc == aln_amd.E_ARG and o.untouched()


def test_a_null_context_is_refused_by_the_profile_entry():
    qp = aln_amd.QueryProfiles([np.ones((3, 2), np.float32)], "AC")
    tp = aln_amd.SeqPool(["ACA"])
    g = _gap()
    hits = np.zeros((1, 1), dtype=aln_amd.HIT_DTYPE)
    n_hits = np.ones(1, np.int32)
    o = _Outputs()
    rc = aln_amd.lib().aln_hits_purge_profiles(None, C.byref(qp.c), None, C.byref(tp.c), C.byref(g), 0, 1, 1,
                                               hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits.ctypes.data_as(_ip), *o.tail())
    assert rc == aln_amd.E_ARG and o.untouched()
