"""aln_hits_pileup / aln_hits_pileup_profiles at the ABI boundary (no GPU): both symbols are exported and bound, the Python
wrappers exist, the header carries the definition in its place, and a NULL context is refused before anything is touched."""
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
    for name in ("aln_hits_pileup", "aln_hits_pileup_profiles"):
        assert hasattr(L, name)
        assert name in aln_amd.EXPORTS
    tail = [C.POINTER(aln_amd.AlnHit), _ip, C.POINTER(aln_amd.AlnHitAlignment), C.POINTER(aln_amd.AlnHitSpan), C.POINTER(C.c_uint8),
            C.POINTER(C.c_uint16), C.c_int32]
    a = aln_amd.lib().aln_hits_pileup.argtypes
    assert len(a) == 15
    assert a[1:5] == [C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnSubmatrix), C.POINTER(aln_amd.AlnGap)]
    assert a[8:] == tail
    p = aln_amd.lib().aln_hits_pileup_profiles.argtypes
    assert len(p) == 15
    assert p[1:5] == [C.POINTER(aln_amd.AlnQProfiles), C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnGap)]
    assert p[8:] == tail
    assert C.sizeof(aln_amd.AlnHitSpan) == 16 == aln_amd.HIT_SPAN_DTYPE.itemsize
    assert aln_amd.HIT_SPAN_DTYPE.names == ("q_lo", "q_hi", "t_lo", "t_hi") == tuple(f[0] for f in aln_amd.AlnHitSpan._fields_)


def test_the_wrappers_are_callable():
    names = list(inspect.signature(aln_amd.hits_pileup).parameters)
    assert names[:9] == ["ctx", "queries", "templates", "hits", "n_hits", "alphabet", "table", "gi", "ge"]
    assert names[9:] == ["q_begin", "align_type", "want_letters", "want_tpos", "want_spans", "line_stride"]
    names = list(inspect.signature(aln_amd.hits_pileup_profiles).parameters)
    assert names[:8] == ["ctx", "profiles", "templates", "hits", "n_hits", "gi", "ge", "consensus"]
    for name in ("q_begin", "align_type", "want_letters", "want_tpos", "want_spans", "line_stride"):
        assert name in names
    for f in (aln_amd.counts_from_pileup, aln_amd.a3m_from_pileup):
        assert callable(f) and f.__doc__


def test_the_header_carries_the_definition_in_its_place():
    header = open(os.path.join(ROOT, "include", "aln_hip.h")).read()
    assert "typedef struct { int32_t q_lo, q_hi, t_lo, t_hi; } aln_hit_span;" in header
    assert "int aln_hits_pileup(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub," in header
    assert "int aln_hits_pileup_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus" in header
    assert header.index("int aln_hits_column_counts_profiles(") < header.index("aln_hit_span;") < header.index(
        "int aln_hits_pileup(") < header.index("int aln_hits_pileup_profiles(") < header.index("int aln_hits_align_multi(")
    for sentence in ("A slot CONTRIBUTES when its status is 0 and, ALN_LOCAL, its score is > 0",
                     "query position i (1 <= i <= Q-2)\n * stands at index p = i - 1 of the slot's line",
                     "tpos = 0, letters = '-'", "tpos = 0, letters = '.'",
                     "spans[s] = { i_lo, i_hi, the j of i_lo, the j of i_hi }",
                     "uint16_t holds every position",
                     "spans, letters and tpos are independent and each may be NULL",
                     "line_stride < Q-2 for any query of",
                     "every output is byte-identical to aln_hits_pileup's on those residues",
                     "aln_hits_pileup(_profiles) call on this context"):
        assert sentence in header, sentence


def _gap():
    g = aln_amd.AlnGap()
    g.model, g.align_type, g.gap_init, g.gap_extn = aln_amd.GAP_AFFINE_CONST, aln_amd.LOCAL, 11.0, 1.0
    return g


class _Outputs:
    def __init__(self):
        self.rec = np.full(16, 0x5A, np.uint8)
        self.spans = np.full(16, 0x5A, np.uint8)
        self.letters = np.full(8, 0x5A, np.uint8)
        self.tpos = np.full(8, 0x5A5A, np.uint16)

    def tail(self):
        return (self.rec.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)), self.spans.ctypes.data_as(C.POINTER(aln_amd.AlnHitSpan)),
                self.letters.ctypes.data_as(C.POINTER(C.c_uint8)), self.tpos.ctypes.data_as(C.POINTER(C.c_uint16)), 8)

    def untouched(self):
        return bool((self.rec == 0x5A).all() and (self.spans == 0x5A).all() and (self.letters == 0x5A).all() and
                    (self.tpos == 0x5A5A).all())


def test_a_null_context_is_refused():
    qp = aln_amd.SeqPool(["AC"])
    tp = aln_amd.SeqPool(["ACA"])
    tab = np.ones((2, 2), np.float32)
    sub = aln_amd.AlnSubmatrix(2, b"AC", tab.ctypes.data_as(C.POINTER(C.c_float)))
    g = _gap()
    hits = np.zeros((1, 1), dtype=aln_amd.HIT_DTYPE)
    n_hits = np.ones(1, np.int32)
    o = _Outputs()
    rc = aln_amd.lib().aln_hits_pileup(None, C.byref(qp.c), C.byref(tp.c), C.byref(sub), C.byref(g), 0, 1, 1,
                                       hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits.ctypes.data_as(_ip), *o.tail())
    assert rc == aln_amd.E_ARG and o.untouched()


def test_a_null_context_is_refused_by_the_profile_entry():
    qp = aln_amd.QueryProfiles([np.ones((2, 2), np.float32)], "AC")
    tp = aln_amd.SeqPool(["ACA"])
    g = _gap()
    hits = np.zeros((1, 1), dtype=aln_amd.HIT_DTYPE)
    n_hits = np.ones(1, np.int32)
    o = _Outputs()
    rc = aln_amd.lib().aln_hits_pileup_profiles(None, C.byref(qp.c), None, C.byref(tp.c), C.byref(g), 0, 1, 1,
                                                hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits.ctypes.data_as(_ip), *o.tail())
    assert rc == aln_amd.E_ARG and o.untouched()
