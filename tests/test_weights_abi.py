"""aln_hits_weights / aln_hits_weights_profiles at the ABI boundary (no GPU): both symbols are exported and bound, the Python
wrappers exist, the header carries the definition in its place, the hint is declared, and a NULL context is refused before
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
    for name in ("aln_hits_weights", "aln_hits_weights_profiles"):
        assert hasattr(L, name)
        assert name in aln_amd.EXPORTS
    tail = [C.POINTER(aln_amd.AlnHit), _ip, C.c_int32, C.POINTER(aln_amd.AlnHitAlignment), _ip, _lp, _ip, _ip]
    a = aln_amd.lib().aln_hits_weights.argtypes
    assert len(a) == 16
    assert a[1:5] == [C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnSubmatrix), C.POINTER(aln_amd.AlnGap)]
    assert a[5:8] == [C.c_int32] * 3 and a[8:] == tail
    p = aln_amd.lib().aln_hits_weights_profiles.argtypes
    assert len(p) == 16
    assert p[1:5] == [C.POINTER(aln_amd.AlnQProfiles), C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnGap)]
    assert p[5:8] == [C.c_int32] * 3 and p[8:] == tail


def test_the_wrappers_are_callable():
    names = list(inspect.signature(aln_amd.hits_weights).parameters)
    assert names[:9] == ["ctx", "queries", "templates", "hits", "n_hits", "alphabet", "table", "gi", "ge"]
    assert names[9:] == ["w_max", "q_begin", "align_type", "want_raw", "want_counts", "want_covered"]
    names = list(inspect.signature(aln_amd.hits_weights_profiles).parameters)
    assert names[:8] == ["ctx", "profiles", "templates", "hits", "n_hits", "gi", "ge", "consensus"]
    assert names[8:] == ["w_max", "q_begin", "align_type", "want_raw", "want_counts", "want_covered"]
    assert list(inspect.signature(aln_amd.weights_from_pileup).parameters) == ["letters_row", "alphabet", "w_max"]
    for f in (aln_amd.hits_weights, aln_amd.hits_weights_profiles, aln_amd.weights_from_pileup):
        assert callable(f) and f.__doc__


def test_the_header_carries_the_definition_in_its_place():
    header = open(os.path.join(ROOT, "include", "aln_hip.h")).read()
    assert "int aln_hits_weights(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub," in header
    assert "int aln_hits_weights_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus" in header
    assert header.index("int aln_hits_pileup_profiles(") < header.index("int aln_hits_weights(") < header.index(
        "int aln_hits_weights_profiles(") < header.index("int aln_hits_align_multi(")
    for sentence in ("Everything is exact integer arithmetic",
                     "A slot CONTRIBUTES exactly when it does there: status 0 and, ALN_LOCAL, score > 0",
                     "'-', '.' and NUL never do",
                     "the number of contributing slots with L[k][p] == alphabet[a]",
                     "the number of letters a with n_p[a] > 0",
                     "floor(2^24 / (k_p * n_p[a]))",
                     "0 where raw[k] == 0, otherwise max(1, floor(w_max * raw[k] / M)) in 64-bit integers",
                     "gets exactly w_max",
                     "w_max is in 1..65535",
                     "The query itself is not a member of the stack",
                     "what aln_hits_column_counts returns for the same\n * hits with `weights` set to this call's weights",
                     "NULL weights, w_max outside 1..65535 (ALN_E_ARG)",
                     "last, an alphabet that holds '.' or '-'",
                     "every\n * output is byte-identical to aln_hits_weights' on those residues",
                     "aln_hits_weights(_profiles) / aln_hits_pileup(_profiles) call on this context"):
        assert sentence in header, sentence


def test_weights_group_rows_is_a_declared_hint():
    assert '"weights_group_rows"' in open(os.path.join(ROOT, "include", "aln_hip.h")).read()
    hints = open(os.path.join(ROOT, "alignment-algos_amd", "csrc", "aln_hints.hip")).read()
    assert '"weights_group_rows", "ALN_WEIGHTS_GROUP_ROWS"' in hints
    assert "`weights_group_rows`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _gap():
    g = aln_amd.AlnGap()
    g.model, g.align_type, g.gap_init, g.gap_extn = aln_amd.GAP_AFFINE_CONST, aln_amd.LOCAL, 11.0, 1.0
    return g


class _Outputs:
    def __init__(self):
        self.rec = np.full(16, 0x5A, np.uint8)
        self.weights = np.full(1, 0x5A5A5A5A, np.int32)
        self.raw = np.full(1, 0x5A5A5A5A5A5A5A5A, np.int64)
        self.counts = np.full(5 * 2, 0x5A5A5A5A, np.int32)
        self.covered = np.full(5, 0x5A5A5A5A, np.int32)

    def tail(self):
        return (1000, self.rec.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)), self.weights.ctypes.data_as(_ip),
                self.raw.ctypes.data_as(_lp), self.counts.ctypes.data_as(_ip), self.covered.ctypes.data_as(_ip))

    def untouched(self):
        return bool((self.rec == 0x5A).all() and (self.weights == 0x5A5A5A5A).all() and (self.raw == 0x5A5A5A5A5A5A5A5A).all() and
                    (self.counts == 0x5A5A5A5A).all() and (self.covered == 0x5A5A5A5A).all())


def test_a_null_context_is_refused():
    qp = aln_amd.SeqPool(["ACA"])
    tp = aln_amd.SeqPool(["ACA"])
    tab = np.ones((2, 2), np.float32)
    sub = aln_amd.AlnSubmatrix(2, b"AC", tab.ctypes.data_as(C.POINTER(C.c_float)))
    g = _gap()
    hits = np.zeros((1, 1), dtype=aln_amd.HIT_DTYPE)
    n_hits = np.ones(1, np.int32)
    o = _Outputs()
    rc = aln_amd.lib().aln_hits_weights(None, C.byref(qp.c), C.byref(tp.c), C.byref(sub), C.byref(g), 0, 1, 1,
                                        hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits.ctypes.data_as(_ip), *o.tail())
    assert rc == aln_amd.E_ARG and o.untouched()


def test_a_null_context_is_refused_by_the_profile_entry():
    qp = aln_amd.QueryProfiles([np.ones((3, 2), np.float32)], "AC")
    tp = aln_amd.SeqPool(["ACA"])
    g = _gap()
    hits = np.zeros((1, 1), dtype=aln_amd.HIT_DTYPE)
    n_hits = np.ones(1, np.int32)
    o = _Outputs()
    rc = aln_amd.lib().aln_hits_weights_profiles(None, C.byref(qp.c), None, C.byref(tp.c), C.byref(g), 0, 1, 1,
                                                 hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits.ctypes.data_as(_ip), *o.tail())
    assert rc == aln_amd.E_ARG and o.untouched()
