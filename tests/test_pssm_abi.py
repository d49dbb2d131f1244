"""aln_hits_pssm / aln_hits_pssm_profiles / aln_pssm_entry at the ABI boundary (no GPU): the three symbols are exported and
bound, the parameter struct is 24 bytes, the Python wrappers exist, the header carries the definition in its place, and a NULL
context is refused before anything is touched."""
import ctypes as C
import inspect
import os

import numpy as np

import aln_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)
_fp = C.POINTER(C.c_float)


def test_the_three_exports_are_bound():
    if not os.path.exists(aln_amd.LIB_PATH):
        aln_amd.build_library()
    L = C.CDLL(aln_amd.LIB_PATH)
    for name in ("aln_hits_pssm", "aln_hits_pssm_profiles", "aln_pssm_entry"):
        assert hasattr(L, name)
        assert name in aln_amd.EXPORTS
    assert C.sizeof(aln_amd.AlnPssmParams) == 24
    assert [(f[0], f[1]) for f in aln_amd.AlnPssmParams._fields_] == [("scale", C.c_int32), ("beta", C.c_int32), ("bg", _ip), ("mix", _ip)]
    assert aln_amd.AlnPssmParams.bg.offset == 8 and aln_amd.AlnPssmParams.mix.offset == 16
    tail = [C.POINTER(aln_amd.AlnHit), _ip, C.c_int32, C.c_int32, C.c_int32, C.POINTER(aln_amd.AlnPssmParams),
            C.POINTER(aln_amd.AlnHitAlignment), _fp, C.POINTER(aln_amd.AlnHitPurge), _ip, _lp, _ip, _ip]
    a = aln_amd.lib().aln_hits_pssm.argtypes
    assert len(a) == 21
    assert a[1:5] == [C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnSubmatrix), C.POINTER(aln_amd.AlnGap)]
    assert a[5:8] == [C.c_int32] * 3 and a[8:] == tail
    p = aln_amd.lib().aln_hits_pssm_profiles.argtypes
    assert len(p) == 21
    assert p[1:5] == [C.POINTER(aln_amd.AlnQProfiles), C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnSeqs), C.POINTER(aln_amd.AlnGap)]
    assert p[5:8] == [C.c_int32] * 3 and p[8:] == tail
    e = aln_amd.lib().aln_pssm_entry
    assert e.argtypes == [C.c_uint64, C.c_uint64, C.c_int32] and e.restype is C.c_int32
    assert aln_amd.pssm_entry(3, 1, 2) == 3 and aln_amd.pssm_entry(1, 3, 2) == -3       # rint(2 log2 3) = rint(3.17)


def test_the_wrappers_are_callable():
    tail = ["max_identity", "min_overlap", "w_max", "q_begin", "align_type", "want_purge", "want_weights", "want_raw", "want_counts",
            "want_covered"]
    names = list(inspect.signature(aln_amd.hits_pssm).parameters)
    assert names[:10] == ["ctx", "queries", "templates", "hits", "n_hits", "alphabet", "table", "gi", "ge", "params"] and names[10:] == tail
    names = list(inspect.signature(aln_amd.hits_pssm_profiles).parameters)
    assert names[:9] == ["ctx", "profiles", "templates", "hits", "n_hits", "gi", "ge", "params", "consensus"] and names[9:] == tail
    assert list(inspect.signature(aln_amd.pssm_rows_from_counts).parameters) == ["counts", "bg", "beta", "scale", "fallback_rows", "mix"]
    assert list(inspect.signature(aln_amd.pssm_entry).parameters) == ["num", "den", "scale"]
    names = list(inspect.signature(aln_amd.iterate_search).parameters)
    assert names[:10] == ["ctx", "queries", "templates", "alphabet", "table", "gi", "ge", "K", "rounds", "params"]
    for f in (aln_amd.hits_pssm, aln_amd.hits_pssm_profiles, aln_amd.pssm_rows_from_counts, aln_amd.pssm_entry, aln_amd.iterate_search):
        assert callable(f) and f.__doc__
    par = aln_amd.AlnPssmParams.make([3, 1], 5, 4, [[3, 1], [2, 2]])
    assert (par.scale, par.beta, par.bg[0], par.bg[1], [par.mix[i] for i in range(4)]) == (4, 5, 3, 1, [3, 1, 2, 2])
    assert not aln_amd.AlnPssmParams.make([3, 1], 5).mix


def test_the_header_carries_the_definition_in_its_place():
    header = open(os.path.join(ROOT, "include", "aln_hip.h")).read()
    assert "typedef struct { int32_t scale, beta; const int32_t* bg; const int32_t* mix; } aln_pssm_params;" in header
    assert "int aln_hits_pssm(aln_ctx* ctx, const aln_seqs* queries, const aln_seqs* templates, const aln_submatrix* sub," in header
    assert "int aln_hits_pssm_profiles(aln_ctx* ctx, const aln_qprofiles* profiles, const aln_seqs* consensus" in header
    assert "int32_t aln_pssm_entry(uint64_t num, uint64_t den, int32_t scale);" in header
    assert header.index("int aln_hits_purge_profiles(") < header.index("The log-odds are defined in integers alone") < \
        header.index("} aln_pssm_params;") < header.index("int aln_hits_pssm(") < header.index("int aln_hits_pssm_profiles(") < \
        header.index("int32_t aln_pssm_entry(") < header.index("int aln_hits_align_multi(")
    for sentence in ("integer background weights, each in 1..1024, B = sum_a bg[a] <= 1024",
                     "Every entry is >= 1 and every row sums to B",
                     "NULL means mix[b][a] = bg[a]",
                     "1..2^26, the pseudo-count mass in the units of the weights",
                     "one of 1, 2, 4, 8: scores are in 1/scale bits",
                     "N is below 2^26",
                     "N == 0: row r of `rows` is the fallback row, copied bit for bit",
                     "g[a]   = sum_b c[b] * mix[b][a]",
                     "num[a] = c[a] * N * B + beta * g[a]",
                     "den[a] = (N + beta) * N * bg[a]",
                     "Both are in [1, 2^63)",
                     "e is the largest e >= 0 with y * 2^e <= x",
                     "mant = floor(x * 2^32 / (y * 2^e))",
                     "lg16 = 16 * e + #{ m in 1..15 : T[m] <= mant }",
                     "s = floor((lg16(num, den) * scale + 8) / 16) when num >= den",
                     "s = -floor((lg16(den, num) * scale + 8) / 16)",
                     "|s| <= 8 * 37",
                     "the thresholds are irrational",
                     "neither 128-bit arithmetic nor a 64-bit division",
                     "32 shift-and-subtract steps",
                     "the sentinel rows (first and last\n * row of every query) zeros",
                     "out and rows are required.  purge, weights, raw, counts and covered may be NULL, each independently",
                     "is byte for byte what aln_hits_purge(_profiles) returns for the same arguments",
                     "NULL par or rows; scale; beta; NULL bg, a bg[a] outside\n * 1..1024, B above 1024; a mix entry below 1, a mix row that does not sum to B",
                     "every output is byte-identical to aln_hits_pssm's on those\n * residues",
                     "needs no GPU, like aln_gapped_strings"):
        assert sentence in header, sentence


def _gap():
    g = aln_amd.AlnGap()
    g.model, g.align_type, g.gap_init, g.gap_extn = aln_amd.GAP_AFFINE_CONST, aln_amd.LOCAL, 11.0, 1.0
    return g


class _Outputs:
    def __init__(self):
        self.par = aln_amd.AlnPssmParams.make([1, 1], 10, 2)
        self.rec = np.full(16, 0x5A, np.uint8)
        self.rows = np.full(5 * 2, 0x5A5A5A5A, np.uint32)
        self.purge = np.full(16, 0x5A, np.uint8)
        self.weights = np.full(1, 0x5A5A5A5A, np.int32)
        self.raw = np.full(1, 0x5A5A5A5A5A5A5A5A, np.int64)
        self.counts = np.full(5 * 2, 0x5A5A5A5A, np.int32)
        self.covered = np.full(5, 0x5A5A5A5A, np.int32)

    def tail(self):
        return (90, 50, 1000, C.byref(self.par), self.rec.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment)),
                self.rows.ctypes.data_as(_fp), self.purge.ctypes.data_as(C.POINTER(aln_amd.AlnHitPurge)),
                self.weights.ctypes.data_as(_ip), self.raw.ctypes.data_as(_lp), self.counts.ctypes.data_as(_ip),
                self.covered.ctypes.data_as(_ip))

    def untouched(self):
        return bool((self.rec == 0x5A).all() and (self.rows == 0x5A5A5A5A).all() and (self.purge == 0x5A).all() and
                    (self.weights == 0x5A5A5A5A).all() and (self.raw == 0x5A5A5A5A5A5A5A5A).all() and
                    (self.counts == 0x5A5A5A5A).all() and (self.covered == 0x5A5A5A5A).all())


def test_a_null_context_is_refused():
    qp = aln_amd.SeqPool(["ACA"])
    tp = aln_amd.SeqPool(["ACA"])
    tab = np.ones((2, 2), np.float32)
    sub = aln_amd.AlnSubmatrix(2, b"AC", tab.ctypes.data_as(_fp))
    g = _gap()
    hits = np.zeros((1, 1), dtype=aln_amd.HIT_DTYPE)
    n_hits = np.ones(1, np.int32)
    o = _Outputs()
    rc = aln_amd.lib().aln_hits_pssm(None, C.byref(qp.c), C.byref(tp.c), C.byref(sub), C.byref(g), 0, 1, 1,
                                     hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits.ctypes.data_as(_ip), *o.tail())
    assert rc == aln_amd.E_ARG and o.untouched()


def test_a_null_context_is_refused_by_the_profile_entry():
    qp = aln_amd.QueryProfiles([np.ones((3, 2), np.float32)], "AC")
    tp = aln_amd.SeqPool(["ACA"])
    g = _gap()
    hits = np.zeros((1, 1), dtype=aln_amd.HIT_DTYPE)
    n_hits = np.ones(1, np.int32)
    o = _Outputs()
    rc = aln_amd.lib().aln_hits_pssm_profiles(None, C.byref(qp.c), None, C.byref(tp.c), C.byref(g), 0, 1, 1,
                                              hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits.ctypes.data_as(_ip), *o.tail())
    assert rc == aln_amd.E_ARG and o.untouched()
