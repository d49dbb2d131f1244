"""The ABI of the gap-row entries (aln_score_profiles_gaps_vs_all, aln_search_topk_profiles_gaps) as aln_amd binds it: exports,
the descriptor, argtypes, the NULL-context refusal, and the header's sentences.  No GPU."""
import ctypes as C
import os
import re

import numpy as np

import aln_amd

ENTRIES = {"aln_score_profiles_gaps_vs_all": 8, "aln_search_topk_profiles_gaps": 11}     # name -> number of arguments
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aln_hip.h")


def test_exports():
    L = aln_amd.lib()
    for name in ENTRIES:
        assert name in aln_amd.EXPORTS and hasattr(L, name), name
    for name in ("score_profiles_gaps_vs_all", "search_topk_profiles_gaps", "QueryGaps", "AlnQGaps"):
        assert callable(getattr(aln_amd, name)), name


def test_descriptor_is_four_float_pointers():
    f = aln_amd.AlnQGaps._fields_
    assert [n for n, _ in f] == ["del_init", "del_extn", "ins_init", "ins_extn"]
    assert all(t is C.POINTER(C.c_float) for _, t in f)
    assert C.sizeof(aln_amd.AlnQGaps) == 32


def test_argtypes():
    L = aln_amd.lib()
    for name, n in ENTRIES.items():
        a = getattr(L, name).argtypes
        assert len(a) == n, name
        assert a[1] is C.POINTER(aln_amd.AlnQProfiles) and a[2] is C.POINTER(aln_amd.AlnQGaps) and a[3] is C.POINTER(aln_amd.AlnSeqs)
        assert a[4] is C.c_int32 and a[5] is C.c_int32 and a[6] is C.c_int32
    assert L.aln_score_profiles_gaps_vs_all.argtypes[7] is C.POINTER(C.c_float)
    s = L.aln_search_topk_profiles_gaps.argtypes
    assert s[7] is C.c_int32 and s[8] is C.c_float and s[9] is C.POINTER(aln_amd.AlnHit) and s[10] is C.POINTER(C.c_int32)


def test_query_gaps_builds_the_pool_arrays():
    q = aln_amd.QueryProfiles([np.ones((3, 2)), np.zeros((0, 2))], "XY")
    g = aln_amd.QueryGaps([[1, 2, 3, 4], [9]], [[5, 6, 7, 8], [9]], [[0, 1, 1, 1], [0]], [[0, 2, 2, 2], [0]])
    assert np.array_equal(g.offsets, q.offsets)
    assert g.del_init.dtype == np.float32 and g.del_init.tolist() == [1, 2, 3, 4, 0, 9, 0] and g.del_extn.tolist() == [5, 6, 7, 8, 0, 9, 0]
    assert g.ins_init.tolist() == [0, 1, 1, 1, 0, 0, 0] and g.ins_extn.tolist() == [0, 2, 2, 2, 0, 0, 0]
    assert C.addressof(g.c.del_init.contents) == g.del_init.ctypes.data and C.addressof(g.c.ins_extn.contents) == g.ins_extn.ctypes.data
    c = aln_amd.QueryGaps.constant(q, 11, 1)
    assert c.del_init.tolist() == [11, 11, 11, 11, 0, 11, 0] and c.ins_extn.tolist() == [1, 1, 1, 1, 0, 1, 0]


def test_null_context_is_refused_with_the_outputs_untouched():
    L = aln_amd.lib()
    q = aln_amd.QueryProfiles([np.ones((3, 2))], "XY")
    g = aln_amd.QueryGaps.constant(q, 11, 1)
    t = aln_amd.SeqPool(["XYX"])
    scores = np.full(1, np.float32(-7.5))
    hits = np.frombuffer(bytearray([0x5A]) * 32, dtype=aln_amd.HIT_DTYPE).copy()
    n_hits = np.full(1, 0x5A5A5A5A, np.int32)
    assert L.aln_score_profiles_gaps_vs_all(None, C.byref(q.c), C.byref(g.c), C.byref(t.c), aln_amd.LOCAL, 0, 1,
                                            scores.ctypes.data_as(C.POINTER(C.c_float))) == aln_amd.E_ARG
    assert L.aln_search_topk_profiles_gaps(None, C.byref(q.c), C.byref(g.c), C.byref(t.c), aln_amd.LOCAL, 0, 1, 2, -np.inf,
                                           hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), n_hits.ctypes.data_as(C.POINTER(C.c_int32))) == aln_amd.E_ARG
    assert scores[0] == np.float32(-7.5) and hits.tobytes() == bytes([0x5A]) * 32 and n_hits[0] == 0x5A5A5A5A


def test_the_header_states_the_definition():
    text = re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())
    text = re.sub(r"\s+", " ", text)
    a = text.index("} aln_qgaps;")
    b = text.index("int aln_score_profiles_gaps_vs_all(")
    assert text.index("aln_search_topk_profiles(aln_ctx*") < a < b < text.index("int aln_search_topk_profiles_gaps(") < text.index("} aln_hit_stats;")
    body = text[a:b]
    for sentence in (
        "del_init[off+i] + del_extn[off+i] * (L-1)",
        "The gap is priced by the row it LEAVES",
        "ins_init[off+a] + sum_{p=a+1..b} ins_extn[off+p]",
        "Every skipped position pays its own price",
        "Entries read: del_* at rows 0..Q-2 and ins_* at rows 1..Q-2",
        "a NaN there changes nothing",
        "max_{1<=k<j-1} D[i-1][k] - del(i-1, j-1-k)",
        "max_{1<=k<i-1} D[k][j-1] - ins(k+1, i-1)",
        "the head deletion into (1, j) costs del(0, j-1)",
        "the head insertion into (i, 1) costs ins(1, i-1)",
        "from (Q-2, k) the cost is del(Q-2, T-2-k)",
        "from (k, T-2) it is ins(k+1, Q-2)",
        "Q = 2 costs del(0, T-2) and T = 2 costs ins(1, Q-2)",
        "byte-identical to aln_score_profiles_vs_all / aln_search_topk_profiles",
        "there is no full-build fallback",
        "(maxs + G) * (maxQ + min(maxT, 2048)) + G + maxs < 2^23",
        "profiles->n above 26 with ALN_E_ARG",
        "a template of more than 2048 columns with ALN_E_TOO_LONG",
        "a negative gap value (ALN_E_ARG); fractional values and the bound (ALN_E_NOT_INTEGRAL)",
    ):
        assert sentence in body, sentence
    assert "aln_qgaps and aln_score_profiles_gaps_vs_all" in text[text.index("A pool of query profiles."):text.index("} aln_qprofiles;")]
