"""The ABI of the entries that align and tally the hits of a search under gap rows (aln_hits_align_profiles_gaps,
aln_hits_column_counts_profiles_gaps) as aln_amd binds it: exports, argtypes, the NULL-context refusal, and the header's
sentences.  No GPU."""
import ctypes as C
import os
import re

import numpy as np

import aln_amd

ENTRIES = {"aln_hits_align_profiles_gaps": 18, "aln_hits_column_counts_profiles_gaps": 15}     # name -> number of arguments
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aln_hip.h")
_ip = C.POINTER(C.c_int32)


def test_exports():
    L = aln_amd.lib()
    for name in ENTRIES:
        assert name in aln_amd.EXPORTS and hasattr(L, name), name
    for name in ("hits_align_profiles_gaps", "hits_column_counts_profiles_gaps"):
        assert callable(getattr(aln_amd, name)), name


def test_argtypes():
    L = aln_amd.lib()
    for name, n in ENTRIES.items():
        a = getattr(L, name).argtypes
        assert len(a) == n, name
        assert a[0] is C.c_void_p and a[1] is C.POINTER(aln_amd.AlnQProfiles) and a[2] is C.POINTER(aln_amd.AlnQGaps)
        assert a[3] is C.POINTER(aln_amd.AlnSeqs) and a[4] is C.POINTER(aln_amd.AlnSeqs)        # consensus, templates
        assert all(a[k] is C.c_int32 for k in (5, 6, 7, 8))                                     # align_type, q_begin, q_end, K
        assert a[9] is C.POINTER(aln_amd.AlnHit) and a[10] is _ip
    a = L.aln_hits_align_profiles_gaps.argtypes
    twin = L.aln_hits_align_profiles.argtypes
    assert list(a[9:]) == list(twin[8:])                                                        # hits .. lengths as the twin has them
    c = L.aln_hits_column_counts_profiles_gaps.argtypes
    twin = L.aln_hits_column_counts_profiles.argtypes
    assert list(c[9:]) == list(twin[8:])                                                        # hits, n_hits, weights, out, counts, covered


def test_null_context_is_refused_with_the_outputs_untouched():
    L = aln_amd.lib()
    q = aln_amd.QueryProfiles([np.ones((3, 2))], "XY")
    g = aln_amd.QueryGaps.constant(q, 11, 1)
    t = aln_amd.SeqPool(["XYX"])
    hits = np.zeros((1, 1), dtype=aln_amd.HIT_DTYPE)
    hits["q_end"], hits["t_end"], hits["score"] = 1, 1, 1
    n_hits = np.ones(1, np.int32)
    poison = bytes([0x5A])
    rec = np.frombuffer(bytearray(poison * 16), dtype=aln_amd.HIT_ALIGNMENT_DTYPE).copy()
    pairs = np.full((1, 1, 8, 2), 0x5A5A5A5A, np.int32)
    tl, ql = C.create_string_buffer(poison * 16, 16), C.create_string_buffer(poison * 16, 16)
    lengths = np.full(1, 0x5A5A5A5A, np.int32)
    counts = np.full((5, 2), 0x5A5A5A5A, np.int32)
    covered = np.full(5, 0x5A5A5A5A, np.int32)
    hp, recp = hits.ctypes.data_as(C.POINTER(aln_amd.AlnHit)), rec.ctypes.data_as(C.POINTER(aln_amd.AlnHitAlignment))
    assert L.aln_hits_align_profiles_gaps(None, C.byref(q.c), C.byref(g.c), None, C.byref(t.c), aln_amd.LOCAL, 0, 1, 1, hp,
                                          n_hits.ctypes.data_as(_ip), recp, pairs.ctypes.data_as(_ip), 8, tl, ql, 16,
                                          lengths.ctypes.data_as(_ip)) == aln_amd.E_ARG
    assert L.aln_hits_column_counts_profiles_gaps(None, C.byref(q.c), C.byref(g.c), None, C.byref(t.c), aln_amd.LOCAL, 0, 1, 1, hp,
                                                  n_hits.ctypes.data_as(_ip), None, recp, counts.ctypes.data_as(_ip),
                                                  covered.ctypes.data_as(_ip)) == aln_amd.E_ARG
    assert rec.tobytes() == poison * 16 and (pairs == 0x5A5A5A5A).all() and tl.raw == poison * 16 and ql.raw == poison * 16
    assert lengths[0] == 0x5A5A5A5A and (counts == 0x5A5A5A5A).all() and (covered == 0x5A5A5A5A).all()


def test_the_header_states_the_alignment():
    text = re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())
    text = re.sub(r"\s+", " ", text)
    a = text.index("} aln_qgaps;")
    b = text.index("int aln_score_profiles_gaps_vs_all(")
    body = text[a:b]                                           # the definition stands next to aln_qgaps
    for sentence in (
        "are aligned under the same rows by aln_hits_align_profiles_gaps and tallied by aln_hits_column_counts_profiles_gaps",
        "They cannot yet be z-scored, piled up, weighted, purged, turned into the next round's rows or aligned into several alignments",
        "THE ALIGNMENT under gap rows",
        "with every cost replaced by del(.,.) / ins(.,.)",
        "match from (i-1, j-1); deletions from (i-1, k), k ascending; insertions from (k, j-1), k ascending",
        "a later candidate wins only when it is STRICTLY greater",
        "match from (Q-2, T-2), then (Q-2, k) with k ascending at del(Q-2, T-2-k), then (k, T-2) with k ascending at ins(k+1, Q-2)",
        "a free end gap costs 0",
        "The LIST is Optimal's (optimal.h:56-74)",
        "the walk stops BEFORE a cell whose score is <= 0",
    ):
        assert sentence in body, sentence
    assert "cannot yet be aligned" not in text
    c = text.index("int aln_hits_column_counts_profiles(")
    d = text.index("int aln_hits_align_profiles_gaps(")
    e = text.index("int aln_hits_column_counts_profiles_gaps(")
    assert c < d < e
    entry = text[c:d]
    for sentence in (
        "THE ANCHOR: with all four arrays constant (del_init = ins_init = gi, del_extn = ins_extn = ge) every output byte",
        "equals aln_hits_align_profiles under { ALN_GAP_AFFINE_CONST, gi, ge, align_type }, for all five align types",
        "INTEGER SCORING ONLY",
        "there is no batch route",
        "A pair without an interior (Q = 2 or T = 2) is filed on the host",
        "Q = 2: -del(0, T-2), T = 2: -ins(1, Q-2)",
        "aln_hits_align_last_routes counts the host-filed slots in its second number",
        'Hint "align_fused_nonlocal" has nothing to switch to and is ignored',
        "Checks, in this order, nothing written when one fails: NULL profiles / gaps / templates / hits / n_hits / out",
        "directly after the profile descriptor, where aln_hits_align_profiles checks it; every n_hits[r] in 0..K",
    ):
        assert sentence in entry, sentence
    counts = text[d:e]
    for sentence in (
        "the record that entry writes when called with pairs == NULL and no line group",
        "A pair without an interior has no interior entry and contributes nothing",
        "every output byte equals aln_hits_column_counts_profiles'",
    ):
        assert sentence in counts, sentence
