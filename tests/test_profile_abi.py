"""The ABI of the position-specific query entries as aln_amd binds it: exports, the descriptor's fields, argtypes.  No GPU."""
import ctypes as C

import numpy as np

import aln_amd

ENTRIES = {"aln_score_profiles_vs_all": 7, "aln_search_topk_profiles": 10}      # name -> number of arguments (include/aln_hip.h)


def test_exports():
    L = aln_amd.lib()
    for name in ENTRIES:
        assert name in aln_amd.EXPORTS and hasattr(L, name), name


def test_descriptor_fields():
    f = aln_amd.AlnQProfiles._fields_
    assert [n for n, _ in f] == ["n_seqs", "offsets", "rows", "n", "alphabet"]
    assert f[0][1] is C.c_int32 and f[3][1] is C.c_int32 and f[4][1] is C.c_char_p
    assert f[1][1] is C.POINTER(C.c_int64) and f[2][1] is C.POINTER(C.c_float)
    assert C.sizeof(aln_amd.AlnQProfiles) == 40 and aln_amd.AlnQProfiles.rows.offset == 16 and aln_amd.AlnQProfiles.alphabet.offset == 32


def test_bindings_and_argtypes():
    L = aln_amd.lib()
    for name, n in ENTRIES.items():
        fn = getattr(L, name)
        assert callable(fn) and len(fn.argtypes) == n, name
        assert fn.argtypes[1] is C.POINTER(aln_amd.AlnQProfiles) and fn.argtypes[2] is C.POINTER(aln_amd.AlnSeqs)
    for name in ("score_profiles_vs_all", "search_topk_profiles", "profiles_from_sequences", "profile_planes", "QueryProfiles"):
        assert callable(getattr(aln_amd, name)), name


def test_query_profiles_adds_the_sentinel_rows():
    a = np.arange(6, dtype=np.float32).reshape(3, 2)
    q = aln_amd.QueryProfiles([a, np.zeros((0, 2))], "XY")
    assert len(q) == 2 and q.offsets.tolist() == [0, 5, 7] and q.rows.shape == (7, 2) and q.rows.dtype == np.float32
    assert np.array_equal(q.rows[1:4], a) and not q.rows[0].any() and not q.rows[4:].any()
    assert q.c.n_seqs == 2 and q.c.n == 2 and q.c.alphabet == b"XY"
    d = aln_amd.profiles_from_sequences(["YX", ""], "XY", [[1, 2], [3, 4]])
    assert d.rows.tolist() == [[0, 0], [3, 4], [1, 2], [0, 0], [0, 0], [0, 0]]
    S = aln_amd.profile_planes(d.profiles[0], "XYY", "XY")
    assert S.dtype == np.float32 and S.tolist() == [[0] * 5, [0, 3, 4, 4, 0], [0, 1, 2, 2, 0], [0] * 5]
