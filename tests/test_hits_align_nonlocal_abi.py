"""The non-local fused route of aln_hits_align at the ABI boundary (no GPU): the route counter is exported and bound, the hint
that switches the route off is declared and documented."""
import ctypes
import os

import aln_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_last_routes_is_exported_and_bound():
    if not os.path.exists(aln_amd.LIB_PATH):
        aln_amd.build_library()
    L = ctypes.CDLL(aln_amd.LIB_PATH)
    assert hasattr(L, "aln_hits_align_last_routes")
    assert "aln_hits_align_last_routes" in aln_amd.EXPORTS
    assert callable(aln_amd.hits_align_routes)
    assert len(aln_amd.lib().aln_hits_align_last_routes.argtypes) == 2
    out = (ctypes.c_int64 * 2)(7, 7)
    assert aln_amd.lib().aln_hits_align_last_routes(None, out) == aln_amd.E_ARG and list(out) == [7, 7]


def test_align_fused_nonlocal_is_a_declared_hint():
    header = open(os.path.join(ROOT, "include", "aln_hip.h")).read()
    assert '"align_fused_nonlocal"' in header and "aln_hits_align_last_routes" in header
    hints = open(os.path.join(ROOT, "alignment-algos_amd", "csrc", "aln_hints.hip")).read()
    assert '"align_fused_nonlocal", "ALN_ALIGN_FUSED_NONLOCAL"' in hints
