"""aln_hits_align at the ABI boundary (no GPU): the symbol is exported, the record is 16 bytes, the binding exists."""
import ctypes
import os

import numpy as np

import aln_amd


def test_hits_align_is_exported_and_bound():
    if not os.path.exists(aln_amd.LIB_PATH):
        aln_amd.build_library()
    L = ctypes.CDLL(aln_amd.LIB_PATH)
    assert hasattr(L, "aln_hits_align")
    assert "aln_hits_align" in aln_amd.EXPORTS
    assert ctypes.sizeof(aln_amd.AlnHitAlignment) == 16
    assert [f[0] for f in aln_amd.AlnHitAlignment._fields_] == ["n_pairs", "status", "score", "identity"]
    assert aln_amd.HIT_ALIGNMENT_DTYPE.itemsize == 16
    assert np.zeros(1, dtype=aln_amd.HIT_ALIGNMENT_DTYPE).tobytes() == bytes(16)
    assert callable(aln_amd.hits_align)
    assert callable(aln_amd.align_hits)
    assert len(aln_amd.lib().aln_hits_align.argtypes) == 17


def test_align_chunk_hits_is_a_declared_hint():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert '"align_chunk_hits"' in open(os.path.join(root, "include", "aln_hip.h")).read()
    assert '"align_chunk_hits", "ALN_ALIGN_CHUNK_HITS"' in open(os.path.join(root, "alignment-algos_amd", "csrc", "aln_hints.hip")).read()
