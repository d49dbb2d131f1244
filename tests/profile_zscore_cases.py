"""Shared by tests/test_profile_zscore_reference.py (CPU) and tests/test_gpu_zscores_profiles.py (GPU): what
aln_hits_zscores_profiles must report, restated on profile_cases.pair_reference (the int64 planes).  Shuffle s of a profile is
the profile with its interior rows in the order aln_amd.shuffle_order gives (pure Python; imported late, so this module imports
neither the library nor torch).  A profile is an (L x n) int64 array WITHOUT the two sentinel rows, as in profile_cases."""
import numpy as np

import profile_cases as pc


def shuffled(seed, q_index, s, profile):
    """-> the (L x n) profile whose row i is the original row a[i], a = shuffle_order(seed, q_index, s, L)"""
    from aln_amd import shuffle_order
    prof = np.asarray(profile).reshape(-1, pc.N)
    return prof[np.asarray(shuffle_order(seed, q_index, s, len(prof)), dtype=np.intp)]


def zstats_reference(seed, q_index, profile, t, mode, gi, ge, n):
    """-> (sum, sumsq, the n scores) as Python ints: shuffle s = 0 .. n-1 of the profile (pool index q_index) against template t"""
    col = [int(pc.pair_reference(shuffled(seed, q_index, s, profile), t, mode, gi, ge)[0]) for s in range(n)]
    return sum(col), sum(v * v for v in col), col
