"""-m gpu: the bookkeeping of the one host driver behind aln_hits_zscores and aln_hits_zscores_profiles (zscores_block,
csrc/search_zscore.hip) on a hit list that exercises every branch of a chunk at once.

Four queries of 10 .. 60 residues, the profiles derived from them; templates of 30, 300 and 2100 residues (length classes 1 and
2, and the full-build route); K = 3 with hand-made lists of 3, 0, 2 and 1 hits: unused slots, a row with no hit at all, rows
that mix slots of the fused kernels with slots of the long route, and a row with long-route slots only.  Six shuffles, local and
one non-local align type.

  - every cut of the rows into chunks ("zscore_chunk_rows" 0, 1, 2; for profiles also "zscore_rows_per_chunk" 0, 1) gives the
    bytes of the unhinted call
  - sum, sumsq and n equal the int64 reference (search_cases.zstats_reference), z the header's formula
  - the derived-profile entry equals the residue entry byte for byte
  - unused slots are all-zero"""
import numpy as np
import pytest

import aln_amd
import gpu_util
import range_cases as rc
import search_cases as sc

pytestmark = pytest.mark.gpu

U32 = np.uint32
SEED = 77
N = 6
K = 3
GI, GE = 11, 1
LISTS = [[0, 1, 2], [], [2, 1], [2]]
TABLE = sc.TABLES["blosum62"]
ZERO = np.zeros(1, dtype=aln_amd.HIT_STATS_DTYPE).tobytes()

_SET = {}


def the_set():
    if not _SET:
        _SET["qs"] = [rc.random_seq(sc.ALPHA, 5100 + k, ln) for k, ln in enumerate((10, 23, 41, 60))]
        _SET["ts"] = [rc.random_seq(sc.ALPHA, 5200 + k, ln) for k, ln in enumerate((30, 300, 2100))]
        _SET["qp"] = aln_amd.profiles_from_sequences(_SET["qs"], sc.ALPHA, TABLE)
    return _SET["qs"], _SET["ts"], _SET["qp"]


_REF = {}


def reference(mode):
    """(row, template) -> (sum, sumsq) over Python ints, and the pair's own score; computed once per align type, read-only"""
    if mode not in _REF:
        qs, ts, _ = the_set()
        ref = {}
        for r, x in enumerate(LISTS):
            for t in set(x):
                s, ss, _ = sc.zstats_reference(SEED, r, qs[r], ts[t], "blosum62", mode, GI, GE, N)
                ref[(r, t)] = (s, ss, sc.pair_reference(qs[r], ts[t], "blosum62", mode, GI, GE)[0])
        _REF[mode] = ref
    return _REF[mode]


@pytest.mark.parametrize("mode", [aln_amd.LOCAL, aln_amd.GLOBAL])
def test_mixed_routes_in_every_chunking(mode):
    qs, ts, qp = the_set()
    assert [(len(t) + 2 + 255) // 256 for t in ts] == [1, 2, 9]
    ref = reference(mode)
    hits = np.zeros((len(LISTS), K), dtype=aln_amd.HIT_DTYPE)
    hits["t"] = -1
    hits["q_end"] = hits["t_end"] = -1
    n_hits = np.array([len(x) for x in LISTS], dtype=np.int32)
    for r, x in enumerate(LISTS):
        for k, t in enumerate(x):
            hits[r, k] = (t, ref[(r, t)][2], -1, -1)
    ctx = gpu_util.ctx()
    residue = lambda: aln_amd.hits_zscores(ctx, qs, ts, hits, n_hits, sc.ALPHA, TABLE, GI, GE, N, seed=SEED,   # noqa: E731
                                           align_type=mode)
    profile = lambda: aln_amd.hits_zscores_profiles(ctx, qp, ts, hits, n_hits, GI, GE, N, seed=SEED, align_type=mode)   # noqa: E731
    base_r, base_p = residue(), profile()
    for rows in (0, 1, 2):
        with ctx.hints(zscore_chunk_rows=rows):
            assert residue().tobytes() == base_r.tobytes(), rows
            for per_chunk in (0, 1):
                with ctx.hints(zscore_rows_per_chunk=per_chunk):
                    assert profile().tobytes() == base_p.tobytes(), (rows, per_chunk)
    assert ctx.get_hint("zscore_chunk_rows") == 0 and ctx.get_hint("zscore_rows_per_chunk") == 0
    used = 0
    for r in range(len(LISTS)):
        for k in range(K):
            st = base_r[r, k]
            if k >= n_hits[r]:
                assert st.tobytes() == ZERO and base_p[r, k].tobytes() == ZERO, (r, k)
                continue
            s, ss, score = ref[(r, int(hits["t"][r, k]))]
            assert (int(st["sum"]), int(st["sumsq"]), int(st["n"])) == (s, ss, N), (r, k, st, s, ss)
            want = sc.z_restated(N, score, s, ss)
            assert st["z"].view(U32) == want.view(U32), (r, k, st["z"], want)
            used += 1
    assert used == 6
    assert base_p.tobytes() == base_r.tobytes()
    assert (np.int64(N) * base_r["sumsq"] != base_r["sum"] * base_r["sum"]).any()
