"""Shared by tests/test_column_counts_reference.py (CPU) and tests/test_gpu_column_counts.py (GPU): what
aln_hits_column_counts / aln_hits_column_counts_profiles must report — a tally, in pure numpy, over the pair lists of the
oracle's build and traceback (orc.dp_build + orc.optimal, as search_cases.nonlocal_reference and
profile_align_cases.oracle_pair make them) — and the sequence sets of the GPU test.  Everything is an integer: there is no
tolerance anywhere.  aln_amd's library is not imported (aln_amd.synth is pure numpy).

  pair_list        (score, list) of a residue pair, all five align types
  profile_list     (score, list) of a (profile, template) pair
  tally            include/aln_hip.h, aln_hits_column_counts, restated: counts per row and covered
  class_set        queries of 130 .. 1 interior residues against templates of every fused length class and one beyond
  homolog_set      homolog_pair queries and templates: lists with deletion and insertion jumps
  hit_array, gap   the GPU tests' hit slots as aln_hit, and SYSTEM's gap descriptor
  check_sets       the assertions on the reference alone; the test modules call it before they use a set
"""
import numpy as np

import aln_amd
import orc
import profile_align_cases as pac
import profile_cases as pc
import range_cases as rc
import search_cases as sc
from aln_amd.synth import homolog_pair

ALPHA = sc.ALPHA
N = len(ALPHA)
_IDX = {ch: k for k, ch in enumerate(ALPHA)}
SYSTEM = ("blosum62", 11, 1)
TABLE = sc.TABLES[SYSTEM[0]]

_LOCAL = {}


def pair_list(q, t, mode, gi=SYSTEM[1], ge=SYSTEM[2], table=SYSTEM[0]):
    """-> (score, list int32 [n, 2] in list order) of orc.dp_build + orc.optimal; computed once per input, left unchanged"""
    if mode != rc.LOCAL:
        return sc.nonlocal_reference(q, t, table, mode, gi, ge)
    key = (q, t, table, gi, ge)
    if key not in _LOCAL:
        S = orc.sim_submatrix(q, t, ALPHA, sc.TABLES[table])
        err, D, PQ, PT = orc.dp_build(S, orc.Gap(mode, gi, ge))
        err2, score, pl = orc.optimal(D, PQ, PT, True)
        assert err == 0 and err2 == 0
        _LOCAL[key] = (score, pl)
    return _LOCAL[key]


def profile_list(profile, t, mode, gi=SYSTEM[1], ge=SYSTEM[2]):
    D, score, pl = pac.oracle_pair(profile, t, ALPHA, mode, gi, ge)
    return score, pl


def interior_entries(pl, Q, T):
    """the entries (i, j) of a list with 1 <= i <= Q-2 and 1 <= j <= T-2"""
    pl = np.asarray(pl, np.int64).reshape(-1, 2)
    keep = (pl[:, 0] >= 1) & (pl[:, 0] <= Q - 2) & (pl[:, 1] >= 1) & (pl[:, 1] <= T - 2)
    return pl[keep]


def tally(q_lens, ts, slots, lists, weights, local):
    """q_lens: residues of every query ROW of the block (without sentinels); slots: (row, template index) per used slot; lists:
    (score, list) per used slot; weights: one int per used slot.  -> (counts: per row an int64 (Q, N) array, covered: one
    int64 array over all rows of the block, sentinel rows included)."""
    counts = [np.zeros((n + 2, N), np.int64) for n in q_lens]
    off = np.concatenate(([0], np.cumsum([n + 2 for n in q_lens])))
    covered = np.zeros(off[-1], np.int64)
    for (r, t), (score, pl), w in zip(slots, lists, weights):
        if w <= 0 or (local and not score > 0):
            continue
        inner = interior_entries(pl, q_lens[r] + 2, len(ts[t]) + 2)
        if len(inner) == 0:
            continue
        letters = np.array([_IDX[ts[t][j - 1]] for j in inner[:, 1]], np.int64)
        np.add.at(counts[r], (inner[:, 0], letters), w)
        covered[off[r] + inner[:, 0].min():off[r] + inner[:, 0].max() + 1] += w
    return counts, covered


def jumps(pl, Q, T):
    """-> (deletion jumps, insertion jumps) between consecutive interior entries of a list"""
    inner = interior_entries(pl, Q, T)
    d = np.diff(inner, axis=0)
    return int(((d[:, 0] == 1) & (d[:, 1] > 1)).sum()), int(((d[:, 1] == 1) & (d[:, 0] > 1)).sum())


# ---- the sets -------------------------------------------------------------------------------------------------------------------
Q_INTERIOR = (130, 65, 64, 63, 2, 1)                                 # longest first: it meets the shortest templates
# columns (sentinels counted): the smallest template with an interior, the last of class 1, the first and last of every other
# class a kernel is kept for, the first of class 8 (local: batches), and the longest template of class 8
T_COLUMNS = (3, 255, 256, 257, 512, 513, 768, 769, 1024, 1025, 1280, 1281, 1536, 1537, 1792, 1793, 2046)
LONG_T = 2100                                                        # residues: beyond the fused kernels


def class_set():
    """-> (queries, templates).  One 130-residue homolog pair (q, h): query k is the first Q_INTERIOR[k] residues of q;
    template c holds h (cut to its length where shorter) near its END, behind random residues — so local end cells lie in
    the last column group of the class — and the last template has LONG_T residues.  Every query therefore aligns to every
    template with jumps."""
    q, h = homolog_pair(4242, 130)
    qs = [q[:n] for n in Q_INTERIOR]
    ts = []
    for k, cols in enumerate(T_COLUMNS + (LONG_T + 2,)):
        n = cols - 2
        core = h[:n]
        tail = rc.random_seq(ALPHA, 700 + k, min(3, n - len(core)))
        ts.append(rc.random_seq(ALPHA, 600 + k, n - len(core) - len(tail)) + core + tail)
        assert len(ts[-1]) == n
    return qs, ts


def class_of(t):
    return (len(t) + 2 + 255) // 256


LONG_ROW = 3                                                         # the 63-residue query also takes the LONG_T template


def class_hits(K=5):
    """-> (template indices [rows, K], n_hits) of the slots over class_set: row r names templates r, r + 6, r + 12 — all 18
    templates are used, every class by two or three query lengths, and the oracle's cubic cost stays small — then slot 0 once
    more (a duplicate in the same launch: its counts double, its adds collide), and row LONG_ROW the LONG_T template as a fifth
    slot, so that both routes add into one query's rows.  Slots beyond n_hits name template 0 and must not be read."""
    assert K == 5
    t = np.zeros((len(Q_INTERIOR), K), np.int32)
    n = np.full(len(Q_INTERIOR), 4, np.int32)
    for r in range(len(Q_INTERIOR)):
        t[r, :4] = [r, r + 6, r + 12, r]
    t[LONG_ROW, 4] = len(T_COLUMNS)
    n[LONG_ROW] = 5
    return t, n


def homolog_set():
    """-> (queries, templates): 8 queries and 10 templates for the two-round loop and the jump assertions — homolog pairs of
    40 .. 120 residues, each query's partner among the templates, two unrelated templates"""
    qs, ts = [], []
    for k, n in enumerate((40, 55, 64, 77, 90, 100, 110, 120)):
        q, t = homolog_pair(900 + k, n)
        qs.append(q)
        ts.append(t)
    ts.append(rc.random_seq(ALPHA, 950, 70))
    ts.append(homolog_pair(903, 77, sub_rate=0.3)[1])               # a second, noisier relative of query 3
    return qs, ts


def all_slots(n_q, n_t):
    return [(r, t) for r in range(n_q) for t in range(n_t)]


def used_slots(n_hits, K):
    return [(r, k) for r in range(len(n_hits)) for k in range(K) if k < n_hits[r]]


def hit_array(t_idx, n_hits, lists, local):
    """the slots t_idx[rows, K] as aln_hit: local slots carry the oracle's score and the cell its list starts from (the entry
    before (Q-1, T-1)); non-local slots carry values that must not be read; unused slots hold a template that must not be"""
    hits = np.zeros(t_idx.shape, dtype=aln_amd.HIT_DTYPE)
    hits["t"] = t_idx
    hits["q_end"], hits["t_end"], hits["score"] = -7, 1 << 20, -1e30
    for (r, k), (score, pl) in zip(used_slots(n_hits, t_idx.shape[1]), lists):
        if local:
            hits["score"][r, k] = score
            hits["q_end"][r, k], hits["t_end"][r, k] = pl[-2]
    return hits


def gap(model=aln_amd.GAP_AFFINE_CONST, align_type=aln_amd.LOCAL):
    """SYSTEM's gap costs as the C ABI's descriptor"""
    g = aln_amd.AlnGap()
    g.model, g.align_type, g.gap_init, g.gap_extn = model, align_type, float(SYSTEM[1]), float(SYSTEM[2])
    return g


_CHECKED = {}


def check_sets():
    """The assertions on the reference alone.  -> dict of what was seen (for the test's message)."""
    if _CHECKED:
        return _CHECKED
    qs, ts = homolog_set()
    derived = pc.derived(qs, TABLE)
    seen = dict(del_jumps=0, ins_jumps=0, gap_rows=0)
    for mode in rc.ALIGN_TYPES:
        local = mode == rc.LOCAL
        slots = all_slots(len(qs), len(ts))
        lists = [pair_list(qs[r], ts[t], mode) for r, t in slots]
        weights = [1 + (r + 3 * t) % 4 for r, t in slots]
        counts, covered = tally([len(q) for q in qs], ts, slots, lists, weights, local)
        # sum(counts) == sum_s w_s * interior pairs
        want = sum(w * len(interior_entries(pl, len(qs[r]) + 2, len(ts[t]) + 2))
                   for (r, t), (score, pl), w in zip(slots, lists, weights) if not local or score > 0)
        assert sum(int(c.sum()) for c in counts) == want
        rowsum = np.concatenate([c.sum(axis=1) for c in counts])
        assert (covered >= rowsum).all()
        seen["gap_rows"] += int((covered > rowsum).sum())
        for (r, t), (score, pl) in zip(slots, lists):
            d, i = jumps(pl, len(qs[r]) + 2, len(ts[t]) + 2)
            seen["del_jumps"] += d
            seen["ins_jumps"] += i
        # rows derived from residues give the residue tally
        plists = [profile_list(derived[r], ts[t], mode) for r, t in slots]
        for (s1, l1), (s2, l2) in zip(lists, plists):
            assert s1 == s2 and np.array_equal(l1, l2)
        pcounts, pcovered = tally([len(p) for p in derived], ts, slots, plists, weights, local)
        assert all(np.array_equal(a, b) for a, b in zip(counts, pcounts)) and np.array_equal(covered, pcovered)
    assert seen["del_jumps"] >= 1 and seen["ins_jumps"] >= 1 and seen["gap_rows"] >= 1, seen
    _CHECKED.update(seen)
    return _CHECKED
