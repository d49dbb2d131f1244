"""Shared by tests/test_pileup_reference.py (CPU) and tests/test_gpu_pileup.py (GPU): what aln_hits_pileup /
aln_hits_pileup_profiles must report — include/aln_hip.h restated in numpy over the pair lists of the oracle's build and
traceback (column_count_cases.pair_list / profile_list).  Everything is an integer or a byte: there is no tolerance anywhere.
aln_amd's library is not imported (counts_from_pileup and aln_amd.synth are pure numpy).

  pileup        letters, tpos and spans of a list of used slots
  check_sets    the assertions on the reference alone; the test modules call it before they use a set
"""
import numpy as np

import aln_amd
import column_count_cases as cc
import range_cases as rc
from column_count_cases import class_hits, class_set, homolog_set, interior_entries, pair_list, profile_list  # noqa: F401

DOT, DASH = ord("."), ord("-")


def pileup(q_lens, ts, slots, lists, local, stride):
    """q_lens: residues of every query ROW of the block (without sentinels); slots: (row, template index) per used slot; lists:
    (score, list) per used slot; stride >= max(q_lens).  -> (letters uint8 [n, stride], tpos uint16 [n, stride], spans int32
    [n, 4] = q_lo, q_hi, t_lo, t_hi), one row per used slot."""
    n = len(slots)
    letters = np.zeros((n, stride), np.uint8)
    tpos = np.zeros((n, stride), np.uint16)
    spans = np.zeros((n, 4), np.int32)
    for s, ((r, t), (score, pl)) in enumerate(zip(slots, lists)):
        L = q_lens[r]
        letters[s, :L] = DOT
        if local and not score > 0:
            continue
        inner = interior_entries(pl, L + 2, len(ts[t]) + 2)
        if len(inner) == 0:
            continue
        i, j = inner[:, 0], inner[:, 1]
        lo, hi = int(i.min()), int(i.max())
        letters[s, lo - 1:hi] = DASH
        letters[s, i - 1] = [ord(ts[t][jj - 1]) for jj in j]
        tpos[s, i - 1] = j
        spans[s] = (lo, hi, int(j[np.argmin(i)]), int(j[np.argmax(i)]))
    return letters, tpos, spans


def used_slots(n_hits, K):
    return [(r, k) for r in range(len(n_hits)) for k in range(K) if k < n_hits[r]]


def sets():
    """-> name -> (queries, templates, slots as (row, template index))"""
    qs, ts = class_set()
    t_idx, n_hits = class_hits(5)
    hq, ht = homolog_set()
    return {"class": (qs, ts, [(r, int(t_idx[r, k])) for r, k in used_slots(n_hits, 5)]),
            "homolog": (hq, ht, cc.all_slots(len(hq), len(ht)))}


_CHECKED = {}


def check_sets(modes=rc.ALIGN_TYPES):
    """The assertions on the reference alone, for both sets and all five align types (a GPU test of one align type asks for
    that type only, so that no single test pays for every list).  -> dict of what was seen, per (set, align type)."""
    for name, (qs, ts, slots) in sets().items():
        q_lens = [len(q) for q in qs]
        stride = max(q_lens)
        for mode in modes:
            if (name, mode) in _CHECKED:
                continue
            local = mode == rc.LOCAL
            lists = [pair_list(qs[r], ts[t], mode) for r, t in slots]
            seen = dict(double_jumps=0, del_jumps=0, ins_jumps=0, dashes=0, dots=0)
            for (r, t), (score, pl) in zip(slots, lists):
                inner = interior_entries(pl, q_lens[r] + 2, len(ts[t]) + 2)
                assert len(np.unique(inner[:, 0])) == len(inner), (name, mode, r, t)        # no interior i twice
                d = np.diff(inner, axis=0)
                seen["double_jumps"] += int(((d[:, 0] > 1) & (d[:, 1] > 1)).sum())
                dj, ij = cc.jumps(pl, q_lens[r] + 2, len(ts[t]) + 2)
                seen["del_jumps"] += dj
                seen["ins_jumps"] += ij
            letters, tpos, spans = pileup(q_lens, ts, slots, lists, local, stride)
            seen["dashes"] = int((letters == DASH).sum())
            seen["dots"] = int((letters == DOT).sum())
            assert seen["double_jumps"] == 0, (name, mode, seen)      # a3m's "inserts after a column" rests on this
            assert min(seen["del_jumps"], seen["ins_jumps"], seen["dashes"], seen["dots"]) >= 1, (name, mode, seen)
            assert ((tpos > 0) == ((letters != DOT) & (letters != DASH) & (letters != 0))).all()
            # the tally of aln_hits_column_counts, read off the pileup
            want, want_cov = cc.tally(q_lens, ts, slots, lists, [1] * len(slots), local)
            off = np.concatenate(([0], np.cumsum([n + 2 for n in q_lens])))
            for r, L in enumerate(q_lens):
                mine = [s for s, (rr, t) in enumerate(slots) if rr == r]
                counts, covered = aln_amd.counts_from_pileup(letters[mine], cc.ALPHA)
                assert np.array_equal(counts[:L], want[r][1:-1]) and not counts[L:].any(), (name, mode, r)
                assert np.array_equal(covered[:L], want_cov[off[r] + 1:off[r + 1] - 1]) and not covered[L:].any(), (name, mode, r)
            _CHECKED[(name, mode)] = seen
    return _CHECKED
