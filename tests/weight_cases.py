"""Shared by tests/test_weights_reference.py (CPU) and tests/test_gpu_weights.py (GPU): what aln_hits_weights /
aln_hits_weights_profiles must report — include/aln_hip.h restated in plain integer loops over the reference pileups of
pileup_cases (oracle pair lists, not the library) — and the slot sets of the GPU test.  Everything is an integer: there is no
tolerance anywhere.  aln_amd's library is not imported.

  slot_weights     weights and raw of one query's letters rows, Python integers throughout
  reference        weights, raw, counts and covered of a hit list
  sets             name -> (queries, templates, template indices [rows, K], n_hits, (table, gi, ge))
  check_sets       the assertions on the reference alone; the test modules call it before they use a set
"""
import numpy as np

import column_count_cases as cc
import pileup_cases as pu
import range_cases as rc
import search_cases as sc

ALPHA = cc.ALPHA
ONE = 1 << 24
W_MAXES = (1, 1000, 65535)


def slot_weights(letters, alphabet, w_max):
    """letters: [K, L] bytes of one query's rows.  -> (weights, raw), two lists of K Python integers."""
    letters = np.asarray(letters, np.uint8)
    K, L = letters.shape
    code = {ord(ch): a for a, ch in enumerate(alphabet)}
    raw = [0] * K
    for p in range(L):
        n = {}
        for k in range(K):
            a = code.get(int(letters[k, p]))
            if a is not None:
                n[a] = n.get(a, 0) + 1
        for k in range(K):
            a = code.get(int(letters[k, p]))
            if a is not None:
                raw[k] += ONE // (len(n) * n[a])
    M = max(raw, default=0)
    return [0 if x == 0 else max(1, w_max * x // M) for x in raw], raw


def position_stats(letters, alphabet):
    """-> (the largest k_p, the largest n_p[a]) over the positions of one query's rows"""
    letters = np.asarray(letters, np.uint8)
    n = np.stack([(letters == ord(ch)).sum(axis=0) for ch in alphabet])
    return int((n > 0).sum(axis=0).max(initial=0)), int(n.max(initial=0))


def reference(q_lens, ts, t_idx, n_hits, lists, local, w_max):
    """t_idx [rows, K], n_hits [rows]; lists: (score, list) per used slot, row-major.  -> dict: weights int32 [rows, K], raw
    int64 [rows, K] (unused slots 0), counts (per row an int64 (Q, N) array) and covered (int64 over all rows of the block) as
    column_count_cases.tally gives them under those weights, unweighted (the same tally with every weight 1), letters (the
    reference pileup, one row per used slot) and slots."""
    K = t_idx.shape[1]
    used = pu.used_slots(n_hits, K)
    slots = [(r, int(t_idx[r, k])) for r, k in used]
    stride = max(max(q_lens), 1)
    letters, _, _ = pu.pileup(q_lens, ts, slots, lists, local, stride)
    weights = np.zeros(t_idx.shape, np.int32)
    raw = np.zeros(t_idx.shape, np.int64)
    for r in range(len(n_hits)):
        mine = [s for s, (rr, k) in enumerate(used) if rr == r]
        if not mine:
            continue
        w, x = slot_weights(letters[mine][:, :q_lens[r]], ALPHA, w_max)
        weights[r, :len(mine)] = w
        raw[r, :len(mine)] = x
    per_slot = [int(weights[r, k]) for r, k in used]
    counts, covered = cc.tally(q_lens, ts, slots, lists, per_slot, local)
    plain, _ = cc.tally(q_lens, ts, slots, lists, [1] * len(slots), local)
    return dict(weights=weights, raw=raw, counts=counts, covered=covered, unweighted=plain, letters=letters, slots=used)


# ---- the sets -------------------------------------------------------------------------------------------------------------------
K65 = 65
N65 = (65, 65, 64, 1, 0, 33, 65, 7)                                   # a full row, the K loop's edge, one slot, none


def sets():
    """class: column_count_cases' class set — queries of 130 .. 1 residues, templates at every class edge, a duplicated slot,
    n_hits below K, row LONG_ROW fed by both routes.  homolog65: 8 x 10 homologs, K = 65, every template several times.
    homolog1: the same with K = 1.  muted: two queries whose every local score is 0."""
    system = ("blosum62",) + cc.SYSTEM[1:]
    qs, ts = cc.class_set()
    t_idx, n_hits = cc.class_hits(5)
    hq, ht = cc.homolog_set()
    t65 = np.array([[(r + k) % len(ht) for k in range(K65)] for r in range(len(hq))], np.int32)
    c = sc.CASES["all_negative"]
    mq, mt = sc.sequences(c)
    return {"class": (qs, ts, t_idx, n_hits, system),
            "homolog65": (hq, ht, t65, np.array(N65, np.int32), system),
            "homolog1": (hq, ht, np.arange(len(hq), dtype=np.int32).reshape(-1, 1), np.ones(len(hq), np.int32), system),
            "muted": (mq[:2], [mt[0], mt[8], mt[9]], np.tile(np.arange(3, dtype=np.int32), (2, 1)), np.full(2, 3, np.int32),
                      (c.table, c.gi, c.ge))}


def set_lists(name, mode):
    """-> the oracle's (score, list) per used slot of a set"""
    qs, ts, t_idx, n_hits, (table, gi, ge) = sets()[name]
    return [cc.pair_list(qs[r], ts[t_idx[r, k]], mode, gi, ge, table) for r, k in pu.used_slots(n_hits, t_idx.shape[1])]


_CHECKED = {}


def check_sets(modes=rc.ALIGN_TYPES):
    """The assertions on the reference alone (a GPU test of one align type asks for that type only).  Every condition is met by
    the homolog65 set under EVERY align type and, but for k_p >= 3, by the class set too; the muted rows are ALN_LOCAL's.  -> what was seen, per (set, align type)."""
    for mode in modes:
        if ("class", mode) in _CHECKED:
            continue
        local = mode == rc.LOCAL
        for name in ("class", "homolog65", "homolog1"):
            qs, ts, t_idx, n_hits, _ = sets()[name]
            q_lens = [len(q) for q in qs]
            lists = set_lists(name, mode)
            ref = reference(q_lens, ts, t_idx, n_hits, lists, local, 1000)
            one = reference(q_lens, ts, t_idx, n_hits, lists, local, 1)
            seen = dict(k_p=0, n_pa=0, uneven_rows=0, clamped=0, equal_duplicates=0, rows_reweighted=0)
            for r in range(len(qs)):
                mine = [s for s, (rr, k) in enumerate(ref["slots"]) if rr == r]
                if mine:
                    kp, npa = position_stats(ref["letters"][mine][:, :q_lens[r]], ALPHA)
                    seen["k_p"], seen["n_pa"] = max(seen["k_p"], kp), max(seen["n_pa"], npa)
                w, x = ref["weights"][r], ref["raw"][r]
                seen["uneven_rows"] += int(len(set(w[x > 0].tolist())) > 1)
                seen["clamped"] += int(((x > 0) & (x < x.max(initial=0)) & (one["weights"][r] == 1)).sum())
                assert (w[x == 0] == 0).all() and (x.max(initial=0) == 0 or w[np.argmax(x)] == 1000), (name, mode, r)
                assert (w[n_hits[r]:] == 0).all() and (x[n_hits[r]:] == 0).all()
                seen["rows_reweighted"] += int(not np.array_equal(ref["counts"][r], ref["unweighted"][r]))
                for a in range(n_hits[r]):                             # equal slots, equal weights
                    for b in range(a + 1, n_hits[r]):
                        if t_idx[r, a] == t_idx[r, b]:
                            assert w[a] == w[b] and x[a] == x[b], (name, mode, r, a, b)
                            seen["equal_duplicates"] += int(x[a] > 0)
            if name != "homolog1":
                # (the class set's templates all carry ONE homolog, so a position shows one letter there: k_p is homolog65's)
                assert seen["k_p"] >= (3 if name == "homolog65" else 1), (name, mode, seen)
                assert seen["n_pa"] >= 2 and seen["uneven_rows"] >= 1 and seen["clamped"] >= 1, (name, mode, seen)
                assert seen["equal_duplicates"] >= 1 and seen["rows_reweighted"] >= 1, (name, mode, seen)
            _CHECKED[(name, mode)] = seen
        if local:
            qs, ts, t_idx, n_hits, _ = sets()["muted"]
            lists = set_lists("muted", mode)
            assert all(score == 0 for score, _ in lists)
            ref = reference([len(q) for q in qs], ts, t_idx, n_hits, lists, True, 1000)
            assert not ref["weights"].any() and not ref["raw"].any() and not any(c.any() for c in ref["counts"])
            _CHECKED[("muted", mode)] = dict(muted_rows=len(qs))
    return _CHECKED
