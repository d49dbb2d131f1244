"""Shared by tests/test_purge_reference.py (CPU) and tests/test_gpu_purge.py (GPU): what aln_hits_purge /
aln_hits_purge_profiles must report — include/aln_hip.h restated in plain integer loops over the reference pileups of
pileup_cases / weight_cases (oracle pair lists, not the library) — and the slot sets of the GPU test.  Everything is an
integer: there is no tolerance anywhere.  aln_amd's library is not imported.

  slot_purge       keeper, same, overlap, letters of one query's letters rows, Python integers throughout
  reference        purge records, and weights, raw, counts and covered of the survivors, of a hit list
  sets             name -> (queries, templates, template indices [rows, K], n_hits, (table, gi, ge))
  check_sets       the assertions on the reference alone; the test modules call it before they use a set
"""
import numpy as np

import column_count_cases as cc
import pileup_cases as pu
import range_cases as rc
import weight_cases as wc
from aln_amd.synth import homolog_pair

ALPHA = cc.ALPHA
PARAMS = ((90, 50), (100, 0), (100, 100), (101, 0))                  # (max_identity, min_overlap)
W_MAX = 1000

# the hand example of include/aln_hip.h's definition: alphabet AC, four rows
HAND = np.array([list(b"AACAC"), list(b"AACAA"), list(b"..CAA"), list(b"A-..C")], np.uint8)
HAND_RECORDS = {(75, 50): [(0, 0, 0, 5), (0, 4, 5, 5), (2, 0, 0, 3), (0, 2, 2, 2)],
                (100, 50): [(0, 0, 0, 5), (1, 0, 0, 5), (1, 3, 3, 3), (0, 2, 2, 2)]}


def slot_purge(letters, alphabet, max_identity, min_overlap):
    """letters: [K, L] bytes of one query's rows.  -> K records (keeper, same, overlap, letters) of Python integers."""
    letters = np.asarray(letters, np.uint8)
    K, L = letters.shape
    code = [[alphabet.find(chr(int(c))) if int(c) not in (0, ord("."), ord("-")) else -1 for c in row] for row in letters]
    count = [sum(1 for a in row if a >= 0) for row in code]
    kept, out = [], []
    for k in range(K):
        if count[k] == 0:
            out.append((-1, 0, 0, 0))
            continue
        rec = None
        for j in kept:                                                 # ascending: the first hit is the smallest keeper
            overlap = same = 0
            for a, b in zip(code[j], code[k]):
                if a >= 0 and b >= 0:
                    overlap += 1
                    same += 1 if a == b else 0
            if overlap >= 1 and 100 * overlap >= min_overlap * count[k] and 100 * same >= max_identity * overlap:
                rec = (j, same, overlap, count[k])
                break
        if rec is None:
            kept.append(k)
            rec = (k, 0, 0, count[k])
        out.append(rec)
    return out


def reference(q_lens, ts, t_idx, n_hits, lists, local, max_identity, min_overlap, w_max=W_MAX):
    """t_idx [rows, K], n_hits [rows]; lists: (score, list) per used slot, row-major.  -> dict: purge int32 [rows, K, 4]
    (keeper, same, overlap, letters; unused slots -1, 0, 0, 0), and weights, raw, counts, covered as weight_cases.reference
    gives them for the hit list in which a slot that is not kept does not contribute (its list's score set to what a muted
    slot's is — under a non-local align type its list is emptied instead), plus that reference's letters and slots."""
    K = t_idx.shape[1]
    used = pu.used_slots(n_hits, K)
    slots = [(r, int(t_idx[r, k])) for r, k in used]
    stride = max(max(q_lens), 1)
    letters, _, _ = pu.pileup(q_lens, ts, slots, lists, local, stride)
    purge = np.zeros(t_idx.shape + (4,), np.int32)
    purge[..., 0] = -1
    for r in range(len(n_hits)):
        mine = [s for s, (rr, k) in enumerate(used) if rr == r]
        if mine:
            purge[r, :len(mine)] = slot_purge(letters[mine][:, :q_lens[r]], ALPHA, max_identity, min_overlap)
    empty = np.zeros((0, 2), np.int32)
    survivors = [(score, pl) if purge[r, k, 0] == k else (0.0, empty) for (r, k), (score, pl) in zip(used, lists)]
    ref = wc.reference(q_lens, ts, t_idx, n_hits, survivors, local, w_max)
    ref["purge"] = purge
    ref["all_letters"] = letters
    return ref


# ---- the sets -------------------------------------------------------------------------------------------------------------------
K130 = 130
N130 = (130, 129, 64, 33, 1, 0)                                      # K, K - 1, a full bit word, half a j tile and one, one, none
LENGTHS = (1, 3, 4, 5, 63, 64, 65, 130)                              # Q - 2: strides that are no multiple of 4, unaligned rows
GRADES = (0.0, 0.03, 0.06, 0.12, 0.2, 0.35)                          # substitution rates of one seed: nested substitutions
K_WIDE = 1024


def graded(seed, n):
    """-> the templates of homolog_pair(seed, n) at GRADES (the same draws decide every grade: a higher rate substitutes a
    superset of positions, the indels are the same), then the first and the second half of the grade-0 template and a full copy
    of it: fragments that do not overlap each other, and a slot that is near both."""
    full = [homolog_pair(seed, n, sub_rate=g)[1] for g in GRADES]
    return full + [full[0][:n // 2], full[0][n // 2:], full[0]]


# where graded()'s pieces stand: slots in this order meet check_sets' conditions (indices into graded())
FRAGMENT_ORDER = (6, 7, 8, 1, 2, 3, 4, 5, 0)                         # two fragments, the copy near both, then the grades


_SETS = {}


def sets():
    """Built once and left unchanged.  class, homolog65, homolog1, muted: weight_cases' sets (K = 5 with both routes in one
    row and a duplicated slot, K = 65 with n_hits of 65, 64, 33, 7, 1, 0, K = 1, two rows whose every local score is 0).
    graded130: six of the homolog set's queries against graded() of each — K = 130, n_hits of N130, every row cycling through
    its own nine pieces, so that duplicates, grades and fragments all occur and a row's bits cross two j tiles and three words.
    lengths: queries of LENGTHS residues in one block, cut from one 130-residue query, K = 5 over graded() of it.
    wide: one 40-residue query, K = 1024 over 12 distinct templates."""
    if _SETS:
        return _SETS
    out = dict(wc.sets())
    system = ("blosum62",) + cc.SYSTEM[1:]
    qs, ts = [], []
    for k, n in enumerate((100, 110, 120, 64, 77, 90)):
        qs.append(homolog_pair(900 + k, n)[0])
        ts += graded(900 + k, n)
    t130 = np.array([[9 * r + FRAGMENT_ORDER[k % 9] for k in range(K130)] for r in range(len(qs))], np.int32)
    out["graded130"] = (qs, ts, t130, np.array(N130, np.int32), system)
    q = homolog_pair(4243, 130)[0]
    lt = graded(4243, 130)
    tl = np.array([[FRAGMENT_ORDER[(r + k) % 9] for k in range(5)] for r in range(len(LENGTHS))], np.int32)
    out["lengths"] = ([q[:n] for n in LENGTHS], lt, tl, np.array((5, 4, 5, 3, 5, 5, 5, 5), np.int32), system)
    wq = homolog_pair(4244, 40)[0]
    wt = graded(4244, 40) + [homolog_pair(4245 + k, 40)[1] for k in range(3)]
    assert len(wt) == 12 and len(set(wt)) >= 10
    tw = np.array([[(k * 7) % 12 for k in range(K_WIDE)]], np.int32)
    out["wide"] = ([wq], wt, tw, np.array([K_WIDE], np.int32), system)
    _SETS.update(out)
    return _SETS


_LISTS = {}


def set_lists(name, mode):
    """-> the oracle's (score, list) per used slot of a set; one oracle call per distinct (query, template) pair"""
    qs, ts, t_idx, n_hits, (table, gi, ge) = sets()[name]
    out = []
    for r, k in pu.used_slots(n_hits, t_idx.shape[1]):
        key = (qs[r], ts[t_idx[r, k]], mode, table, gi, ge)
        if key not in _LISTS:
            _LISTS[key] = cc.pair_list(qs[r], ts[t_idx[r, k]], mode, gi, ge, table)
        out.append(_LISTS[key])
    return out


_REFS = {}


def set_reference(name, mode, max_identity, min_overlap):
    """reference() of a set, computed once and left unchanged"""
    key = (name, mode, max_identity, min_overlap)
    if key not in _REFS:
        qs, ts, t_idx, n_hits, _ = sets()[name]
        _REFS[key] = reference([len(q) for q in qs], ts, t_idx, n_hits, set_lists(name, mode), mode == rc.LOCAL, max_identity,
                               min_overlap)
    return _REFS[key]


_CHECKED = {}


def check_sets(modes=rc.ALIGN_TYPES):
    """The assertions on the reference alone (a GPU test of one align type asks for that type only): every condition the
    kernels can get wrong occurs in the sets, under every align type asked for.  -> what was seen, per align type."""
    for mode in modes:
        if mode in _CHECKED:
            continue
        local = mode == rc.LOCAL
        seen = dict(purged_at_90_kept_at_100=0, duplicate_purged_at_100=0, chain_kept=0, two_keepers=0, overlap_decides=0,
                    kept=0, used_without_record=0, rows_nothing_purged=0, rows_all_but_first=0, rows_reweighted=0,
                    wide_kept=0, wide_purged=0)
        for name, (qs, ts, t_idx, n_hits, _) in sets().items():
            if name == "muted" and not local:
                continue
            q_lens = [len(q) for q in qs]
            ref = {p: set_reference(name, mode, *p) for p in PARAMS}
            plain = wc.reference(q_lens, ts, t_idx, n_hits, set_lists(name, mode), local, W_MAX)
            # under 101 nothing is purged and the weights are aln_hits_weights'
            r101 = ref[(101, 0)]
            for what in ("weights", "raw", "covered"):
                assert np.array_equal(r101[what], plain[what]), (name, mode, what)
            assert all(np.array_equal(a, b) for a, b in zip(r101["counts"], plain["counts"])), (name, mode)
            k101 = r101["purge"][..., 0]
            assert ((k101 == -1) | (k101 == np.arange(t_idx.shape[1])[None, :])).all(), (name, mode)
            assert ((k101 >= 0) == (plain["raw"] > 0)).all(), (name, mode)       # a letter weighs, and only a letter
            for r in range(len(qs)):
                n = int(n_hits[r])
                mine = [s for s, (rr, k) in enumerate(ref[(90, 50)]["slots"]) if rr == r]
                rows = ref[(90, 50)]["all_letters"][mine][:, :q_lens[r]]
                p90, p100, p100all = ref[(90, 50)]["purge"][r], ref[(100, 0)]["purge"][r], ref[(100, 100)]["purge"][r]
                for p in (p90, p100, p100all):
                    assert (p[n:] == (-1, 0, 0, 0)).all(), (name, mode, r)
                    assert (p[:, 2] >= p[:, 1]).all() and (p[:, 3] >= p[:, 2]).all()
                for k in range(n):
                    keeper = int(p90[k, 0])
                    seen["kept"] += int(keeper == k and p90[k, 3] > 0)
                    seen["used_without_record"] += int(tuple(p90[k]) == (-1, 0, 0, 0))
                    seen["purged_at_90_kept_at_100"] += int(0 <= keeper < k and p100[k, 0] == k)
                    j = int(p100[k, 0])
                    seen["duplicate_purged_at_100"] += int(0 <= j < k and np.array_equal(rows[j], rows[k]))
                    seen["overlap_decides"] += int(p100all[k, 0] == k and 0 <= j < k)
                    for par, p in (((90, 50), p90), ((100, 0), p100)):
                        if p[k, 0] != k or p[k, 3] == 0:
                            continue
                        near_purged = [jj for jj in range(k) if 0 <= p[jj, 0] < jj and is_near(rows[jj], rows[k], *par)]
                        seen["chain_kept"] += int(bool(near_purged))
                    if 0 <= j < k:
                        near_kept = [jj for jj in range(k) if p100[jj, 0] == jj and is_near(rows[jj], rows[k], 100, 0)]
                        assert near_kept[0] == j, (name, mode, r, k)
                        seen["two_keepers"] += int(len(near_kept) >= 2)
                if n >= 2 and name != "muted":
                    kept_all = [(p[:n, 0] == np.arange(n)) for p in (p90, p100)]
                    seen["rows_nothing_purged"] += int(kept_all[1].all() or kept_all[0].all())
                    seen["rows_all_but_first"] += int(kept_all[0][0] and not kept_all[0][1:].any() and (p90[1:n, 0] == 0).all())
                seen["rows_reweighted"] += int(not np.array_equal(ref[(90, 50)]["weights"][r], plain["weights"][r]))
                if name == "wide":
                    seen["wide_kept"] += int((p90[:, 0] == np.arange(K_WIDE)).sum())
                    seen["wide_purged"] += int(((p90[:, 0] >= 0) & (p90[:, 0] != np.arange(K_WIDE))).sum())
            # purged slots weigh nothing, kept slots with a letter weigh
            for par, x in ref.items():
                keeper = x["purge"][..., 0]
                is_kept = keeper == np.arange(t_idx.shape[1])[None, :]
                assert ((x["weights"] > 0) == is_kept).all() and ((x["raw"] > 0) == is_kept).all(), (name, mode, par)
        need = [k for k in seen if not (k == "used_without_record" and not local)]
        assert all(seen[k] >= 1 for k in need), (mode, seen)
        assert seen["wide_kept"] >= 2 and seen["wide_purged"] >= 2, (mode, seen)
        _CHECKED[mode] = seen
    return _CHECKED


def is_near(row_j, row_k, max_identity, min_overlap):
    """NEAR of two letters rows (j before k), Python integers"""
    code = lambda c: ALPHA.find(chr(int(c))) if int(c) not in (0, ord("."), ord("-")) else -1
    a, b = [code(c) for c in row_j], [code(c) for c in row_k]
    overlap = sum(1 for x, y in zip(a, b) if x >= 0 and y >= 0)
    same = sum(1 for x, y in zip(a, b) if x >= 0 and x == y)
    count = sum(1 for y in b if y >= 0)
    return overlap >= 1 and 100 * overlap >= min_overlap * count and 100 * same >= max_identity * overlap
