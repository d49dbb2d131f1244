"""No GPU: the zero rule of a lean build (csrc/dp_affine_tag.hip LEAN + aln_device.h::lean_score) restated in numpy.

A lean build leaves no score plane; the pointer word of a cell says whether the cell scores 0 (tests/lean_zero_cases.py states the
rule).  From the oracle's D / PQ / PT (orc.dp_build, local) this file builds those words, walks them with a restatement of the
local traceback that looks at nothing else, and compares the list with orc.optimal's, on the pairs the GPU file runs.  Every case
has to contain what it is for, and forgetting the mark of the interior zero cells has to change the list wherever the walk stops
inside the matrix."""
import functools

import numpy as np
import pytest

import lean_cases as lc
import lean_zero_cases as z
import orc


@functools.lru_cache(maxsize=None)
def oracle(q, t, table, gi, ge):
    S = orc.sim_submatrix(q, t, z.ALPHA, z.TABLES[table])
    rc_, D, PQ, PT = orc.dp_build(S, orc.Gap(orc.LOCAL, gi, ge))
    assert rc_ == 0
    rc_, sc, want = orc.optimal(D, PQ, PT, True)
    assert rc_ == 0
    return D, PQ, PT, sc, want


def all_pairs():
    out = [(c.name, c.q, c.t, c.table, c.gi, c.ge) for c in z.cases()]
    out += [("ragged%d" % k, q, t, "blosum62", 11, 1) for k, (q, t) in enumerate(z.ragged_pairs())]
    return out


NAMES = [p[0] for p in all_pairs()]


@pytest.mark.parametrize("name", NAMES)
def test_marked_words_alone_reproduce_optimal(name):
    _, q, t, table, gi, ge = next(p for p in all_pairs() if p[0] == name)
    D, PQ, PT, sc, want = oracle(q, t, table, gi, ge)
    best = lc.find_max_cell(D)
    assert D[best] == sc
    W = z.lean_words(D, PQ, PT)
    got, end, stop = z.walk(W, best)
    assert np.array_equal(got, want), (name, got[:4].tolist(), want[:4].tolist())
    # bits 0 .. 12 decode like the full build's word, in every written cell
    full = z.encode_words(PQ, PT)
    written = full != z.NULLW
    low = W[written] & 0x1FFF
    assert np.array_equal(np.where(low == z.ZERO_MATCH, z.P_MATCH, low), full[written])
    # the int64 reference the GPU file uses for these sizes agrees with the oracle
    S, H, L = z.reference(q, t, table, gi, ge)
    assert np.array_equal(H, D.astype(np.int64)) and np.array_equal(L, want)


@pytest.mark.parametrize("name", [c.name for c in z.cases()])
def test_each_case_holds_what_it_is_for(name):
    c = z.case(name)
    D, PQ, PT, sc, want = oracle(c.q, c.t, c.table, c.gi, c.ge)
    z.check_purpose(c, D, want)
    W = z.lean_words(D, PQ, PT)
    got, end, stop = z.walk(W, lc.find_max_cell(D))
    if c.kind == "negative":                                          # an all-zero plane: every interior word is a zero word
        Q, T = D.shape
        assert D.max() == 0
        inner = W[2:Q - 1, 2:T - 1]
        assert (inner == z.ZERO_MATCH).all()
        assert (W[1, 1:T - 1] & z.ZERO_BIT).all() and (W[1:Q - 1, 1] & z.ZERO_BIT).all()
        assert len(got) == (2 if Q == 3 else 3)
        return
    i, j = c.cell
    if c.kind == "diag":
        assert end == "diag0" and stop == c.cell
        if i >= 2 and j >= 2:                                         # a zero cell with a match word next to the path
            assert W[i, j] == z.ZERO_MATCH
        elif i == 1:                                                  # a zero cell of row 1 with a gap word
            assert W[i, j] == (z.ORIGIN_DEL | z.ZERO_BIT)
        else:                                                         # ... of column 1
            assert W[i, j] == (z.ORIGIN_INS | z.ZERO_BIT)
        return
    # a jump lands on the path's first cell, which scores > 0 by the rule
    assert z.lean_score(W[i, j]) == 1.0
    if i == 1 or j == 1:
        assert end == "border" and W[i, j] == (z.ORIGIN_DEL if i == 1 else z.ORIGIN_INS)
    else:
        assert end == "diag0" and stop == (i - 1, j - 1) and W[i - 1, j - 1] == z.ZERO_MATCH


def test_a_paid_gap_never_lands_on_a_zero_cell():
    """the only words that are both a gap pointer and a zero word belong to row 1 and column 1"""
    for name, q, t, table, gi, ge in all_pairs():
        D, PQ, PT, sc, want = oracle(q, t, table, gi, ge)
        full = z.encode_words(PQ, PT)
        Q, T = D.shape
        gap = (full != z.NULLW) & (((full >> 11) & 3) != 3)
        gap[1, :] = False
        gap[:, 1] = False
        gap[Q - 1, T - 1] = False
        i, j = np.nonzero(gap)
        k = z.TAGMAX - (full[gap].astype(np.int64) & z.TAGMAX)
        dele = ((full[gap] >> 11) & 3) == 2
        src = np.where(dele, D[i - 1, np.where(dele, k, 0)], D[np.where(dele, 0, k), j - 1])
        assert (src > 0).all(), name


def test_forgetting_the_mark_changes_every_stop_inside_the_matrix():
    inside = 0
    for c in z.cases():
        D, PQ, PT, sc, want = oracle(c.q, c.t, c.table, c.gi, c.ge)
        best = lc.find_max_cell(D)
        got, end, stop = z.walk(z.lean_words(D, PQ, PT), best)
        if not (end == "diag0" and stop[0] >= 2 and stop[1] >= 2):
            continue
        inside += 1
        bad, _, _ = z.walk(z.lean_words(D, PQ, PT, forget_mark=True), best)
        assert not np.array_equal(bad, want), c.name
        assert len(bad) > len(want), c.name                           # the walk runs on through cells that score 0
    assert inside >= 11, inside
