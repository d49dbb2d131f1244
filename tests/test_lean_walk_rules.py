"""No GPU: the rules of a lean build (csrc/dp_affine_tag.hip LEAN + traceback_kernel's score source 2) restated in numpy.

A lean build leaves no score plane: bit 15 of a cell's 16-bit pointer word says "score > 0".  From the oracle's D / PQ / PT
(orc.dp_build, local) this file builds those words with a restatement of aln_device.h::encode_ptr (dialect 1) plus the flag, walks
them with a restatement of the local traceback that looks at nothing else, and compares the list with orc.optimal's.  Every way a
local walk can end has to occur among the pairs."""
import numpy as np
import pytest

import orc
from aln_amd.synth import homolog_pair

NULLW = 0xFFFF
TAGMAX = 2047


def encode_word(i, j, pq, pt):
    """encode_ptr, mode 1: prio << 11 | tag"""
    if pq < 0 or pt < 0:
        return NULLW
    if pq == i - 1 and pt == j - 1:
        return 3 << 11
    if pq == i - 1:
        return (2 << 11) | (TAGMAX - pt)
    return (1 << 11) | (TAGMAX - pq)


def decode_word(w, i, j):
    """decode_ptr, mode 1: bits 13..15 are not looked at"""
    prio, k = (w >> 11) & 3, TAGMAX - (w & TAGMAX)
    if prio == 3:
        return i - 1, j - 1
    if prio == 2:
        return i - 1, k
    return k, j - 1


def lean_words(D, PQ, PT):
    Q, T = D.shape
    W = np.full((Q, T), NULLW, dtype=np.uint16)
    for i in range(Q):
        for j in range(T):
            w = encode_word(i, j, int(PQ[i, j]), int(PT[i, j]))
            if w != NULLW:
                assert w < (1 << 13)
                if D[i, j] > 0 and not (i == Q - 1 and j == T - 1):      # the final cell is dp_corner_kernel's: never flagged
                    w |= 0x8000
            else:
                assert D[i, j] == 0                                     # an untouched cell keeps 0xFFFF exactly
            W[i, j] = w
    return W


def flag_score(w):
    return 1.0 if (w != NULLW and (w & 0x8000)) else 0.0


def find_max(D):
    """optimal.h:108-124: seed (Q-2,T-2), the first strictly greater cell in row-major order replaces it (the kernel has this
    from its registers, not from a plane)"""
    Q, T = D.shape
    mq, mt = Q - 2, T - 2
    sub = D[:Q - 1, :T - 1]
    k = int(np.argmax(sub))
    if sub.flat[k] > D[mq, mt]:
        mq, mt = divmod(k, T - 1)
    return mq, mt


def walk(W, best):
    """the local loop of optimal.h:79-105 on the words alone -> list in list order, how it ended"""
    Q, T = W.shape
    lst = [(Q - 1, T - 1), best]
    q, t = best
    end = "loop"
    while q > 0:
        w = int(W[q, t])
        if w == NULLW:
            q, t = -1, -1
            end = "null"
            break
        pq, pt = decode_word(w, q, t)
        diag = (pq, pt) == (q - 1, t - 1)
        q, t = pq, pt
        if flag_score(int(W[q, t])) <= 0:
            end = "border" if (diag and (q == 0 or t == 0)) else ("diag0" if diag else "gap0")
            break
        lst.append((q, t))
    if q != 0 and t != 0:
        lst.append((0, 0))
    return np.array(lst[::-1], dtype=np.int32).reshape(-1, 2), end


def _pairs():
    out = [("ACDEF", "ACDEF"),            # starts at (1,1): the diagonal step leaves the matrix
           ("WCDEF", "AAWCDEF"),          # starts in row 1, column 3: a jump to the origin
           ("AAWCDEF", "WCDEF"),          # starts in column 1, row 3
           ("PPWCW", "GGGWCW"),           # starts inside: the diagonal neighbour scores 0
           ("", "ACD"), ("ACD", ""), ("A", "A"), ("W", "P")]
    rng = np.random.RandomState(20260)
    for k in range(52):                   # tie-heavy: two- and three-letter sequences
        alpha = ("AG", "ST", "ILV", "DEN")[k % 4]
        n, m = rng.randint(1, 41), rng.randint(1, 41)
        out.append(("".join(rng.choice(list(alpha), n)), "".join(rng.choice(list(alpha), m))))
    for k in range(40):                   # gap-heavy: homologs with an insertion and a deletion
        out.append(homolog_pair(300 + k, 22 + (k % 19), indel=2 + k % 4))
    return out


@pytest.mark.parametrize("gi,ge", [(11, 1), (2, 0)])
def test_flagged_words_alone_reproduce_optimal(blosum62, gi, ge):
    alpha, table = blosum62
    census = {"border": 0, "diag0": 0, "gap0": 0}
    pairs = _pairs()
    assert len(pairs) == 100
    for q, t in pairs:
        S = orc.sim_submatrix(q, t, alpha, table)
        rc, D, PQ, PT = orc.dp_build(S, orc.Gap(orc.LOCAL, gi, ge))
        assert rc == 0
        rc, sc, want = orc.optimal(D, PQ, PT, True)
        assert rc == 0
        best = find_max(D)
        assert D[best] == sc
        got, end = walk(lean_words(D, PQ, PT), best)
        assert np.array_equal(got, want), (q, t, gi, ge, got.tolist(), want.tolist())
        if end in census:
            census[end] += 1
    print("endings", gi, ge, census)
    assert all(v > 0 for v in census.values()), census
