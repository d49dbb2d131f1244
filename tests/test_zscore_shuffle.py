"""CPU-only: aln_amd.shuffle_query, the Python statement of the permutation aln_hits_zscores applies to a query
(include/aln_hip.h): pinned values, permutation property, degenerate lengths, and a coarse uniformity check."""
import collections
import itertools

import aln_amd

AA = "ACDEFGHIKLMNPQRSTVWY"

PINNED = [
    ((12345, 3, 7), "YVHTLMIKSNCEARDPGQFW"),
    ((12345, 3, 8), "IETGNQYHFSCPRMAVDWLK"),
    ((0, 0, 0), "NQEMWKLRICHFDATSPYVG"),
    ((0xFFFFFFFF, 70000, 4095), "EHKTIGSYMDACVQWLRNFP"),
]


def test_key_is_pinned():
    f = aln_amd._fmix32
    assert f((f((f(12345 ^ 0x9E3779B9) + 3) & 0xFFFFFFFF) + 7) & 0xFFFFFFFF) == 0x0993E6A4


def test_pinned_shuffles():
    for (seed, q, s), want in PINNED:
        assert aln_amd.shuffle_query(seed, q, s, AA) == want, (seed, q, s)


def test_is_a_permutation():
    for n in (2, 3, 20, 257):
        src = (AA * 13)[:n]
        for s in range(5):
            out = aln_amd.shuffle_query(77, 4, s, src)
            assert len(out) == n and sorted(out) == sorted(src)
    outs = {aln_amd.shuffle_query(77, 4, s, AA) for s in range(20)}
    assert len(outs) == 20                                   # shuffles differ from one another
    assert aln_amd.shuffle_query(77, 5, 0, AA) != aln_amd.shuffle_query(77, 4, 0, AA)
    assert aln_amd.shuffle_query(78, 4, 0, AA) != aln_amd.shuffle_query(77, 4, 0, AA)


def test_degenerate_lengths_come_back_unchanged():
    for s in range(4):
        assert aln_amd.shuffle_query(9, 1, s, "") == ""
        assert aln_amd.shuffle_query(9, 1, s, "W") == "W"


def test_orders_of_three_residues_are_about_equally_likely():
    cnt = collections.Counter(aln_amd.shuffle_query(1, 0, s, "ABC") for s in range(60000))
    assert sorted(cnt) == sorted("".join(p) for p in itertools.permutations("ABC"))
    assert all(9000 <= v <= 11000 for v in cnt.values()), cnt
