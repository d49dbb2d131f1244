"""The exact log-odds rule of aln_hits_pssm (include/aln_hip.h) without a GPU: the header's constants, the Python-integer
restatement aln_amd.pssm_rows_from_counts on an example worked by hand, the library's host helper aln_pssm_entry against the
Python integers, the 2^63 bound, and the background case against the float64 pssm_from_counts it replaces.

The hand example: n = 4, bg = (2, 2, 2, 2) so B = 8, beta = 2, scale = 2, mix = 5 on the diagonal and 1 elsewhere (rows sum to 8).
  row 0  c = (3, 1, 0, 0), N = 4.  g = 3 mix[0] + 1 mix[1] = (16, 8, 4, 4).  num = c N B + beta g = (96 + 32, 32 + 16, 8, 8) =
         (128, 48, 8, 8); den = (N + beta) N bg = 6 * 4 * 2 = 48.
         128 / 48: e = 1 (96 <= 128 < 192), mant / 2^32 = 4/3, 16 log2(4/3) = 6.64 -> 6, lg16 = 22, s = floor((44 + 8) / 16) = 3.
         48 / 48: lg16 = 0, s = 0.   8 / 48 -> lg16(48, 8): e = 2 (32 <= 48 < 64), mant / 2^32 = 3/2, 16 log2(3/2) = 9.36 -> 9,
         lg16 = 41, s = -floor((82 + 8) / 16) = -5.                                        row = (3, 0, -5, -5)
  row 1  c = 0: the fallback row (0.5, -1.25, 7, -0.0), bit for bit (the sign of the zero too).
  row 2  c = (0, 0, 0, 1000), N = 1000.  g = 1000 mix[3] = (1000, 1000, 1000, 5000).  num = (2000, 2000, 2000, 8 010 000);
         den = 1002 * 1000 * 2 = 2 004 000.
         2000 / 2004000 -> lg16(2004000, 2000): the ratio is 1002, e = 9, mant / 2^32 = 1002/512 = 1.957, 16 log2 = 15.4987 -> 15,
         lg16 = 159, s = -floor((318 + 8) / 16) = -20.   8010000 / 2004000 = 3.997: e = 1, mant / 2^32 = 1.9985, 16 log2 = 15.98
         -> 15, lg16 = 31, s = floor((62 + 8) / 16) = 4.                                   row = (-20, -20, -20, 4)
"""
import math
import os
import random
import re

import numpy as np

import aln_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (1, 2, 4, 8)


def header_constants():
    header = open(os.path.join(ROOT, "include", "aln_hip.h")).read()
    at = header.index("with T[m] = floor(2^(32 + m/16)):")
    return [int(x, 16) for x in re.findall(r"0x1[0-9a-f]{8}\b", header[at:at + 400])]


def test_the_constants_are_nested_integer_square_roots():
    want = []
    for m in range(1, 16):
        v = 1 << (512 + m)
        for _ in range(4):
            v = math.isqrt(v)
        want.append(v)
    assert header_constants() == want and list(aln_amd.PSSM_T) == want
    assert all((1 << 32) < t < (1 << 33) for t in want) and want == sorted(want)


def test_the_hand_example():
    mix = [[5, 1, 1, 1], [1, 5, 1, 1], [1, 1, 5, 1], [1, 1, 1, 5]]
    fallback = np.array([[9, 9, 9, 9], [0.5, -1.25, 7, -0.0], [9, 9, 9, 9]], np.float32)
    counts = [[3, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1000]]
    got = aln_amd.pssm_rows_from_counts(counts, [2, 2, 2, 2], 2, 2, fallback, mix)
    want = np.array([[3, 0, -5, -5], [0.5, -1.25, 7, -0.0], [-20, -20, -20, 4]], np.float32)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    # the mix matters: with background pseudo-counts row 0 reads (3 N B + 2 N 2) / 48 = 112 / 48 and 16 / 48
    plain = aln_amd.pssm_rows_from_counts(counts, [2, 2, 2, 2], 2, 2, fallback)
    assert plain[1].tobytes() == want[1].tobytes() and plain[0].tolist() == [2, 0, -3, -3] and not np.array_equal(plain, got)
    assert aln_amd._lg16(128, 48) == 22 and aln_amd._lg16(48, 8) == 41 and aln_amd._lg16(2004000, 2000) == 159
    assert aln_amd._lg16(8010000, 2004000) == 31 and aln_amd._lg16(48, 48) == 0


def corners():
    top = (1 << 63) - 1
    out = [(1, 1), (7, 7), (top, top), (1 << 37, 1), (1, 1 << 37), (1 << 62, 1 << 25), (1 << 25, 1 << 62), (top, 1), (1, top),
           (top, top - 1), (top - 1, top), ((1 << 62) + 1, top), (top, (1 << 62) + 1), (top, 1 << 62), (3, 2), (2, 3)]
    for t in aln_amd.PSSM_T:                                           # mant == T[m] and T[m] - 1, unshifted and shifted
        for num in (t, t - 1):
            out += [(num, 1 << 32), (1 << 32, num), (num << 29, 1 << 32), (num << 7, 1 << 20)]
    return out


def test_the_host_helper_equals_the_python_integers():
    rng = random.Random(20261021)
    cases = corners()
    for _ in range(6000):
        num = rng.getrandbits(rng.randint(1, 63)) or 1
        den = rng.getrandbits(rng.randint(1, 63)) or 1
        cases.append((num, den))
    for _ in range(2000):                                              # close ratios: the mantissa decides
        den = rng.getrandbits(rng.randint(20, 62)) | 1
        cases.append((min(den + rng.getrandbits(rng.randint(1, 20)), (1 << 63) - 1), den))
    seen = set()
    for num, den in cases:
        for scale in SCALES:
            want = aln_amd.pssm_score(num, den, scale)
            got = aln_amd.pssm_entry(num, den, scale)
            assert got == want, (num, den, scale, got, want)
            assert aln_amd.pssm_entry(den, num, scale) == -got, (num, den, scale)
            seen.add(got)
    assert aln_amd.pssm_entry(1 << 37, 1, 8) == 8 * 37 and aln_amd.pssm_entry(1, 1 << 37, 8) == -8 * 37
    assert 0 in seen and min(seen) < -8 * 37 and max(seen) > 8 * 37    # (the helper takes any ratio below 2^63)
    # mant == T[m] counts m, T[m] - 1 does not
    for m, t in enumerate(aln_amd.PSSM_T, 1):
        assert aln_amd._lg16(t, 1 << 32) == m and aln_amd._lg16(t - 1, 1 << 32) == m - 1
        assert aln_amd._lg16(t << 3, 1 << 32) == 48 + m
    # what the helper refuses
    for num, den, scale in ((0, 5, 2), (5, 0, 2), (5, 5, 3), (5, 5, 0), (5, 5, 16), (1 << 63, 5, 2), (5, 1 << 63, 2), ((1 << 64) - 1, 1, 1)):
        assert aln_amd.pssm_entry(num, den, scale) == 0, (num, den, scale)


def test_num_and_den_stay_below_2_to_the_63():
    N, B, beta = 1024 * 65535 - 1, 1024, 1 << 26
    assert N < (1 << 26)
    # the largest num: every count on one letter, whose mix row gives it all but n - 1 of B; the largest den: bg[a] = B
    num = N * N * B + beta * N * B
    den = (N + beta) * N * 1024
    assert 1 <= num < (1 << 63) and 1 <= den < (1 << 63)
    rows = aln_amd.pssm_rows_from_counts([[N, 0]], [1023, 1], beta, 8, np.zeros((1, 2), np.float32))
    c = [N, 0]
    for a, bg in enumerate((1023, 1)):
        n_, d_ = c[a] * N * B + beta * N * bg, (N + beta) * N * bg
        assert 1 <= n_ < (1 << 63) and 1 <= d_ < (1 << 63)
        assert rows[0, a] == aln_amd.pssm_entry(n_, d_, 8) == aln_amd.pssm_score(n_, d_, 8)
    assert abs(aln_amd.pssm_score(1, 1 << 37, 8)) == 8 * 37


def test_the_background_case_agrees_with_pssm_from_counts():
    """pssm_from_counts rounds scale * log2(odds) in float64; the integer rule rounds the same real number.  They are compared
    wherever the float64 value is further than 1e-6 from a half-integer (the fixed-point slack of the rule is about 3e-9 at
    scale 8); at most 1 % of the entries may be left out."""
    rng = np.random.default_rng(42)
    compared = excluded = 0
    for n in (4, 20):
        for scale in SCALES:
            L = 240
            bg = rng.integers(1, 1024 // n + 1, size=n)
            B = int(bg.sum())
            assert B <= 1024
            beta = int(rng.choice((1, 7, 1000, 123457, 1 << 26)))
            top = rng.choice((3, 50, 1000, 65535, 2000000), size=(L, 1))
            counts = rng.integers(0, top + 1, size=(L, n)) * (rng.random((L, n)) < 0.6)
            counts[::17] = 0
            fallback = rng.integers(-4, 12, size=(L, n)).astype(np.float32)
            got = aln_amd.pssm_rows_from_counts(counts, bg, beta, scale, fallback)
            want = aln_amd.pssm_from_counts(counts, bg / B, fallback, pseudo=float(beta), scale=float(scale))
            c = counts.astype(np.float64)
            N = c.sum(axis=1, keepdims=True)
            bgf = (bg / B).reshape(1, -1)
            with np.errstate(divide="ignore", invalid="ignore"):
                x = scale * np.log2((c + beta * bgf) / ((N + beta) * bgf))
            near_tie = (N > 0) & (np.abs(x - np.floor(x) - 0.5) < 1e-6)
            assert (got[~near_tie] == want[~near_tie]).all(), (n, scale, int((got != want)[~near_tie].sum()))
            assert (got[(N == 0)[:, 0]] == fallback[(N == 0)[:, 0]]).all() and (N == 0).sum() >= 10
            compared += int((~near_tie).sum())
            excluded += int(near_tie.sum())
    print("entries compared:", compared, "left out near a tie:", excluded)
    assert compared >= 20000 and excluded <= 0.01 * (compared + excluded)
