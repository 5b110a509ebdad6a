"""CPU tests of the exact model of the pooled sum (tests/pool_ref.py: exact_sum_bits, round_to_f32_bits, exact_pool), so that the
reference is trusted before tests/test_gpu_pool_exact.py asks the GPU: against float64 wherever float64 is exact, against
np.float32 on hand-written ties, at the inf threshold, at the 2^-96 truncation, and the representability guard of the driver."""
import math
from fractions import Fraction

import numpy as np
import pytest

import pool_ref as R

FLT_MAX = 0x7F7FFFFF


def bits(v):
    return int(np.float32(v).view(np.uint32))


def value(b):
    return float(np.uint32(b).view(np.float32))


def test_equals_float64_where_float64_is_exact():
    # exponent fields within a span of 25 and at most 8 partials: every partial and every partial sum fits 24 + 25 + 3 = 52 bits,
    # so the float64 sum is exact and np.float32 of it is the one rounding; bit 0 of every partial is at 2^-96 or above
    rng = np.random.default_rng(1)
    for _ in range(20000):
        n = int(rng.integers(1, 9))
        lo = int(rng.integers(127 - 73, 254 - 25 - 3))
        ex = rng.integers(lo, lo + 26, n).astype(np.uint32)
        p = (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)) | (ex << np.uint32(23)) | rng.integers(0, 1 << 23, n).astype(np.uint32)
        if rng.random() < 0.3 and n >= 2:                                  # an exact cancellation of the largest term
            i = int(np.argmax(ex))
            p[(i + 1) % n] = p[i] ^ np.uint32(0x80000000)
        want = np.float32(math.fsum(p.view(np.float32).astype(np.float64).tolist()))
        assert R.exact_sum_bits(p.tolist()) == bits(want + np.float32(0.0)), [hex(v) for v in p]      # + 0.0: a zero total is +0.0


@pytest.mark.parametrize("terms", [
    [2 ** 24, 1],                                  # tie, even below: stays
    [2 ** 24 + 2, 1],                              # tie, odd below: up
    [2 ** 24 + 2, -1],                             # tie from above, odd: down to 2^24
    [2 ** 24 + 4, -1],                             # tie from above, to the even 2^24 + 4
    [2 ** 24 - 1, Fraction(1, 2)],                 # tie at an odd mantissa of all ones: up into the next binade
    [2 ** 24, 1, Fraction(1, 1 << 20)],            # above the tie
    [2 ** 24, 1, -Fraction(1, 1 << 20)],           # below the tie
    [-(2 ** 24), -1],
    [-(2 ** 24 + 2), -1],
    [-(2 ** 24 - 1), -Fraction(1, 2)],
    [Fraction(2 ** 24 + 2, 1 << 90), Fraction(1, 1 << 90)],
    [2.0 ** 100, 1.0, -(2.0 ** 100)],              # float64 loses this one; every term here is exact in f32 and the total in float64
])
def test_equals_float32_of_the_fraction_on_ties(terms):
    total = sum(Fraction(t) for t in terms)
    assert Fraction(float(total)) == total                                  # exact in float64, so np.float32 rounds it once
    assert R.exact_sum_bits([bits(float(t)) for t in terms]) == bits(np.float32(float(total)))


def test_a_sticky_bit_three_limbs_down_breaks_the_tie():
    tie = [bits(2.0 ** 24), bits(1.0)]
    assert R.exact_sum_bits(tie) == bits(2.0 ** 24)
    assert R.exact_sum_bits(tie + [bits(2.0 ** -96)]) == bits(2.0 ** 24 + 2)
    assert R.exact_sum_bits(tie + [bits(-2.0 ** -96)]) == bits(2.0 ** 24)
    up = [bits(2.0 ** 24 + 2), bits(1.0)]
    assert R.exact_sum_bits(up + [bits(-2.0 ** -96)]) == bits(2.0 ** 24 + 2)
    assert R.exact_sum_bits(up) == R.exact_sum_bits(up + [bits(2.0 ** -96)]) == bits(2.0 ** 24 + 4)


def test_rounding_step_equals_float32_of_an_integer():
    # np.float32(int) goes through float64; for a 60-bit integer that first rounding could only matter if bits 7 .. 35 spelled a
    # near-tie (2^-28 per case), and the hand-written ties above do not depend on it
    rng = np.random.default_rng(2)
    for _ in range(10000):
        v = int(rng.integers(1 << 59, 1 << 60)) >> int(rng.integers(0, 36))
        v = -v if rng.random() < 0.5 else v
        assert R.round_to_f32_bits(v, 0) == bits(np.float32(v)), v
    for v in [1, 3, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 3, (1 << 25) - 1, (1 << 60) - 1, (1 << 59) + (1 << 35), (1 << 59) + (3 << 35)]:
        assert R.round_to_f32_bits(v, 0) == bits(np.float32(v)) and R.round_to_f32_bits(-v, 0) == bits(np.float32(-v))
    assert R.round_to_f32_bits(0) == 0


def test_inf_threshold():
    cut = ((1 << 128) - (1 << 103)) << 96                                   # (FLT_MAX + 2^103) * 2^96
    assert R.round_to_f32_bits(cut - 1) == FLT_MAX and R.round_to_f32_bits(cut) == 0x7F800000
    assert R.round_to_f32_bits(1 - cut) == 0x80000000 | FLT_MAX and R.round_to_f32_bits(-cut) == 0xFF800000
    assert R.round_to_f32_bits(1 << 300) == 0x7F800000
    assert R.exact_sum_bits([FLT_MAX, bits(2.0 ** 103)]) == 0x7F800000
    assert R.exact_sum_bits([FLT_MAX, bits(2.0 ** 103), bits(-2.0 ** -96)]) == FLT_MAX
    assert R.exact_sum_bits([FLT_MAX, bits(2.0 ** 103 - 2.0 ** 79)]) == FLT_MAX
    assert R.exact_sum_bits([bits(2.0 ** 127)] * 2) == 0x7F800000
    assert R.exact_sum_bits([bits(2.0 ** 127)] * 2 + [bits(-2.0 ** 127)]) == bits(2.0 ** 127)
    assert R.exact_sum_bits([bits(-2.0 ** 127)] * 2) == 0xFF800000


def test_truncation_at_2_pow_minus_96_and_zero_totals():
    assert R.exact_sum_bits([]) == 0
    assert R.exact_sum_bits([0x80000000] * 5) == 0                          # only -0.0: +0.0
    assert R.exact_sum_bits([bits(3.5), bits(-3.5)]) == 0
    assert R.exact_sum_bits([0x007FFFFF, 0x807FFFFF, 0x00000001]) == 0      # subnormals count as nothing
    assert R.exact_sum_bits([bits(2.0 ** -97)] * 8) == 0                    # each below 2^-96: nothing, though they add up to 2^-94
    assert R.exact_sum_bits([bits(1.75 * 2.0 ** -96)]) == bits(2.0 ** -96)  # towards zero
    assert R.exact_sum_bits([bits(-1.75 * 2.0 ** -96)]) == bits(-2.0 ** -96)
    assert R.exact_sum_bits([bits(-1.75 * 2.0 ** -96), bits(1.75 * 2.0 ** -96)]) == 0
    x = (2 ** 23 + 1) * 2.0 ** -97                                          # bit 0 below 2^-96: cut
    assert R.exact_sum_bits([bits(x)]) == bits(2.0 ** -74)
    y = (2 ** 23 + 1) * 2.0 ** -96                                          # 2^-73 and up: unchanged
    assert R.exact_sum_bits([bits(y)]) == bits(y)
    with pytest.raises(ValueError):
        R.exact_sum_bits([0x7F800000])
    with pytest.raises(ValueError):
        R.exact_sum_bits([0x7FC00000])


def test_f32_bits_of_scaled():
    for v in [1.0, -1.5, 2.0 ** -149, 3 * 2.0 ** -149, 2.0 ** -126, value(FLT_MAX), -value(0x00FFFFFF)]:
        num, den = Fraction(v).numerator, Fraction(v).denominator
        assert R.f32_bits_of_scaled(num, -(den.bit_length() - 1)) == bits(v)
        assert R.f32_bits_of_scaled(num << 7, -(den.bit_length() - 1) - 7) == bits(v)
    for S, q in [((1 << 24) + 1, 0), (1, 128), (1, -150), (3, -150), ((1 << 24) - 1, 105)]:
        with pytest.raises(ValueError):
            R.f32_bits_of_scaled(S, q)


def test_driver_guards_representability():
    x = np.zeros((1, 1, 16, 128), np.float32)
    lab = np.zeros((1, 16, 128), np.int32)
    x[0, 0, 3, 5], x[0, 0, 9, 70] = 2.0 ** 24, 1.0                          # two tiles: two exact partials, one tie
    assert R.exact_pool(x, lab, 1)[0, 0, 0] == bits(2.0 ** 24)
    x[0, 0, 9, 70], x[0, 0, 9, 60] = 0.0, 1.0                               # one tile: its partial 2^24 + 1 is no f32
    with pytest.raises(ValueError, match="not representable"):
        R.exact_pool(x, lab, 1)
    x[0, 0, 9, 60] = 2.0 ** -100                                            # a spread of 124 binades inside one tile
    with pytest.raises(ValueError, match="not representable"):
        R.exact_pool(x, lab, 1)
    x[0, 0, 3, 5] = -(2.0 ** -100)                                          # ... and an exact cancellation over that spread
    x[0, 0, 4, 4] = 2.0 ** 20
    x[0, 0, 15, 63] = -(2.0 ** 20)
    assert R.exact_pool(x, lab, 1)[0, 0, 0] == 0
    with pytest.raises(ValueError, match="finite"):
        R.exact_pool(np.full((1, 1, 2, 2), np.inf, np.float32), np.zeros((1, 2, 2), np.int32), 1)


def test_driver_equals_float64_on_small_integers():
    rng = np.random.default_rng(3)
    x = rng.integers(-1023, 1024, (2, 3, 37, 150)).astype(np.float32) * np.float32(2.0 ** -10)
    lab = rng.integers(-2, 12, (2, 37, 150)).astype(np.int16)
    got = R.exact_pool(x, lab, 10)
    ref = R.pool(x, lab, 10)["sum"]                                         # exact in float64, and in f32: below 2^24 * 2^-10
    assert np.array_equal(got.view(np.float32).astype(np.float64), ref)
    assert np.array_equal(got, (ref.astype(np.float32) + np.float32(0.0)).view(np.uint32))
