"""tests/accum_ref.py held to its own contract on the CPU: the numpy restatements of pt_accum.h's to_fix and
fix_value against exact arithmetic (fractions.Fraction, Python ints), and the word split, the side sum and the run
count on hand-worked examples.  tests/test_gpu_accum.py then holds the device to accum_ref."""
from fractions import Fraction

import numpy as np

import accum_ref as R


def test_to_fix_restatement_meets_the_contract():
    x = np.concatenate([R.conversion_edges(), R.seeded_values(2000, 1)])
    x = x[R.fix_ok(x)]
    assert len(x) > 2000 and (x < 0).any() and (x > 0).any()
    v = R.to_fix(x)
    for xi, vi in zip(x.tolist(), v.tolist()):
        R.to_fix_contract(xi, vi)


def test_to_fix_equals_exact_rounding_on_seeded_values():
    """No seeded value is a double-rounding input (those need some 30 set bits in a row below 2^-45)."""
    x = R.seeded_values(2000, 1)
    assert R.to_fix(x).tolist() == [R.round_half_even(v) for v in x.tolist()]


def test_to_fix_hand_values():
    u = 2.0 ** -44
    cases = {0.0: 0, -0.0: 0, 5e-324: 0, -5e-324: 0, u: 1, -u: -1, 0.5 * u: 0, -0.5 * u: 0, 1.5 * u: 2, -1.5 * u: -2,
             2.5 * u: 2, -2.5 * u: -2, 0.25 * u: 0, 1.0: 1 << 44, -1.0: -(1 << 44), 1.0 - 2.0 ** -53: 1 << 44,
             float(np.nextafter(R.FIX_BIG, 0)): (1 << 63) - (1 << 10), -float(np.nextafter(R.FIX_BIG, 0)): -(1 << 63) + (1 << 10),
             64.0: 1 << 50, 8192.0: 1 << 57}
    x = np.array(list(cases))
    assert R.to_fix(x).tolist() == list(cases.values())


def test_to_fix_double_rounding_input_is_pinned():
    """x = -(2^-45 + 2^-72): x·2^44 = -0.5000000037, round-half-even -1; the five operations give 0 (s - floor(s)
    rounds up to 1 - 2^-33, and the magic-number add then sees an exact tie).  Inside the stated bound."""
    x = R.NEG_TIE
    assert x == -(2.0 ** -45 + 2.0 ** -72)
    assert R.round_half_even(x) == -1
    assert int(R.to_fix(x)) == 0
    e = abs(0 - R.exact_scaled(x))
    assert e == Fraction(1, 2) + Fraction(1, 1 << 28) and e <= R.TO_FIX_BOUND
    R.to_fix_contract(x, 0)


def test_fix_ok():
    x = np.array([0.0, 524287.99, 524288.0, -524288.0, np.inf, -np.inf, np.nan, -np.nextafter(524288.0, 0)])
    assert R.fix_ok(x).tolist() == [True, True, False, False, False, False, False, True]


def test_split_words():
    assert R.split(0) == (0, 0)
    assert R.split(-1) == (-1, (1 << 64) - 1)
    assert R.split(1 << 63) == (0, 1 << 63)
    assert R.split(-(1 << 63)) == (-1, 1 << 63)
    assert R.split(-(1 << 63) - 1) == (-1, (1 << 63) - 1)
    assert R.split(1 << 64) == (1, 0)
    assert R.split(-(1 << 64) - 1) == (-2, (1 << 64) - 1)
    for t in R.fix_value_totals():
        hi, lo = R.split(t)
        assert hi * (1 << 64) + lo == t and 0 <= lo < 1 << 64


def test_fix_value_restatement_meets_the_contract():
    """One-word totals are converted correctly rounded; two-word ones (|T| >= 2^63: the conversion of lo, the
    product by a power of two (exact) and the sum round, without cancellation below half of |T|) within 2^-51."""
    ts = R.fix_value_totals()
    assert sum(not R.fits64(t) for t in ts) > 50 and sum(R.fits64(t) for t in ts) > 50
    for t in ts:
        R.fix_value_contract(t, R.fix_value_int(t))
    assert R.fix_value_int(1 << 63) == 2.0 ** 19
    assert R.fix_value_int(-(1 << 63)) == -2.0 ** 19
    assert R.fix_value_int(1 << 64) == 2.0 ** 20
    assert R.fix_value_int(-(1 << 63) - 1) == -2.0 ** 19     # the exact value, -2^19 - 2^-44, rounds to it
    assert R.fix_value_int(-3) == -3 * 2.0 ** -44


def test_fix_value_contract_rejects_the_two_word_form_of_a_negative_total():
    """What the one-step branch is for: T = -1 through the two-word form is 0, not -2^-44."""
    two = float(np.float64(-1.0) * 1048576.0 + np.float64(2.0 ** 64) * (1.0 / 17592186044416.0))
    assert two == 0.0
    try:
        R.fix_value_contract(-1, two)
    except AssertionError:
        return
    raise AssertionError("the contract accepted a wrong value")


def test_accumulate_hand_example():
    """Three accumulators: 0 takes a carry (two terms of 2^19 - 2^-34, T = 2^64 - 2^11), 1 a borrow and side terms
    (inf and -inf give NaN), 2 nothing."""
    a = float(np.nextafter(R.FIX_BIG, 0))
    idx = [0, 0, 1, 1, 1, 1, 2]
    rgb = [[a, 1.0, 0.0], [a, -1.0, 0.0], [-a, 2.0 ** 19, np.inf], [-a, 2.0 ** 20, -np.inf], [-a, 0.0, 0.0],
           [0.0, -0.0, 1e300], [0.0, 0.0, 0.0]]
    has = [1, 1, 1, 1, 1, 0, 1]
    T, lo, hi, big, val = R.accumulate(idx, rgb, 3, has)
    assert T[0] == [(1 << 64) - (1 << 11), 0, 0]
    assert T[1] == [-3 * ((1 << 63) - (1 << 10)), 0, 0]
    assert T[2] == [0, 0, 0]
    assert (int(hi[0, 0]), int(lo[0, 0])) == (0, (1 << 64) - (1 << 11))
    assert (int(hi[0, 1]), int(lo[0, 1])) == (-2, (1 << 63) + 3 * (1 << 10))
    assert big[1, 1] == 3 * 2.0 ** 19 and np.isnan(big[2, 1]) and big[2, 0] == 0.0
    assert val[0].tolist() == [2 * a, 0.0, 0.0]
    assert val[1, 0] == -3 * a and val[1, 1] == 3 * 2.0 ** 19 and np.isnan(val[1, 2])
    assert val[2].tolist() == [0.0, 0.0, 0.0]


def test_run_counts_hand_examples():
    def rc(idx, has=None):
        has = [1] * len(idx) if has is None else has
        return R.run_counts(idx, has, (len(idx) + 63) // 64).tolist()
    assert rc([5] * 64) == [1]
    assert rc(list(range(64))) == [64]
    assert rc([1, 1, 2, 2, 1]) == [3]                               # A B A: two runs of A
    assert rc([1, 1, 9, 1, 2], [1, 1, 0, 1, 1]) == [2]              # a hole does not split a run
    assert rc([1, 9, 2], [1, 0, 1]) == [2]
    assert rc([3] * 70) == [1, 1]                                   # a run that crosses a row is two
    assert rc([3] * 64 + [4] * 3, [0] * 64 + [1, 0, 1]) == [0, 1]   # a row without an adder
    assert rc([7] * 64, [1] + [0] * 63) == [1] and rc([7] * 64, [0] * 63 + [1]) == [1]
