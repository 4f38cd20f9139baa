"""Exact reference for ptsharp_amd/csrc/pt_accum.h (tests/test_accum_ref.py on the CPU, tests/test_gpu_accum.py).

Two kinds of statement, kept apart:
  * restatements (to_fix, fix_value): the header's own fp64 operations, one numpy operation each.  The device
    must equal them bit for bit; test_accum_ref.py holds them to the exact contract below;
  * the exact contract, in Python ints and fractions.Fraction, which models none of the algorithm:
      to_fix      |V - x·2^44| <= 1/2 + 2^-22 for every |x| < 2^19, and V = round-half-even(x·2^44) for x >= 0
                  (for a small negative x, s - floor(s) rounds: NEG_TIE below gives 0 where exact rounding gives -1);
      accumulator T(i,k) = Σ V over the terms of accumulator i, channel k with |x| < 2^19 and x != 0, as an int;
                  the words are lo = T mod 2^64 and hi = T >> 64; the remaining terms are summed in fp64 (callers
                  choose them so that this sum does not depend on the order);
      fix_value   T·2^-44 correctly rounded when T fits 64 signed bits, within 2^-51 relative otherwise;
      run count   per 64-slot row, the adding lanes whose previous adding lane has another index, or has none.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

FIX_BIG = 2.0 ** 19      # kFixBig: at or above, the fp64 side sum
FIX_WAVE = 2.0 ** 13     # kFixWave: at or above, a lane of fix_add_wave adds on its own
FIX_LDS = 64.0           # kFixLds: the same with a block's LDS table
SCALE = 1 << 44
TO_FIX_BOUND = Fraction(1, 2) + Fraction(1, 1 << 22)
NEG_TIE = -(2.0 ** -45 + 2.0 ** -72)   # s - floor(s) = 1 - 2^-33 - 2^-60 rounds to 1 - 2^-33, the magic add ties to even: V = 0
_MAGIC = np.float64(2.0 ** 52)


def fix_ok(x) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(x, np.float64)) < FIX_BIG    # False for NaN too


def to_fix(x) -> np.ndarray:
    """The five fp64 operations of to_fix, for |x| < 2^19: int64 V."""
    x = np.asarray(x, np.float64)
    assert fix_ok(x).all()
    s = x * np.float64(4096.0)
    f = np.floor(s)
    frac = s - f
    y = frac * np.float64(4294967296.0)
    m = y + _MAGIC
    lo = m.view(np.int64) - _MAGIC.view(np.int64)
    return f.astype(np.int32).astype(np.int64) * np.int64(4294967296) + lo


def exact_scaled(x: float) -> Fraction:
    return Fraction(float(x)) * SCALE


def round_half_even(x: float) -> int:
    return round(exact_scaled(x))    # Fraction.__round__: to nearest, ties to even


def to_fix_contract(x: float, v: int) -> None:
    """Raises unless V meets to_fix's contract for x."""
    e = abs(v - exact_scaled(x))
    assert e <= TO_FIX_BOUND, f"to_fix({float(x).hex()}) = {v}: off by {float(e)}"
    if x >= 0:
        assert v == round_half_even(x), f"to_fix({float(x).hex()}) = {v}, round-half-even {round_half_even(x)}"


def split(t: int):
    """T -> (hi signed, lo unsigned), T = hi·2^64 + lo."""
    return t >> 64, t & ((1 << 64) - 1)


def fix_value(hi, lo) -> np.ndarray:
    """fix_value restated: hi int64, lo uint64 arrays."""
    hi = np.asarray(hi, np.int64)
    lo = np.asarray(lo, np.uint64)
    slo = lo.view(np.int64)
    inv = np.float64(1.0 / 17592186044416.0)
    one = slo.astype(np.float64) * inv
    two = hi.astype(np.float64) * np.float64(1048576.0) + lo.astype(np.float64) * inv
    return np.where(hi == (slo >> np.int64(63)), one, two)


def fix_value_int(t: int) -> float:
    hi, lo = split(t)
    return float(fix_value(np.array([hi], np.int64), np.array([lo], np.uint64))[0])


def fits64(t: int) -> bool:
    return -(1 << 63) <= t < (1 << 63)


def exact_value(t: int) -> float:
    """T·2^-44 correctly rounded."""
    return float(Fraction(t, SCALE))


def fix_value_contract(t: int, v: float) -> None:
    if fits64(t):
        assert v == exact_value(t), f"T = {t}: {v!r} is not the correctly rounded {exact_value(t)!r}"
    else:
        e = abs(Fraction(v) - Fraction(t, SCALE))
        assert e <= Fraction(abs(t), SCALE) / (1 << 51), f"T = {t}: {v!r} off by {float(e)}"


def accumulate(idx, rgb, n: int, has=None):
    """The terms (idx [m], rgb [m][3], has [m] or None) into n accumulators.
    Returns T (n x 3 list of Python ints), lo (uint64 [3][n]), hi (int64 [3][n]: the header's planar layout, channel
    k of accumulator i at k·n + i once flattened), big (float64 [3][n]: the side sums, added in slot order) and
    value (float64 [n][3]: fix_value + big)."""
    idx = np.asarray(idx, np.int64)
    rgb = np.asarray(rgb, np.float64).reshape(-1, 3)
    has = np.ones(len(idx), bool) if has is None else np.asarray(has, bool)
    T = [[0, 0, 0] for _ in range(n)]
    big = np.zeros((3, n), np.float64)
    assert len(idx) == len(rgb) == len(has) and (len(idx) == 0 or (0 <= idx.min() and idx.max() < n))
    with np.errstate(invalid="ignore", over="ignore"):
        adds = has[:, None] & (rgb != 0.0)
        ok = fix_ok(rgb)
        v = to_fix(np.where(ok, rgb, 0.0))
        for j, k in zip(*np.nonzero(adds & ok)):
            T[idx[j]][k] += int(v[j, k])
        for j, k in zip(*np.nonzero(adds & ~ok)):
            big[k, idx[j]] += rgb[j, k]
        lo = np.zeros((3, n), np.uint64)
        hi = np.zeros((3, n), np.int64)
        for i in range(n):
            for k in range(3):
                h, l = split(T[i][k])
                hi[k, i], lo[k, i] = h, l
        value = (fix_value(hi, lo) + big).T.copy()
    return T, lo, hi, big, value


def run_counts(idx, has, rows: int) -> np.ndarray:
    """Runs per 64-slot row (slots past len(idx) add nothing)."""
    out = np.zeros(rows, np.uint32)
    for r in range(rows):
        prev = None
        for j in range(64 * r, min(64 * r + 64, len(idx))):
            if not has[j]:
                continue
            if prev is None or idx[prev] != idx[j]:
                out[r] += 1
            prev = j
    return out


# ---- inputs shared by the CPU and GPU tests
def neighbours(x: float):
    return [float(np.nextafter(x, -np.inf)), float(x), float(np.nextafter(x, np.inf))]


def conversion_edges() -> np.ndarray:
    """Finite conversion inputs at the edges (|x| >= 2^19 among them: fix_ok false, no V)."""
    e = [0.0, -0.0, 5e-324, -5e-324, NEG_TIE, 1.0 - 2.0 ** -53]
    for m in (2.0 ** -46, 2.0 ** -45, 1.5 * 2.0 ** -44, 2.5 * 2.0 ** -44):   # below half a unit, a tie, two more ties
        e += [m, -m]
    for k in (0, 1, 7, 4095, 4096, 123457, (1 << 31) - 1):                    # floor(s) boundaries, either side
        for d in (-(2.0 ** -60), 2.0 ** -60):
            e += [k / 4096.0 + d, -(k / 4096.0) + d]
    for b in (FIX_LDS, FIX_WAVE, FIX_BIG):
        e += neighbours(b) + neighbours(-b)
    return np.array(e, np.float64)


def seeded_values(n: int, seed: int) -> np.ndarray:
    """n values, 53 random mantissa bits, exponents -70 to 18, both signs."""
    rng = np.random.default_rng(seed)
    m = 1.0 + rng.integers(0, 1 << 52, n).astype(np.float64) * 2.0 ** -52
    return np.ldexp(m, rng.integers(-70, 19, n)) * rng.choice([-1.0, 1.0], n)


def fix_value_totals(seed: int = 7):
    """T at fix_value's branch boundary, seeded T up to 100 bits, and the totals of single conversions."""
    t = [0, 1, -1, (1 << 63) - 1, -(1 << 63), 1 << 63, -(1 << 63) - 1, 1 << 64, -(1 << 64), (1 << 64) + 1, -(1 << 64) - 1]
    rng = np.random.default_rng(seed)
    for _ in range(200):
        bits = int(rng.integers(1, 101))
        v = int.from_bytes(rng.bytes(13), "little") & ((1 << bits) - 1)
        t.append(-v if rng.integers(0, 2) else v)
    x = np.concatenate([conversion_edges(), seeded_values(200, seed + 1)])
    t += [int(v) for v in to_fix(x[fix_ok(x)])]
    return t
