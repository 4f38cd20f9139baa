"""ptsharp_amd/csrc/pt_accum.h on the device, against tests/accum_ref.py.

Sections 1-4 drive the unchanged header through tests/native/accum_gpu.hip (libpt_accum_check.so, built by the
product Makefile with the product's flags): the conversion and fix_value bit for bit against their fp64 restatements
(which tests/test_accum_ref.py holds to the exact contract), and the register, per-lane, wave-aggregated and
LDS-table sums against exact Python-int totals: the raw low and high words, the fp64 side sums, the values fix_take
returns, the planes cleared afterwards, the guard accumulator that lanes without a term point at, and the runs issued.
Side-sum inputs are chosen so that their fp64 sum does not depend on the order (at most two terms per accumulator
and channel, or multiples of 2^19 whose partial sums are exact).

Section 5 sends the same regimes through the real engines against the oracle: emitters whose terms straddle kFixWave
and kFixBig and whose pixel totals are 2^63, 2^64 and 2^65, and direct-light terms of 2^13 and more through
k_wf_nee_accum's LDS table and flush.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import accum_ref as R
import oracle_lib as O
from parity import check, render_both, render_gpu, same_buffer
from ptsharp_amd import _abi, tiles_for_rank
from ptsharp_amd.geometry import Colour, Vector
from ptsharp_amd.scene import Camera, DefaultSampler, Material, Plane, Scene, Sphere

pytestmark = pytest.mark.gpu

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "libpt_accum_check.so")
ENGINES = pytest.mark.parametrize("engine", [_abi.ENGINE_MEGAKERNEL, _abi.ENGINE_WAVEFRONT], ids=["mega", "wave"])
A19 = float(np.nextafter(2.0 ** 19, 0))    # 2^19 - 2^-34, the largest fixed-point term: V = 2^63 - 2^10
A13 = 2.0 ** 13 - 2.0 ** -40               # below kFixWave: 64 of them in one run sum to 2^63 - 2^10
A6 = 64.0 - 2.0 ** -44                     # below kFixLds: 4096 of them in one table entry sum to 2^62 - 2^12
NAN, INF = float("nan"), float("inf")


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Harness:
    def __init__(self, lib):
        self.lib = lib

    def to_fix(self, x):
        x = np.ascontiguousarray(x, np.float64)
        v, ok = np.full(len(x), -7, np.int64), np.full(len(x), -7, np.int32)
        rc = self.lib.acc_to_fix(_p(x, C.c_double), C.c_int64(len(x)), _p(v, C.c_longlong), _p(ok, C.c_int32))
        assert rc == 0, f"acc_to_fix: HIP error {rc}"
        return v, ok

    def fix_value(self, totals):
        hl = [R.split(t) for t in totals]
        hi, lo = np.array([h for h, _ in hl], np.int64), np.array([l for _, l in hl], np.uint64)
        out = np.full(len(hi), NAN)
        rc = self.lib.acc_fix_value(_p(hi, C.c_longlong), _p(lo, C.c_ulonglong), C.c_int64(len(hi)), _p(out, C.c_double))
        assert rc == 0, f"acc_fix_value: HIP error {rc}"
        return hi, lo, out

    def fixreg(self, cases):
        """cases: a list of [count][3] term lists (count <= 64)."""
        n = len(cases)
        terms, counts = np.full((n, 64, 3), NAN), np.array([len(c) for c in cases], np.int32)
        for i, c in enumerate(cases):
            terms[i, :len(c)] = np.asarray(c, np.float64).reshape(-1, 3)
        lo, hi = np.full((n, 3), 7, np.uint64), np.full((n, 3), 7, np.int64)
        big, val = np.full((n, 3), 7.0), np.full((n, 3), 7.0)
        rc = self.lib.acc_fixreg(_p(terms, C.c_double), _p(counts, C.c_int32), C.c_int64(n), _p(lo, C.c_ulonglong),
                                 _p(hi, C.c_longlong), _p(big, C.c_double), _p(val, C.c_double))
        assert rc == 0, f"acc_fixreg: HIP error {rc}"
        return lo, hi, big, val

    def add(self, mode, idx, rgb, n, has=None, grid=2):
        idx = np.ascontiguousarray(idx, np.uint32)
        rgb = np.ascontiguousarray(np.asarray(rgb, np.float64).reshape(-1, 3))
        m = len(idx)
        assert len(rgb) == m and (m == 0 or int(idx.max()) < n)
        u = lambda: np.full(3 * n, 7, np.uint64)
        d = lambda: np.full(3 * n, 7.0)
        o = dict(w=u(), hi=u(), big=d(), taken=d(), w2=u(), hi2=u(), big2=d())
        planes = [_p(o["w"], C.c_ulonglong), _p(o["hi"], C.c_ulonglong), _p(o["big"], C.c_double), _p(o["taken"], C.c_double),
                  _p(o["w2"], C.c_ulonglong), _p(o["hi2"], C.c_ulonglong), _p(o["big2"], C.c_double)]
        if mode == "lane":
            assert has is None
            rc = self.lib.acc_add_lane(_p(idx, C.c_uint32), _p(rgb, C.c_double), C.c_int64(m), C.c_int64(n), *planes)
        else:
            has = np.ascontiguousarray(np.ones(m, np.uint8) if has is None else np.asarray(has, np.uint8))
            span = 256 if mode == "wave" else 4096
            o["runs"] = np.full((m + span - 1) // span * (span // 64), 999, np.uint32)
            fn = self.lib.acc_add_wave if mode == "wave" else self.lib.acc_add_wave_lds
            rc = fn(_p(idx, C.c_uint32), _p(rgb, C.c_double), _p(has, C.c_uint8), C.c_int64(m), C.c_int64(n), C.c_int(grid),
                    *planes, _p(o["runs"], C.c_uint32))
        assert rc == 0, f"acc_add_{mode}: HIP error {rc}"
        o["hi"], o["hi2"] = o["hi"].view(np.int64), o["hi2"].view(np.int64)
        return o


@pytest.fixture(scope="module")
def acc(gpu):
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} is missing: `make -C ptsharp_amd/csrc` (what build() runs) builds it from "
                    "tests/native/accum_gpu.hip; there is no fallback")
    return Harness(C.CDLL(LIB))


def expect(o, idx, rgb, n, has=None, guard=True):
    """Every output of an acc_add_* call against the exact reference."""
    idx, rgb = np.asarray(idx), np.asarray(rgb, np.float64).reshape(-1, 3)
    hasb = np.ones(len(idx), bool) if has is None else np.asarray(has, bool)
    if guard:
        assert not (idx[hasb] == n - 1).any(), "the test's own terms use the guard accumulator"
    T, lo, hi, big, val = R.accumulate(idx, rgb, n, hasb)
    bad = np.flatnonzero(o["w"] != lo.reshape(-1))
    assert bad.size == 0, f"low words differ at (channel, accumulator) {[(int(b) // n, int(b) % n) for b in bad[:8]]}"
    bad = np.flatnonzero(o["hi"] != hi.reshape(-1))
    assert bad.size == 0, f"high words differ at (channel, accumulator) {[(int(b) // n, int(b) % n) for b in bad[:8]]}"
    assert np.array_equal(o["big"], big.reshape(-1), equal_nan=True), "side sums differ"
    assert np.array_equal(o["taken"].reshape(n, 3), val, equal_nan=True), "fix_take's values differ"
    for i in range(n):     # the values against exact arithmetic too, where no side sum takes part
        for k in range(3):
            if big[k, i] == 0.0:
                R.fix_value_contract(T[i][k], float(o["taken"][3 * i + k]))
    assert not o["w2"].any() and not o["hi2"].any(), "fix_take left words behind"
    assert np.array_equal(o["big2"].view(np.uint64), np.zeros(3 * n, np.uint64)), "fix_take left a side sum behind"
    if guard:
        g = [k * n + n - 1 for k in range(3)]
        assert not o["w"][g].any() and not o["hi"][g].any() and np.array_equal(o["big"][g].view(np.uint64), np.zeros(3, np.uint64)), \
            "a lane without a term wrote to the guard accumulator"
    if "runs" in o:
        want = R.run_counts(idx, hasb, len(o["runs"]))
        assert np.array_equal(o["runs"], want), f"run counts {o['runs'].tolist()} != {want.tolist()}"
    return T


# ---------------------------------------------------------------- 1. conversion
def test_to_fix_bit_equal_and_in_contract(acc):
    x = np.concatenate([R.conversion_edges(), R.seeded_values(2000, 1)])
    v, ok = acc.to_fix(np.concatenate([x, [NAN, INF, -INF]]))
    want_ok = R.fix_ok(x)
    assert ok.tolist() == want_ok.astype(int).tolist() + [0, 0, 0]
    assert 0 < (~want_ok).sum() < 20        # the edges at and past ±2^19 only
    xs, vs = x[want_ok], v[:len(x)][want_ok]
    bad = np.flatnonzero(vs != R.to_fix(xs))
    assert bad.size == 0, f"to_fix differs from its restatement at {[xs[b].hex() for b in bad[:8]]}"
    for xi, vi in zip(xs.tolist(), vs.tolist()):
        R.to_fix_contract(xi, vi)
    assert vs[xs == R.NEG_TIE].tolist() == [0]      # the double-rounding input (accum_ref.NEG_TIE)


# ---------------------------------------------------------------- 2. fix_value
def test_fix_value_bit_equal_and_in_contract(acc):
    ts = R.fix_value_totals()
    hi, lo, out = acc.fix_value(ts)
    want = R.fix_value(hi, lo)
    bad = np.flatnonzero(out.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, f"fix_value differs from its restatement at T = {[ts[b] for b in bad[:8]]}"
    for t, v in zip(ts, out.tolist()):
        R.fix_value_contract(t, v)


# ---------------------------------------------------------------- 3. register and per-lane sums
def _sequences():
    rng = np.random.default_rng(3)
    col = lambda a: [[a, a / 2, a / 4]] * 64
    alt = [[A19 if j % 2 else -A19, -A19 + j * 2.0 ** -30 if j % 2 else A19, (-1) ** j * 1.0] for j in range(64)]
    side = [[2.0 ** 19, 1e300, INF], [1.5, -2.0 ** -44, 0.25], [3 * 2.0 ** 19, 1e300, 1e300], [-A19, NAN, -INF],
            [INF, 1.0, -INF], [-INF, 2.0, 0.0]]      # r: 2^21 exact, then inf - inf; g: 2e300 then NaN; b: inf, then -inf: NaN
    return {
        "carry": col(A19),                                  # 64 · 2^19: two carries out of the low word and more
        "borrow": col(-A19),
        "alternate": alt,                                   # carries and borrows cancel
        "zeros": [[0.0, -0.0, 0.0]] * 5,
        "side": side,
        "two-side": [[2.0 ** 19, -1e300, 3.0], [-2.0 ** 20, 1e300, -3.0]],
        "inf-side": [[INF, -INF, 1e300], [5.0, -5.0, 1e300], [2.0 ** 19, -2.0 ** 19, 0.0]],
        "seeded": (rng.uniform(-1, 1, (64, 3)) * 2.0 ** rng.integers(-50, 20, (64, 3))).tolist(),
        "seeded-big": rng.uniform(-A19, A19, (64, 3)).tolist(),
        "one": [[-2.0 ** -44, 2.0 ** -44, R.NEG_TIE]],
        "none": [],
    }


def test_fixreg(acc):
    seqs = _sequences()
    names = list(seqs)
    lo, hi, big, val = acc.fixreg([seqs[k] for k in names])
    for c, name in enumerate(names):
        t = np.asarray(seqs[name], np.float64).reshape(-1, 3)
        T, elo, ehi, ebig, eval_ = R.accumulate(np.zeros(len(t), int), t, 1)
        assert lo[c].tolist() == elo[:, 0].tolist(), f"{name}: low words"
        assert hi[c].tolist() == ehi[:, 0].tolist(), f"{name}: high words"
        assert np.array_equal(big[c], ebig[:, 0], equal_nan=True), f"{name}: side sums"
        assert np.array_equal(val[c], eval_[0], equal_nan=True), f"{name}: values"
    c = names.index("carry")
    assert hi[c, 0] == 31 and (hi[names.index("borrow")] < 0).all()      # 64·(2^63 - 2^10) = 31·2^64 + (2^64 - 2^16)
    assert hi[names.index("alternate"), 0] == 0


def test_add_lane_sequences_planar(acc):
    """The sequences of test_fixreg spread over the accumulators of n = 5 (the side-sum ones apart, so that every
    side sum stays free of the order): channel k of accumulator i is word k·5 + i of each plane."""
    seqs = _sequences()
    where = {"carry": 0, "seeded": 0, "borrow": 1, "two-side": 1, "one": 1, "alternate": 2, "zeros": 2, "side": 3,
             "seeded-big": 4, "inf-side": 4}
    assert set(where) | {"none"} == set(seqs)
    idx, rgb = [], []
    for name, i in where.items():
        idx += [i] * len(seqs[name])
        rgb += seqs[name]
    o = acc.add("lane", idx, rgb, 5)
    T = expect(o, idx, rgb, 5, guard=False)
    assert T[0][0] > 1 << 64 and T[1][0] < -(1 << 64)
    assert int(o["w"][1 * 5 + 0]) == T[0][1] % (1 << 64) and int(o["hi"][1 * 5 + 0]) == T[0][1] >> 64


@pytest.mark.parametrize("n", [1, 5])
def test_add_lane_4096_threads(acc, n):
    rng = np.random.default_rng(10 + n)
    rgb = rng.uniform(-A19, A19, (4096, 3))
    rgb[:, 1] = np.abs(rgb[:, 1])                           # one channel carries only
    rgb[rng.integers(0, 4096, 40), rng.integers(0, 3, 40)] = 0.0
    rgb[7, 0], rgb[9, 0], rgb[11, 2] = 2.0 ** 19, 5 * 2.0 ** 19, -2.0 ** 25      # side sums exact in any order
    idx = rng.integers(0, n, 4096)
    T = expect(acc.add("lane", idx, rgb, n), idx, rgb, n, guard=False)
    assert T[0][1] >= 1 << 64


# ---------------------------------------------------------------- 4a. fix_add_wave without a table
def _small(rng, m, scale=8.0):
    return rng.uniform(-scale, scale, (m, 3))


def _runs(lengths, keys):
    """Consecutive runs: the i-th has lengths[i] slots of index keys[i]."""
    return np.repeat(np.asarray(keys), np.asarray(lengths))


def _wave_patterns():
    rng = np.random.default_rng(5)
    P = {}
    P["same64"] = (np.full(64, 3), _small(rng, 64), None, 5)
    P["distinct64"] = (np.arange(64), _small(rng, 64), None, 65)
    # runs of 1, 2, 3, 5, 8, 13 and 32 (64 slots in all) after a first run of 7: no run starts on a row, runs cross
    # rows (64) and blocks (256); 37 indices in turn, so an index comes back in a non-adjacent run
    lens = [7] + [1, 2, 3, 5, 8, 13, 32] * 16
    idx = _runs(lens, np.arange(len(lens)) % 37)[:1024]
    P["runs"] = (idx, _small(rng, 1024, 2.0 ** 12), None, 38)
    # holes: lane 0, inside runs, between two runs of different indices, lane 63; a row that ends inside a run with
    # lane 0 of the next row a hole; one index on both sides of a gap (one run); only holes between the two ends
    has = np.ones(256, bool)
    idx = np.zeros(256, int)
    idx[0:11], idx[11:13], idx[13:41], idx[41:64] = 1, 9, 2, 3
    has[[0, 3, 4, 7, 11, 12, 63]] = False
    has[20:31] = False
    idx[64:128] = 4
    has[[64, 70, 71, 100]] = False
    idx[128:160], idx[160:192] = 5, 6
    has[140:150] = False
    has[158:162] = False                                     # the gap between the runs of 5 and 6
    idx[192:256] = 7
    has[193:255] = False                                     # lanes 0 and 63 of one run, 62 holes between
    P["holes"] = (idx, _small(rng, 256), has, 10)
    has = np.ones(192, bool)
    has[64:128] = False
    P["empty-row"] = (_runs([30, 34, 64, 20, 44], [0, 1, 2, 0, 1]), _small(rng, 192), has, 4)
    has = np.zeros(128, bool)
    has[0], has[127] = True, True
    P["lane0-lane63"] = (np.r_[np.full(64, 2), np.full(64, 1)], _small(rng, 128), has, 4)
    P["a-b-a"] = (_runs([10, 5, 10, 20, 19], [1, 2, 1, 2, 1]), _small(rng, 64), None, 4)
    # run sums of ±(2^63 - 2^10), and their cancellation
    sg = np.r_[np.ones(64), -np.ones(64), np.tile([1.0, -1.0], 32)]
    P["run-near-2^63"] = (_runs([64, 64, 64], [0, 1, 2]), sg[:, None] * np.array([A13, A13, A13 / 2]), None, 4)
    # 64 lanes at and just above the limit on one index: each adds alone; summed as one run they would pass 2^63
    # (64·2^13 = 2^19: T = 2^63 exactly, which a signed 64-bit run sum cannot hold)
    rgb = np.r_[np.tile([2.0 ** 13, A13, 2.0 ** 13], (64, 1)), np.tile([2.0 ** 14 - 2.0 ** -39, -2.0 ** 13, 2.0 ** 14], (64, 1))]
    P["lanes-at-2^13"] = (_runs([64, 64], [0, 1]), rgb, None, 3)
    # one channel at or above 2^13 goes alone, the lane's others join the run
    rgb = _small(rng, 64)
    rgb[4] = [2.0 ** 13, 1.0, -2.0]
    rgb[9] = [3.0, -2.0 ** 14 - 0.375, A13]
    rgb[20] = [A19, -A19, 2.0 ** 13]
    rgb[40, 1] = -2.0 ** 13
    P["one-channel-alone"] = (_runs([16, 16, 32], [0, 1, 0]), rgb, None, 3)
    # a side-sum lane and a NaN lane in the middle of a run: the others are still summed
    rgb = _small(rng, 64)
    rgb[5] = [2.0 ** 19, 1.0, 2.0]
    rgb[7] = [NAN, 1.0, 1.0]
    rgb[9] = [3.0, INF, -INF]
    rgb[30] = [1e300, -INF, 5 * 2.0 ** 19]
    rgb[31] = [1e300, 0.5, -2.0 ** 19]
    P["side-lanes-in-run"] = (_runs([20, 44], [0, 1]), rgb, None, 3)
    P["has-zero-terms"] = (_runs([20, 44, 64], [0, 1, 0]), np.tile([0.0, -0.0, 0.0], (128, 1)), None, 3)
    x = _small(rng, 16)
    rgb = np.concatenate([x, -x, x[:8], -x[:8] * [1, 1, 0]])
    P["cancels"] = (_runs([32, 16], [0, 1]), rgb, None, 3)
    return P


WAVE = _wave_patterns()


@pytest.mark.parametrize("name", list(WAVE))
def test_add_wave(acc, name):
    idx, rgb, has, n = WAVE[name]
    T = expect(acc.add("wave", idx, rgb, n, has), idx, rgb, n, has)
    if name == "run-near-2^63":
        assert T[0][0] == (1 << 63) - (1 << 10) and T[1][0] == -T[0][0] and T[2] == [0, 0, 0]
    if name == "lanes-at-2^13":
        assert T[0][0] == 1 << 63 and T[1][2] == 1 << 64
    if name == "cancels":
        assert T[0] == [0, 0, 0] and T[1][:2] == [0, 0] and T[1][2] != 0


def test_add_wave_equals_add_lane(acc):
    """The same terms through either path leave the same words."""
    idx, rgb, has, n = WAVE["runs"]
    a, b = acc.add("wave", idx, rgb, n), acc.add("lane", idx, rgb, n)
    for k in ("w", "hi", "big", "taken"):
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- 4b. fix_add_wave with a block's LDS table
def _lds_patterns():
    rng = np.random.default_rng(6)
    P = {}
    # a window of 4096 slots on one key: +, -, and alternating; one window per block
    sg = np.r_[np.ones(4096), -np.ones(4096), np.tile([1.0, -1.0], 2048)]
    P["entry-near-2^62"] = (_runs([4096] * 3, [0, 1, 2]), sg[:, None] * np.array([A6, A6 / 2, A6]), None, 4, 3)
    # 1024 keys in one window of a 512-entry table: at least half the runs find their probe sequence full
    P["more-keys-than-entries"] = (np.arange(4096) // 4, _small(rng, 4096, 64.0), None, 1025, 1)
    # nine keys with home slot 100 under idx + (idx >> 9)·8 mod 512, eight slots in a probe sequence
    keys = np.array([512 * q + (100 - 8 * q) % 512 for q in range(9)])
    assert len(set(keys.tolist())) == 9 and {int(k + (k >> 9) * 8) % 512 for k in keys} == {100}
    P["nine-keys-one-home"] = (keys[(np.arange(4096) // 3) % 9], _small(rng, 4096, 64.0), None, int(keys.max()) + 2, 1)
    # terms past each limit inside runs of table terms
    m = 2048
    rgb = _small(rng, m, 64.0)
    where = rng.choice(m, 96, replace=False)
    rgb[where[:32], rng.integers(0, 3, 32)] = rng.uniform(64.0, 2.0 ** 13, 32) * rng.choice([-1, 1], 32)
    rgb[where[32:64], rng.integers(0, 3, 32)] = rng.uniform(2.0 ** 13, A19, 32) * rng.choice([-1, 1], 32)
    rgb[where[64:], rng.integers(0, 3, 32)] = 2.0 ** 19 * rng.integers(1, 9, 32) * rng.choice([-1, 1], 32)
    rgb[where[0]] = [64.0, -64.0, A6]
    rgb[where[1]] = [2.0 ** 13, A13, -2.0 ** 19]
    lens = rng.integers(1, 40, 200)
    idx = _runs(lens, rng.integers(0, 50, 200))[:m]
    assert len(idx) == m
    has = rng.random(m) < 0.9
    P["terms-past-each-limit"] = (idx, rgb, has, 51, 2)
    # two windows per block, three blocks, the same keys in every window
    m = 6 * 4096
    lens = rng.integers(1, 48, 2000)
    idx = _runs(lens, rng.integers(0, 300, 2000))[:m]
    assert len(idx) == m
    P["windows-and-blocks"] = (idx, _small(rng, m, 64.0), rng.random(m) < 0.8, 301, 3)
    return P


LDS = _lds_patterns()


@pytest.mark.parametrize("name", list(LDS))
def test_add_wave_lds(acc, name):
    idx, rgb, has, n, grid = LDS[name]
    T = expect(acc.add("lds", idx, rgb, n, has, grid), idx, rgb, n, has)
    if name == "entry-near-2^62":
        assert T[0][0] == (1 << 62) - (1 << 12) and T[1][0] == -T[0][0] and T[2] == [0, 0, 0]


# ---------------------------------------------------------------- 5. the same regimes through the engines
def _emitter(emittance, fh, sign=1.0):
    """scenes.emitter's geometry: a lone light sphere, colour ±(1/4, 1/2, 1), in a black environment."""
    scene = Scene()
    colour = Colour(sign * 0.25, sign * 0.5, sign * 1.0)
    scene.Add(Sphere.NewSphere(Vector(0, 0, 0), 1, Material.LightMaterial(colour, emittance)))
    return scene, Camera.LookAt(Vector(0, 0, 4), Vector(0, 0, 0), Vector(0, 1, 0), 40), DefaultSampler.NewSampler(fh, 4)


@ENGINES
@pytest.mark.parametrize("fh", [1, 16])
@pytest.mark.parametrize("emittance,sign,spp", [(2.0 ** 15, 1, 1), (-2.0 ** 15, 1, 1), (2.0 ** 15, -1, 1), (2.0 ** 18, 1, 8),
                                                (2.0 ** 20, 1, 1)], ids=["2^15", "-2^15", "2^15-negative-colour", "2^18x8", "2^20"])
def test_emitter_large_terms(gpu, emittance, sign, spp, fh, engine):
    """A camera hit adds Color·Emittance·FH/⌊√FH⌋² = Color·Emittance (FH 1 and 16).  2^15: terms of 2^13, 2^14 and
    2^15 straddle kFixWave.  A negative emittance emits nothing (the reference tests Emittance > 0, Sampler.cs:73): the
    frame is black on both sides; the negative terms of the same sizes come from the negated colour at 2^15.  2^18 at
    8 spp: a covered pixel's totals are 2^63 (fix_value's boundary), 2^64 (a carry, low word 0) and 2^65.  2^20: one
    channel below kFixBig, two in the fp64 side sum, where every term of a pixel is the same power of two, so the
    sum is exact in any order.  Bit-exact against the oracle, and the analytic value."""
    s, c, smp = _emitter(emittance, fh, sign)
    g, gr, o, orr = render_both(s, c, smp, 48, 40, spp=spp, seed=5, engine=engine)
    check(g, gr, o, orr, exact=True)
    if emittance < 0:
        assert not g.M.any() and not o.M.any()
        return
    e = sign * emittance
    lit = g.M[g.N > 0].reshape(-1, 3)
    full = lit[np.abs(lit[:, 2]).argmax()]
    assert full.tolist() == [0.25 * e, 0.5 * e, e]
    assert (lit == [0.25 * e, 0.5 * e, e]).all(axis=1).sum() > 100       # the fully covered pixels, not one
    assert set(np.unique(lit * (spp / e))) <= set(np.arange(0, 4 * spp + 1) / 4.0)   # a pixel: j of spp samples hit


DIRECT_TERMS = 13    # see test_direct_light_large_terms


def _simplesphere(scale):
    """scenes.simplesphere with the light's emittance 8·scale, FirstHitSamples 4, MaxBounces 1."""
    scene = Scene()
    material = Material.DiffuseMaterial(Colour.White)
    scene.Add(Plane.NewPlane(Vector(0, 0, 0), Vector(0, 0, 1), material))
    scene.Add(Sphere.NewSphere(Vector(0, 0, 1), 1.0, material))
    scene.Add(Sphere.NewSphere(Vector(0, 0, 5.0), 1.0, Material.LightMaterial(Colour.White, 8 * scale)))
    camera = Camera.LookAt(Vector(3, 3, 3), Vector(0, 0, 0.5), Vector(0, 0, 1), 50)
    return scene, camera, DefaultSampler.NewSampler(4, 1)


_direct = {}


def _direct_case(w, h):
    """The scene scaled by the largest 2^k that keeps every pixel's pass sum below 2^19, and its oracle Buffer."""
    if (w, h) not in _direct:
        s, c, smp = _simplesphere(1.0)
        base, _ = O.render(O.OracleScene(s), c, smp, w, h, 1, seed=61)
        top = float(base.M.max())
        assert top > 0 and float(base.M.min()) >= 0
        k = math.ceil(19 - math.log2(top)) - 1
        while top * 2.0 ** k >= 2.0 ** 19:
            k -= 1
        s, c, smp = _simplesphere(2.0 ** k)
        o, orays = O.render(O.OracleScene(s), c, smp, w, h, 1, seed=61)
        _direct[(w, h)] = (k, o, orays)
    return _direct[(w, h)]


def _assert_direct_bounds(c, w, h, M):
    """1 spp, one pass: M is the pixel's pass sum.  No camera ray can see the light (so no term is an emission
    term): its nearest point is further from the view axis than the frame's corner."""
    to = Vector(0, 0, 5.0).Sub(c.p)
    d = to.Length()
    axis_angle = math.acos((to.X * c.w.X + to.Y * c.w.Y + to.Z * c.w.Z) / d) - math.asin(1.0 / d)
    corner = math.atan(math.hypot(1.0 + 2.0 / h, (w + 2.0) / h) / c.m)       # one pixel of margin for the jitter
    assert axis_angle > corner
    assert M.min() >= 0 and M.max() < 2.0 ** 19                                # no side-sum term: bit identity must hold
    assert M.max() >= DIRECT_TERMS * 2.0 ** 13                                 # so some term is >= 2^13
    assert ((M >= 64.0) & (M < 2.0 ** 13)).any()


def test_direct_light_large_terms(gpu, monkeypatch):
    """Direct-light terms of 2^13 and more through k_wf_nee_accum (its LDS table takes terms below 64 only, and
    fix_add_wave's runs terms below 2^13).

    Terms per pixel and pass, m = 13: one camera sample (1 spp); its vertex adds at most one emission term and, for
    each of its 4 children (FirstHitSamples 4, SpecularModeNaive: one mode per stratum), one light term
    (LightModeRandom, one light); each child's vertex (depth 1 = MaxBounces, samples = 1) adds at most one emission
    or environment term and one light term, and its own child is past MaxBounces: 1 + 4·(1 + 2).  All terms are
    non-negative (white surfaces, a positive light), so a pass sum of m·2^13 or more holds a term of 2^13 or more."""
    w, h = 48, 32
    k, o, orays = _direct_case(w, h)
    s, c, smp = _simplesphere(2.0 ** k)
    _assert_direct_bounds(c, w, h, o.M)
    monkeypatch.delenv("PT_LANES", raising=False)
    a, ra = render_gpu(s, c, smp, w, h, 1, seed=61, engine=_abi.ENGINE_WAVEFRONT)
    check(a, ra, o, orays)
    _assert_direct_bounds(c, w, h, a.M)
    b, rb = render_gpu(s, c, smp, w, h, 1, seed=61, engine=_abi.ENGINE_MEGAKERNEL)
    assert ra == rb
    same_buffer(a, b)
    monkeypatch.setenv("PT_LANES", "0")
    l, rl = render_gpu(s, c, smp, w, h, 1, seed=61, engine=_abi.ENGINE_WAVEFRONT)
    assert ra == rl
    same_buffer(a, l)


@ENGINES
def test_direct_light_large_terms_tile_split(gpu, engine):
    """A three-way tile split sums to the full frame bit for bit.  96x64 here: a 48x32 frame has two 32x32 tiles, and
    a rank without tiles renders the whole frame.  The scale is chosen for this frame, under the same two bounds."""
    w, h = 96, 64
    k, o, orays = _direct_case(w, h)
    s, c, smp = _simplesphere(2.0 ** k)
    _assert_direct_bounds(c, w, h, o.M)
    full, rays = render_gpu(s, c, smp, w, h, 1, seed=61, engine=engine)
    check(full, rays, o, orays)
    parts = [render_gpu(s, c, smp, w, h, 1, seed=61, tiles=tiles_for_rank(w, h, r, 3), engine=engine)[0] for r in range(3)]
    assert np.array_equal(sum(p.N for p in parts), full.N)
    assert np.array_equal(sum(p.M for p in parts), full.M)
    assert np.array_equal(sum(p.V for p in parts), full.V)
