"""The variance-guided à-trous denoiser (pt_denoise) restated in numpy from its specification, as the
yardstick of the denoise tests (test_denoise_host.py, test_gpu_denoise.py).  It shares no code with
ptsharp_amd: not pt_denoise.h, not the kernels.  Whole-image arrays, one shifted view per tap, the
taps visited row-major (dy outer, dx inner, −r to +r), so every sum is taken in the order the
specification fixes and the result differs from a correct implementation only in the last bit of
exp and of a division.

  denoise(M, V, N, iterations=5, sigma_colour=4.0) -> (colour [H,W,3], variance [H,W,3]) float64
  valid(M, V, N)                                    -> [H,W] bool
  atrous_blur(c, valid, iterations)                 -> the plain renormalised B3-spline à-trous blur
  rmse_ratio / tonemapped_rmse                      -> the quality measure of the render tests

A pixel is valid when N >= 1 and all of M and V are finite; an invalid pixel is never a tap and
passes through as a centre (colour M as it stands, variance 0).
"""
from __future__ import annotations

import functools

import numpy as np

B3 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0


def valid(M, V, N) -> np.ndarray:
    return (np.asarray(N) >= 1) & np.isfinite(M).all(axis=2) & np.isfinite(V).all(axis=2)


def _shift(a, dy, dx, fill=0):
    """b[y, x] = a[y + dy, x + dx] inside the image, `fill` outside."""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    y0, y1 = max(0, -dy), min(H, H - dy)
    x0, x1 = max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def prepare(M, V, N):
    """(c, s2, ok): steps 1-4 of Prepare."""
    M, V, N = np.asarray(M, np.float64), np.asarray(V, np.float64), np.asarray(N, np.int32)
    ok = valid(M, V, N)
    H, W = N.shape
    n = N.astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        temporal = V / ((n - 1.0) * n)
        # the spatial estimate: two passes over the valid 5x5 neighbourhood
        total = np.zeros((H, W, 3))
        count = np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                okq = _shift(ok, dy, dx, False)
                total = total + np.where(okq[..., None], _shift(M, dy, dx), 0.0)
                count = count + okq
        mean = total / count[..., None]
        ss = np.zeros((H, W, 3))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                okq = _shift(ok, dy, dx, False)
                e = _shift(M, dy, dx) - mean
                ss = ss + np.where(okq[..., None], e * e, 0.0)
        spatial = np.where(count[..., None] >= 2, ss / (count[..., None] - 1.0), 0.0)
        s2 = np.where(N[..., None] >= 2, temporal, spatial)
        s2 = np.where(ok[..., None], s2, 0.0)
        # one 3x3 binomial blur over the valid taps, renormalised
        k = np.array([1.0, 2.0, 1.0])
        acc = np.zeros((H, W, 3))
        wsum = np.zeros((H, W))
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                okq = _shift(ok, dy, dx, False)
                wt = k[dy + 1] * k[dx + 1]
                acc = acc + np.where(okq[..., None], wt * _shift(s2, dy, dx), 0.0)
                wsum = wsum + np.where(okq, wt, 0.0)
        blurred = np.where(ok[..., None], acc / wsum[..., None], 0.0)
    return M.copy(), blurred, ok


def level(c, s2, ok, step, sigma_colour):
    H, W = ok.shape
    sigma2 = np.float64(sigma_colour) * np.float64(sigma_colour)
    with np.errstate(all="ignore"):
        den = sigma2 * s2 + 1e-12
        wsum = np.zeros((H, W))
        csum = np.zeros((H, W, 3))
        ssum = np.zeros((H, W, 3))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                okq = _shift(ok, dy * step, dx * step, False)
                if not okq.any():
                    continue
                cq = _shift(c, dy * step, dx * step)
                sq = _shift(s2, dy * step, dx * step)
                e = cq - c
                t = (e * e) / den
                d = (0.0 + t[..., 0]) + t[..., 1] + t[..., 2]
                wt = np.where(okq, (B3[dy + 2] * B3[dx + 2]) * np.exp(-d), 0.0)
                wsum = wsum + wt
                csum = csum + np.where(okq[..., None], wt[..., None] * cq, 0.0)
                ssum = ssum + np.where(okq[..., None], (wt * wt)[..., None] * sq, 0.0)
        c_out = np.where(ok[..., None], csum / wsum[..., None], c)
        s_out = np.where(ok[..., None], ssum / (wsum * wsum)[..., None], s2)
    return c_out, s_out


def denoise(M, V, N, iterations: int = 5, sigma_colour: float = 4.0):
    c, s2, ok = prepare(M, V, N)
    for j in range(iterations):
        c, s2 = level(c, s2, ok, 1 << j, sigma_colour)
    return c, s2


def atrous_blur(c, ok, iterations: int):
    """The renormalised B3-spline à-trous blur of the valid pixels: what the filter is when every
    colour weight is 1.  Separately written: an explicit convolution, pixel by pixel."""
    c = np.asarray(c, np.float64).copy()
    H, W = ok.shape
    for j in range(iterations):
        s = 1 << j
        out = c.copy()
        for y in range(H):
            for x in range(W):
                if not ok[y, x]:
                    continue
                acc, ws = np.zeros(3), 0.0
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        qy, qx = y + dy * s, x + dx * s
                        if 0 <= qy < H and 0 <= qx < W and ok[qy, qx]:
                            wt = B3[dy + 2] * B3[dx + 2]
                            acc = acc + wt * c[qy, qx]
                            ws = ws + wt
                out[y, x] = acc / ws
        c = out
    return c


# ------------------------------------------------------------------ quality measure
def tonemapped_rmse(c, truth) -> float:
    """RMSE of clip(c, 0, 1)^(1/2.2) against the same of `truth`."""
    a = np.clip(np.asarray(c, np.float64), 0.0, 1.0) ** (1.0 / 2.2)
    b = np.clip(np.asarray(truth, np.float64), 0.0, 1.0) ** (1.0 / 2.2)
    return float(np.sqrt(np.mean((a - b) ** 2)))


def rmse_ratio(denoised, noisy, truth) -> float:
    return tonemapped_rmse(denoised, truth) / tonemapped_rmse(noisy, truth)


# ------------------------------------------------------------------ shared inputs
def seeded(w: int, h: int, seed: int | None = None):
    """A noisy two-region picture with its Welford state: M a smooth ramp with a vertical edge plus
    noise, N in 2..5 with about a fifth of the pixels at N = 1, V = the noise variance scaled as
    (N−1)·N·s2 would be (zero where N = 1, as AddSample leaves it)."""
    rng = np.random.default_rng(7000 + 1000 * w + h if seed is None else seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([0.2 + 0.5 * xx / max(w - 1, 1), 0.6 - 0.3 * yy / max(h - 1, 1),
                     np.where(xx * 2 >= w, 0.9, 0.15) + 0.0 * yy], axis=2)
    sd = 0.02 + 0.1 * rng.random((h, w, 3))
    N = rng.integers(2, 6, (h, w)).astype(np.int32)
    N[rng.random((h, w)) < 0.2] = 1
    n = N.astype(np.float64)[..., None]
    M = base + sd * rng.standard_normal((h, w, 3)) / np.sqrt(n)
    V = sd * sd * (n - 1.0) * (0.5 + rng.random((h, w, 3)))
    return M, V, N


@functools.lru_cache(maxsize=None)
def seeded_with_specials():
    """seeded(101, 70) with every special pixel (read-only): NaN and +inf in M, inf in V, N = 0 holes
    and a whole missing 32x32 tile, N = 1 among N >= 2, exact-zero variance beside noisy pixels, and
    one firefly of 1e6."""
    M, V, N = seeded(101, 70, seed=4242)
    M[3, 5, 1] = np.nan
    M[3, 6] = np.nan
    M[10, 50, 0] = np.inf
    M[69, 100, 2] = np.inf
    V[20, 20, 2] = np.inf
    V[0, 0, 0] = np.inf
    for y, x in [(5, 5), (5, 6), (6, 5), (40, 99), (69, 0), (0, 100)]:
        N[y, x] = 0
    N[32:64, 64:96] = 0               # tile (2, 1) of the 32x32 grid never rendered
    M[32:64, 64:96] = 0.0
    V[32:64, 64:96] = 0.0
    N[12:15, 30:33] = 1               # a clump of single-pass pixels
    V[12:15, 30:33] = 0.0
    V[50:54, 10:14] = 0.0             # exact-zero variance with N >= 2, beside noisy pixels
    N[50:54, 10:14] = 3
    M[50:54, 10:14] = [0.25, 0.5, 0.75]
    M[25, 70] = [1e6, 1e6, 1e6]       # a firefly; its variance of the mean is 1 (see firefly_with_its_variance)
    N[25, 70] = 4
    V[25, 70] = [12.0, 12.0, 12.0]
    near = np.zeros(N.shape, bool)    # no single-pass pixel within its 5x5: their spatial estimate would be 4e10
    near[23:28, 68:73] = True
    V[near & (N == 1)] = 2e-3
    N[near & (N == 1)] = 2
    for a in (M, V, N):
        a.setflags(write=False)
    return M, V, N


@functools.lru_cache(maxsize=None)
def firefly_with_its_variance():
    """seeded(37, 19) with a firefly of 1e6 that carries the Welford variance one 4e6 sample among four
    leaves (V = 1.2e13, s2 = 1e12).  For ONE level only: its s2 reaches far pixels through weights
    w² with d of 10 to 20, where a last-bit difference in exp or in c is multiplied by d, and every
    further level multiplies it again.  Measured on the restatement itself with exp perturbed by
    ±1 ulp, such a pixel in seeded_with_specials() moved the propagated variance by up to 2.5e-11
    after 5 levels: a property of the filter on that input, which no implementation can avoid, so
    the multi-level comparisons use a firefly whose own variance is moderate, with no single-pass
    pixel beside it (its 5x5 estimate would be as large), and this input checks the 1e12 dynamic range where the arithmetic is still comparable bit for bit."""
    M, V, N = seeded(37, 19, seed=99)
    M[9, 20] = [1e6, 1e6, 1e6]
    N[9, 20] = 4
    V[9, 20] = [1.2e13, 1.2e13, 1.2e13]
    for a in (M, V, N):
        a.setflags(write=False)
    return M, V, N


@functools.lru_cache(maxsize=None)
def reference(w: int, h: int, iterations: int, special: bool = False):
    """denoise() of seeded(w, h) (or of seeded_with_specials()), computed once and read-only."""
    M, V, N = seeded_with_specials() if special else seeded(w, h)
    c, s2 = denoise(M, V, N, iterations)
    c.setflags(write=False)
    s2.setflags(write=False)
    return c, s2
