"""Buffer.Image restated from PTSharpCore/Buffer.cs, pixel by pixel, as the yardstick of the image
tests (test_image_host.py, test_gpu_image.py).  It shares no code with ptsharp_amd: not
Buffer.Image, not pt_image.h.

  colour(M, V, N, channel) -> [H, W, 3] float64   the Colour Buffer.Image builds for each pixel
  image(M, V, N, channel)  -> [H, W, 3] uint8     its (byte)Math.Clamp(c * 255, 0, 255), NaN -> 0
  near_boundary(c)                                where a 1-ulp difference in c could change the byte

Scalar numpy float64 arithmetic throughout: IEEE division by zero and NaN propagate as they do in
C#, and `**` is the C library's pow.
"""
from __future__ import annotations

import functools

import numpy as np

COLOR, VARIANCE, STDDEV, SAMPLES, ALBEDO, NORMAL = range(6)   # Buffer.cs:8-16
CHANNELS = (COLOR, VARIANCE, STDDEV, SAMPLES, ALBEDO, NORMAL)
F = np.float64


def _variance(v, n):  # Pixel.Variance, Buffer.cs:48-55
    if n < 2:
        return [F(0), F(0), F(0)]
    return [F(v[k]) / F(int(n) - 1) for k in range(3)]


def _albedo(m):  # CalculateAlbedo, Buffer.cs:240-282
    r, g, b = F(m[0]), F(m[1]), F(m[2])
    if np.isnan(r) or np.isnan(g) or np.isnan(b):
        return [F(0), F(0), F(0)]
    mx = max(max(r, g), b)
    if mx == 0:
        return [F(0), F(0), F(0)]
    out = []
    for c in (r / mx, g / mx, b / mx):
        if c < 0:
            c = F(0)
        elif c > 1:
            c = F(1)
        out.append(c)   # Math.Clamp leaves a NaN (inf / inf) as it is
    return out


def _normal(M, x, y):  # GetNormalAt + CalculateNormal, Buffer.cs:99-124,222-233
    H, W = M.shape[:2]

    def px(xx, yy, k):  # GetPixelOrDefault: a new Pixel() outside the image
        return F(M[yy, xx, k]) if 0 <= xx < W and 0 <= yy < H else F(0)

    nx = (px(x - 1, y - 1, 0) + 2 * px(x - 1, y, 0) + px(x - 1, y + 1, 0)
          - px(x + 1, y - 1, 0) - 2 * px(x + 1, y, 0) - px(x + 1, y + 1, 0)) / F(8)
    ny = (px(x - 1, y - 1, 1) + 2 * px(x, y - 1, 1) + px(x + 1, y - 1, 1)
          - px(x - 1, y + 1, 1) - 2 * px(x, y + 1, 1) - px(x + 1, y + 1, 1)) / F(8)
    nz = F(1)
    length = np.sqrt(nx * nx + ny * ny + nz * nz)
    X, Y, Z = (np.float32(c / length) for c in (nx, ny, nz))   # new Vector(double, double, double): floats
    return [(F(X) + F(1)) * F(0.5), (F(Y) + F(1)) * F(0.5), F(Z)]


def colour(M, V, N, channel) -> np.ndarray:
    M, V, N = np.asarray(M, np.float64), np.asarray(V, np.float64), np.asarray(N, np.int32)
    H, W = N.shape
    out = np.zeros((H, W, 3), np.float64)
    max_samples = F(0)
    if channel == SAMPLES:  # Buffer.cs:138-146
        for n in N.ravel():
            max_samples = max(max_samples, F(n))
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                if channel == COLOR:
                    c = [F(M[y, x, k]) ** F(1.0 / 2.2) for k in range(3)]
                elif channel == VARIANCE:
                    c = _variance(V[y, x], N[y, x])
                elif channel == STDDEV:
                    c = [s ** F(np.float32(0.5)) for s in _variance(V[y, x], N[y, x])]
                elif channel == SAMPLES:
                    # the reference divides by maxSamples as it is; the project maps its 0/0 to 0
                    p = F(N[y, x]) / (max_samples if max_samples >= 1 else F(1))
                    c = [p, p, p]
                elif channel == ALBEDO:
                    c = _albedo(M[y, x])
                elif channel == NORMAL:
                    c = _normal(M, x, y)
                else:
                    raise ValueError(channel)
                out[y, x] = c
    return out


def to_bytes(c: np.ndarray) -> np.ndarray:
    out = np.zeros(c.shape, np.uint8)
    flat, o = c.ravel(), out.ravel()
    with np.errstate(all="ignore"):
        for i, ci in enumerate(flat):
            v = F(ci) * F(255)
            if np.isnan(v) or v <= 0:
                o[i] = 0
            elif v >= 255:
                o[i] = 255
            else:
                o[i] = int(v)   # (byte): toward zero
    return out


def image(M, V, N, channel) -> np.ndarray:
    return to_bytes(colour(M, V, N, channel))


def near_boundary(c) -> np.ndarray:
    """True where 0 < |c·255 − rint(c·255)| < 1e-9 and c·255 < 256: the values whose byte a 1-ulp
    difference in pow, sqrt or a division could change."""
    with np.errstate(all="ignore"):
        v = np.asarray(c, np.float64) * 255.0
        d = np.abs(v - np.rint(v))
        return (d > 0) & (d < 1e-9) & (v < 256)


# ------------------------------------------------------------------ shared inputs
def seeded(w: int, h: int, seed: int = 2024):
    """M = random·1.5, V = random·3, N = integers(0, 6), drawn in that order."""
    rng = np.random.default_rng(seed)
    M = rng.random((h, w, 3)) * 1.5
    V = rng.random((h, w, 3)) * 3
    N = rng.integers(0, 6, (h, w)).astype(np.int32)
    return M, V, N


def special_rows(w: int, rows: int = 2):
    """`rows` rows of w pixels whose M components run through 0, -0.0, 1, 2, 1e300, +inf, -1, NaN in
    every pairing, with one pixel holding a single NaN, one all-equal pixel, one all-zero pixel and
    one (inf, inf, 1); V runs through the same values and -0.25; N through 0, 1, 2, -1."""
    vals = np.array([0.0, -0.0, 1.0, 2.0, 1e300, np.inf, -1.0, np.nan])
    n = w * rows
    i = np.arange(n)
    M = np.stack([vals[i % 8], vals[(i // 8 + i) % 8], vals[(i // 3) % 8]], axis=1)
    vv = np.append(vals, -0.25)
    V = np.stack([vv[(i + 2) % 9], vv[(i // 2) % 9], vv[(2 * i + 1) % 9]], axis=1)
    N = np.array([0, 1, 2, -1, 2, 3], np.int32)[i % 6]
    fixed = [((0.5, np.nan, 0.25), (1.0, -0.25, 4.0), 2), ((0.75, 0.75, 0.75), (0.5, 0.5, 0.5), 2),
             ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0), ((np.inf, np.inf, 1.0), (np.inf, 2.0, 1e300), 3),
             ((-1.0, -2.0, -0.5), (3.0, -0.0, 1.0), 2), ((0.25, 2.0, 1.0), (1.0, 1.0, 1.0), 1)]
    for j, (m, v, cnt) in enumerate(fixed):
        at = (5 + 4 * j) % n
        M[at], V[at], N[at] = m, v, cnt
    return M.reshape(rows, w, 3), V.reshape(rows, w, 3), N.reshape(rows, w)


@functools.lru_cache(maxsize=None)
def seeded_101x70():
    """The seeded 101x70 buffer and its six reference colours and images (computed once, read-only)."""
    M, V, N = seeded(101, 70)
    cols = {ch: colour(M, V, N, ch) for ch in CHANNELS}
    imgs = {ch: to_bytes(cols[ch]) for ch in CHANNELS}
    for a in (M, V, N, *cols.values(), *imgs.values()):
        a.setflags(write=False)
    return M, V, N, cols, imgs


@functools.lru_cache(maxsize=None)
def seeded_with_specials():
    """The seeded 101x70 buffer with special_rows(101) appended: 101x72."""
    M, V, N = seeded(101, 70)
    sm, sv, sn = special_rows(101)
    M, V, N = np.concatenate([M, sm]), np.concatenate([V, sv]), np.concatenate([N, sn])
    cols = {ch: colour(M, V, N, ch) for ch in CHANNELS}
    imgs = {ch: to_bytes(cols[ch]) for ch in CHANNELS}
    for a in (M, V, N, *cols.values(), *imgs.values()):
        a.setflags(write=False)
    return M, V, N, cols, imgs
