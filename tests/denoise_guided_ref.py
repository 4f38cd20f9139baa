"""The feature-guided à-trous denoiser (pt_denoise_guided) restated in numpy from its specification,
as the yardstick of test_features_host.py and test_gpu_features.py.  It shares no code with
ptsharp_amd; prepare, the validity rule and the seeded Buffers are denoise_ref's (the guided filter
changes only the tap weight).

  denoise_guided(M, V, N, albedo, normal, depth, kind, iterations, sigma_colour, sigma_normal,
                 sigma_albedo, sigma_depth) -> (colour [H,W,3], variance [H,W,3]) float64
  seeded_features(w, h)                     -> (albedo f64, normal f32, depth f64, kind i32)

The guide is the fp32 record the device keeps (normal, (float)depth, (float)albedo, hit = kind >= 0),
widened back to fp64.  A tap whose hit flag differs from the centre's is skipped like an invalid tap;
for the others w(q) = h(dx,dy) · exp(−d), d being, added in this order,
    d_colour                                         (denoise_ref.level's term)
  + (Σ_k (a_q,k − a_p,k)²) / sigma_albedo²           if sigma_albedo > 0
  + (Σ_k (n_q,k − n_p,k)²) / sigma_normal²           if the centre is a hit and sigma_normal > 0
  + (z_q − z_p)² / ((sigma_depth·z_p)·(sigma_depth·z_p))   if the centre is a hit and sigma_depth > 0
each Σ_k summed from 0.0 over k = 0, 1, 2.
"""
from __future__ import annotations

import functools

import numpy as np

import denoise_ref as D

DEFAULTS = dict(iterations=5, sigma_colour=4.0, sigma_normal=0.3, sigma_albedo=0.3, sigma_depth=0.1)


def guide_of(albedo, normal, depth, kind):
    """(a, n, z, hit): the fp32 guide record's values as float64 arrays, and the hit flag."""
    a = np.asarray(albedo, np.float64).astype(np.float32).astype(np.float64)
    n = np.asarray(normal, np.float32).astype(np.float64)
    z = np.asarray(depth, np.float64).astype(np.float32).astype(np.float64)
    return a, n, z, np.asarray(kind) >= 0


def _sq3(e):
    return ((0.0 + e[..., 0] * e[..., 0]) + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def level_guided(c, s2, ok, guide, step, sigma_colour, sigma_normal, sigma_albedo, sigma_depth):
    a, n, z, hit = guide
    H, W = ok.shape
    sigma2 = np.float64(sigma_colour) * np.float64(sigma_colour)
    sa2 = np.float64(sigma_albedo) * np.float64(sigma_albedo)
    sn2 = np.float64(sigma_normal) * np.float64(sigma_normal)
    sd = np.float64(sigma_depth) * z
    den_depth = sd * sd
    with np.errstate(all="ignore"):
        den = sigma2 * s2 + 1e-12
        wsum = np.zeros((H, W))
        csum = np.zeros((H, W, 3))
        ssum = np.zeros((H, W, 3))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                okq = D._shift(ok, dy * step, dx * step, False)
                if not okq.any():
                    continue
                sh = lambda x, fill=0: D._shift(x, dy * step, dx * step, fill)   # noqa: E731
                okq = okq & (sh(hit, False) == hit)
                cq, sq = sh(c), sh(s2)
                e = cq - c
                t = (e * e) / den
                d = (0.0 + t[..., 0]) + t[..., 1] + t[..., 2]
                if sigma_albedo > 0:
                    d = d + _sq3(sh(a) - a) / sa2
                if sigma_normal > 0:
                    d = np.where(hit, d + _sq3(sh(n) - n) / sn2, d)
                if sigma_depth > 0:
                    ez = sh(z) - z
                    d = np.where(hit, d + (ez * ez) / den_depth, d)
                wt = np.where(okq, (D.B3[dy + 2] * D.B3[dx + 2]) * np.exp(-d), 0.0)
                wsum = wsum + wt
                csum = csum + np.where(okq[..., None], wt[..., None] * cq, 0.0)
                ssum = ssum + np.where(okq[..., None], (wt * wt)[..., None] * sq, 0.0)
        c_out = np.where(ok[..., None], csum / wsum[..., None], c)
        s_out = np.where(ok[..., None], ssum / (wsum * wsum)[..., None], s2)
    return c_out, s_out


def denoise_guided(M, V, N, albedo, normal, depth, kind, iterations=5, sigma_colour=4.0, sigma_normal=0.3,
                   sigma_albedo=0.3, sigma_depth=0.1):
    c, s2, ok = D.prepare(M, V, N)
    guide = guide_of(albedo, normal, depth, kind)
    for j in range(iterations):
        c, s2 = level_guided(c, s2, ok, guide, 1 << j, sigma_colour, sigma_normal, sigma_albedo, sigma_depth)
    return c, s2


# ------------------------------------------------------------------ shared inputs
def seeded_features(w: int, h: int, seed: int | None = None):
    """Piecewise-smooth features of a w x h frame: three hit regions split by two slanted lines, each
    with its own slowly varying unit normal, albedo and depth ramp, and a miss region in the top right
    corner (kind −1, depth 1e9, normal 0, a smooth 'sky' albedo).  The contrasts are moderate: with the
    default sigmas a tap across a region border has a guide distance of a few units, never in the
    hundreds, so a weight is never so small that a last-bit difference upstream is multiplied into
    the 1e-11 bar, and the hit / miss border is exact by the flag."""
    rng = np.random.default_rng(9000 + 1000 * w + h if seed is None else seed)
    yy, xx = np.mgrid[0:h, 0:w]
    u, v = xx / max(w - 1, 1), yy / max(h - 1, 1)
    region = (u + 0.3 * v > 0.45).astype(np.int32) + (v - 0.2 * u > 0.6).astype(np.int32)   # 0, 1, 2
    miss = (u > 0.7) & (v < 0.3)
    base_n = np.array([[0.0, 0.0, 1.0], [0.25, 0.0, 0.97], [0.0, 0.3, 0.95]])
    nrm = base_n[region] + 0.05 * np.stack([u, v, 0.0 * u], axis=2) + 0.004 * rng.standard_normal((h, w, 3))
    nrm = nrm / np.linalg.norm(nrm, axis=2, keepdims=True)
    base_a = np.array([[0.60, 0.55, 0.50], [0.50, 0.62, 0.45], [0.55, 0.48, 0.62]])
    alb = base_a[region] + 0.05 * np.stack([u, v, u * v], axis=2) + 0.003 * rng.standard_normal((h, w, 3))
    base_z = np.array([4.0, 4.6, 5.1])
    z = base_z[region] + 0.5 * u + 0.3 * v + 0.002 * rng.standard_normal((h, w))
    kind = (region % 3).astype(np.int32)
    sky = np.stack([0.3 + 0.1 * u, 0.4 + 0.1 * v, 0.7 + 0.0 * u], axis=2)
    alb = np.where(miss[..., None], sky, alb)
    nrm = np.where(miss[..., None], 0.0, nrm)
    z = np.where(miss, 1e9, z)
    kind = np.where(miss, -1, kind).astype(np.int32)
    return alb.astype(np.float64), nrm.astype(np.float32), z.astype(np.float64), kind


@functools.lru_cache(maxsize=None)
def reference(w: int, h: int, iterations: int, special: bool = False):
    """denoise_guided() of denoise_ref.seeded(w, h) (or seeded_with_specials()) with seeded_features(w, h)
    and the default sigmas, computed once and read-only."""
    M, V, N = D.seeded_with_specials() if special else D.seeded(w, h)
    c, s2 = denoise_guided(M, V, N, *seeded_features(w, h), iterations=iterations)
    c.setflags(write=False)
    s2.setflags(write=False)
    return c, s2
