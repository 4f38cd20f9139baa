// pt_denoise.h — the variance-guided à-trous denoiser per pixel (pt_denoise).
//
// One text for the device (pt_denoise.hip) and for a host check program
// (tests/native/denoise_check.cpp): every function is `__host__ __device__ inline`, and the two
// qualifiers are defined away when the compiler is not hipcc.  All storage and arithmetic are fp64,
// without contraction; exp and the divisions are the only operations whose last bit may depend on
// the maths library.  Every stencil sums row-major over its taps: dy outer, dx inner, −r to +r.
//
// A pixel is valid when N >= 1 and all of M and V are finite.  An invalid pixel is never a tap; as a
// centre it passes through (colour = M as it stands, variance 0).
//
//   prepare   c = M;  s2 = V / ((N−1)·N) for N >= 2, else the unbiased sample variance of M over
//             the valid pixels of the in-image 5x5 neighbourhood (two-pass; 0 with fewer than 2)
//   blur      s2 <- its 3x3 binomial blur over the valid in-image taps, renormalised (once)
//   level j   the edge-avoiding 5x5 B3-spline tap set at step 2^j (Dammertz et al. 2010), colour
//             distance scaled by the centre's own variance (as in SVGF):
//               d(q) = Σ_k (c_q,k − c_p,k)² / (sigma² · s2_p,k + 1e-12),  w(q) = h(dx,dy) · exp(−d(q))
//               c'_p = Σ w·c_q / Σ w,   s2'_p = Σ w²·s2_q / (Σ w)²
//
// The feature-guided level (pt_denoise_guided) is the same level with a guide record per pixel
// (DenoiseGuideRec: first-hit normal, depth, albedo and a hit flag, fp32, widened to fp64 here).  A tap
// whose hit flag differs from the centre's is skipped like an invalid one; for the others
//   d(q) = d_colour(q)                                          (the sum above, as it stands)
//        + (Σ_k (a_q,k − a_p,k)²) / sigma_albedo²               if sigma_albedo > 0
//        + (Σ_k (n_q,k − n_p,k)²) / sigma_normal²               if the centre is a hit and sigma_normal > 0
//        + (z_q − z_p)² / ((sigma_depth · z_p) · (sigma_depth · z_p))   if the centre is a hit and sigma_depth > 0
// added in that order, each Σ_k from 0.0 in the order k = 0, 1, 2, and one exp per tap as before.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

#pragma clang fp contract(off)

namespace pt {

__host__ __device__ inline bool denoise_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for NaN

__host__ __device__ inline bool denoise_valid(const double* m3, const double* v3, int32_t n) {
    if (n < 1) return false;
    for (int k = 0; k < 3; k++)
        if (!denoise_finite(m3[k]) || !denoise_finite(v3[k])) return false;
    return true;
}

// Pixel offsets are formed in 64 bits (an int product overflows past 2^31 / 3 pixels).
__host__ __device__ inline size_t denoise_index(int32_t w, int32_t x, int32_t y) { return (size_t)y * (size_t)w + (size_t)x; }

// Prepare, steps 1-3, for pixel (x, y) of the Buffer {m, v, n}: its validity, c and the unblurred s2.
__host__ __device__ inline bool denoise_prepare_at(const double* m, const double* v, const int32_t* n, int32_t w, int32_t h,
                                                   int32_t x, int32_t y, double c[3], double s2[3]) {
    const size_t p = denoise_index(w, x, y);
    for (int k = 0; k < 3; k++) {
        c[k] = m[3 * p + k];
        s2[k] = 0.0;
    }
    const int32_t np = n[p];
    if (!denoise_valid(m + 3 * p, v + 3 * p, np)) return false;
    if (np >= 2) {
        const double div = (double)(np - 1) * (double)np;
        for (int k = 0; k < 3; k++) s2[k] = v[3 * p + k] / div;
        return true;
    }
    // N = 1: no temporal variance yet; the spatial one of the 5x5 neighbourhood stands in
    double sum[3] = {0.0, 0.0, 0.0};
    int32_t count = 0;
    for (int dy = -2; dy <= 2; dy++)
        for (int dx = -2; dx <= 2; dx++) {
            const int32_t qx = x + dx, qy = y + dy;
            if (qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
            const size_t q = denoise_index(w, qx, qy);
            if (!denoise_valid(m + 3 * q, v + 3 * q, n[q])) continue;
            for (int k = 0; k < 3; k++) sum[k] = sum[k] + m[3 * q + k];
            count++;
        }
    if (count < 2) return true;
    double mean[3], ss[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 3; k++) mean[k] = sum[k] / (double)count;
    for (int dy = -2; dy <= 2; dy++)
        for (int dx = -2; dx <= 2; dx++) {
            const int32_t qx = x + dx, qy = y + dy;
            if (qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
            const size_t q = denoise_index(w, qx, qy);
            if (!denoise_valid(m + 3 * q, v + 3 * q, n[q])) continue;
            for (int k = 0; k < 3; k++) {
                const double e = m[3 * q + k] - mean[k];
                ss[k] = ss[k] + e * e;
            }
        }
    for (int k = 0; k < 3; k++) s2[k] = ss[k] / (double)(count - 1);
    return true;
}

// Prepare, step 4: the (1,2,1)x(1,2,1) blur of s2 at a valid (x, y) over the valid in-image taps,
// divided by the weights used.  An invalid centre keeps its 0.
__host__ __device__ inline void denoise_blur_at(const double* s2, const uint8_t* valid, int32_t w, int32_t h, int32_t x,
                                                int32_t y, double out[3]) {
    out[0] = out[1] = out[2] = 0.0;
    if (!valid[denoise_index(w, x, y)]) return;
    double sum[3] = {0.0, 0.0, 0.0}, wsum = 0.0;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int32_t qx = x + dx, qy = y + dy;
            if (qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
            const size_t q = denoise_index(w, qx, qy);
            if (!valid[q]) continue;
            const double wt = (double)((2 - (dx < 0 ? -dx : dx)) * (2 - (dy < 0 ? -dy : dy)));
            for (int k = 0; k < 3; k++) sum[k] = sum[k] + wt * s2[3 * q + k];
            wsum = wsum + wt;
        }
    for (int k = 0; k < 3; k++) out[k] = sum[k] / wsum;
}

// One tap of a level: its weight from the centre's colour and the centre's three denominators, and
// its terms added to the running sums.  `hq` is h(dx, dy).
__host__ __device__ inline void denoise_tap(double hq, const double cq[3], const double sq[3], const double cp[3],
                                            const double den[3], double& wsum, double csum[3], double ssum[3]) {
    double d = 0.0;
    for (int k = 0; k < 3; k++) {
        const double e = cq[k] - cp[k];
        d = d + (e * e) / den[k];
    }
    const double wt = hq * exp(-d);
    wsum = wsum + wt;
    const double w2 = wt * wt;
    for (int k = 0; k < 3; k++) {
        csum[k] = csum[k] + wt * cq[k];
        ssum[k] = ssum[k] + w2 * sq[k];
    }
}

// (1,4,6,4,1)/16 ⊗ (1,4,6,4,1)/16: exact in binary
__host__ __device__ inline double denoise_h(int dx, int dy) {
    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    const int kx = ax == 0 ? 6 : (ax == 1 ? 4 : 1), ky = ay == 0 ? 6 : (ay == 1 ? 4 : 1);
    return (double)(kx * ky) / 256.0;
}

__host__ __device__ inline void denoise_denominators(const double sp[3], double sigma2, double den[3]) {
    for (int k = 0; k < 3; k++) den[k] = sigma2 * sp[k] + 1e-12;
}

__host__ __device__ inline void denoise_finish(double wsum, const double csum[3], const double ssum[3], double c_out[3],
                                               double s2_out[3]) {
    const double w2 = wsum * wsum;
    for (int k = 0; k < 3; k++) {
        c_out[k] = csum[k] / wsum;
        s2_out[k] = ssum[k] / w2;
    }
}

// Level with step `step` at pixel (x, y), from whole arrays; sigma2 = sigma_colour · sigma_colour.
__host__ __device__ inline void denoise_level_at(const double* c, const double* s2, const uint8_t* valid, int32_t w, int32_t h,
                                                 int32_t x, int32_t y, int32_t step, double sigma2, double c_out[3],
                                                 double s2_out[3]) {
    const size_t p = denoise_index(w, x, y);
    double cp[3], sp[3];
    for (int k = 0; k < 3; k++) {
        cp[k] = c[3 * p + k];
        sp[k] = s2[3 * p + k];
    }
    if (!valid[p]) {
        for (int k = 0; k < 3; k++) {
            c_out[k] = cp[k];
            s2_out[k] = sp[k];   // 0 since prepare
        }
        return;
    }
    double den[3], wsum = 0.0, csum[3] = {0.0, 0.0, 0.0}, ssum[3] = {0.0, 0.0, 0.0};
    denoise_denominators(sp, sigma2, den);
    for (int dy = -2; dy <= 2; dy++) {
        const int64_t qy = (int64_t)y + (int64_t)dy * (int64_t)step;
        if (qy < 0 || qy >= (int64_t)h) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int64_t qx = (int64_t)x + (int64_t)dx * (int64_t)step;
            if (qx < 0 || qx >= (int64_t)w) continue;
            const size_t q = denoise_index(w, (int32_t)qx, (int32_t)qy);
            if (!valid[q]) continue;
            const double cq[3] = {c[3 * q], c[3 * q + 1], c[3 * q + 2]};
            const double sq[3] = {s2[3 * q], s2[3 * q + 1], s2[3 * q + 2]};
            denoise_tap(denoise_h(dx, dy), cq, sq, cp, den, wsum, csum, ssum);
        }
    }
    denoise_finish(wsum, csum, ssum, c_out, s2_out);
}

// ------------------------------------------------------------------ the feature-guided level
// The guide record of a pixel: two 16-byte halves, so a tap is two 16-byte loads and 64 consecutive
// pixels are 2048 contiguous bytes.  A miss has n = 0, depth = 1e9 (Hit.INF), the environment's
// colour as its albedo, and hit = 0.
struct alignas(16) DenoiseGuideRec {
    float n[3];
    float depth;
    float a[3];
    float hit;   // 1.f or 0.f
};

// Per-call constants of the guide terms: sigma_albedo², sigma_normal² and sigma_depth; 0 = term off.
struct DenoiseGuideSigmas {
    double albedo2, normal2, depth;
};

// The guide terms of tap q for centre p, added to the colour distance d in the order of the head
// comment.  den_depth = (sigma_depth · z_p)², formed once per centre (denoise_guide_depth_den).
__host__ __device__ inline double denoise_guide_distance(double d, const DenoiseGuideRec& gq, const DenoiseGuideRec& gp,
                                                         const DenoiseGuideSigmas& sg, double den_depth) {
    if (sg.albedo2 > 0.0) {
        double s = 0.0;
        for (int k = 0; k < 3; k++) {
            const double e = (double)gq.a[k] - (double)gp.a[k];
            s = s + e * e;
        }
        d = d + s / sg.albedo2;
    }
    if (gp.hit != 0.f) {
        if (sg.normal2 > 0.0) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) {
                const double e = (double)gq.n[k] - (double)gp.n[k];
                s = s + e * e;
            }
            d = d + s / sg.normal2;
        }
        if (sg.depth > 0.0) {
            const double e = (double)gq.depth - (double)gp.depth;
            d = d + (e * e) / den_depth;
        }
    }
    return d;
}

__host__ __device__ inline double denoise_guide_depth_den(const DenoiseGuideRec& gp, const DenoiseGuideSigmas& sg) {
    const double sd = sg.depth * (double)gp.depth;
    return sd * sd;
}

// denoise_tap with the guide terms added to d before the one exp.
__host__ __device__ inline void denoise_tap_guided(double hq, const double cq[3], const double sq[3], const double cp[3],
                                                   const double den[3], const DenoiseGuideRec& gq, const DenoiseGuideRec& gp,
                                                   const DenoiseGuideSigmas& sg, double den_depth, double& wsum, double csum[3],
                                                   double ssum[3]) {
    double d = 0.0;
    for (int k = 0; k < 3; k++) {
        const double e = cq[k] - cp[k];
        d = d + (e * e) / den[k];
    }
    d = denoise_guide_distance(d, gq, gp, sg, den_depth);
    const double wt = hq * exp(-d);
    wsum = wsum + wt;
    const double w2 = wt * wt;
    for (int k = 0; k < 3; k++) {
        csum[k] = csum[k] + wt * cq[k];
        ssum[k] = ssum[k] + w2 * sq[k];
    }
}

// denoise_level_at with the guide records `g` ([P], row-major like c).
__host__ __device__ inline void denoise_level_guided_at(const double* c, const double* s2, const uint8_t* valid,
                                                        const DenoiseGuideRec* g, int32_t w, int32_t h, int32_t x, int32_t y,
                                                        int32_t step, double sigma2, const DenoiseGuideSigmas& sg,
                                                        double c_out[3], double s2_out[3]) {
    const size_t p = denoise_index(w, x, y);
    double cp[3], sp[3];
    for (int k = 0; k < 3; k++) {
        cp[k] = c[3 * p + k];
        sp[k] = s2[3 * p + k];
    }
    if (!valid[p]) {
        for (int k = 0; k < 3; k++) {
            c_out[k] = cp[k];
            s2_out[k] = sp[k];   // 0 since prepare
        }
        return;
    }
    const DenoiseGuideRec gp = g[p];
    const double den_depth = denoise_guide_depth_den(gp, sg);
    double den[3], wsum = 0.0, csum[3] = {0.0, 0.0, 0.0}, ssum[3] = {0.0, 0.0, 0.0};
    denoise_denominators(sp, sigma2, den);
    for (int dy = -2; dy <= 2; dy++) {
        const int64_t qy = (int64_t)y + (int64_t)dy * (int64_t)step;
        if (qy < 0 || qy >= (int64_t)h) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int64_t qx = (int64_t)x + (int64_t)dx * (int64_t)step;
            if (qx < 0 || qx >= (int64_t)w) continue;
            const size_t q = denoise_index(w, (int32_t)qx, (int32_t)qy);
            if (!valid[q]) continue;
            const DenoiseGuideRec gq = g[q];
            if ((gq.hit != 0.f) != (gp.hit != 0.f)) continue;
            const double cq[3] = {c[3 * q], c[3 * q + 1], c[3 * q + 2]};
            const double sq[3] = {s2[3 * q], s2[3 * q + 1], s2[3 * q + 2]};
            denoise_tap_guided(denoise_h(dx, dy), cq, sq, cp, den, gq, gp, sg, den_depth, wsum, csum, ssum);
        }
    }
    denoise_finish(wsum, csum, ssum, c_out, s2_out);
}

}  // namespace pt
