// pt_image.h — Buffer.Image per pixel (Buffer.cs:134-282): a Buffer channel as 8-bit colour.
//
// One text for the device (pt_image.hip, k_image_resolve) and for a host check program
// (tests/native/image_check.cpp): every function is `__host__ __device__ inline`, and the two
// qualifiers are defined away when the compiler is not hipcc.  All arithmetic is fp64 in the
// reference's order, without contraction; pow, sqrt and the divisions are the only operations
// whose last bit may depend on the maths library.
//
// Every channel ends in image_byte(c) = (byte)Math.Clamp(c·255, 0, 255) (Buffer.cs:157-159), with
// the one case C# leaves open, a NaN, mapped to 0 (as the project's Buffer.Image does).
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

enum { kChColor = 0, kChVariance = 1, kChStdDev = 2, kChSamples = 3, kChAlbedo = 4, kChNormal = 5, kChCount = 6 };

__host__ __device__ inline uint8_t image_byte(double c) {
    const double v = c * 255.0;
    if (!(v > 0.0)) return 0;        // NaN, -inf, negative, ±0
    if (v >= 255.0) return 255;      // +inf too
    return (uint8_t)(int)v;          // truncates toward zero
}

// Pixel.Variance (Buffer.cs:48-55)
__host__ __device__ inline double image_variance(double v, int32_t n) { return n < 2 ? 0.0 : v / (double)(n - 1); }

// Color, Variance, StandardDeviation: one component.  `x` is M (Color) or V (the other two).
template <int CH>
__host__ __device__ inline double image_component(double x, int32_t n) {
    if (CH == kChColor) return pow(x, 1.0 / 2.2);                  // Colour.Pow(1.0 / 2.2), Buffer.cs:156
    if (CH == kChVariance) return image_variance(x, n);
    return pow(image_variance(x, n), 0.5);                         // Pixel.StandardDeviation, Buffer.cs:57 (0.5f)
}

// Samples / maxSamples on all three components (Buffer.cs:138-146,176-178); maxSamples starts at 0,
// and the reference's 0/0 (an empty Buffer) is 0 here.
__host__ __device__ inline double image_samples(int32_t n, int32_t max_n) {
    return (double)n / (double)(max_n > 1 ? max_n : 1);
}

// CalculateAlbedo (Buffer.cs:240-282): M over its largest component, clamped to [0, 1]; a NaN
// clamp result (inf / inf) stays NaN, as Math.Clamp leaves it.
__host__ __device__ inline double image_clamp01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }
__host__ __device__ inline void image_albedo(const double m[3], double c[3]) {
    c[0] = c[1] = c[2] = 0.0;
    if (m[0] != m[0] || m[1] != m[1] || m[2] != m[2]) return;
    const double rg = m[0] < m[1] ? m[1] : m[0];
    const double mx = rg < m[2] ? m[2] : rg;
    if (mx == 0.0) return;
    for (int k = 0; k < 3; k++) c[k] = image_clamp01(m[k] / mx);
}

// M[k] of pixel (x, y), 0 outside the image (GetPixelOrDefault's new Pixel(), Buffer.cs:235-238)
__host__ __device__ inline double image_m_at(const double* m, int32_t w, int32_t h, int32_t x, int32_t y, int k) {
    if (x < 0 || y < 0 || x >= w || y >= h) return 0.0;
    return m[((size_t)y * (size_t)w + (size_t)x) * 3 + (size_t)k];
}

// GetNormalAt + CalculateNormal (Buffer.cs:99-124,222-233): Sobel differences of the neighbours'
// red (x) and green (y), nz = 1, normalised, each component through Vector's floats
// (Vector.cs:222-225), then x and y mapped to [0, 1] and z left as it is.
__host__ __device__ inline void image_normal(const double* m, int32_t w, int32_t h, int32_t x, int32_t y, double c[3]) {
    const double tl_r = image_m_at(m, w, h, x - 1, y - 1, 0), tl_g = image_m_at(m, w, h, x - 1, y - 1, 1);
    const double tr_r = image_m_at(m, w, h, x + 1, y - 1, 0), tr_g = image_m_at(m, w, h, x + 1, y - 1, 1);
    const double bl_r = image_m_at(m, w, h, x - 1, y + 1, 0), bl_g = image_m_at(m, w, h, x - 1, y + 1, 1);
    const double br_r = image_m_at(m, w, h, x + 1, y + 1, 0), br_g = image_m_at(m, w, h, x + 1, y + 1, 1);
    const double l_r = image_m_at(m, w, h, x - 1, y, 0), r_r = image_m_at(m, w, h, x + 1, y, 0);
    const double t_g = image_m_at(m, w, h, x, y - 1, 1), b_g = image_m_at(m, w, h, x, y + 1, 1);
    double nx = (tl_r + 2 * l_r + bl_r - tr_r - 2 * r_r - br_r) / 8.0;
    double ny = (tl_g + 2 * t_g + tr_g - bl_g - 2 * b_g - br_g) / 8.0;
    double nz = 1.0;
    const double length = sqrt(nx * nx + ny * ny + nz * nz);
    nx /= length;
    ny /= length;
    nz /= length;
    const float X = (float)nx, Y = (float)ny, Z = (float)nz;
    c[0] = ((double)X + 1.0) * 0.5;
    c[1] = ((double)Y + 1.0) * 0.5;
    c[2] = (double)Z;
}

// Pixel i of the flattened image on channel `channel`, from whole arrays: the host check's entry
// (the kernel calls the pieces above on the values it has loaded).
__host__ __device__ inline void image_resolve_at(int channel, const double* m, const double* v, const int32_t* n,
                                                 int32_t w, int32_t h, int32_t max_n, size_t i, uint8_t rgb[3]) {
    double c[3];
    if (channel == kChSamples) {
        c[0] = c[1] = c[2] = image_samples(n[i], max_n);
    } else if (channel == kChAlbedo) {
        image_albedo(m + 3 * i, c);
    } else if (channel == kChNormal) {
        image_normal(m, w, h, (int32_t)(i % (size_t)w), (int32_t)(i / (size_t)w), c);
    } else {
        for (int k = 0; k < 3; k++)
            c[k] = channel == kChColor      ? image_component<kChColor>(m[3 * i + k], 0)
                   : channel == kChVariance ? image_component<kChVariance>(v[3 * i + k], n[i])
                                            : image_component<kChStdDev>(v[3 * i + k], n[i]);
    }
    for (int k = 0; k < 3; k++) rgb[k] = image_byte(c[k]);
}

}  // namespace pt
