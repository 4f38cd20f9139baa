// pt_denoise.hip — the variance-guided à-trous denoiser on the device (pt_denoise).
//
// Three kernels, each one lane per pixel in blocks of 64x4 (a wave is 64 consecutive pixels of a
// row), each calling the per-pixel text of pt_denoise.h:
//   k_denoise_prepare  Buffer {M, V, N} -> c, the unblurred s2 and the validity byte
//   k_denoise_blur     s2 -> its 3x3 binomial blur (once)
//   k_denoise_level_t  one à-trous level at step s, from one {c, s2} pair into the other; its guided
//                      instantiation also reads the features' guide records (pt_denoise_guided)
// With a lane per pixel along x every tap of the stencil, whatever the step, is a load of 64
// consecutive pixels (1536 contiguous bytes of c, as many of s2, 64 validity bytes), so no level
// needs a gather; the reuse between the rows y, y±s, y±2s is left to L2 and the Infinity Cache.
// No LDS staging: it could only pay at steps 1 and 2, and the level is bound by its fp64 exp and
// divisions, not by bytes (DESIGN.md §4b has the measured rate).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_denoise.h"

#pragma clang fp contract(off)

namespace pt {

constexpr int kDenoiseBlockX = 64, kDenoiseBlockY = 4;

__global__ __launch_bounds__(kDenoiseBlockX * kDenoiseBlockY) void k_denoise_prepare(
    const double* __restrict__ m, const double* __restrict__ v, const int32_t* __restrict__ n, double* __restrict__ c_out,
    double* __restrict__ s2_out, uint8_t* __restrict__ valid_out, int32_t W, int32_t H) {
    const int32_t x = (int32_t)(blockIdx.x * kDenoiseBlockX + threadIdx.x), y = (int32_t)(blockIdx.y * kDenoiseBlockY + threadIdx.y);
    if (x >= W || y >= H) return;
    double c[3], s2[3];
    const bool ok = denoise_prepare_at(m, v, n, W, H, x, y, c, s2);
    const size_t p = denoise_index(W, x, y);
    valid_out[p] = ok ? 1 : 0;
    for (int k = 0; k < 3; k++) {
        c_out[3 * p + k] = c[k];
        s2_out[3 * p + k] = s2[k];
    }
}

__global__ __launch_bounds__(kDenoiseBlockX * kDenoiseBlockY) void k_denoise_blur(
    const double* __restrict__ s2, const uint8_t* __restrict__ valid, double* __restrict__ s2_out, int32_t W, int32_t H) {
    const int32_t x = (int32_t)(blockIdx.x * kDenoiseBlockX + threadIdx.x), y = (int32_t)(blockIdx.y * kDenoiseBlockY + threadIdx.y);
    if (x >= W || y >= H) return;
    double out[3];
    denoise_blur_at(s2, valid, W, H, x, y, out);
    const size_t p = denoise_index(W, x, y);
    for (int k = 0; k < 3; k++) s2_out[3 * p + k] = out[k];
}

// GUIDED = false is pt_denoise's level (`guide` unused, denoise_level_at alone); GUIDED = true adds the guide
// record's terms to each tap's distance (pt_denoise_guided): two more 16-byte loads per tap.
template <bool GUIDED>
__global__ __launch_bounds__(kDenoiseBlockX * kDenoiseBlockY) void k_denoise_level_t(
    const double* __restrict__ c, const double* __restrict__ s2, const uint8_t* __restrict__ valid,
    const DenoiseGuideRec* __restrict__ guide, double* __restrict__ c_out, double* __restrict__ s2_out, int32_t W, int32_t H,
    int32_t step, double sigma2, DenoiseGuideSigmas sg) {
    const int32_t x = (int32_t)(blockIdx.x * kDenoiseBlockX + threadIdx.x), y = (int32_t)(blockIdx.y * kDenoiseBlockY + threadIdx.y);
    if (x >= W || y >= H) return;
    double co[3], so[3];
    if (GUIDED) denoise_level_guided_at(c, s2, valid, guide, W, H, x, y, step, sigma2, sg, co, so);
    else denoise_level_at(c, s2, valid, W, H, x, y, step, sigma2, co, so);
    const size_t p = denoise_index(W, x, y);
    for (int k = 0; k < 3; k++) {
        c_out[3 * p + k] = co[k];
        s2_out[3 * p + k] = so[k];
    }
}

// Bytes of the denoiser's workspace: two {c, s2} pairs of [P][3] doubles, then P validity bytes.
size_t denoise_workspace_bytes(int32_t W, int32_t H) {
    const size_t P = (size_t)W * (size_t)H;
    return 4 * 3 * P * sizeof(double) + P;
}

// Filter the Buffer {m, v, n} with `iterations` levels on `stream`.  `ws` is denoise_workspace_bytes
// of device memory; the result is pair *out_pair (0 or 1): c at ws + pair·6P doubles, s2 3P doubles
// after it.  iterations and sigma are valid (pt_denoise checks them).  With `guide` ([P] records of 32
// bytes, pt_features.hip) the levels are the guided ones, with sigma_albedo, sigma_normal and
// sigma_depth in `gs` (pt_denoise_guided checks them); without, pt_denoise's.
static hipError_t launch_levels(const double* m, const double* v, const int32_t* n, void* ws, const DenoiseGuideRec* guide,
                                const double gs[3], int32_t W, int32_t H, int32_t iterations, double sigma, int* out_pair,
                                hipStream_t stream) {
    const size_t P = (size_t)W * (size_t)H;
    double* base = (double*)ws;
    double* c[2] = {base, base + 6 * P};
    double* s2[2] = {base + 3 * P, base + 9 * P};
    uint8_t* valid = (uint8_t*)(base + 12 * P);
    const dim3 block(kDenoiseBlockX, kDenoiseBlockY);
    const dim3 grid((unsigned)((W + kDenoiseBlockX - 1) / kDenoiseBlockX), (unsigned)((H + kDenoiseBlockY - 1) / kDenoiseBlockY));
    hipLaunchKernelGGL(k_denoise_prepare, grid, block, 0, stream, m, v, n, c[0], s2[1], valid, W, H);
    hipLaunchKernelGGL(k_denoise_blur, grid, block, 0, stream, (const double*)s2[1], (const uint8_t*)valid, s2[0], W, H);
    const double sigma2 = sigma * sigma;
    const DenoiseGuideSigmas sg = guide ? DenoiseGuideSigmas{gs[0] * gs[0], gs[1] * gs[1], gs[2]} : DenoiseGuideSigmas{0.0, 0.0, 0.0};
    int src = 0;
    for (int32_t j = 0; j < iterations; j++, src ^= 1) {
        if (guide)
            hipLaunchKernelGGL((k_denoise_level_t<true>), grid, block, 0, stream, (const double*)c[src], (const double*)s2[src],
                               (const uint8_t*)valid, guide, c[src ^ 1], s2[src ^ 1], W, H, (int32_t)1 << j, sigma2, sg);
        else
            hipLaunchKernelGGL((k_denoise_level_t<false>), grid, block, 0, stream, (const double*)c[src], (const double*)s2[src],
                               (const uint8_t*)valid, guide, c[src ^ 1], s2[src ^ 1], W, H, (int32_t)1 << j, sigma2, sg);
    }
    *out_pair = src;
    return hipGetLastError();
}

hipError_t launch_denoise(const double* m, const double* v, const int32_t* n, void* ws, int32_t W, int32_t H,
                          int32_t iterations, double sigma, int* out_pair, hipStream_t stream) {
    return launch_levels(m, v, n, ws, nullptr, nullptr, W, H, iterations, sigma, out_pair, stream);
}

// `guide` is the features' guide records (features_guide, pt_features.hip).
hipError_t launch_denoise_guided(const double* m, const double* v, const int32_t* n, void* ws, const void* guide,
                                 int32_t W, int32_t H, int32_t iterations, double sigma, double sigma_albedo,
                                 double sigma_normal, double sigma_depth, int* out_pair, hipStream_t stream) {
    const double gs[3] = {sigma_albedo, sigma_normal, sigma_depth};
    return launch_levels(m, v, n, ws, (const DenoiseGuideRec*)guide, gs, W, H, iterations, sigma, out_pair, stream);
}

}  // namespace pt
