// pt_image.hip — a Buffer channel resolved to an 8-bit image on the device (pt_read_image).
//
// k_image_resolve<channel, format>: a thread resolves 4 consecutive pixels of the flattened image.
// Their M (or V) is 96 contiguous, 16-B-aligned bytes (six 16-B loads), their N one 16-B load, and
// their output 12 B (RGB8) or 16 B (RGBA8) of whole dwords, so a wave reads one contiguous 6 KiB
// run and writes one contiguous 768-B or 1-KiB run: no byte stores, no row handling (rows of an
// RGB8 image are not dword-aligned when W is odd; the flattened image is).  The staging image is
// padded to a multiple of 4 pixels; the one thread whose group crosses P loads its pixels one by
// one under a bound and resolves zeros for the rest.  The Normal channel's 3x3 stencil reads the
// neighbours' red and green straight from global memory: the three rows a wave touches are in L2.
//
// k_image_max_n: the Samples channel's maxSamples (Buffer.cs:138-146) — grid-stride max of N,
// shuffles inside a wave, LDS across the block's waves, one atomicMax per block into a word the
// caller has cleared (so the result is max(0, max N)).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ptsharp_hip.h"
#include "pt_image.h"

#pragma clang fp contract(off)

namespace pt {

constexpr int kImageBlock = 256;
constexpr int kImageMaxBlocks = 2048;   // 8 blocks per CU; larger images grid-stride

__global__ __launch_bounds__(kImageBlock) void k_image_max_n(const int32_t* __restrict__ n, size_t P,
                                                             int32_t* __restrict__ out) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const size_t groups = P / 4;
    int32_t mx = 0;
    for (size_t g = tid; g < groups; g += stride) {
        const int4 q = reinterpret_cast<const int4*>(n)[g];
        mx = max(max(mx, max(q.x, q.y)), max(q.z, q.w));
    }
    if (tid < P - 4 * groups) mx = max(mx, n[4 * groups + tid]);   // the up-to-3 pixels past the last group
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, __shfl_down(mx, off, 64));
    __shared__ int32_t s_wave[kImageBlock / 64];
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kImageBlock / 64; w++) mx = max(mx, s_wave[w]);
        if (mx > 0) atomicMax(out, mx);
    }
}

template <int CH, int FMT>
__global__ __launch_bounds__(kImageBlock) void k_image_resolve(const double* __restrict__ m, const double* __restrict__ v,
                                                               const int32_t* __restrict__ n,
                                                               const int32_t* __restrict__ max_n,
                                                               uint32_t* __restrict__ out, int32_t W, int32_t H) {
    constexpr bool kReadsColour = CH == kChColor || CH == kChAlbedo || CH == kChVariance || CH == kChStdDev;
    constexpr bool kReadsN = CH == kChVariance || CH == kChStdDev || CH == kChSamples;
    const double* __restrict__ src = (CH == kChVariance || CH == kChStdDev) ? v : m;
    const size_t P = (size_t)W * (size_t)H, groups = (P + 3) / 4;
    const int32_t mx = CH == kChSamples ? *max_n : 0;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
        const size_t i0 = 4 * g;
        const bool full = i0 + 4 <= P;
        double x[12];
        int32_t cnt[4] = {0, 0, 0, 0};
        if (kReadsColour) {
            if (full) {
                const double2* p = reinterpret_cast<const double2*>(src + 3 * i0);
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    const double2 t = p[j];
                    x[2 * j] = t.x;
                    x[2 * j + 1] = t.y;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 12; j++) x[j] = (i0 + (size_t)(j / 3) < P) ? src[3 * i0 + (size_t)j] : 0.0;
            }
        }
        if (kReadsN) {
            if (full) {
                const int4 q = *reinterpret_cast<const int4*>(n + i0);
                cnt[0] = q.x; cnt[1] = q.y; cnt[2] = q.z; cnt[3] = q.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++) cnt[q] = (i0 + (size_t)q < P) ? n[i0 + (size_t)q] : 0;
            }
        }
        uint32_t b[12];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            double c[3] = {0.0, 0.0, 0.0};
            if (CH == kChSamples) {
                c[0] = c[1] = c[2] = image_samples(cnt[q], mx);
            } else if (CH == kChAlbedo) {
                image_albedo(&x[3 * q], c);
            } else if (CH == kChNormal) {
                const size_t i = i0 + (size_t)q;
                if (i < P) image_normal(m, W, H, (int32_t)(i % (size_t)W), (int32_t)(i / (size_t)W), c);
            } else {
#pragma unroll
                for (int k = 0; k < 3; k++) c[k] = image_component<CH>(x[3 * q + k], cnt[q]);
            }
#pragma unroll
            for (int k = 0; k < 3; k++) b[3 * q + k] = image_byte(c[k]);
        }
        if (FMT == PT_IMAGE_RGBA8) {
            uint4 o;
            o.x = b[0] | (b[1] << 8) | (b[2] << 16) | 0xFF000000u;
            o.y = b[3] | (b[4] << 8) | (b[5] << 16) | 0xFF000000u;
            o.z = b[6] | (b[7] << 8) | (b[8] << 16) | 0xFF000000u;
            o.w = b[9] | (b[10] << 8) | (b[11] << 16) | 0xFF000000u;
            reinterpret_cast<uint4*>(out)[g] = o;
        } else {
            out[3 * g] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
            out[3 * g + 1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
            out[3 * g + 2] = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
        }
    }
}

template <int CH>
static void launch_format(int format, dim3 grid, hipStream_t stream, const double* m, const double* v, const int32_t* n,
                          const int32_t* max_n, uint32_t* out, int32_t W, int32_t H) {
    if (format == PT_IMAGE_RGBA8)
        hipLaunchKernelGGL((k_image_resolve<CH, PT_IMAGE_RGBA8>), grid, dim3(kImageBlock), 0, stream, m, v, n, max_n, out, W, H);
    else
        hipLaunchKernelGGL((k_image_resolve<CH, PT_IMAGE_RGB8>), grid, dim3(kImageBlock), 0, stream, m, v, n, max_n, out, W, H);
}

// Bytes of the staging image pt_read_image resolves into (either format) and, after it, the max-N word.
size_t image_staging_bytes(int32_t W, int32_t H) { return (((size_t)W * (size_t)H + 3) / 4) * 16; }

// Resolve `channel` of the Buffer {m, v, n} into `out` (image_staging_bytes, 16-B aligned) on `stream`;
// `max_n` is a device word of the caller's.  channel and format are valid (pt_read_image checks them).
hipError_t launch_image_resolve(int channel, int format, const double* m, const double* v, const int32_t* n,
                                int32_t* max_n, uint32_t* out, int32_t W, int32_t H, hipStream_t stream) {
    const size_t P = (size_t)W * (size_t)H, groups = (P + 3) / 4;
    auto blocks = [](size_t threads) {
        const size_t b = (threads + kImageBlock - 1) / kImageBlock;
        return dim3((unsigned)(b < (size_t)kImageMaxBlocks ? (b ? b : 1) : (size_t)kImageMaxBlocks));
    };
    if (channel == PT_CHANNEL_SAMPLES) {
        hipError_t e = hipMemsetAsync(max_n, 0, sizeof(int32_t), stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_image_max_n, blocks(groups), dim3(kImageBlock), 0, stream, n, P, max_n);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const dim3 grid = blocks(groups);
    switch (channel) {
        case PT_CHANNEL_COLOR: launch_format<kChColor>(format, grid, stream, m, v, n, max_n, out, W, H); break;
        case PT_CHANNEL_VARIANCE: launch_format<kChVariance>(format, grid, stream, m, v, n, max_n, out, W, H); break;
        case PT_CHANNEL_STDDEV: launch_format<kChStdDev>(format, grid, stream, m, v, n, max_n, out, W, H); break;
        case PT_CHANNEL_SAMPLES: launch_format<kChSamples>(format, grid, stream, m, v, n, max_n, out, W, H); break;
        case PT_CHANNEL_ALBEDO: launch_format<kChAlbedo>(format, grid, stream, m, v, n, max_n, out, W, H); break;
        default: launch_format<kChNormal>(format, grid, stream, m, v, n, max_n, out, W, H); break;
    }
    return hipGetLastError();
}

}  // namespace pt
