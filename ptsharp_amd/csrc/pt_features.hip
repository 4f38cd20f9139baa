// pt_features.hip — first-hit feature buffers (pt_render_features / pt_write_features).
//
// k_features: one lane per pixel of the whole frame, one primary ray each: Camera.CastRay(x, y, W, H,
// 0.5, 0.5) with the lens ignored (the host passes aperture_radius 0, so no random number is drawn),
// the megakernel's trace() with its per-lane LDS stack exactly as k_intersect has it, then Hit.Info
// (hit_info: position, the shading normal after the flip with normal and bump maps, the material id,
// the MaterialAt colour), or sampleEnvironment on a miss.  Blocks of 256 with the 64 KiB stack (two
// blocks per CU, as k_intersect); a wave is an 8x8 pixel tile, a block 16x16, so a wave's primary
// rays traverse the BVH together; the price is that each array is written as 8 row pieces per wave.
// A lane outside the image returns before the trace, as k_intersect's lanes past n do: march_pending
// counts the active lanes itself, and the march gives the same bits either way (pt_device.h).
//
// k_features_pack: the guide records of features a host wrote (pt_write_features), by the same
// packing text (guide_pack).
//
// Features of P = W·H pixels are one allocation (features_bytes), in this order, every part 32-byte
// aligned when the base is:
//   albedo [P][3] f64 | depth [P] f64 | guide [P] 32-B records | normal [P][3] f32 | kind [P] i32 | material [P] i32
// Every offset is formed in 64 bits.
#include <hip/hip_runtime.h>

#include "pt_denoise.h"
#include "pt_device.h"

#pragma clang fp contract(off)

namespace pt {

constexpr int kFeatBlock = 256;
using FStack = LdsStack<kFeatBlock>;

size_t features_bytes(int32_t W, int32_t H) {
    const size_t P = (size_t)W * (size_t)H;
    return P * (3 * sizeof(double) + sizeof(double) + sizeof(DenoiseGuideRec) + 3 * sizeof(float) + 2 * sizeof(int32_t));
}

struct Features {
    double* albedo;
    double* depth;
    DenoiseGuideRec* guide;
    float* normal;
    int32_t* kind;
    int32_t* material;
};

static Features features_of(void* base, int32_t W, int32_t H) {
    const size_t P = (size_t)W * (size_t)H;
    Features f;
    f.albedo = (double*)base;
    f.depth = f.albedo + 3 * P;
    f.guide = (DenoiseGuideRec*)(f.depth + P);
    f.normal = (float*)(f.guide + P);
    f.kind = (int32_t*)(f.normal + 3 * P);
    f.material = f.kind + P;
    return f;
}

// part: pt_feature (0 albedo, 1 normal, 2 depth, 3 kind, 4 material); its address and size in bytes.
void* features_part(void* base, int32_t W, int32_t H, int part, size_t* bytes) {
    const size_t P = (size_t)W * (size_t)H;
    const Features f = features_of(base, W, H);
    switch (part) {
        case 0: *bytes = 3 * P * sizeof(double); return f.albedo;
        case 1: *bytes = 3 * P * sizeof(float); return f.normal;
        case 2: *bytes = P * sizeof(double); return f.depth;
        case 3: *bytes = P * sizeof(int32_t); return f.kind;
        default: *bytes = P * sizeof(int32_t); return f.material;
    }
}

const void* features_guide(void* base, int32_t W, int32_t H) { return features_of(base, W, H).guide; }

// The guide record of a pixel: {n.xyz, (float)depth} {(float)albedo.rgb, hit}, written as two 16-byte stores.
__device__ __forceinline__ void guide_pack(DenoiseGuideRec* guide, size_t p, float nx, float ny, float nz, double depth,
                                           double ar, double ag, double ab, bool hit) {
    float4* g = (float4*)(guide + p);
    g[0] = make_float4(nx, ny, nz, (float)depth);
    g[1] = make_float4((float)ar, (float)ag, (float)ab, hit ? 1.f : 0.f);
}

template <bool FULL>
__global__ __launch_bounds__(kFeatBlock) void k_features(DevScene S, DevCamera cam, int32_t W, int32_t H, Features F) {
    __shared__ uint32_t s_stack[kStackMax * kFeatBlock];
    const FStack stack{s_stack + threadIdx.x};
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t x64 = (int64_t)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int64_t y64 = (int64_t)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x64 >= (int64_t)W || y64 >= (int64_t)H) return;
    const int x = (int)x64, y = (int)y64;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    v3 o, d;
    cast_ray(cam, x, y, W, H, 0.5, 0.5, 0ull, o, d);   // aperture_radius is 0: the key is never used
    Counters ctr{0, 0, 0, 0};
    const HitRec h = trace<false, FULL>(S, o, d, stack, ctr);
    const bool hit = h.t < kHitInf;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    double a[3], depth = kHitInf;
    int32_t kind = -1, mat = -1;
    if (hit) {
        const Shade sh = hit_info<false, FULL>(S, h, o, d, ctr);
        nx = sh.nrm.x; ny = sh.nrm.y; nz = sh.nrm.z;
        a[0] = sh.col[0]; a[1] = sh.col[1]; a[2] = sh.col[2];
        depth = h.t;
        kind = h.kind;
        mat = sh.mat;
    } else {
        const double3 env = environment<FULL>(S, d);   // sampleEnvironment (Sampler.cs:177-189)
        a[0] = env.x; a[1] = env.y; a[2] = env.z;
    }
    F.albedo[3 * p] = a[0]; F.albedo[3 * p + 1] = a[1]; F.albedo[3 * p + 2] = a[2];
    F.normal[3 * p] = nx; F.normal[3 * p + 1] = ny; F.normal[3 * p + 2] = nz;
    F.depth[p] = depth;
    F.kind[p] = kind;
    F.material[p] = mat;
    guide_pack(F.guide, p, nx, ny, nz, depth, a[0], a[1], a[2], hit);
}

__global__ __launch_bounds__(256) void k_features_pack(Features F, uint64_t P) {
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= P) return;
    guide_pack(F.guide, (size_t)p, F.normal[3 * p], F.normal[3 * p + 1], F.normal[3 * p + 2], F.depth[p], F.albedo[3 * p],
               F.albedo[3 * p + 1], F.albedo[3 * p + 2], F.kind[p] >= 0);
}

// The feature pass of the whole W x H frame into `base` (features_bytes) on `stream`.
hipError_t launch_features(const DevScene& S, const DevCamera& cam, void* base, int32_t W, int32_t H, hipStream_t stream) {
    const Features F = features_of(base, W, H);
    const dim3 grid((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16)), block(kFeatBlock);
    if (S.full != 0) hipLaunchKernelGGL((k_features<true>), grid, block, 0, stream, S, cam, W, H, F);
    else hipLaunchKernelGGL((k_features<false>), grid, block, 0, stream, S, cam, W, H, F);
    return hipGetLastError();
}

// The guide records of the albedo, normal, depth and kind already in `base`.
hipError_t launch_features_pack(void* base, int32_t W, int32_t H, hipStream_t stream) {
    const Features F = features_of(base, W, H);
    const uint64_t P = (uint64_t)W * (uint64_t)H;
    hipLaunchKernelGGL(k_features_pack, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, F, P);
    return hipGetLastError();
}

}  // namespace pt
