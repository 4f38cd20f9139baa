// pt_query.hip — ray queries that say what was hit and where (pt_intersect_hits).
//
// k_intersect_hits<FULL, INFO>: one lane per ray, the megakernel's trace() with its per-lane LDS stack exactly as
// k_intersect and k_features have it (256 lanes, kStackMax words each: 64 KiB per block, two blocks per CU; the
// kernel uses no other LDS).  A lane past n returns before the trace, as k_intersect's does.  Then
//   identity  the hit's record position turned into the host's own numbering through the tables of QueryDevTables
//             (pt_query.h): a few 4-byte loads per ray, each guarded by its table's length, so an index outside a
//             table gives -1 and never an access outside an array;
//   INFO      Hit.Info (hit_info: position, the normal after the flip with normal and bump maps, inside, material, the
//             MaterialAt colour and gloss), or sampleEnvironment on a miss, as k_features runs them.
// Without INFO the kernel is k_intersect plus the identity lookups: hit_info is not instantiated.
// The source triangle under a hit through an instanced mesh needs the BLAS position, which HitRec does not carry:
// instance_position repeats the nested traversal ext_hit_info runs (same transformed ray, same blas_hit, so the same
// triangle), only for such hits and only when `prim` is wanted.  The render kernels' device functions are untouched.
// Every output pointer is a kernel argument: a NULL one is skipped by a branch the whole grid takes alike.  Stores are
// plain vector stores; every index is formed in 64 bits.
#include <hip/hip_runtime.h>

#include "pt_device.h"
#include "pt_query.h"

#pragma clang fp contract(off)

namespace pt {

constexpr int kQueryBlock = 256;
using QStack = LdsStack<kQueryBlock>;

__device__ __forceinline__ int32_t table_at(const int32_t* __restrict__ table, int64_t n, int64_t i) {
    return (table && i >= 0 && i < n) ? table[i] : -1;
}

// The position in its BLAS's records of the triangle a ray hits through transformed shape X (over a mesh), or -1
__device__ __forceinline__ int64_t instance_position(const DevScene& S, const QueryDevTables& T, const DevXform& X, v3 o, v3 d) {
    if (X.rec < 0 || X.rec >= T.num_blas) return -1;
    const v3 so = mat_position(X.inv, o), sd = mat_direction(X.inv, d);   // as ext_hit_info maps the ray
    const HitRec ih = blas_hit(S, X.rec, so, sd);
    if (ih.idx < 0) return -1;
    return (int64_t)S.blas[X.rec].rec_off + (int64_t)ih.idx;
}

// index, prim and shape of hit h (pt_hit_arrays, include/ptsharp_hip.h)
template <bool FULL>
__device__ __forceinline__ void identity(const DevScene& S, const QueryDevTables& T, const HitRec& h, v3 o, v3 d,
                                         bool want_prim, int32_t& index, int32_t& prim, int32_t& shape) {
    index = prim = shape = -1;
    const int64_t pos = h.idx;
    if (h.kind == KIND_TRI) {
        index = prim = table_at(T.tri_src, T.tri_src_n, pos);
        shape = table_at(T.tri_slot, T.tri_slot_n, index);
        return;
    }
    if (h.kind == KIND_PLANE) {
        if (pos < 0 || pos >= (int64_t)S.num_planes) return;
        index = (int32_t)f2u(S.planes[2 * pos + 1].w);
        shape = table_at(T.plane_slot, T.plane_slot_n, index);
        return;
    }
    if (pos < 0 || pos >= (int64_t)S.ana_count) return;
    const float4* r = S.ana_recs + 3 * pos;
    index = (int32_t)f2u(r[1].w);
    int32_t off = 0, cnt = 0;
    switch (h.kind) {
        case KIND_SPHERE: off = T.ana_off[KIND_SPHERE]; cnt = T.ana_cnt[KIND_SPHERE]; break;
        case KIND_CUBE: off = T.ana_off[KIND_CUBE]; cnt = T.ana_cnt[KIND_CUBE]; break;
        case KIND_SDF: off = T.ana_off[KIND_SDF]; cnt = T.ana_cnt[KIND_SDF]; break;
        case KIND_VOLUME: off = T.ana_off[KIND_VOLUME]; cnt = T.ana_cnt[KIND_VOLUME]; break;
        case KIND_XFORM: off = T.ana_off[KIND_XFORM]; cnt = T.ana_cnt[KIND_XFORM]; break;
        default: break;
    }
    if (index < 0 || index >= cnt) { index = -1; return; }
    shape = table_at(T.ana_slot, T.ana_slot_n, (int64_t)off + index);
    if (FULL && want_prim && h.kind == KIND_XFORM) {
        const DevXform& X = S.xforms[index];
        if (X.kind == KIND_MESH) prim = table_at(T.blas_src, T.blas_src_n, instance_position(S, T, X, o, d));
    }
}

template <bool FULL, bool INFO>
__global__ __launch_bounds__(kQueryBlock) void k_intersect_hits(DevScene S, QueryDevTables T, int64_t n,
                                                                const float* __restrict__ o3, const float* __restrict__ d3,
                                                                QueryOut out) {
    __shared__ uint32_t s_stack[kStackMax * kQueryBlock];
    const QStack stack{s_stack + threadIdx.x};
    const int64_t i = (int64_t)blockIdx.x * kQueryBlock + (int64_t)threadIdx.x;
    if (i >= n) return;
    const v3 o{o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]};
    const v3 d{d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]};
    Counters ctr{0, 0, 0, 0};
    const HitRec h = trace<false, FULL>(S, o, d, stack, ctr);
    const bool hit = h.t < kHitInf;
    if (out.t) out.t[i] = h.t;
    if (out.kind) out.kind[i] = hit ? h.kind : -1;
    if (out.index || out.prim || out.shape) {
        int32_t index = -1, prim = -1, shape = -1;
        if (hit) identity<FULL>(S, T, h, o, d, out.prim != nullptr, index, prim, shape);
        if (out.index) out.index[i] = index;
        if (out.prim) out.prim[i] = prim;
        if (out.shape) out.shape[i] = shape;
    }
    if (INFO) {
        v3 pos = zero3(), nrm = zero3();
        int32_t inside = 0, mat = -1;
        double a[3], gloss = 0.0;
        if (hit) {
            const Shade sh = hit_info<false, FULL>(S, h, o, d, ctr);
            pos = sh.pos; nrm = sh.nrm;
            inside = sh.inside; mat = sh.mat;
            a[0] = sh.col[0]; a[1] = sh.col[1]; a[2] = sh.col[2];
            gloss = sh.gloss;
        } else {
            const double3 env = environment<FULL>(S, d);   // sampleEnvironment (Sampler.cs:177-189), as k_features
            a[0] = env.x; a[1] = env.y; a[2] = env.z;
        }
        if (out.position) { out.position[3 * i] = pos.x; out.position[3 * i + 1] = pos.y; out.position[3 * i + 2] = pos.z; }
        if (out.normal) { out.normal[3 * i] = nrm.x; out.normal[3 * i + 1] = nrm.y; out.normal[3 * i + 2] = nrm.z; }
        if (out.inside) out.inside[i] = inside;
        if (out.material) out.material[i] = mat;
        if (out.albedo) { out.albedo[3 * i] = a[0]; out.albedo[3 * i + 1] = a[1]; out.albedo[3 * i + 2] = a[2]; }
        if (out.gloss) out.gloss[i] = gloss;
    }
}

// FULL as the kernel this variant extends picks it: with INFO k_features' (textures or §8f row 4 shapes), without
// k_intersect's (row 4 shapes only).  trace() gives the same bits either way on a scene without row 4 shapes.
hipError_t launch_intersect_hits(const DevScene& S, const QueryDevTables& T, int64_t n, const float* o3, const float* d3,
                                 const QueryOut& out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (n > kQueryChunkMax) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + kQueryBlock - 1) / kQueryBlock)), block(kQueryBlock);
    const bool info = query_wants_info(out);
    const bool full = info ? S.full != 0 : S.full_geom != 0;
    if (info && full) hipLaunchKernelGGL((k_intersect_hits<true, true>), grid, block, 0, stream, S, T, n, o3, d3, out);
    else if (info) hipLaunchKernelGGL((k_intersect_hits<false, true>), grid, block, 0, stream, S, T, n, o3, d3, out);
    else if (full) hipLaunchKernelGGL((k_intersect_hits<true, false>), grid, block, 0, stream, S, T, n, o3, d3, out);
    else hipLaunchKernelGGL((k_intersect_hits<false, false>), grid, block, 0, stream, S, T, n, o3, d3, out);
    return hipGetLastError();
}

}  // namespace pt
