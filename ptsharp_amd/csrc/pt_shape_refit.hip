// pt_shape_refit.hip — the kernels of pt_update_shapes (gfx950): new sphere, cube and matrix parameters written
// into the records and transforms, and a bottom-up refit of the analytic BVH4, the arithmetic in pt_shape_refit.h
// (shared with the host check).
//   k_shapes_xforms   one thread per transformed shape: DevXform::m / inv, its ext_recs row when the inner shape
//                     is a sphere or cube, its padded world box into the xform scratch.
//   k_shapes_records  one thread per analytic record position: rows 0-2 of spheres and cubes, the record's padded
//                     box into rec_box (a transformed shape's from the xform scratch).
//   k_shapes_heavy    one thread per heavy record: the box of the record it names.
//   k_shapes_level    one launch per depth, the deepest first, one thread per node of that depth.
// Launches on one stream are ordered, so each kernel reads only what earlier launches wrote: no atomics.  Every
// store is a plain vector store or plain C++, every index 64-bit.  No write's address depends on
// the data: indices come from records, slots and thread numbers, and each is checked against its array.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_scene.h"
#include "pt_shape_refit.h"

namespace pt {

static_assert(kShapeSphere == KIND_SPHERE && kShapeCube == KIND_CUBE && kShapeSdf == KIND_SDF &&
              kShapeVolume == KIND_VOLUME && kShapeXform == KIND_XFORM, "pt_shape_refit.h names pt_scene.h's kinds");

constexpr int kShapeBlock = 256;

__global__ __launch_bounds__(kShapeBlock) void k_shapes_xforms(ShapeParams P, DevXform* __restrict__ xforms,
                                                               uint32_t* __restrict__ ext_recs,
                                                               const int32_t* __restrict__ inner_kind,
                                                               const int32_t* __restrict__ inner_index,
                                                               const float* __restrict__ inner_box, float* __restrict__ xbox) {
    const int64_t t = (int64_t)blockIdx.x * kShapeBlock + threadIdx.x;
    if (t >= (int64_t)P.num_transformed) return;
    shape_refit_xform(t, P, xforms, ext_recs, inner_kind, inner_index, inner_box, xbox, nullptr);
}

__global__ __launch_bounds__(kShapeBlock) void k_shapes_records(int64_t num_recs, ShapeParams P, uint32_t* __restrict__ recs,
                                                                float* __restrict__ rec_box, const float* __restrict__ xbox) {
    const int64_t i = (int64_t)blockIdx.x * kShapeBlock + threadIdx.x;
    if (i >= num_recs) return;
    shape_refit_record(i, P, recs, rec_box, xbox);
}

__global__ __launch_bounds__(kShapeBlock) void k_shapes_heavy(int64_t num_heavy, int64_t num_recs, uint32_t* __restrict__ heavy,
                                                              const float* __restrict__ rec_box) {
    const int64_t h = (int64_t)blockIdx.x * kShapeBlock + threadIdx.x;
    if (h >= num_heavy) return;
    shape_refit_heavy(h, num_recs, heavy, rec_box);
}

__global__ __launch_bounds__(kShapeBlock) void k_shapes_level(const uint32_t* __restrict__ level_nodes, int64_t count,
                                                              int64_t num_nodes, int64_t num_recs, uint32_t* nodes,
                                                              float* node_box, const float* __restrict__ rec_box) {
    const int64_t i = (int64_t)blockIdx.x * kShapeBlock + threadIdx.x;
    if (i >= count) return;
    const int64_t ni = (int64_t)level_nodes[i];
    if (ni >= num_nodes) return;
    shape_refit_node(ni, num_nodes, num_recs, nodes, node_box, rec_box);
}

// The whole refit on `stream`.  P's arrays, the tables and the scratch are device memory; level_off (host) holds
// the levels' bounds in level_nodes (device), the root's level first.
hipError_t launch_shape_refit(const ShapeParams& P, int64_t num_nodes, int64_t num_recs, int64_t num_heavy, int64_t num_levels,
                              const uint32_t* level_off, const uint32_t* level_nodes, uint32_t* nodes, uint32_t* recs,
                              uint32_t* ext_recs, DevXform* xforms, uint32_t* heavy, const int32_t* inner_kind,
                              const int32_t* inner_index, const float* inner_box, float* xbox, float* rec_box, float* node_box,
                              hipStream_t stream) {
    if (num_recs <= 0) return hipSuccess;
    const auto blocks = [](int64_t n) { return dim3((unsigned)((n + kShapeBlock - 1) / kShapeBlock)); };
    hipError_t e;
    if (P.num_transformed > 0) {
        hipLaunchKernelGGL(k_shapes_xforms, blocks(P.num_transformed), dim3(kShapeBlock), 0, stream, P, xforms, ext_recs,
                           inner_kind, inner_index, inner_box, xbox);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_shapes_records, blocks(num_recs), dim3(kShapeBlock), 0, stream, num_recs, P, recs, rec_box, xbox);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (num_heavy > 0) {
        hipLaunchKernelGGL(k_shapes_heavy, blocks(num_heavy), dim3(kShapeBlock), 0, stream, num_heavy, num_recs, heavy, rec_box);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    for (int64_t l = num_levels - 1; l >= 0; l--) {
        const int64_t count = (int64_t)level_off[l + 1] - (int64_t)level_off[l];
        if (count <= 0) continue;
        hipLaunchKernelGGL(k_shapes_level, blocks(count), dim3(kShapeBlock), 0, stream, level_nodes + level_off[l], count,
                           num_nodes, num_recs, nodes, node_box, rec_box);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace pt
