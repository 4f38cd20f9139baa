// pt_refit.hip — the kernels of pt_update_triangles (gfx950): a bottom-up refit of the 8-wide quantized
// triangle BVH from new vertices, the arithmetic in pt_refit.h (shared with the host check).
//   k_refit_leaves  one thread per leaf chunk: its 1..3 triangles' shading records, its geometry words, its
//                   exact box.
//   k_refit_level   one launch per depth, the deepest first, one thread per node of that depth: the
//                   children's exact boxes requantized, the node's own exact box.  Launches on one stream
//                   are ordered, so a level reads only boxes that earlier launches wrote: no atomics.
// Every store is a plain vector store, every index 64-bit.  No write depends on the data.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_refit.h"

namespace pt {

constexpr int kRefitBlock = 256;

__global__ __launch_bounds__(kRefitBlock) void k_refit_leaves(int64_t num_chunks, uint32_t* __restrict__ chunks,
                                                              uint32_t* __restrict__ recs, const int32_t* __restrict__ src_of_pos,
                                                              const float* __restrict__ v1, const float* __restrict__ v2,
                                                              const float* __restrict__ v3, const float* __restrict__ n1,
                                                              const float* __restrict__ n2, const float* __restrict__ n3,
                                                              float* __restrict__ chunk_box) {
    const int64_t ci = (int64_t)blockIdx.x * kRefitBlock + threadIdx.x;
    if (ci >= num_chunks) return;
    refit_chunk(ci, chunks, recs, src_of_pos, v1, v2, v3, n1, n2, n3, chunk_box);
}

__global__ __launch_bounds__(kRefitBlock) void k_refit_level(const uint32_t* __restrict__ level_nodes, int64_t count,
                                                             uint32_t* nodes, float* node_box, const float* __restrict__ chunk_box) {
    const int64_t i = (int64_t)blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= count) return;
    refit_node((int64_t)level_nodes[i], nodes, node_box, chunk_box);
}

// The whole refit on `stream`.  level_nodes (device) holds the node indices by depth, level_off (host) the
// levels' bounds, the root's level first.
hipError_t launch_refit(int64_t num_chunks, int64_t num_levels, const uint32_t* level_off, const uint32_t* level_nodes,
                        uint32_t* nodes, uint32_t* chunks, uint32_t* recs, const int32_t* src_of_pos, const float* v1,
                        const float* v2, const float* v3, const float* n1, const float* n2, const float* n3,
                        float* node_box, float* chunk_box, hipStream_t stream) {
    if (num_chunks <= 0) return hipSuccess;
    const auto blocks = [](int64_t n) { return dim3((unsigned)((n + kRefitBlock - 1) / kRefitBlock)); };
    hipLaunchKernelGGL(k_refit_leaves, blocks(num_chunks), dim3(kRefitBlock), 0, stream, num_chunks, chunks, recs, src_of_pos,
                       v1, v2, v3, n1, n2, n3, chunk_box);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (int64_t l = num_levels - 1; l >= 0; l--) {
        const int64_t count = (int64_t)level_off[l + 1] - (int64_t)level_off[l];
        if (count <= 0) continue;
        hipLaunchKernelGGL(k_refit_level, blocks(count), dim3(kRefitBlock), 0, stream, level_nodes + level_off[l], count, nodes,
                           node_box, chunk_box);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace pt
