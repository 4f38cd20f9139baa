// pt_blas_refit.hip — the kernels of pt_update_meshes for instanced meshes (gfx950): new vertices written into the
// BLAS triangle records, each mesh's unpadded box, and a bottom-up refit of every BLAS, the arithmetic in
// pt_blas_refit.h (shared with the host check).
//   k_blas_tris         one thread per BLAS triangle position: its blas_recs rows, its blas_shade rows when normals
//                       come along, its padded box into the tri_box scratch.
//   k_blas_bounds       one block per kBlasSpan positions of one BLAS: the unpadded min / max of their vertices, by a
//                       64-lane shuffle reduction, then LDS across the block's waves, into one partial per block.
//   k_blas_bounds_fold  one thread per BLAS: its blocks' partials folded in block order into blas_box.
//   k_blas_inner        one thread per transformed shape: its mesh's box into its xf_inner_box row.
//   k_blas_level        one launch per depth, the deepest first, one thread per node of that depth over all BLASes.
// Launches on one stream are ordered, so each kernel reads only what earlier launches wrote: no atomics, and min / max
// are exact, so no reduction order changes a value.  Every store is a plain vector store or plain C++, every index
// 64-bit.  No write's address depends on the data: indices come from tables, slots and thread
// numbers, and each is checked against its array.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_blas_refit.h"

namespace pt {

constexpr int kBlasBlock = 256;
constexpr int kBlasWave = 64;
constexpr int kBlasPerThread = 8;
constexpr int kBlasSpan = kBlasBlock * kBlasPerThread;   // positions one block of k_blas_bounds folds

__global__ __launch_bounds__(kBlasBlock) void k_blas_tris(int64_t num_pos, int64_t num_triangles, uint32_t* __restrict__ recs,
                                                          uint32_t* __restrict__ shade, const int32_t* __restrict__ src_of_pos,
                                                          const float* __restrict__ v1, const float* __restrict__ v2,
                                                          const float* __restrict__ v3, const float* __restrict__ n1,
                                                          const float* __restrict__ n2, const float* __restrict__ n3,
                                                          float* __restrict__ tri_box) {
    const int64_t pos = (int64_t)blockIdx.x * kBlasBlock + threadIdx.x;
    if (pos >= num_pos) return;
    const int64_t s = (int64_t)src_of_pos[pos];
    if (s < 0 || s >= num_triangles) return;
    blas_refit_tri(pos, s, recs, shade, v1, v2, v3, n1, n2, n3, tri_box);
}

// block_blas / block_first: per block its BLAS and its first position (host tables: a block never spans two BLASes)
__global__ __launch_bounds__(kBlasBlock) void k_blas_bounds(int64_t num_pos, int64_t num_triangles, int64_t num_blas,
                                                            const int32_t* __restrict__ desc,
                                                            const int32_t* __restrict__ block_blas,
                                                            const int32_t* __restrict__ block_first,
                                                            const int32_t* __restrict__ src_of_pos,
                                                            const float* __restrict__ v1, const float* __restrict__ v2,
                                                            const float* __restrict__ v3, float* __restrict__ block_part) {
    __shared__ float part[kBlasBlock / kBlasWave][6];
    const int64_t b = (int64_t)block_blas[blockIdx.x];
    float box[6];
    blas_bounds_empty(box);
    if (b >= 0 && b < num_blas) {
        const int64_t begin = max((int64_t)desc[4 * b + 2], (int64_t)0);   // the BLAS's positions are [begin, end)
        const int64_t end = min((int64_t)desc[4 * b + 2] + (int64_t)desc[4 * b + 3], num_pos);
        const int64_t first = (int64_t)block_first[blockIdx.x];
        for (int k = 0; k < kBlasPerThread; k++) {
            const int64_t pos = first + (int64_t)k * kBlasBlock + threadIdx.x;
            if (pos < begin || pos >= end) continue;
            const int64_t s = (int64_t)src_of_pos[pos];
            if (s < 0 || s >= num_triangles) continue;
            blas_bounds_tri(s, v1, v2, v3, box);
        }
    }
    for (int off = kBlasWave / 2; off > 0; off >>= 1) {
        float other[6];
        for (int k = 0; k < 6; k++) other[k] = __shfl_down(box[k], off, kBlasWave);
        blas_bounds_merge(box, other);
    }
    const int wave = threadIdx.x / kBlasWave;
    if (threadIdx.x % kBlasWave == 0)
        for (int k = 0; k < 6; k++) part[wave][k] = box[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlasBlock / kBlasWave; w++) blas_bounds_merge(box, part[w]);
        float* out = block_part + (int64_t)blockIdx.x * 6;
        for (int k = 0; k < 6; k++) out[k] = box[k];
    }
}

// blas_block_off: the blocks of BLAS b are [blas_block_off[b], blas_block_off[b + 1])
__global__ __launch_bounds__(kBlasBlock) void k_blas_bounds_fold(int64_t num_blas, int64_t num_blocks,
                                                                 const int32_t* __restrict__ desc,
                                                                 const int32_t* __restrict__ blas_block_off,
                                                                 const float* __restrict__ block_part, float* __restrict__ blas_box) {
    const int64_t b = (int64_t)blockIdx.x * kBlasBlock + threadIdx.x;
    if (b >= num_blas) return;
    float box[6];
    blas_bounds_empty(box);
    const int64_t lo = max((int64_t)blas_block_off[b], (int64_t)0), hi = min((int64_t)blas_block_off[b + 1], num_blocks);
    for (int64_t i = lo; i < hi; i++) blas_bounds_merge(box, block_part + i * 6);
    blas_bounds_finish((int64_t)desc[4 * b + 3], box);
    for (int k = 0; k < 6; k++) blas_box[b * 6 + k] = box[k];
}

__global__ __launch_bounds__(kBlasBlock) void k_blas_inner(int64_t num_transformed, int64_t num_blas,
                                                           const int32_t* __restrict__ xf_blas, const float* __restrict__ blas_box,
                                                           float* __restrict__ xf_inner_box) {
    const int64_t t = (int64_t)blockIdx.x * kBlasBlock + threadIdx.x;
    if (t >= num_transformed) return;
    const int64_t b = (int64_t)xf_blas[t];
    if (b < 0 || b >= num_blas) return;
    for (int k = 0; k < 6; k++) xf_inner_box[t * 6 + k] = blas_box[b * 6 + k];
}

__global__ __launch_bounds__(kBlasBlock) void k_blas_level(const uint32_t* __restrict__ level_nodes,
                                                           const int32_t* __restrict__ level_blas, int64_t count, int64_t num_blas,
                                                           const int32_t* __restrict__ desc, int64_t total_nodes, int64_t total_tris,
                                                           uint32_t* nodes, float* node_box, const float* __restrict__ tri_box) {
    const int64_t i = (int64_t)blockIdx.x * kBlasBlock + threadIdx.x;
    if (i >= count) return;
    const int64_t b = (int64_t)level_blas[i];
    if (b < 0 || b >= num_blas) return;
    const BlasDesc B{desc[4 * b], desc[4 * b + 1], desc[4 * b + 2], desc[4 * b + 3]};
    blas_refit_node((int64_t)level_nodes[i], B, total_nodes, total_tris, nodes, node_box, tri_box);
}

int64_t blas_bounds_span() { return kBlasSpan; }

// The BLAS refit on `stream`, up to the transformed shapes' inner boxes: launch_shape_refit carries them on.  The
// tables and the scratch are device memory; level_off (host) holds the levels' bounds, the roots' level first.
hipError_t launch_blas_refit(int64_t num_blas, int64_t num_pos, int64_t num_nodes, int64_t num_triangles, int64_t num_transformed,
                             int64_t num_blocks, int64_t num_levels, const uint32_t* level_off, const uint32_t* level_nodes,
                             const int32_t* level_blas, const int32_t* desc, const int32_t* src_of_pos, const int32_t* block_blas,
                             const int32_t* block_first, const int32_t* blas_block_off, const int32_t* xf_blas, uint32_t* nodes,
                             uint32_t* recs, uint32_t* shade, const float* v1, const float* v2, const float* v3, const float* n1,
                             const float* n2, const float* n3, float* tri_box, float* node_box, float* block_part, float* blas_box,
                             float* xf_inner_box, hipStream_t stream) {
    if (num_blas <= 0) return hipSuccess;
    const auto blocks = [](int64_t n) { return dim3((unsigned)((n + kBlasBlock - 1) / kBlasBlock)); };
    hipError_t e;
    if (num_pos > 0) {
        hipLaunchKernelGGL(k_blas_tris, blocks(num_pos), dim3(kBlasBlock), 0, stream, num_pos, num_triangles, recs, shade, src_of_pos,
                           v1, v2, v3, n1, n2, n3, tri_box);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (num_blocks > 0) {
        hipLaunchKernelGGL(k_blas_bounds, dim3((unsigned)num_blocks), dim3(kBlasBlock), 0, stream, num_pos, num_triangles, num_blas,
                           desc, block_blas, block_first, src_of_pos, v1, v2, v3, block_part);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_blas_bounds_fold, blocks(num_blas), dim3(kBlasBlock), 0, stream, num_blas, num_blocks, desc, blas_block_off,
                       block_part, blas_box);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (num_transformed > 0) {
        hipLaunchKernelGGL(k_blas_inner, blocks(num_transformed), dim3(kBlasBlock), 0, stream, num_transformed, num_blas, xf_blas,
                           blas_box, xf_inner_box);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    for (int64_t l = num_levels - 1; l >= 0; l--) {
        const int64_t count = (int64_t)level_off[l + 1] - (int64_t)level_off[l];
        if (count <= 0) continue;
        hipLaunchKernelGGL(k_blas_level, blocks(count), dim3(kBlasBlock), 0, stream, level_nodes + level_off[l],
                           level_blas + level_off[l], count, num_blas, desc, num_nodes, num_pos, nodes, node_box, tri_box);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace pt
