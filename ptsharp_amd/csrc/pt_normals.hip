// pt_normals.hip — the kernels of pt_update_triangles_normals and pt_read_tri_normals (gfx950): the normals of
// moved triangles computed on the device from the staged positions, the arithmetic in pt_normals.h (shared with the
// host check).
//   k_normals_face      one thread per source triangle: its face normal into its three slots of the staged
//                       normal arrays.  PT_NORMALS_FACE ends here.
//   k_normals_keys      one thread per corner position: word w of the key of the corner at that position (the
//                       corners in corner order before the first pass).
//   (the sort)          four stable least-significant-digit passes of rocPRIM's device radix sort over {key word,
//                       corner}: z, y, x, then the group, of which only the bits a mesh index needs are sorted.
//                       Equal keys stay in corner order.
//   k_normals_segments  one thread per sorted position: the first corner of a run of equal keys sums the run in
//                       order, normalises and writes every corner of the run.  A run is walked by one thread.
//   k_normals_gather    pt_read_tri_normals: one thread per BVH position, rows 3-5 of its shading record to its
//                       source triangle's slots.
// Every store is a plain vector store, every index 64-bit; the sums are ordered: no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

#include "pt_normals.h"

namespace pt {

constexpr int kNormalsBlock = 256;

__global__ __launch_bounds__(kNormalsBlock) void k_normals_face(int64_t n, const float* __restrict__ v1, const float* __restrict__ v2,
                                                                const float* __restrict__ v3, float* __restrict__ n1,
                                                                float* __restrict__ n2, float* __restrict__ n3) {
    const int64_t t = (int64_t)blockIdx.x * kNormalsBlock + threadIdx.x;
    if (t >= n) return;
    float f[3];
    normals_face(v1 + 3 * t, v2 + 3 * t, v3 + 3 * t, f);
    for (int k = 0; k < 3; k++) { n1[3 * t + k] = f[k]; n2[3 * t + k] = f[k]; n3[3 * t + k] = f[k]; }
}

// order == nullptr: position i holds corner i, which is also written to `iota`
__global__ __launch_bounds__(kNormalsBlock) void k_normals_keys(int64_t total, int w, const uint32_t* __restrict__ order,
                                                                uint32_t* __restrict__ iota, const int32_t* __restrict__ group,
                                                                const float* __restrict__ v1, const float* __restrict__ v2,
                                                                const float* __restrict__ v3, uint32_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * kNormalsBlock + threadIdx.x;
    if (i >= total) return;
    const uint32_t c = order ? order[i] : (uint32_t)i;
    if (!order) iota[i] = c;
    keys[i] = normals_key_word(w, c, group, v1, v2, v3);
}

__global__ __launch_bounds__(kNormalsBlock) void k_normals_segments(int64_t total, const uint32_t* __restrict__ sorted,
                                                                    const int32_t* __restrict__ group, const float* __restrict__ v1,
                                                                    const float* __restrict__ v2, const float* __restrict__ v3,
                                                                    float* n1, float* n2, float* n3) {
    const int64_t i = (int64_t)blockIdx.x * kNormalsBlock + threadIdx.x;
    if (i >= total) return;
    normals_segment(i, total, sorted, group, v1, v2, v3, n1, n2, n3);
}

__global__ __launch_bounds__(kNormalsBlock) void k_normals_gather(int64_t num_pos, const uint32_t* __restrict__ recs,
                                                                  const int32_t* __restrict__ src_of_pos, float* __restrict__ n1,
                                                                  float* __restrict__ n2, float* __restrict__ n3) {
    const int64_t pos = (int64_t)blockIdx.x * kNormalsBlock + threadIdx.x;
    if (pos >= num_pos) return;
    const uint32_t* r = recs + pos * 32 + 12;   // rows 3-5: n1, n2, n3, then the material word
    const int64_t s = (int64_t)src_of_pos[pos];
    for (int k = 0; k < 3; k++) {
        n1[3 * s + k] = __uint_as_float(r[k]);
        n2[3 * s + k] = __uint_as_float(r[3 + k]);
        n3[3 * s + k] = __uint_as_float(r[6 + k]);
    }
}

namespace {
dim3 normals_blocks(int64_t n) { return dim3((unsigned)((n + kNormalsBlock - 1) / kNormalsBlock)); }
// bits that hold every group word 0..num_groups
unsigned normals_group_bits(int32_t num_groups) {
    unsigned b = 1;
    while (b < 32 && ((uint64_t)1 << b) <= (uint64_t)num_groups) b++;
    return b;
}
}  // namespace

// The sort's temporary for `corners` pairs (the largest of its passes).
hipError_t normals_sort_temp_bytes(int64_t corners, int32_t num_groups, size_t* out) {
    *out = 0;
    rocprim::double_buffer<uint32_t> keys(nullptr, nullptr), vals(nullptr, nullptr);
    for (unsigned bits : {32u, normals_group_bits(num_groups)}) {
        size_t b = 0;
        const hipError_t e = rocprim::radix_sort_pairs(nullptr, b, keys, vals, (size_t)corners, 0u, bits, (hipStream_t) nullptr);
        if (e != hipSuccess) return e;
        if (b > *out) *out = b;
    }
    return hipSuccess;
}

// Face normals of the n staged triangles into n1..n3 on `stream`; with smooth, Mesh.SmoothNormals per group after
// them.  keys_a .. vals_b: 3 n words each; temp: normals_sort_temp_bytes.
hipError_t launch_normals(bool smooth, int64_t n, const float* v1, const float* v2, const float* v3, float* n1, float* n2,
                          float* n3, const int32_t* group, int32_t num_groups, uint32_t* keys_a, uint32_t* keys_b,
                          uint32_t* vals_a, uint32_t* vals_b, void* temp, size_t temp_bytes, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_normals_face, normals_blocks(n), dim3(kNormalsBlock), 0, stream, n, v1, v2, v3, n1, n2, n3);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !smooth) return e;
    const int64_t total = 3 * n;
    rocprim::double_buffer<uint32_t> keys(keys_a, keys_b), vals(vals_a, vals_b);
    for (int w = 0; w < 4; w++) {
        hipLaunchKernelGGL(k_normals_keys, normals_blocks(total), dim3(kNormalsBlock), 0, stream, total, w,
                           w ? (const uint32_t*)vals.current() : (const uint32_t*)nullptr, w ? (uint32_t*)nullptr : vals.current(),
                           group, v1, v2, v3, keys.current());
        if ((e = hipGetLastError()) != hipSuccess) return e;
        size_t bytes = temp_bytes;
        e = rocprim::radix_sort_pairs(temp, bytes, keys, vals, (size_t)total, 0u, w == 3 ? normals_group_bits(num_groups) : 32u, stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_normals_segments, normals_blocks(total), dim3(kNormalsBlock), 0, stream, total,
                       (const uint32_t*)vals.current(), group, v1, v2, v3, n1, n2, n3);
    return hipGetLastError();
}

hipError_t launch_normals_gather(int64_t num_pos, const uint32_t* recs, const int32_t* src_of_pos, float* n1, float* n2,
                                 float* n3, hipStream_t stream) {
    if (num_pos <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_normals_gather, normals_blocks(num_pos), dim3(kNormalsBlock), 0, stream, num_pos, recs, src_of_pos, n1,
                       n2, n3);
    return hipGetLastError();
}

}  // namespace pt
