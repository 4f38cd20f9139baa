// pt_rebuild.hip — the kernels of pt_rebuild_meshes and pt_tri_bvh_cost (gfx950): the world triangle BVH re-sorted
// into the balanced object-median tree of pt_rebuild.h, the arithmetic shared with the host check.
//   k_rebuild_tri_keys   one thread per position: its triangle's three ordered keys, and the position itself as the
//                        sort's value (the values name positions of the order the rebuild started from).
//   per round that sorts (pt_rebuild.h rebuild_round_sorts):
//   k_rebuild_bounds_init / k_rebuild_bounds
//                        the segments' key bounds.  A wave whose lanes all fall in one segment folds across its lanes
//                        and issues one set of atomicMin / atomicMax, else every lane issues its own.  min and max are
//                        exact and order-independent: the result does not depend on the arrival order.
//   k_rebuild_sort_keys  one thread per position: (segment << 32) | the ordered key of the segment's axis, the key 0
//                        in a segment that keeps its order.
//   (the sort)           rocPRIM's stable device radix sort over the bits in use.
//   k_rebuild_gather     rows 3-7 of the records (normals, material word, uv) and the source triangle, from each
//                        triangle's old position to a scratch copy in the new order;
//   k_rebuild_store      the scratch copy into the records and src_of_pos;
//   k_rebuild_topology   the nodes' words 3-7, the chunks' word 0, the level list.
// The refit (pt_refit.hip launch_refit) then writes every box, record row 0-2 and chunk line.
//   k_bvh_cost           pt_tri_bvh_cost: one thread per node, its slot areas in fp64; rocPRIM's reduce sums them.
// Every store is a plain vector store, every index 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce.hpp>

#include "pt_rebuild.h"

namespace pt {

constexpr int kRebuildBlock = 256;
constexpr int kRebuildRows = 5;   // rows 3-7 of a 128-B record move with their triangle

__global__ __launch_bounds__(kRebuildBlock) void k_rebuild_tri_keys(int64_t P, const int32_t* __restrict__ src_of_pos,
                                                                    const float* __restrict__ v1, const float* __restrict__ v2,
                                                                    const float* __restrict__ v3, uint32_t* __restrict__ keys3,
                                                                    uint32_t* __restrict__ vals) {
    const int64_t p = (int64_t)blockIdx.x * kRebuildBlock + threadIdx.x;
    if (p >= P) return;
    const int64_t s = (int64_t)src_of_pos[p];
    uint32_t k[3];
    rebuild_keys(v1 + 3 * s, v2 + 3 * s, v3 + 3 * s, k);
    for (int a = 0; a < 3; a++) keys3[3 * p + a] = k[a];
    vals[p] = (uint32_t)p;
}

__global__ __launch_bounds__(kRebuildBlock) void k_rebuild_bounds_init(int64_t num_segments, uint32_t* __restrict__ bounds) {
    const int64_t j = (int64_t)blockIdx.x * kRebuildBlock + threadIdx.x;
    if (j >= num_segments) return;
    for (int a = 0; a < 3; a++) { bounds[6 * j + a] = 0xFFFFFFFFu; bounds[6 * j + 3 + a] = 0u; }
}

// vals[p]: the start position of the triangle now at p (p < P: a value outside is clamped, so no access leaves keys3)
__global__ __launch_bounds__(kRebuildBlock) void k_rebuild_bounds(int64_t P, int shift, const uint32_t* __restrict__ vals,
                                                                  const uint32_t* __restrict__ keys3, uint32_t* bounds) {
    const int64_t p = (int64_t)blockIdx.x * kRebuildBlock + threadIdx.x;
    const bool live = p < P;
    const int64_t q = live ? p : P - 1;   // a lane past the end joins the last segment with neutral bounds
    const uint32_t j = rebuild_segment_of(q, shift);
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    if (live) {
        int64_t t = (int64_t)vals[p];
        if (t >= P) t = P - 1;
        for (int a = 0; a < 3; a++) lo[a] = hi[a] = keys3[3 * t + a];
    }
    const uint32_t j0 = (uint32_t)__shfl((int)j, 0);
    if (__all(j == j0)) {
        for (int d = 1; d < 64; d <<= 1)
            for (int a = 0; a < 3; a++) {
                lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], d));
                hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], d));
            }
        if ((threadIdx.x & 63) == 0)
            for (int a = 0; a < 3; a++) { atomicMin(bounds + 6 * (int64_t)j + a, lo[a]); atomicMax(bounds + 6 * (int64_t)j + 3 + a, hi[a]); }
    } else if (live) {
        for (int a = 0; a < 3; a++) { atomicMin(bounds + 6 * (int64_t)j + a, lo[a]); atomicMax(bounds + 6 * (int64_t)j + 3 + a, hi[a]); }
    }
}

__global__ __launch_bounds__(kRebuildBlock) void k_rebuild_sort_keys(int64_t P, int shift, const uint32_t* __restrict__ vals,
                                                                     const uint32_t* __restrict__ keys3,
                                                                     const uint32_t* __restrict__ bounds, uint64_t* __restrict__ keys) {
    const int64_t p = (int64_t)blockIdx.x * kRebuildBlock + threadIdx.x;
    if (p >= P) return;
    const uint32_t j = rebuild_segment_of(p, shift);
    uint32_t key = 0u;
    if (rebuild_segment_sorted(j, shift, P)) {
        uint32_t b[6];
        for (int a = 0; a < 6; a++) b[a] = bounds[6 * (int64_t)j + a];
        int64_t t = (int64_t)vals[p];
        if (t >= P) t = P - 1;
        key = keys3[3 * t + rebuild_axis(b)];
    }
    keys[p] = ((uint64_t)j << 32) | (uint64_t)key;
}

// one thread per (new position, row): scratch row and, with row 0, the source triangle
__global__ __launch_bounds__(kRebuildBlock) void k_rebuild_gather(int64_t P, const uint32_t* __restrict__ vals,
                                                                  const int32_t* __restrict__ src_of_pos,
                                                                  const uint32_t* __restrict__ recs, RefitRow* __restrict__ rows,
                                                                  int32_t* __restrict__ new_src) {
    const int64_t i = (int64_t)blockIdx.x * kRebuildBlock + threadIdx.x;
    if (i >= P * kRebuildRows) return;
    const int64_t p = i / kRebuildRows;
    const int row = (int)(i - p * kRebuildRows);
    int64_t t = (int64_t)vals[p];
    if (t >= P) t = P - 1;
    rows[i] = ((const RefitRow*)(recs + t * (int64_t)kRefitWords))[3 + row];
    if (row == 0) new_src[p] = src_of_pos[t];
}

__global__ __launch_bounds__(kRebuildBlock) void k_rebuild_store(int64_t P, const RefitRow* __restrict__ rows,
                                                                 const int32_t* __restrict__ new_src, uint32_t* __restrict__ recs,
                                                                 int32_t* __restrict__ src_of_pos) {
    const int64_t i = (int64_t)blockIdx.x * kRebuildBlock + threadIdx.x;
    if (i >= P * kRebuildRows) return;
    const int64_t p = i / kRebuildRows;
    const int row = (int)(i - p * kRebuildRows);
    ((RefitRow*)(recs + p * (int64_t)kRefitWords))[3 + row] = rows[i];
    if (row == 0) src_of_pos[p] = new_src[p];
}

// thread i: chunk i's word 0 and node i's words 3-7
__global__ __launch_bounds__(kRebuildBlock) void k_rebuild_topology(RebuildPlan R, uint32_t* __restrict__ nodes,
                                                                    uint32_t* __restrict__ chunks, uint32_t* __restrict__ level_nodes) {
    const int64_t i = (int64_t)blockIdx.x * kRebuildBlock + threadIdx.x;
    if (i < R.num_chunks) chunks[i * (int64_t)kRefitWords] = rebuild_chunk_word0(i, R.P);
    if (i < R.num_nodes) {
        uint32_t w[5];
        rebuild_node_words(R, i, w);
        uint32_t* n = nodes + i * (int64_t)kRefitWords;
        n[3] = w[0];
        ((RefitRow*)n)[1] = RefitRow{w[1], w[2], w[3], w[4]};
        level_nodes[i] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(kRebuildBlock) void k_bvh_cost(int64_t num_nodes, const uint32_t* __restrict__ nodes,
                                                            double* __restrict__ inner, double* __restrict__ leaf) {
    const int64_t i = (int64_t)blockIdx.x * kRebuildBlock + threadIdx.x;
    if (i >= num_nodes) return;
    double own;
    rebuild_node_cost(nodes + i * (int64_t)kRefitWords, inner + i, leaf + i, &own);
}

namespace {
dim3 rebuild_blocks(int64_t n) { return dim3((unsigned)((n + kRebuildBlock - 1) / kRebuildBlock)); }
size_t rebuild_up(size_t b) { return (b + 255) & ~(size_t)255; }
unsigned rebuild_bits(uint64_t max_value) {   // bits that hold 0..max_value
    unsigned b = 0;
    while (b < 32 && (max_value >> b) != 0) b++;
    return b;
}
}  // namespace

// The parts of a rebuild's workspace for P positions, each 256-B aligned: [keys a b | vals a b | keys3 | bounds | rows |
// new_src | the sort's temporary]
struct RebuildDev {
    uint64_t* keys[2];
    uint32_t* vals[2];
    uint32_t* keys3;
    uint32_t* bounds;
    RefitRow* rows;
    int32_t* new_src;
    void* temp;
    size_t temp_bytes, bytes;
};
static RebuildDev rebuild_layout(int64_t P, size_t temp_bytes, void* base) {
    RebuildDev r{};
    size_t at = 0;
    char* p = (char*)base;
    const size_t n = (size_t)P;
    for (int k = 0; k < 2; k++) { r.keys[k] = (uint64_t*)(p + at); at += rebuild_up(n * sizeof(uint64_t)); }
    for (int k = 0; k < 2; k++) { r.vals[k] = (uint32_t*)(p + at); at += rebuild_up(n * sizeof(uint32_t)); }
    r.keys3 = (uint32_t*)(p + at); at += rebuild_up(n * 3 * sizeof(uint32_t));
    r.bounds = (uint32_t*)(p + at); at += rebuild_up((n / 6 + 1) * 6 * sizeof(uint32_t));   // the last round has the most segments
    r.rows = (RefitRow*)(p + at); at += rebuild_up(n * kRebuildRows * sizeof(RefitRow));
    r.new_src = (int32_t*)(p + at); at += rebuild_up(n * sizeof(int32_t));
    r.temp = p + at; at += rebuild_up(temp_bytes);
    r.temp_bytes = temp_bytes;
    r.bytes = at + 256;   // never an empty allocation
    return r;
}

// k_rebuild_tri_keys on `stream` (pt_blas_rebuild.hip forms the keys of the BLAS positions with it)
hipError_t launch_rebuild_tri_keys(int64_t P, const int32_t* src_of_pos, const float* v1, const float* v2, const float* v3,
                                   uint32_t* keys3, uint32_t* vals, hipStream_t stream) {
    if (P <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rebuild_tri_keys, rebuild_blocks(P), dim3(kRebuildBlock), 0, stream, P, src_of_pos, v1, v2, v3, keys3, vals);
    return hipGetLastError();
}

// The sort's temporary for P pairs, and the whole workspace's size with it.
hipError_t rebuild_workspace_bytes(int64_t P, size_t* temp_bytes, size_t* bytes) {
    *temp_bytes = 0;
    rocprim::double_buffer<uint64_t> keys(nullptr, nullptr);
    rocprim::double_buffer<uint32_t> vals(nullptr, nullptr);
    for (unsigned end_bit = 32u; end_bit <= 64u; end_bit++) {   // the largest over the bit ranges a round may sort
        size_t b = 0;
        const hipError_t e = rocprim::radix_sort_pairs(nullptr, b, keys, vals, (size_t)P, 0u, end_bit, (hipStream_t) nullptr);
        if (e != hipSuccess) return e;
        if (b > *temp_bytes) *temp_bytes = b;
    }
    *bytes = rebuild_layout(P, *temp_bytes, nullptr).bytes;
    return hipSuccess;
}

// The whole re-sort on `stream`, before the refit: the order from src_of_pos and the vertices, the records' rows 3-7 and
// src_of_pos permuted, the topology of plan R and its level list written.  ws: rebuild_workspace_bytes(R.P).
hipError_t launch_rebuild(const RebuildPlan& R, void* ws, size_t temp_bytes, uint32_t* nodes, uint32_t* chunks, uint32_t* recs,
                          int32_t* src_of_pos, uint32_t* level_nodes, const float* v1, const float* v2, const float* v3,
                          hipStream_t stream) {
    const int64_t P = R.P;
    if (P <= 0) return hipSuccess;
    const RebuildDev D = rebuild_layout(P, temp_bytes, ws);
    rocprim::double_buffer<uint64_t> keys(D.keys[0], D.keys[1]);
    rocprim::double_buffer<uint32_t> vals(D.vals[0], D.vals[1]);
    hipError_t e;
    if ((e = launch_rebuild_tri_keys(P, src_of_pos, v1, v2, v3, D.keys3, vals.current(), stream)) != hipSuccess) return e;
    for (int r = 1; r <= rebuild_rounds(R); r++) {
        if (!rebuild_round_sorts(R, r)) continue;
        const int shift = rebuild_shift(R, r);
        const int64_t segments = (int64_t)rebuild_segment_of(P - 1, shift) + 1;
        hipLaunchKernelGGL(k_rebuild_bounds_init, rebuild_blocks(segments), dim3(kRebuildBlock), 0, stream, segments, D.bounds);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_rebuild_bounds, rebuild_blocks(P), dim3(kRebuildBlock), 0, stream, P, shift,
                           (const uint32_t*)vals.current(), (const uint32_t*)D.keys3, D.bounds);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_rebuild_sort_keys, rebuild_blocks(P), dim3(kRebuildBlock), 0, stream, P, shift,
                           (const uint32_t*)vals.current(), (const uint32_t*)D.keys3, (const uint32_t*)D.bounds, keys.current());
        if ((e = hipGetLastError()) != hipSuccess) return e;
        size_t bytes = D.temp_bytes;
        e = rocprim::radix_sort_pairs(D.temp, bytes, keys, vals, (size_t)P, 0u, 32u + rebuild_bits((uint64_t)segments - 1), stream);
        if (e != hipSuccess) return e;
    }
    const int64_t moves = P * kRebuildRows;
    hipLaunchKernelGGL(k_rebuild_gather, rebuild_blocks(moves), dim3(kRebuildBlock), 0, stream, P, (const uint32_t*)vals.current(),
                       (const int32_t*)src_of_pos, (const uint32_t*)recs, D.rows, D.new_src);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_rebuild_store, rebuild_blocks(moves), dim3(kRebuildBlock), 0, stream, P, (const RefitRow*)D.rows,
                       (const int32_t*)D.new_src, recs, src_of_pos);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_rebuild_topology, rebuild_blocks(R.num_chunks > R.num_nodes ? R.num_chunks : R.num_nodes), dim3(kRebuildBlock), 0, stream, R, nodes, chunks, level_nodes);
    return hipGetLastError();
}

// pt_tri_bvh_cost's sums on `stream`: sums[0] = Σ inner slot areas, sums[1] = Σ leaf slot areas (device doubles).
// ws holds [inner | leaf | the reduce's temporary]: bvh_cost_workspace_bytes.
static hipError_t bvh_cost_temp(int64_t num_nodes, size_t* temp) {
    *temp = 0;
    return rocprim::reduce(nullptr, *temp, (const double*)nullptr, (double*)nullptr, 0.0, (size_t)num_nodes, rocprim::plus<double>(),
                           (hipStream_t) nullptr);
}
hipError_t bvh_cost_workspace_bytes(int64_t num_nodes, size_t* bytes) {
    size_t temp = 0;
    const hipError_t e = bvh_cost_temp(num_nodes, &temp);
    *bytes = 2 * rebuild_up((size_t)num_nodes * sizeof(double)) + rebuild_up(temp) + 256;
    return e;
}
hipError_t launch_bvh_cost(int64_t num_nodes, const uint32_t* nodes, void* ws, double* sums, hipStream_t stream) {
    if (num_nodes <= 0) return hipSuccess;
    size_t temp = 0;
    hipError_t e = bvh_cost_temp(num_nodes, &temp);
    if (e != hipSuccess) return e;
    const size_t arr = rebuild_up((size_t)num_nodes * sizeof(double));
    double* inner = (double*)ws;
    double* leaf = (double*)((char*)ws + arr);
    void* tmp = (char*)ws + 2 * arr;
    hipLaunchKernelGGL(k_bvh_cost, rebuild_blocks(num_nodes), dim3(kRebuildBlock), 0, stream, num_nodes, nodes, inner, leaf);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = rocprim::reduce(tmp, temp, (const double*)inner, sums, 0.0, (size_t)num_nodes, rocprim::plus<double>(), stream);
    if (e != hipSuccess) return e;
    return rocprim::reduce(tmp, temp, (const double*)leaf, sums + 1, 0.0, (size_t)num_nodes, rocprim::plus<double>(), stream);
}

}  // namespace pt
