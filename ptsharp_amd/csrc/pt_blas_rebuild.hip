// pt_blas_rebuild.hip — the kernels of pt_rebuild_blas and pt_blas_cost (gfx950): every instanced mesh's BLAS
// re-sorted into the balanced object-median tree of pt_blas_rebuild.h, the arithmetic shared with the
// host check.
//   (keys)               pt_rebuild.hip's k_rebuild_tri_keys over the BLAS positions: three ordered keys per position,
//                        formed once, and the position itself as the sort's value.
//   per shift s above the tail's, over all BLASes with 2 h >= s at once:
//   k_blasrb_bounds_init / k_blasrb_bounds
//                        the segments' key bounds, kept at the segment's first position.  A wave whose lanes all fall
//                        in one segment folds across its lanes and issues one set of atomicMin / atomicMax, else every
//                        lane issues its own.  min and max are exact: the result does not depend on the arrival order.
//   k_blasrb_sort_keys   (global first position of the segment << 32) | the ordered key of the segment's axis, the key
//                        0 where the segment keeps its order (a BLAS that takes no part is one such segment).
//   (the sort)           rocPRIM's stable device radix sort over the bits in use.
//   k_blasrb_tail        one workgroup per segment of at most kBlasTailMax positions: keys and positions into LDS,
//                        every remaining round there (bounds by a wave fold and LDS atomics, the axis, one bitonic
//                        network over (sub-segment, key, current rank), so the result is the stable order), the final
//                        permutation written once.
//   k_blasrb_gather / k_blasrb_store
//                        blas_shade's three rows, blas_uv's two and the source triangle, through a scratch copy.
//   k_blasrb_topology    node words 24-31 and the empty slots' box words of every rebuilt BLAS.
// The BLAS refit (pt_blas_refit.hip) then writes every box and record row.
//   k_blas_cost_nodes / k_blas_cost_sum
//                        pt_blas_cost: one thread per node, its slot areas in fp64; one block per BLAS sums them in a
//                        fixed order.
// Every store is a plain vector store, every index 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "pt_blas_rebuild.h"

namespace pt {

// pt_rebuild.hip
hipError_t launch_rebuild_tri_keys(int64_t P, const int32_t* src_of_pos, const float* v1, const float* v2, const float* v3,
                                   uint32_t* keys3, uint32_t* vals, hipStream_t stream);

constexpr int kBlasRbBlock = 256;
constexpr int kBlasTailMax = 1024;                            // positions one workgroup sorts in LDS
constexpr int kBlasTailPer = kBlasTailMax / kBlasRbBlock;     // per thread
constexpr int kBlasRbRows = 5;                                // blas_shade rows 0-2, blas_uv rows 0-1

// One BLAS as the rebuild sees it (four int32 each): h == 0 keeps its topology and its order
struct BlasRbItem {
    int32_t rec_off, n, h, node_off;
};

// the global first position of p's segment in the round of shift s, or -1 where p's BLAS takes no part
__device__ inline int64_t blasrb_segment(int64_t p, int s, const int32_t* __restrict__ pos_blas, const BlasRbItem* __restrict__ items,
                                         int64_t num_blas, int64_t* n_out, int64_t* r0_out) {
    const int64_t b = (int64_t)pos_blas[p];
    *n_out = 0;
    *r0_out = p;
    if (b < 0 || b >= num_blas) return -1;
    const BlasRbItem it = items[b];
    *n_out = it.n;
    *r0_out = it.rec_off;
    const int64_t q = p - (int64_t)it.rec_off;
    if (it.h <= 0 || 2 * it.h < s || q < 0 || q >= (int64_t)it.n) return -1;
    return (int64_t)it.rec_off + blas_rebuild_segment_first(q, s);
}

__global__ __launch_bounds__(kBlasRbBlock) void k_blasrb_bounds_init(int64_t P, int shift, int64_t num_blas,
                                                                     const int32_t* __restrict__ pos_blas,
                                                                     const BlasRbItem* __restrict__ items,
                                                                     uint32_t* __restrict__ bounds) {
    const int64_t p = (int64_t)blockIdx.x * kBlasRbBlock + threadIdx.x;
    if (p >= P) return;
    int64_t n, r0;
    if (blasrb_segment(p, shift, pos_blas, items, num_blas, &n, &r0) != p) return;
    for (int a = 0; a < 3; a++) { bounds[6 * p + a] = 0xFFFFFFFFu; bounds[6 * p + 3 + a] = 0u; }
}

// vals[p]: the start position of the triangle now at p (a value outside is clamped, so no access leaves keys3)
__global__ __launch_bounds__(kBlasRbBlock) void k_blasrb_bounds(int64_t P, int shift, int64_t num_blas,
                                                                const int32_t* __restrict__ pos_blas,
                                                                const BlasRbItem* __restrict__ items,
                                                                const uint32_t* __restrict__ vals,
                                                                const uint32_t* __restrict__ keys3, uint32_t* bounds) {
    const int64_t p = (int64_t)blockIdx.x * kBlasRbBlock + threadIdx.x;
    const bool live = p < P;
    int64_t n, r0;
    const int64_t f = blasrb_segment(live ? p : P - 1, shift, pos_blas, items, num_blas, &n, &r0);   // a lane past the end
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};                  // joins the last segment
    if (live && f >= 0) {
        int64_t t = (int64_t)vals[p];
        if (t >= P) t = P - 1;
        for (int a = 0; a < 3; a++) lo[a] = hi[a] = keys3[3 * t + a];
    }
    const int f32lo = (int)(uint32_t)f;   // f < 2^31, or -1
    if (__all(f32lo == __shfl(f32lo, 0))) {
        if (f < 0) return;
        for (int d = 1; d < 64; d <<= 1)
            for (int a = 0; a < 3; a++) {
                lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], d));
                hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], d));
            }
        if ((threadIdx.x & 63) == 0)
            for (int a = 0; a < 3; a++) { atomicMin(bounds + 6 * f + a, lo[a]); atomicMax(bounds + 6 * f + 3 + a, hi[a]); }
    } else if (live && f >= 0) {
        for (int a = 0; a < 3; a++) { atomicMin(bounds + 6 * f + a, lo[a]); atomicMax(bounds + 6 * f + 3 + a, hi[a]); }
    }
}

__global__ __launch_bounds__(kBlasRbBlock) void k_blasrb_sort_keys(int64_t P, int shift, int64_t num_blas,
                                                                   const int32_t* __restrict__ pos_blas,
                                                                   const BlasRbItem* __restrict__ items,
                                                                   const uint32_t* __restrict__ vals,
                                                                   const uint32_t* __restrict__ keys3,
                                                                   const uint32_t* __restrict__ bounds, uint64_t* __restrict__ keys) {
    const int64_t p = (int64_t)blockIdx.x * kBlasRbBlock + threadIdx.x;
    if (p >= P) return;
    int64_t n, r0;
    const int64_t f = blasrb_segment(p, shift, pos_blas, items, num_blas, &n, &r0);
    uint32_t key = 0u;
    if (f >= 0 && blas_rebuild_segment_sorted(f - r0, shift, n)) {
        uint32_t b[6];
        for (int a = 0; a < 6; a++) b[a] = bounds[6 * f + a];
        int64_t t = (int64_t)vals[p];
        if (t >= P) t = P - 1;
        key = keys3[3 * t + rebuild_axis(b)];
    }
    keys[p] = ((uint64_t)(f >= 0 ? f : r0) << 32) | (uint64_t)key;
}

// tail: four int32 per workgroup {global first position, count, starting shift, 0}
__global__ __launch_bounds__(kBlasRbBlock) void k_blasrb_tail(int64_t P, const int32_t* __restrict__ tail,
                                                              const uint32_t* __restrict__ keys3, uint32_t* vals) {
    __shared__ uint32_t k3[kBlasTailMax * 3];           // the three keys, by the triangle's rank at the load
    __shared__ uint32_t val[kBlasTailMax];              // its start position, by the same
    __shared__ uint32_t cur[kBlasTailMax];              // per local position: the rank at the load of the triangle there
    __shared__ uint64_t comp[kBlasTailMax];             // (sub-segment << 44) | (key << 12) | local position
    __shared__ uint32_t bnd[(kBlasTailMax / 8) * 6];    // per sub-segment: min x y z, max x y z
    const int64_t first = (int64_t)tail[4 * (int64_t)blockIdx.x];
    const int cnt = tail[4 * (int64_t)blockIdx.x + 1];
    const int s0 = tail[4 * (int64_t)blockIdx.x + 2];
    if (s0 < 1 || s0 > 8 || cnt < 1 || cnt > (4 << s0) || first < 0 || first + cnt > P) return;   // (uniform)
    const int size0 = 4 << s0;   // <= kBlasTailMax
    const int tid = (int)threadIdx.x;
    for (int e = 0; e < kBlasTailPer; e++) {
        const int l = e * kBlasRbBlock + tid;
        if (l >= cnt) continue;
        int64_t t = (int64_t)vals[first + l];
        if (t >= P) t = P - 1;
        val[l] = (uint32_t)t;
        cur[l] = (uint32_t)l;
        for (int a = 0; a < 3; a++) k3[3 * l + a] = keys3[3 * t + a];
    }
    __syncthreads();
    for (int s = s0; s >= 1; s--) {
        const int seg = 4 << s;
        const int nseg = (cnt + seg - 1) / seg;
        for (int j = tid; j < nseg; j += kBlasRbBlock)
            for (int a = 0; a < 3; a++) { bnd[6 * j + a] = 0xFFFFFFFFu; bnd[6 * j + 3 + a] = 0u; }
        __syncthreads();
        // a wave's 64 lanes hold 64 consecutive positions: aligned groups of min(seg, 64) lanes share a sub-segment
        const int width = seg < 64 ? seg : 64;
        for (int e = 0; e < kBlasTailPer; e++) {
            const int l = e * kBlasRbBlock + tid;
            if (e * kBlasRbBlock >= size0) break;   // (uniform)
            uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
            if (l < cnt) {
                const uint32_t c = cur[l];
                for (int a = 0; a < 3; a++) lo[a] = hi[a] = k3[3 * c + a];
            }
            for (int d = 1; d < width; d <<= 1)
                for (int a = 0; a < 3; a++) {
                    lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], d));
                    hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], d));
                }
            if ((l & (width - 1)) == 0 && l < cnt) {
                const int j = l >> (s + 2);
                for (int a = 0; a < 3; a++) { atomicMin(&bnd[6 * j + a], lo[a]); atomicMax(&bnd[6 * j + 3 + a], hi[a]); }
            }
        }
        __syncthreads();
        for (int e = 0; e < kBlasTailPer; e++) {
            const int l = e * kBlasRbBlock + tid;
            if (l >= size0) continue;
            uint64_t c = ((uint64_t)1 << 63) | (uint64_t)l;   // past the end: stays behind every triangle
            if (l < cnt) {
                const int j = l >> (s + 2);
                uint32_t key = 0u;
                if (blas_rebuild_segment_sorted((int64_t)j * seg, s, (int64_t)cnt)) {
                    uint32_t b[6];
                    for (int a = 0; a < 6; a++) b[a] = bnd[6 * j + a];
                    key = k3[3 * cur[l] + rebuild_axis(b)];
                }
                c = ((uint64_t)j << 44) | ((uint64_t)key << 12) | (uint64_t)l;
            }
            comp[l] = c;
        }
        __syncthreads();
        // every aligned block of seg entries ascending: bitonic, the last merge of each block upwards
        for (int k = 2; k <= seg; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < size0 / 2; i += kBlasRbBlock) {
                    const int a = 2 * j * (i / j) + (i % j), b = a + j;
                    const bool up = k == seg || (a & k) == 0;
                    const uint64_t x = comp[a], y = comp[b];
                    if ((x > y) == up) { comp[a] = y; comp[b] = x; }
                }
                __syncthreads();
            }
        uint32_t next[kBlasTailPer];
#pragma unroll
        for (int e = 0; e < kBlasTailPer; e++) {
            const int l = e * kBlasRbBlock + tid;
            next[e] = l < cnt ? cur[(uint32_t)(comp[l] & 0xFFFu) < (uint32_t)cnt ? (uint32_t)(comp[l] & 0xFFFu) : 0u] : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < kBlasTailPer; e++) {
            const int l = e * kBlasRbBlock + tid;
            if (l < cnt) cur[l] = next[e];
        }
        __syncthreads();
    }
    for (int e = 0; e < kBlasTailPer; e++) {
        const int l = e * kBlasRbBlock + tid;
        if (l < cnt) vals[first + l] = val[cur[l] < (uint32_t)cnt ? cur[l] : 0u];
    }
}

// one thread per (new position, row): scratch row and, with row 0, the source triangle.  uv may be NULL.
__global__ __launch_bounds__(kBlasRbBlock) void k_blasrb_gather(int64_t P, const uint32_t* __restrict__ vals,
                                                                const int32_t* __restrict__ src_of_pos,
                                                                const RefitRow* __restrict__ shade, const RefitRow* __restrict__ uv,
                                                                RefitRow* __restrict__ rows, int32_t* __restrict__ new_src) {
    const int64_t i = (int64_t)blockIdx.x * kBlasRbBlock + threadIdx.x;
    if (i >= P * kBlasRbRows) return;
    const int64_t p = i / kBlasRbRows;
    const int row = (int)(i - p * kBlasRbRows);
    int64_t t = (int64_t)vals[p];
    if (t >= P) t = P - 1;
    if (row < 3) rows[i] = shade[3 * t + row];
    else if (uv) rows[i] = uv[2 * t + (row - 3)];
    if (row == 0) new_src[p] = src_of_pos[t];
}

__global__ __launch_bounds__(kBlasRbBlock) void k_blasrb_store(int64_t P, const RefitRow* __restrict__ rows,
                                                               const int32_t* __restrict__ new_src, RefitRow* __restrict__ shade,
                                                               RefitRow* __restrict__ uv, int32_t* __restrict__ src_of_pos) {
    const int64_t i = (int64_t)blockIdx.x * kBlasRbBlock + threadIdx.x;
    if (i >= P * kBlasRbRows) return;
    const int64_t p = i / kBlasRbRows;
    const int row = (int)(i - p * kBlasRbRows);
    if (row < 3) shade[3 * p + row] = rows[i];
    else if (uv) uv[2 * p + (row - 3)] = rows[i];
    if (row == 0) src_of_pos[p] = new_src[p];
}

// blocks_per_blas blocks per BLAS: thread -> (BLAS, node relative to it)
__global__ __launch_bounds__(kBlasRbBlock) void k_blasrb_topology(int64_t num_blas, int64_t blocks_per_blas, int64_t total_nodes,
                                                                  const BlasRbItem* __restrict__ items, uint32_t* __restrict__ nodes) {
    const int64_t b = (int64_t)blockIdx.x / blocks_per_blas;
    const int64_t local = ((int64_t)blockIdx.x % blocks_per_blas) * kBlasRbBlock + threadIdx.x;
    if (b >= num_blas) return;
    const BlasRbItem it = items[b];
    if (it.h <= 0) return;
    BlasPlan R;
    if (!blas_rebuild_plan((int64_t)it.n, R) || local >= R.num_nodes) return;
    const int64_t g = (int64_t)it.node_off + local;
    if (it.node_off < 0 || g >= total_nodes) return;
    blas_rebuild_node_write(R, local, nodes + g * (int64_t)kShapeNodeWords);
}

// desc: BlasDesc per BLAS
__global__ __launch_bounds__(kBlasRbBlock) void k_blas_cost_nodes(int64_t num_blas, int64_t blocks_per_blas, int64_t total_nodes,
                                                                  const int32_t* __restrict__ desc, const uint32_t* __restrict__ nodes,
                                                                  double* __restrict__ inner, double* __restrict__ leaf) {
    const int64_t b = (int64_t)blockIdx.x / blocks_per_blas;
    const int64_t local = ((int64_t)blockIdx.x % blocks_per_blas) * kBlasRbBlock + threadIdx.x;
    if (b >= num_blas) return;
    const int64_t n0 = desc[4 * b], nn = desc[4 * b + 1];
    if (n0 < 0 || local >= nn || n0 + local >= total_nodes) return;
    double own;
    blas_node_cost(nodes + (n0 + local) * (int64_t)kShapeNodeWords, inner + n0 + local, leaf + n0 + local, &own);
}

// one block per BLAS: thread t adds nodes t, t + 256, ... in that order, then the block's partials fold pairwise
__global__ __launch_bounds__(kBlasRbBlock) void k_blas_cost_sum(int64_t num_blas, int64_t total_nodes, const int32_t* __restrict__ desc,
                                                                const uint32_t* __restrict__ nodes, const double* __restrict__ inner,
                                                                const double* __restrict__ leaf, double* __restrict__ out) {
    __shared__ double si[kBlasRbBlock], sl[kBlasRbBlock];
    const int64_t b = (int64_t)blockIdx.x;
    const int64_t n0 = desc[4 * b], nn = desc[4 * b + 1];
    const bool ok = n0 >= 0 && nn > 0 && n0 + nn <= total_nodes;
    double a = 0.0, c = 0.0;
    if (ok)
        for (int64_t i = threadIdx.x; i < nn; i += kBlasRbBlock) { a += inner[n0 + i]; c += leaf[n0 + i]; }
    si[threadIdx.x] = a;
    sl[threadIdx.x] = c;
    __syncthreads();
    for (int d = kBlasRbBlock / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) { si[threadIdx.x] += si[threadIdx.x + d]; sl[threadIdx.x] += sl[threadIdx.x + d]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double ri = 0.0, rl = 0.0, area = 0.0, o[3];
        if (ok) blas_node_cost(nodes + n0 * (int64_t)kShapeNodeWords, &ri, &rl, &area);
        blas_cost_finish(si[0], sl[0], area, o);
        for (int k = 0; k < 3; k++) out[3 * b + k] = o[k];
    }
}

namespace {
dim3 blasrb_blocks(int64_t n) { return dim3((unsigned)((n + kBlasRbBlock - 1) / kBlasRbBlock)); }
size_t blasrb_up(size_t b) { return (b + 255) & ~(size_t)255; }
unsigned blasrb_bits(uint64_t max_value) {   // bits that hold 0..max_value
    unsigned b = 0;
    while (b < 32 && (max_value >> b) != 0) b++;
    return b;
}
}  // namespace

int64_t blas_tail_max() { return kBlasTailMax; }

// The parts of a BLAS rebuild's workspace for P positions in num_blas BLASes, each 256-B aligned: [keys a b | vals a b |
// keys3 | bounds | rows | new_src | items | pos_blas | tail | the sort's temporary]
struct BlasRbDev {
    uint64_t* keys[2];
    uint32_t* vals[2];
    uint32_t* keys3;
    uint32_t* bounds;
    RefitRow* rows;
    int32_t* new_src;
    BlasRbItem* items;
    int32_t* pos_blas;
    int32_t* tail;
    void* temp;
    size_t temp_bytes, bytes;
};
static BlasRbDev blasrb_layout(int64_t num_blas, int64_t P, size_t temp_bytes, void* base) {
    BlasRbDev r{};
    size_t at = 0;
    char* p = (char*)base;
    const size_t n = (size_t)P, nb = (size_t)num_blas;
    for (int k = 0; k < 2; k++) { r.keys[k] = (uint64_t*)(p + at); at += blasrb_up(n * sizeof(uint64_t)); }
    for (int k = 0; k < 2; k++) { r.vals[k] = (uint32_t*)(p + at); at += blasrb_up(n * sizeof(uint32_t)); }
    r.keys3 = (uint32_t*)(p + at); at += blasrb_up(n * 3 * sizeof(uint32_t));
    r.bounds = (uint32_t*)(p + at); at += blasrb_up(n * 6 * sizeof(uint32_t));   // a segment's bounds sit at its first position
    r.rows = (RefitRow*)(p + at); at += blasrb_up(n * kBlasRbRows * sizeof(RefitRow));
    r.new_src = (int32_t*)(p + at); at += blasrb_up(n * sizeof(int32_t));
    r.items = (BlasRbItem*)(p + at); at += blasrb_up(nb * sizeof(BlasRbItem));
    r.pos_blas = (int32_t*)(p + at); at += blasrb_up(n * sizeof(int32_t));
    r.tail = (int32_t*)(p + at); at += blasrb_up((n / 64 + nb + 1) * 4 * sizeof(int32_t));   // the smallest tail has the most workgroups
    r.temp = p + at; at += blasrb_up(temp_bytes);
    r.temp_bytes = temp_bytes;
    r.bytes = at + 256;   // never an empty allocation
    return r;
}

// The sort's temporary for P pairs, and the whole workspace's size with it.
hipError_t blas_rebuild_workspace_bytes(int64_t num_blas, int64_t P, size_t* temp_bytes, size_t* bytes) {
    *temp_bytes = 0;
    rocprim::double_buffer<uint64_t> keys(nullptr, nullptr);
    rocprim::double_buffer<uint32_t> vals(nullptr, nullptr);
    for (unsigned end_bit = 32u; end_bit <= 64u; end_bit++) {   // the largest over the bit ranges a round may sort
        size_t b = 0;
        const hipError_t e = rocprim::radix_sort_pairs(nullptr, b, keys, vals, (size_t)P, 0u, end_bit, (hipStream_t) nullptr);
        if (e != hipSuccess) return e;
        if (b > *temp_bytes) *temp_bytes = b;
    }
    *bytes = blasrb_layout(num_blas, P, *temp_bytes, nullptr).bytes;
    return hipSuccess;
}

// What the first use puts into the workspace: each position's BLAS (host array of P int32, alive until the stream
// has run the copy).
hipError_t blas_rebuild_upload(void* ws, size_t temp_bytes, int64_t num_blas, int64_t P, const int32_t* pos_blas, hipStream_t stream) {
    if (P <= 0) return hipSuccess;
    const BlasRbDev D = blasrb_layout(num_blas, P, temp_bytes, ws);
    return hipMemcpyAsync(D.pos_blas, pos_blas, (size_t)P * sizeof(int32_t), hipMemcpyHostToDevice, stream);
}

// The whole re-sort on `stream`, before the BLAS refit: the order from src_of_pos and the vertices, blas_shade,
// blas_uv (may be NULL) and src_of_pos permuted, the topology of every BLAS with h > 0 written.  items: num_blas
// BlasRbItem, tail: blas_tail_table's rows (pt_update_layout.h) (host arrays, alive until the stream has run their copies).
hipError_t launch_blas_rebuild(void* ws, size_t temp_bytes, int64_t num_blas, int64_t P, int64_t total_nodes, const int32_t* items,
                               const int32_t* tail, int64_t num_tail, int64_t tail_T, uint32_t* nodes, uint32_t* shade, uint32_t* uv,
                               int32_t* src_of_pos, const float* v1, const float* v2, const float* v3, hipStream_t stream) {
    if (P <= 0 || num_blas <= 0) return hipSuccess;
    const BlasRbDev D = blasrb_layout(num_blas, P, temp_bytes, ws);
    if (num_tail > (int64_t)(P / 64 + num_blas + 1)) return hipErrorInvalidValue;
    hipError_t e;
    if ((e = hipMemcpyAsync(D.items, items, (size_t)num_blas * sizeof(BlasRbItem), hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
    if (num_tail > 0)
        if ((e = hipMemcpyAsync(D.tail, tail, (size_t)num_tail * 4 * sizeof(int32_t), hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
    rocprim::double_buffer<uint64_t> keys(D.keys[0], D.keys[1]);
    rocprim::double_buffer<uint32_t> vals(D.vals[0], D.vals[1]);
    if ((e = launch_rebuild_tri_keys(P, src_of_pos, v1, v2, v3, D.keys3, vals.current(), stream)) != hipSuccess) return e;
    // the global rounds: the shifts whose segments are larger than the tail
    int sT = 0;
    if (tail_T > 0) while (((int64_t)4 << sT) < tail_T) sT++;
    int s_max = 0;
    int64_t max_plan_nodes = 0;
    for (int64_t b = 0; b < num_blas; b++) {
        const int h = items[4 * b + 2];
        if (h <= 0) continue;
        s_max = 2 * h > s_max ? 2 * h : s_max;
        BlasPlan R;
        if (blas_rebuild_plan((int64_t)items[4 * b + 1], R) && R.num_nodes > max_plan_nodes) max_plan_nodes = R.num_nodes;
    }
    if (s_max == 0) return hipSuccess;   // every BLAS keeps its topology
    for (int s = s_max; s > sT; s--) {
        bool sorts = false;
        for (int64_t b = 0; b < num_blas && !sorts; b++)
            sorts = items[4 * b + 2] > 0 && 2 * items[4 * b + 2] >= s && blas_rebuild_round_sorts((int64_t)items[4 * b + 1], s);
        if (!sorts) continue;
        hipLaunchKernelGGL(k_blasrb_bounds_init, blasrb_blocks(P), dim3(kBlasRbBlock), 0, stream, P, s, num_blas,
                           (const int32_t*)D.pos_blas, (const BlasRbItem*)D.items, D.bounds);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_blasrb_bounds, blasrb_blocks(P), dim3(kBlasRbBlock), 0, stream, P, s, num_blas, (const int32_t*)D.pos_blas,
                           (const BlasRbItem*)D.items, (const uint32_t*)vals.current(), (const uint32_t*)D.keys3, D.bounds);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_blasrb_sort_keys, blasrb_blocks(P), dim3(kBlasRbBlock), 0, stream, P, s, num_blas,
                           (const int32_t*)D.pos_blas, (const BlasRbItem*)D.items, (const uint32_t*)vals.current(),
                           (const uint32_t*)D.keys3, (const uint32_t*)D.bounds, keys.current());
        if ((e = hipGetLastError()) != hipSuccess) return e;
        size_t bytes = D.temp_bytes;
        e = rocprim::radix_sort_pairs(D.temp, bytes, keys, vals, (size_t)P, 0u, 32u + blasrb_bits((uint64_t)P - 1), stream);
        if (e != hipSuccess) return e;
    }
    if (num_tail > 0) {
        hipLaunchKernelGGL(k_blasrb_tail, dim3((unsigned)num_tail), dim3(kBlasRbBlock), 0, stream, P, (const int32_t*)D.tail,
                           (const uint32_t*)D.keys3, vals.current());
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const int64_t moves = P * kBlasRbRows;
    hipLaunchKernelGGL(k_blasrb_gather, blasrb_blocks(moves), dim3(kBlasRbBlock), 0, stream, P, (const uint32_t*)vals.current(),
                       (const int32_t*)src_of_pos, (const RefitRow*)shade, (const RefitRow*)uv, D.rows, D.new_src);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_blasrb_store, blasrb_blocks(moves), dim3(kBlasRbBlock), 0, stream, P, (const RefitRow*)D.rows,
                       (const int32_t*)D.new_src, (RefitRow*)shade, (RefitRow*)uv, src_of_pos);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int64_t bpb = (max_plan_nodes + kBlasRbBlock - 1) / kBlasRbBlock;
    hipLaunchKernelGGL(k_blasrb_topology, dim3((unsigned)(bpb * num_blas)), dim3(kBlasRbBlock), 0, stream, num_blas, bpb, total_nodes,
                       (const BlasRbItem*)D.items, nodes);
    return hipGetLastError();
}

// pt_blas_cost on `stream`: out (device, 3 doubles per BLAS).  ws holds [inner | leaf], a double per node each:
// blas_cost_workspace_bytes.  desc: the device's BlasDesc rows; max_nodes: the largest node count among them.
size_t blas_cost_workspace_bytes(int64_t total_nodes) { return 2 * blasrb_up((size_t)total_nodes * sizeof(double)) + 256; }
hipError_t launch_blas_cost(int64_t num_blas, int64_t total_nodes, int64_t max_nodes, const int32_t* desc, const uint32_t* nodes,
                            void* ws, double* out, hipStream_t stream) {
    if (num_blas <= 0) return hipSuccess;
    double* inner = (double*)ws;
    double* leaf = (double*)((char*)ws + blasrb_up((size_t)total_nodes * sizeof(double)));
    const int64_t bpb = (max_nodes + kBlasRbBlock - 1) / kBlasRbBlock;
    if (bpb > 0) {
        hipLaunchKernelGGL(k_blas_cost_nodes, dim3((unsigned)(bpb * num_blas)), dim3(kBlasRbBlock), 0, stream, num_blas, bpb, total_nodes,
                           desc, nodes, inner, leaf);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_blas_cost_sum, dim3((unsigned)num_blas), dim3(kBlasRbBlock), 0, stream, num_blas, total_nodes, desc, nodes,
                       (const double*)inner, (const double*)leaf, out);
    return hipGetLastError();
}

}  // namespace pt
