// pt_rebuild.h — the arithmetic of pt_rebuild_meshes and pt_tri_bvh_cost, shared by the device kernels
// (pt_rebuild.hip) and the host (tests/native/rebuild_check.cpp drives the same functions): every function is
// `__host__ __device__ inline`, makes no HIP call and compiles with g++.  Build with -ffp-contract=off.
//
// A rebuild replaces the topology of the 8-wide quantized triangle BVH (pt_bvh.h Bvh8Result) by a balanced
// object-median tree whose shape depends on the number of positions P alone:
//   chunks  chunk ci holds positions 3 ci .. min(3 ci + 3, P) - 1; L = ceil(P / 3) chunks.
//   nodes   h = the least integer >= 1 with 3 * 8^h >= P levels.  The deepest level h - 1 has ceil(L / 8) nodes, node j
//           there with leaf slots for chunks 8 j .. min(8 j + 8, L) - 1; every level above groups 8 consecutive nodes
//           of the level below.  Nodes are numbered level by level, the root 0, so a child's index exceeds its
//           parent's.  A node without leaf slots has word 5 = 0x80000000 and word 6 = 0.
//   order   from the current order, rounds r = 1 .. 3 h over segments of C_(r-1) = 3 * 8^h / 2^(r-1) positions: a
//           segment that holds more than C_r triangles is sorted, stable and ascending, by the key min3 + max3 (one
//           fp32 addition) of the axis whose keys span the largest fp32 extent over the segment (ties: the lowest
//           axis), compared as rebuild_ordered of its bits.
// Boxes, quantization, records and chunk lines then come from the refit (pt_refit.h) over the new order.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "pt_refit.h"

namespace pt {

constexpr int kRebuildMaxLevels = 9;   // 7 pushes per level: 63 <= kStackMax (pt_bvh.h)

struct RebuildPlan {
    int64_t P;                                   // positions
    int32_t h;                                   // levels
    int64_t num_chunks, num_nodes;
    int64_t level_off[kRebuildMaxLevels + 1];    // level l (0: the root) is nodes [level_off[l], level_off[l + 1])
};

// false: P needs more than kRebuildMaxLevels levels (or is negative); P == 0 gives an empty plan
__host__ __device__ inline bool rebuild_plan(int64_t P, RebuildPlan& R) {
    R.P = P;
    R.h = 0;
    R.num_chunks = R.num_nodes = 0;
    for (int l = 0; l <= kRebuildMaxLevels; l++) R.level_off[l] = 0;
    if (P < 0) return false;
    if (P == 0) return true;
    int h = 1;
    int64_t cap = 24;
    while (cap < P) {
        if (++h > kRebuildMaxLevels) return false;
        cap *= 8;
    }
    R.h = h;
    R.num_chunks = (P + 2) / 3;
    int64_t count[kRebuildMaxLevels];
    int64_t n = R.num_chunks;
    for (int l = h - 1; l >= 0; l--) { n = (n + 7) / 8; count[l] = n; }
    for (int l = 0; l < h; l++) R.level_off[l + 1] = R.level_off[l] + count[l];
    for (int l = h; l < kRebuildMaxLevels; l++) R.level_off[l + 1] = R.level_off[h];
    R.num_nodes = R.level_off[h];
    return true;
}

// the worst root-to-leaf sum of (children - 1): a traversal's stack need
__host__ __device__ inline int rebuild_stack_bound(const RebuildPlan& R) { return 7 * R.h; }

// word 0 of chunk ci
__host__ __device__ inline uint32_t rebuild_chunk_word0(int64_t ci, int64_t P) {
    const int64_t left = P - 3 * ci;
    const uint32_t cnt = left < 3 ? (uint32_t)left : 3u;
    return (uint32_t)(3 * ci) | ((cnt - 1u) << 29);
}

// words 3..7 of node ni (word 3's bits 0-23, the exponents, are the refit's: 0 here)
__host__ __device__ inline void rebuild_node_words(const RebuildPlan& R, int64_t ni, uint32_t out[5]) {
    int l = 0;
    while (l + 1 < R.h && ni >= R.level_off[l + 1]) l++;
    const int64_t j = ni - R.level_off[l];
    if (l == R.h - 1) {   // leaf slots: chunks 8 j ..
        const int64_t left = R.num_chunks - 8 * j;
        const int nc = left < 8 ? (int)left : 8;
        uint32_t cnt_bits = 0;
        for (int k = 0; k < 8; k++)
            if (k < nc) cnt_bits |= (rebuild_chunk_word0(8 * j + k, R.P) >> 29) << (2 * k);
        out[0] = (uint32_t)nc << 28;
        out[1] = 0u;
        out[2] = 0x80000000u + (uint32_t)(8 * j);
        out[3] = cnt_bits;
    } else {
        const int64_t below = R.level_off[l + 2] - R.level_off[l + 1];
        const int64_t left = below - 8 * j;
        const int nc = left < 8 ? (int)left : 8;
        out[0] = ((uint32_t)nc << 28) | ((uint32_t)nc << 24);
        out[1] = (uint32_t)(R.level_off[l + 1] + 8 * j);
        out[2] = 0x80000000u;
        out[3] = 0u;
    }
    out[4] = 0u;
}

// ---- the order
// rounds of a plan; round r = 1 .. rounds sorts segments of rebuild_segment(R, r) positions that hold more than half
// of that.  A round with P <= half a segment sorts nothing.
__host__ __device__ inline int rebuild_rounds(const RebuildPlan& R) { return 3 * R.h; }
// C_(r-1) = 3 << rebuild_shift(R, r)
__host__ __device__ inline int rebuild_shift(const RebuildPlan& R, int r) { return 3 * R.h - r + 1; }
__host__ __device__ inline int64_t rebuild_segment(const RebuildPlan& R, int r) { return (int64_t)3 << rebuild_shift(R, r); }
__host__ __device__ inline bool rebuild_round_sorts(const RebuildPlan& R, int r) { return R.P > rebuild_segment(R, r) / 2; }
// the segment of position p in a round of shift s (p < 2^31)
__host__ __device__ inline uint32_t rebuild_segment_of(int64_t p, int s) { return (uint32_t)(p >> s) / 3u; }
// whether segment j of that round is sorted: it holds more than half a segment's positions
__host__ __device__ inline bool rebuild_segment_sorted(uint32_t j, int s, int64_t P) {
    const int64_t seg = (int64_t)3 << s, first = (int64_t)j * seg;
    const int64_t cnt = (first + seg < P ? first + seg : P) - first;
    return cnt > seg / 2;
}

// key bits in an order that compares as the floats do (-0 below +0), and back
__host__ __device__ inline uint32_t rebuild_ordered(uint32_t u) { return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__host__ __device__ inline uint32_t rebuild_unordered(uint32_t o) { return o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
// the three ordered keys of a triangle: min3 + max3 per axis on the raw vertices
__host__ __device__ inline void rebuild_keys(const float* v1, const float* v2, const float* v3, uint32_t out[3]) {
    for (int k = 0; k < 3; k++) {
        const float lo = fminf(fminf(v1[k], v2[k]), v3[k]);
        const float hi = fmaxf(fmaxf(v1[k], v2[k]), v3[k]);
        out[k] = rebuild_ordered(refit_bits(lo + hi));
    }
}
// the axis of a segment from its bounds {min x, y, z, max x, y, z} as ordered keys: the largest fp32 extent, ties to
// the lowest axis (a comparison with a NaN extent is false: still an axis in 0..2)
__host__ __device__ inline int rebuild_axis(const uint32_t b[6]) {
    float ext[3];
    for (int k = 0; k < 3; k++) ext[k] = refit_float(rebuild_unordered(b[3 + k])) - refit_float(rebuild_unordered(b[k]));
    int ax = 0;
    if (ext[1] > ext[ax]) ax = 1;
    if (ext[2] > ext[ax]) ax = 2;
    return ax;
}

// ---- pt_tri_bvh_cost: a node's slot boxes decoded in fp64 as origin + q 2^(e - 127)
__host__ __device__ inline double rebuild_half_value(uint32_t h16) {   // the integers refit_half_of_int makes
    h16 &= 0xFFFFu;
    if (h16 == 0) return 0.0;
    const int e = (int)(h16 >> 10) - 15;
    return (double)((1u << 10) | (h16 & 0x3FFu)) * refit_pow2(e - 10);
}
__host__ __device__ inline double rebuild_box_area(const double lo[3], const double hi[3]) {
    const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    return 2.0 * (dx * dy + dy * dz + dz * dx);
}
// the areas of node w's inner slots and leaf slots summed, and the area of the union of its slot boxes
__host__ __device__ inline void rebuild_node_cost(const uint32_t* w, double* inner, double* leaf, double* own) {
    const int nc = (int)(w[3] >> 28), nin = (int)((w[3] >> 24) & 15u);
    double ulo[3] = {INFINITY, INFINITY, INFINITY}, uhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double si = 0.0, sl = 0.0;
    for (int k = 0; k < 8; k++) {
        if (k >= nc) continue;
        double lo[3], hi[3];
        for (int ax = 0; ax < 3; ax++) {
            const double o = (double)refit_float(w[ax]);
            const double step = refit_pow2((int)((w[3] >> (8 * ax)) & 0xFFu) - 127);
            lo[ax] = o + rebuild_half_value(w[8 + 8 * ax + k / 2] >> (16 * (k & 1))) * step;
            hi[ax] = o + rebuild_half_value(w[12 + 8 * ax + k / 2] >> (16 * (k & 1))) * step;
            ulo[ax] = fmin(ulo[ax], lo[ax]);
            uhi[ax] = fmax(uhi[ax], hi[ax]);
        }
        const double a = rebuild_box_area(lo, hi);
        if (k < nin) si += a; else sl += a;
    }
    *inner = si;
    *leaf = sl;
    *own = nc > 0 ? rebuild_box_area(ulo, uhi) : 0.0;
}

}  // namespace pt
