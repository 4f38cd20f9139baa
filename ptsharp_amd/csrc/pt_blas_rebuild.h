// pt_blas_rebuild.h — the arithmetic of pt_rebuild_blas and pt_blas_cost, shared by the device kernels
// (pt_blas_rebuild.hip) and the host (tests/native/blas_rebuild_check.cpp drives the same functions): every function
// is `__host__ __device__ inline`, makes no HIP call and compiles with g++.  Build with -ffp-contract=off.  The twin
// of pt_rebuild.h for the object-space BVH4 of an instanced mesh (pt_blas_refit.h).
//
// A rebuild replaces the topology of one BLAS by a balanced object-median tree whose shape depends on its number of
// triangles n alone:
//   leaves  leaf j holds positions 4 j .. min(4 j + 4, n) - 1, its ref 0x80000000 | (cnt - 1) << 29 | 4 j (relative to
//           the BLAS's rec_off); L = ceil(n / 4) leaves.
//   nodes   h = the least integer >= 1 with 4 * 4^h >= n levels.  The deepest level h - 1 has ceil(L / 4) nodes with
//           leaf refs only; every level above groups 4 consecutive nodes of the level below.  Nodes are numbered level
//           by level from the root, relative to node_off, so a child's index exceeds its parent's (shape_refit_node
//           needs that).  Unused slots are kEmpty4 with zero box words (collapse_bvh4's); words 28-31 are 0.
//   order   from the current order, rounds s = 2 h .. 1 over segments of 4 << s positions counted from the BLAS's
//           first position: a segment that holds more than 4 << (s - 1) triangles is sorted, stable and ascending, by
//           rebuild_ordered(min3 + max3) of the axis whose keys span the largest fp32 extent over the segment (ties:
//           the lowest axis): pt_rebuild.h's rebuild_keys and rebuild_axis.  A smaller segment keeps its order.
// Boxes and records then come from the BLAS refit (pt_blas_refit.h) over the new order.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "pt_rebuild.h"      // rebuild_keys, rebuild_axis, rebuild_ordered, rebuild_box_area
#include "pt_blas_refit.h"   // kShapeNodeWords, kShapeEmpty

namespace pt {

constexpr int kBlasRebuildMaxLevels = 10;   // 3 pushes per level: 30 <= kStack4Budget (pt_bvh.h)

struct BlasPlan {
    int64_t n;            // triangles
    int32_t h;            // levels (0: no tree)
    int64_t num_leaves, num_nodes;
};

// nodes of level l (0: the root) of a plan with L leaves and h levels, and the first node of that level
__host__ __device__ inline int64_t blas_rebuild_level_count(int64_t L, int h, int l) {
    const int sh = 2 * (h - l);
    return (L + ((int64_t)1 << sh) - 1) >> sh;
}
__host__ __device__ inline int64_t blas_rebuild_level_off(int64_t L, int h, int l) {
    int64_t at = 0;
    for (int m = 0; m < l; m++) at += blas_rebuild_level_count(L, h, m);
    return at;
}

// false: n needs more than kBlasRebuildMaxLevels levels (or is negative); n == 0 gives an empty plan
__host__ __device__ inline bool blas_rebuild_plan(int64_t n, BlasPlan& R) {
    R.n = n;
    R.h = 0;
    R.num_leaves = R.num_nodes = 0;
    if (n < 0) return false;
    if (n == 0) return true;
    int h = 1;
    int64_t cap = 16;
    while (cap < n) {
        if (++h > kBlasRebuildMaxLevels) return false;
        cap *= 4;
    }
    R.h = h;
    R.num_leaves = (n + 3) / 4;
    R.num_nodes = blas_rebuild_level_off(R.num_leaves, h, h);
    return true;
}

// the worst root-to-leaf sum of (children - 1): a traversal's stack need
__host__ __device__ inline int blas_rebuild_stack_bound(const BlasPlan& R) { return 3 * R.h; }

// the ref of leaf j
__host__ __device__ inline uint32_t blas_rebuild_leaf_ref(int64_t j, int64_t n) {
    const int64_t left = n - 4 * j;
    const uint32_t cnt = left < 4 ? (uint32_t)left : 4u;
    return 0x80000000u | ((cnt - 1u) << 29) | (uint32_t)(4 * j);
}

// words 24..27 of node ni (relative to the BLAS)
__host__ __device__ inline void blas_rebuild_node_refs(const BlasPlan& R, int64_t ni, uint32_t refs[4]) {
    int l = 0;
    int64_t off = 0;
    while (l + 1 < R.h && ni >= off + blas_rebuild_level_count(R.num_leaves, R.h, l)) {
        off += blas_rebuild_level_count(R.num_leaves, R.h, l);
        l++;
    }
    const int64_t j = ni - off;
    const bool deepest = l == R.h - 1;
    const int64_t below = deepest ? R.num_leaves : blas_rebuild_level_count(R.num_leaves, R.h, l + 1);
    const int64_t below_off = off + blas_rebuild_level_count(R.num_leaves, R.h, l);
    for (int k = 0; k < 4; k++) {
        const int64_t c = 4 * j + k;
        if (c >= below) refs[k] = kShapeEmpty;
        else if (deepest) refs[k] = blas_rebuild_leaf_ref(c, R.n);
        else refs[k] = (uint32_t)(below_off + c);
    }
}

// All eight topology words of node ni into its line, and zero box words for its empty slots (the refit leaves empty
// slots alone).  w: the node's kShapeNodeWords words.
__host__ __device__ inline void blas_rebuild_node_write(const BlasPlan& R, int64_t ni, uint32_t* w) {
    uint32_t refs[4];
    blas_rebuild_node_refs(R, ni, refs);
    for (int k = 0; k < 4; k++)
        if (refs[k] == kShapeEmpty)
            for (int ax = 0; ax < 3; ax++) { w[8 * ax + k] = 0u; w[8 * ax + 4 + k] = 0u; }
    RefitRow* r = (RefitRow*)w;
    r[6] = RefitRow{refs[0], refs[1], refs[2], refs[3]};
    r[7] = RefitRow{0u, 0u, 0u, 0u};
}

// ---- the order
// the first shift of a plan; shifts run from it down to 1
__host__ __device__ inline int blas_rebuild_first_shift(const BlasPlan& R) { return 2 * R.h; }
// the first position (relative to the BLAS) of the segment of position q in the round of shift s
__host__ __device__ inline int64_t blas_rebuild_segment_first(int64_t q, int s) { return (q >> (s + 2)) << (s + 2); }
// whether the segment that starts at `first` is sorted in that round: it holds more than half a segment's positions
__host__ __device__ inline bool blas_rebuild_segment_sorted(int64_t first, int s, int64_t n) {
    const int64_t seg = (int64_t)4 << s;
    const int64_t cnt = (first + seg < n ? first + seg : n) - first;
    return cnt > seg / 2;
}
// whether the round of shift s sorts anything in a BLAS of n triangles
__host__ __device__ inline bool blas_rebuild_round_sorts(int64_t n, int s) { return n > ((int64_t)2 << s); }

// ---- pt_blas_cost: a node's slot boxes are plain fp32, widened to fp64
// the areas of node w's inner slots and leaf slots summed, and the area of the union of its slot boxes
__host__ __device__ inline void blas_node_cost(const uint32_t* w, double* inner, double* leaf, double* own) {
    double ulo[3] = {INFINITY, INFINITY, INFINITY}, uhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double si = 0.0, sl = 0.0;
    bool any = false;
    for (int k = 0; k < 4; k++) {
        const uint32_t ref = w[24 + k];
        if (ref == kShapeEmpty) continue;
        any = true;
        double lo[3], hi[3];
        for (int ax = 0; ax < 3; ax++) {
            lo[ax] = (double)refit_float(w[8 * ax + k]);
            hi[ax] = (double)refit_float(w[8 * ax + 4 + k]);
            ulo[ax] = fmin(ulo[ax], lo[ax]);
            uhi[ax] = fmax(uhi[ax], hi[ax]);
        }
        const double a = rebuild_box_area(lo, hi);
        if (ref & 0x80000000u) sl += a; else si += a;
    }
    *inner = si;
    *leaf = sl;
    *own = any ? rebuild_box_area(ulo, uhi) : 0.0;
}
// out[0..2] of pt_blas_cost from a BLAS's sums and its root's own area
__host__ __device__ inline void blas_cost_finish(double inner, double leaf, double area, double out[3]) {
    out[0] = out[1] = 0.0;
    out[2] = area;
    if (area > 0.0) {
        out[0] = (area + inner) / area;
        out[1] = leaf / area;
    }
}

}  // namespace pt
