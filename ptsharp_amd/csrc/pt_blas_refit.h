// pt_blas_refit.h — the arithmetic of pt_update_meshes for instanced meshes, shared by the device kernels
// (pt_blas_refit.hip) and the host (tests/native/blas_check.cpp drives the same functions tris, bounds, levels):
// every function is `__host__ __device__ inline`, makes no HIP call and compiles with g++.  Build with
// -ffp-contract=off.
//
// A BLAS is the object-space BVH4 of one instanced mesh (pt_scene_compile.cpp Compiler::blases): plain fp32 child
// boxes in collapse_bvh4's format, the analytic BVH's, over the mesh's padded triangle boxes.  A BLAS refit keeps
// its topology and recomputes, from new vertices, what depends on coordinates:
//   blas_refit_tri     one BLAS triangle position: blas_recs rows 0-2 (pack_tri_geom), blas_shade rows 0-2 when
//                normals come along (pack_tri_shade, the material word kept), its padded box (tri_padded_box)
//   blas_bounds_tri    one triangle folded into an unpadded min / max box: Mesh.BoundingBox, the MESH case of
//                shape_box, the inner box of every transformed shape over the mesh
//   blas_refit_node    one node of one BLAS, after every node below it: shape_refit_node on the BLAS's own bases
//                (child references and leaf firsts inside a BLAS are relative to its node_off / rec_off)
// The host builder's BVH2 boxes are exact unions of the padded triangle boxes, and min / max are exact and
// associative, so a refit with the vertices a scene was built from reproduces every word; of the unpadded box every
// value (fminf(-0, +0) may be either zero: after mat_box and pad_box the bits agree again).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "pt_refit.h"         // RefitRow, refit_tri_geom, refit_tri_box
#include "pt_shape_refit.h"   // shape_refit_node

namespace pt {

constexpr int kBlasRecWords = 12;   // words per BLAS triangle in blas_recs and in blas_shade (three 16-B rows)

// One BLAS as a refit sees it (BlasRefitTables::desc, four int32 each): DevBlas' offsets and the mesh's triangle count
struct BlasDesc {
    int32_t node_off, num_nodes, rec_off, num_tris;
};

// One BLAS triangle position `pos` whose source triangle is `s`.  recs / shade: kBlasRecWords words per position;
// v1..n3: [num_triangles][3] in pt_scene_desc order (n1 NULL: the normals stay); tri_box: 6 floats per position.
__host__ __device__ inline void blas_refit_tri(int64_t pos, int64_t s, uint32_t* recs, uint32_t* shade, const float* v1,
                                               const float* v2, const float* v3, const float* n1, const float* n2,
                                               const float* n3, float* tri_box) {
    const float* a = v1 + 3 * s;
    const float* b = v2 + 3 * s;
    const float* c = v3 + 3 * s;
    float g[9], lo[3], hi[3];
    refit_tri_geom(a, b, c, g);
    refit_tri_box(a, b, c, lo, hi);
    RefitRow* r = (RefitRow*)(recs + pos * (int64_t)kBlasRecWords);
    r[0] = refit_row(g[0], g[1], g[2], g[3]);
    r[1] = refit_row(g[4], g[5], g[6], g[7]);
    r[2] = refit_row(g[8], 0.f, 0.f, 0.f);
    if (n1) {
        const float* p = n1 + 3 * s;
        const float* q = n2 + 3 * s;
        const float* u = n3 + 3 * s;
        RefitRow* h = (RefitRow*)(shade + pos * (int64_t)kBlasRecWords);
        const uint32_t mat = h[2].y;   // the material word stays
        h[0] = refit_row(p[0], p[1], p[2], q[0]);
        h[1] = refit_row(q[1], q[2], u[0], u[1]);
        h[2] = RefitRow{refit_bits(u[2]), mat, 0u, 0u};
    }
    float* tb = tri_box + pos * 6;
    for (int k = 0; k < 3; k++) { tb[k] = lo[k]; tb[3 + k] = hi[k]; }
}

// The empty unpadded box, and one box folded into another
__host__ __device__ inline void blas_bounds_empty(float* box) {
    for (int k = 0; k < 3; k++) { box[k] = INFINITY; box[3 + k] = -INFINITY; }
}
__host__ __device__ inline void blas_bounds_merge(float* box, const float* other) {
    for (int k = 0; k < 3; k++) { box[k] = fminf(box[k], other[k]); box[3 + k] = fmaxf(box[3 + k], other[3 + k]); }
}
// Source triangle `s` folded into box (6 floats: min, max), its vertices in shape_box's order: v1, v2, v3
__host__ __device__ inline void blas_bounds_tri(int64_t s, const float* v1, const float* v2, const float* v3, float* box) {
    const float* a = v1 + 3 * s;
    const float* b = v2 + 3 * s;
    const float* c = v3 + 3 * s;
    for (int k = 0; k < 3; k++) {
        box[k] = fminf(fminf(fminf(box[k], a[k]), b[k]), c[k]);
        box[3 + k] = fmaxf(fmaxf(fmaxf(box[3 + k], a[k]), b[k]), c[k]);
    }
}
// A mesh without triangles has the box shape_box gives it: zeros
__host__ __device__ inline void blas_bounds_finish(int64_t num_tris, float* box) {
    if (num_tris <= 0) for (int k = 0; k < 6; k++) box[k] = 0.f;
}

// Node `local` (relative to the BLAS) of BLAS B, after every node of the levels below it.  nodes: kShapeNodeWords
// words per node of all BLASes; node_box: 6 floats per node; tri_box: 6 floats per BLAS triangle position.  total_nodes
// / total_tris bound the arrays: a BLAS that leaves them is kept as it is.
__host__ __device__ inline void blas_refit_node(int64_t local, const BlasDesc& B, int64_t total_nodes, int64_t total_tris,
                                                uint32_t* nodes, float* node_box, const float* tri_box) {
    const int64_t n0 = B.node_off, nn = B.num_nodes, r0 = B.rec_off, nt = B.num_tris;
    if (n0 < 0 || nn < 0 || r0 < 0 || nt < 0 || n0 + nn > total_nodes || r0 + nt > total_tris) return;
    if (local < 0 || local >= nn) return;
    shape_refit_node(local, nn, nt, nodes + n0 * (int64_t)kShapeNodeWords, node_box + n0 * 6, tri_box + r0 * 6);
}

}  // namespace pt
