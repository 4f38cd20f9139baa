// pt_shape_refit.h — the arithmetic of pt_update_shapes, shared by the device kernels (pt_shape_refit.hip) and
// the host (tests/native/shapes_check.cpp drives the same functions xforms, records, heavy, levels): every
// function is `__host__ __device__ inline`, makes no HIP call and compiles with g++.  Build with -ffp-contract=off.
//
// A shape refit keeps the topology of the analytic BVH4 (pt_bvh.h collapse_bvh4: plain fp32 child boxes, SoA) and
// recomputes, from new sphere, cube and matrix parameters, what depends on coordinates:
//   shape_sphere_box / shape_cube_box / shape_xform_boxes   a shape's BVH box as pt_scene_compile.cpp ana_boxes
//                computes it (and, for a transformed shape, the unpadded TransformedShape.BoundingBox its light needs)
//   shape_sphere_rows / shape_cube_rows                       the record rows of make_rec
//   shape_refit_xform    one transformed shape: DevXform::m / inv, its ext_recs row, its padded world box
//   shape_refit_record   one analytic record: rows 0-2 of a sphere or cube, the record's padded box
//   shape_refit_heavy    one heavy record: the box of the record it names
//   shape_refit_node     one BVH4 node, after every node below it: a leaf slot is the union of its records' boxes,
//                an inner slot its child's box; empty slots and words 24-31 (topology) stay
// The host builder's BVH2 boxes are exact unions of the padded record boxes, and min / max are exact and
// associative, so a refit with the parameters a scene was built from reproduces every word.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "pt_ext.h"     // v3, mk, mat_box, DevXform
#include "pt_refit.h"   // RefitRow, refit_bits, refit_pad_box

namespace pt {

constexpr int kShapeNodeWords = 32;    // words per BVH4 node (pt_bvh.h kNode4Words)
constexpr int kShapeRecWords = 12;     // words per analytic record (three 16-B rows)
constexpr int kShapeHeavyWords = 8;    // words per heavy record (two rows)
constexpr uint32_t kShapeEmpty = 0x7FFFFFFFu;   // pt_bvh.h kEmpty4
// the kinds a record or a DevXform names (pt_scene.h PrimKind; equal to the pt_shape_kind values)
constexpr int32_t kShapeSphere = 0, kShapeCube = 1, kShapeSdf = 5, kShapeVolume = 6, kShapeXform = 7;

// What an update moves, in pt_scene_desc order (host: ShapeRefitTables' arrays; device: the staged copies)
struct ShapeParams {
    int32_t num_spheres, num_cubes, num_transformed;
    const float* sphere_center;    // [num_spheres][3]
    const double* sphere_radius;   // [num_spheres]
    const float* cube_min;         // [num_cubes][3]
    const float* cube_max;
    const double* xform_matrix;    // [num_transformed][16] row-major
    const double* xform_inverse;
};

// march_pad (pt_scene_compile.cpp): hits of marched shapes can sit just outside their box
PT_HD double shape_march_pad(int32_t kind) { return kind == kShapeSdf ? 2e-3 : kind == kShapeVolume ? 4.0 / 512 : 0.0; }

// The BVH box of a sphere: ana_boxes' outward-rounded c -/+ r in double, then pad_box
PT_HD void shape_sphere_box(const float* c, double r, float* lo, float* hi) {
    for (int q = 0; q < 3; q++) {
        const double cc = c[q];
        lo[q] = nextafterf((float)(cc - r), -INFINITY);
        hi[q] = nextafterf((float)(cc + r), INFINITY);
    }
    refit_pad_box(lo, hi);
}
// The BVH box of a cube: pad_box on its corners
PT_HD void shape_cube_box(const float* mn, const float* mx, float* lo, float* hi) {
    for (int q = 0; q < 3; q++) { lo[q] = mn[q]; hi[q] = mx[q]; }
    refit_pad_box(lo, hi);
}
// Sphere.BoundingBox as a Box of Vectors (shape_box): the inner box of a transformed sphere
PT_HD void shape_sphere_bounds(const float* c, double r, v3& mn, v3& mx) {
    mn = mk((double)c[0] - r, (double)c[1] - r, (double)c[2] - r);
    mx = mk((double)c[0] + r, (double)c[1] + r, (double)c[2] + r);
}
// A transformed shape over the inner box imn..imx of an inner shape of kind `kind`: lo / hi its BVH box (the
// inner box widened by march_pad, through mat_box, rounded as ana_boxes rounds it, then pad_box), bmn / bmx the
// unpadded TransformedShape.BoundingBox
PT_HD void shape_xform_boxes(const double* m, int32_t kind, v3 imn, v3 imx, float* lo, float* hi, v3& bmn, v3& bmx) {
    mat_box(m, imn, imx, bmn, bmx);
    const double mp = shape_march_pad(kind);
    const v3 pmn = mk((double)imn.x - mp, (double)imn.y - mp, (double)imn.z - mp);
    const v3 pmx = mk((double)imx.x + mp, (double)imx.y + mp, (double)imx.z + mp);
    v3 a, b;
    mat_box(m, pmn, pmx, a, b);
    lo[0] = a.x; lo[1] = a.y; lo[2] = a.z;   // ana_boxes adds a march_pad of 0 in double: the same floats
    hi[0] = b.x; hi[1] = b.y; hi[2] = b.z;
    refit_pad_box(lo, hi);
}

// make_rec's rows of a sphere and of a cube; `index` and `mat` are the record's own words 7 and 8
PT_HD void shape_sphere_rows(const float* c, double r, uint32_t index, uint32_t mat, RefitRow* out) {
    uint64_t rb;
    __builtin_memcpy(&rb, &r, 8);
    out[0] = RefitRow{refit_bits(c[0]), refit_bits(c[1]), refit_bits(c[2]), (uint32_t)kShapeSphere};
    out[1] = RefitRow{0u, 0u, 0u, index};
    out[2] = RefitRow{mat, (uint32_t)(rb & 0xFFFFFFFFu), (uint32_t)(rb >> 32), 0u};
}
PT_HD void shape_cube_rows(const float* mn, const float* mx, uint32_t index, uint32_t mat, RefitRow* out) {
    out[0] = RefitRow{refit_bits(mn[0]), refit_bits(mn[1]), refit_bits(mn[2]), (uint32_t)kShapeCube};
    out[1] = RefitRow{refit_bits(mx[0]), refit_bits(mx[1]), refit_bits(mx[2]), index};
    out[2] = RefitRow{mat, 0u, 0u, 0u};
}

// One transformed shape `t`.  xforms: the scene's DevXform array; ext_recs: kShapeRecWords words per transformed
// shape; inner_kind / inner_index: its inner shape (an index outside P's arrays leaves the shape as it is);
// inner_box: 6 floats per transformed shape, the inner box of the kinds that never move; xbox: 6 floats per
// transformed shape, its padded world box; bounds (may be NULL): 6 floats, the unpadded BoundingBox.
PT_HD void shape_refit_xform(int64_t t, const ShapeParams& P, DevXform* xforms, uint32_t* ext_recs, const int32_t* inner_kind,
                             const int32_t* inner_index, const float* inner_box, float* xbox, float* bounds) {
    const double* m = P.xform_matrix + t * 16;
    const double* inv = P.xform_inverse + t * 16;
    DevXform* X = xforms + t;
    for (int k = 0; k < 12; k++) { X->m[k] = m[k]; X->inv[k] = inv[k]; }   // rows12
    const int32_t kind = inner_kind[t];
    const int64_t j = (int64_t)inner_index[t];
    const float* ib = inner_box + t * 6;
    v3 imn = v3{ib[0], ib[1], ib[2]}, imx = v3{ib[3], ib[4], ib[5]};
    RefitRow* r = (RefitRow*)(ext_recs + t * (int64_t)kShapeRecWords);
    if (kind == kShapeSphere && j >= 0 && j < (int64_t)P.num_spheres) {
        const float* c = P.sphere_center + 3 * j;
        const double rad = P.sphere_radius[j];
        shape_sphere_bounds(c, rad, imn, imx);
        RefitRow rows[3];
        shape_sphere_rows(c, rad, r[1].w, r[2].x, rows);
        r[0] = rows[0]; r[1] = rows[1]; r[2] = rows[2];
    } else if (kind == kShapeCube && j >= 0 && j < (int64_t)P.num_cubes) {
        const float* mn = P.cube_min + 3 * j;
        const float* mx = P.cube_max + 3 * j;
        imn = v3{mn[0], mn[1], mn[2]}; imx = v3{mx[0], mx[1], mx[2]};
        RefitRow rows[3];
        shape_cube_rows(mn, mx, r[1].w, r[2].x, rows);
        r[0] = rows[0]; r[1] = rows[1]; r[2] = rows[2];
    }
    float lo[3], hi[3];
    v3 bmn, bmx;
    shape_xform_boxes(m, kind, imn, imx, lo, hi, bmn, bmx);
    float* xb = xbox + t * 6;
    for (int k = 0; k < 3; k++) { xb[k] = lo[k]; xb[3 + k] = hi[k]; }
    if (bounds) { bounds[0] = bmn.x; bounds[1] = bmn.y; bounds[2] = bmn.z; bounds[3] = bmx.x; bounds[4] = bmx.y; bounds[5] = bmx.z; }
}

// One analytic record at position `i`.  recs: kShapeRecWords words per record; rec_box: 6 floats per record (a
// top-level SDF's or Volume's keeps the upload's); xbox: shape_refit_xform's.  The kind and the scene index are the
// record's own words 3 and 7; the material and index words stay.
PT_HD void shape_refit_record(int64_t i, const ShapeParams& P, uint32_t* recs, float* rec_box, const float* xbox) {
    RefitRow* r = (RefitRow*)(recs + i * (int64_t)kShapeRecWords);
    const int32_t kind = (int32_t)r[0].w;
    const int64_t j = (int64_t)r[1].w;
    float lo[3], hi[3];
    if (kind == kShapeSphere && j < (int64_t)P.num_spheres) {
        const float* c = P.sphere_center + 3 * j;
        const double rad = P.sphere_radius[j];
        RefitRow rows[3];
        shape_sphere_rows(c, rad, r[1].w, r[2].x, rows);
        r[0] = rows[0]; r[1] = rows[1]; r[2] = rows[2];
        shape_sphere_box(c, rad, lo, hi);
    } else if (kind == kShapeCube && j < (int64_t)P.num_cubes) {
        const float* mn = P.cube_min + 3 * j;
        const float* mx = P.cube_max + 3 * j;
        RefitRow rows[3];
        shape_cube_rows(mn, mx, r[1].w, r[2].x, rows);
        r[0] = rows[0]; r[1] = rows[1]; r[2] = rows[2];
        shape_cube_box(mn, mx, lo, hi);
    } else if (kind == kShapeXform && j < (int64_t)P.num_transformed) {
        const float* xb = xbox + j * 6;
        for (int k = 0; k < 3; k++) { lo[k] = xb[k]; hi[k] = xb[3 + k]; }
    } else {
        return;
    }
    float* rb = rec_box + i * 6;
    for (int k = 0; k < 3; k++) { rb[k] = lo[k]; rb[3 + k] = hi[k]; }
}

// One heavy record `h`: {box lo, record index} {box hi, 0}; the index (lo.w) stays and names the box
PT_HD void shape_refit_heavy(int64_t h, int64_t num_recs, uint32_t* heavy, const float* rec_box) {
    RefitRow* r = (RefitRow*)(heavy + h * (int64_t)kShapeHeavyWords);
    const uint32_t idx = r[0].w;
    if ((int64_t)idx >= num_recs) return;
    const float* b = rec_box + (int64_t)idx * 6;
    r[0] = RefitRow{refit_bits(b[0]), refit_bits(b[1]), refit_bits(b[2]), idx};
    r[1] = RefitRow{refit_bits(b[3]), refit_bits(b[4]), refit_bits(b[5]), 0u};
}

// A BVH4 slot's box: the union of `count` consecutive boxes (6 floats each) from `first`
PT_HD void shape_slot_union(const float* boxes, int64_t first, int count, float* lo, float* hi) {
    for (int k = 0; k < 3; k++) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    for (int t = 0; t < count; t++) {
        const float* b = boxes + (first + t) * 6;
        for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], b[k]); hi[k] = fmaxf(hi[k], b[3 + k]); }
    }
}

// One node `ni`, after every node of the levels below it.  nodes: kShapeNodeWords words per node; node_box: 6
// floats per node; rec_box: 6 floats per record.  A slot whose reference leaves the arrays is kept as it is.
PT_HD void shape_refit_node(int64_t ni, int64_t num_nodes, int64_t num_recs, uint32_t* nodes, float* node_box,
                            const float* rec_box) {
    uint32_t* w = nodes + ni * (int64_t)kShapeNodeWords;
    uint32_t line[24];
    for (int k = 0; k < 24; k++) line[k] = w[k];
    float nlo[3] = {INFINITY, INFINITY, INFINITY}, nhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < 4; k++) {
        const uint32_t ref = w[24 + k];
        if (ref == kShapeEmpty) continue;
        float lo[3], hi[3];
        if (ref & 0x80000000u) {
            const int64_t first = (int64_t)(ref & 0x1FFFFFFFu);
            const int cnt = (int)((ref >> 29) & 3u) + 1;
            if (first + cnt > num_recs) continue;
            shape_slot_union(rec_box, first, cnt, lo, hi);
        } else {
            if ((int64_t)ref >= num_nodes || (int64_t)ref <= ni) continue;
            shape_slot_union(node_box, (int64_t)ref, 1, lo, hi);
        }
        for (int ax = 0; ax < 3; ax++) {
            line[8 * ax + k] = refit_bits(lo[ax]);
            line[8 * ax + 4 + k] = refit_bits(hi[ax]);
            nlo[ax] = fminf(nlo[ax], lo[ax]);
            nhi[ax] = fmaxf(nhi[ax], hi[ax]);
        }
    }
    RefitRow* r = (RefitRow*)w;
    for (int k = 0; k < 6; k++) r[k] = RefitRow{line[4 * k], line[4 * k + 1], line[4 * k + 2], line[4 * k + 3]};
    float* nb = node_box + ni * 6;
    for (int k = 0; k < 3; k++) { nb[k] = nlo[k]; nb[3 + k] = nhi[k]; }
}

}  // namespace pt
