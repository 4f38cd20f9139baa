// pt_skin.h — the arithmetic of pt_skin_meshes, shared by the device kernel (pt_skin.hip) and the host
// (tests/native/skin_check.cpp): `PT_HD`, no HIP call, compiles with g++.  Build with -ffp-contract=off.
//
// Linear blend skinning of one triangle of the rest pose, built from Matrix.MulPosition / MulDirection
// (Matrix.cs:134-150):
//   skin_corner    one corner: its rest position p and rest normal n, kSkinInfluences influences (b[k], w[k]).  An
//                  influence is live when w[k] != 0 (false only for +-0; a NaN weight is live).  For each live k in
//                  ascending order the term is (double)w[k] * P_k per component, P_k the three fp64 sums mat_position
//                  forms (m[0]*x + m[1]*y + m[2]*z + m[3], left to right) before any conversion; the accumulator is
//                  the first live term, every further live term is added to it (it never starts from 0, so -0
//                  survives); the result is one conversion of the accumulator to fp32.  With `normals` the normal is
//                  blended the same way from mat_direction's three fp64 sums (no translation), converted once, then
//                  normalised by the fp32 normalize mat_direction ends in; without, it is copied.  With no live
//                  influence position and normal are copied bit for bit.  A dead influence is skipped by a branch: its
//                  index is not used and its matrix is never read.
//   skin_triangle  in and out are the triangle's 18 floats V1 V2 V3 N1 N2 N3; bones and weights its [3][4] rows.  A
//                  triangle that is not `moved` (a loose one) is copied bit for bit, whatever its weights.
// rows + b * stride is the first three rows of bone b's row-major 4x4 matrix (12 doubles; the fourth row is never
// read): stride 16 for the caller's array, 12 for the kernel's LDS table.  One live influence of weight 1 gives
// exactly pose_triangle's result for that bone (1.0 * P is P).
#pragma once
#include <stdint.h>

#include "pt_ext.h"

namespace pt {

constexpr int kSkinInfluences = 4;   // PT_SKIN_INFLUENCES

template <class Index>
PT_HD void skin_corner(const double* rows, int stride, const Index* b, const float* w, bool normals, const float* p,
                       const float* n, float* po, float* no) {
    double ax = 0, ay = 0, az = 0, nx = 0, ny = 0, nz = 0;
    bool live = false;
    for (int k = 0; k < kSkinInfluences; k++) {
        if (!(w[k] != 0.f)) continue;
        const double* m = rows + (int64_t)b[k] * stride;
        const double wk = (double)w[k];
        const double x = wk * (m[0] * p[0] + m[1] * p[1] + m[2] * p[2] + m[3]);
        const double y = wk * (m[4] * p[0] + m[5] * p[1] + m[6] * p[2] + m[7]);
        const double z = wk * (m[8] * p[0] + m[9] * p[1] + m[10] * p[2] + m[11]);
        ax = live ? ax + x : x;
        ay = live ? ay + y : y;
        az = live ? az + z : z;
        if (normals) {
            const double dx = wk * (m[0] * n[0] + m[1] * n[1] + m[2] * n[2]);
            const double dy = wk * (m[4] * n[0] + m[5] * n[1] + m[6] * n[2]);
            const double dz = wk * (m[8] * n[0] + m[9] * n[1] + m[10] * n[2]);
            nx = live ? nx + dx : dx;
            ny = live ? ny + dy : dy;
            nz = live ? nz + dz : dz;
        }
        live = true;
    }
    v3 rp = v3{p[0], p[1], p[2]}, rn = v3{n[0], n[1], n[2]};
    if (live) {
        rp = mk(ax, ay, az);
        if (normals) rn = normalize(mk(nx, ny, nz));
    }
    po[0] = rp.x; po[1] = rp.y; po[2] = rp.z;
    no[0] = rn.x; no[1] = rn.y; no[2] = rn.z;
}

template <class Index>
PT_HD void skin_triangle(const double* rows, int stride, bool moved, bool normals, const Index* bones, const float* weights,
                         const float* in, float* out) {
    if (!moved) {
        for (int i = 0; i < 18; i++) out[i] = in[i];
        return;
    }
    for (int c = 0; c < 3; c++)
        skin_corner(rows, stride, bones + kSkinInfluences * c, weights + kSkinInfluences * c, normals, in + 3 * c, in + 9 + 3 * c,
                    out + 3 * c, out + 9 + 3 * c);
}

}  // namespace pt
