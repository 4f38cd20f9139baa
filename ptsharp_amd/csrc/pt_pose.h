// pt_pose.h — the arithmetic of pt_pose_meshes, shared by the device kernel (pt_pose.hip) and the host
// (tests/native/pose_check.cpp): `PT_HD`, no HIP call, compiles with g++.  Build with -ffp-contract=off.
//
// Mesh.Transform (Mesh.cs:254-274) on one triangle of the rest pose:
//   pose_triangle  in and out are the triangle's 18 floats V1 V2 V3 N1 N2 N3.  A moved triangle's vertices are
//                  Matrix.MulPosition(m, V) and, with `normals`, its normals Matrix.MulDirection(m, N): pt_ext.h's
//                  mat_position and mat_direction, the fp64 products summed left to right, one conversion to fp32,
//                  then the fp32 Normalize.  Everything else is copied: a triangle that is not moved (a loose
//                  triangle, a masked mesh) bit for bit, and the normals of a moved one when `normals` is false
//                  (the caller derives them from the posed positions afterwards).
// m is the first three rows of the row-major 4x4 matrix (12 doubles); MulPosition ignores the fourth.
#pragma once
#include "pt_ext.h"

namespace pt {

PT_HD void pose_triangle(const double* m, bool moved, bool normals, const float* in, float* out) {
    for (int k = 0; k < 6; k++) {
        const v3 a = v3{in[3 * k], in[3 * k + 1], in[3 * k + 2]};
        v3 r = a;
        if (moved && k < 3) r = mat_position(m, a);
        if (moved && k >= 3 && normals) r = mat_direction(m, a);
        out[3 * k] = r.x;
        out[3 * k + 1] = r.y;
        out[3 * k + 2] = r.z;
    }
}

}  // namespace pt
