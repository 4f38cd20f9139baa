// pt_motion.h — where a visible surface point was one frame ago, and the temporal merge of Welford
// states (pt_render_motion, pt_accumulate_temporal).
//
// One text for the device (pt_motion.hip) and for a host check program (tests/native/motion_check.cpp):
// every function is `__host__ __device__ inline`, and the two qualifiers are defined away when the
// compiler is not hipcc.  All arithmetic is fp64 on the fp32 or fp64 values the device holds, without
// contraction, and every sum is written in the order it is made: a·b + c·d + e·f is ((a·b) + (c·d)) + (e·f).
// The divisions and the one sqrt are the only operations whose last bit may depend on the compiler.
//
// The previous position P' of the hit point P = o + t·d, by the kind of shape under the ray:
//   world triangle    u, v from the current record {v1, e1, e2} by Möller–Trumbore (motion_bary), then
//                     P' = v1' + u·e1' + v·e2' from the snapshot's record of the same source triangle
//   instanced mesh    the same with the object-space ray blas_hit traces and the BLAS record, then
//                     P' = m' · (v1' + u·e1' + v·e2') with the snapshot's matrix of the instance
//   sphere            P' = c' + (P − c)·(r'/r)
//   cube              per axis s = (P_k − lo_k)/(hi_k − lo_k), 0 where hi_k == lo_k; P'_k = lo'_k + s·(hi'_k − lo'_k)
//   TransformedShape  over anything but a mesh: P' = m' · (inv · P).  The inner shape is taken as rigid:
//                     a sphere or cube that pt_update_shapes resizes inside its instance is not followed.
//   plane, top-level SDFShape, top-level Volume, and a hit whose identity the tables do not give: P' = P
//   miss              the direction d stands in for P' − cam'.p (the environment is at infinity)
// and its projection, the inverse of Camera.CastRay (motion_project).
//
// The merge (temporal_status, temporal_merge) is Chan's pairwise update of two Welford states with the
// history's weight capped at max_history samples.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

#pragma clang fp contract(off)

namespace pt {

constexpr double kMotionInf = 1e9;   // Hit.INF: the depth of a miss

enum MotionStatus : int32_t { MOTION_OK = 0, MOTION_OUTSIDE = 1, MOTION_NO_SNAPSHOT = 2 };
enum TemporalStatus : int32_t { TEMPORAL_MERGED = 0, TEMPORAL_NO_HISTORY = 1, TEMPORAL_MOTION = 2, TEMPORAL_HISTORY_INVALID = 3,
                                TEMPORAL_IDENTITY = 4, TEMPORAL_DEPTH = 5, TEMPORAL_INVALID = 7 };

// The previous frame's camera: pt_camera's fp32 vectors widened, and m
struct MotionCamera {
    double p[3], u[3], v[3], w[3];
    double m;
};

__host__ __device__ inline bool motion_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for NaN

__host__ __device__ inline double motion_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__host__ __device__ inline void motion_cross(const double a[3], const double b[3], double out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// P = o + t·d
__host__ __device__ inline void motion_point(const double o[3], const double d[3], double t, double P[3]) {
    for (int k = 0; k < 3; k++) P[k] = o[k] + t * d[k];
}

// Barycentrics of the ray's point on the plane of record {v1, e1, e2} (Möller–Trumbore)
__host__ __device__ inline void motion_bary(const double o[3], const double d[3], const double v1[3], const double e1[3],
                                            const double e2[3], double& u, double& v) {
    double pvec[3], tvec[3], qvec[3];
    motion_cross(d, e2, pvec);
    const double det = motion_dot(e1, pvec);
    for (int k = 0; k < 3; k++) tvec[k] = o[k] - v1[k];
    u = motion_dot(tvec, pvec) / det;
    motion_cross(tvec, e1, qvec);
    v = motion_dot(d, qvec) / det;
}

// v1' + u·e1' + v·e2'
__host__ __device__ inline void motion_tri_point(const double v1[3], const double e1[3], const double e2[3], double u, double v,
                                                 double out[3]) {
    for (int k = 0; k < 3; k++) out[k] = (v1[k] + u * e1[k]) + v * e2[k];
}

// Rows 1-3 of a 3x4 matrix times the position x
__host__ __device__ inline void motion_mat_point(const double m[12], const double x[3], double out[3]) {
    for (int r = 0; r < 3; r++) out[r] = ((m[4 * r] * x[0] + m[4 * r + 1] * x[1]) + m[4 * r + 2] * x[2]) + m[4 * r + 3];
}

__host__ __device__ inline void motion_sphere_point(const double P[3], const double c[3], double r, const double c1[3], double r1,
                                                    double out[3]) {
    const double s = r1 / r;
    for (int k = 0; k < 3; k++) out[k] = c1[k] + (P[k] - c[k]) * s;
}

__host__ __device__ inline void motion_cube_point(const double P[3], const double lo[3], const double hi[3], const double lo1[3],
                                                  const double hi1[3], double out[3]) {
    for (int k = 0; k < 3; k++) {
        const double s = hi[k] == lo[k] ? 0.0 : (P[k] - lo[k]) / (hi[k] - lo[k]);
        out[k] = lo1[k] + s * (hi1[k] - lo1[k]);
    }
}

// P' = m' · (inv · P)
__host__ __device__ inline void motion_xform_point(const double P[3], const double inv[12], const double m1[12], double out[3]) {
    double q[3];
    motion_mat_point(inv, P, q);
    motion_mat_point(m1, q, out);
}

// The inverse of Camera.CastRay for r = P' − cam'.p (or the direction of a miss): the continuous pixel
// coordinates in the previous W x H image, the nearest pixel floor(x' + 0.5) + W·floor(y' + 0.5), and
// the status.  Behind the previous camera (c <= 0) or not finite: status 1, xy = (−1, −1), pixel −1.
// Outside the previous image: status 1, pixel −1, xy as computed.
__host__ __device__ inline int32_t motion_project(const MotionCamera& cam, int32_t W, int32_t H, const double r[3], double xy[2],
                                                  int32_t& pixel) {
    pixel = -1;
    const double a = motion_dot(r, cam.u), b = motion_dot(r, cam.v), c = motion_dot(r, cam.w);
    if (!(c > 0.0) || !motion_finite(a) || !motion_finite(b) || !motion_finite(c)) {
        xy[0] = xy[1] = -1.0;
        return MOTION_OUTSIDE;
    }
    const double aspect = (double)W / (double)H;
    const double px = (-(a / c) * cam.m) / aspect;
    const double py = -(b / c) * cam.m;
    const double x = ((px + 1.0) / 2.0) * ((double)W - 1.0);
    const double y = ((py + 1.0) / 2.0) * ((double)H - 1.0);
    if (!motion_finite(x) || !motion_finite(y)) {
        xy[0] = xy[1] = -1.0;
        return MOTION_OUTSIDE;
    }
    xy[0] = x;
    xy[1] = y;
    const double qx = floor(x + 0.5), qy = floor(y + 0.5);
    if (qx < 0.0 || qy < 0.0 || qx >= (double)W || qy >= (double)H) return MOTION_OUTSIDE;
    pixel = (int32_t)((int64_t)qx + (int64_t)W * (int64_t)qy);   // < W·H, which the context keeps below 2^31
    return MOTION_OK;
}

// A hit's previous position to its outputs: r = P' − cam'.p, prev_depth = |r| (1e9 if not finite)
__host__ __device__ inline int32_t motion_project_point(const MotionCamera& cam, int32_t W, int32_t H, const double P1[3],
                                                        double xy[2], double& depth, int32_t& pixel) {
    double r[3];
    for (int k = 0; k < 3; k++) r[k] = P1[k] - cam.p[k];
    depth = sqrt(motion_dot(r, r));
    if (!motion_finite(depth)) depth = kMotionInf;
    return motion_project(cam, W, H, r, xy, pixel);
}

// ------------------------------------------------------------------ the temporal merge
// A pixel is valid when N >= 1 and all of M and V are finite (pt_denoise.h's rule, restated so that
// this header stands alone).
__host__ __device__ inline bool temporal_valid(const double* m3, const double* v3, int32_t n) {
    if (n < 1) return false;
    for (int k = 0; k < 3; k++)
        if (!motion_finite(m3[k]) || !motion_finite(v3[k])) return false;
    return true;
}

// The first rule that applies to pixel p, whose history tap is pixel q (only read when the earlier rules pass)
__host__ __device__ inline int32_t temporal_status(bool cur_valid, bool have_history, int32_t motion_status, bool hist_valid,
                                                   int32_t shape_p, int32_t prim_p, int32_t shape_q, int32_t prim_q,
                                                   double prev_depth_p, double hist_depth_q, double sigma_depth) {
    if (!cur_valid) return TEMPORAL_INVALID;
    if (!have_history) return TEMPORAL_NO_HISTORY;
    if (motion_status != MOTION_OK) return TEMPORAL_MOTION;
    if (!hist_valid) return TEMPORAL_HISTORY_INVALID;
    if (shape_p != shape_q || prim_p != prim_q) return TEMPORAL_IDENTITY;
    if (sigma_depth > 0.0 && fabs(prev_depth_p - hist_depth_q) > sigma_depth * prev_depth_p) return TEMPORAL_DEPTH;
    return TEMPORAL_MERGED;
}

// Chan's pairwise update of the current state {mc, vc, nc} with the history {mh, vh, nh}, the history
// weighing at most max_history samples (and no more than keeps nc + nh' inside int32).  nh' = 0 (only
// with max_history = 0) leaves the current state as it stands.
__host__ __device__ inline void temporal_merge(const double mc[3], const double vc[3], int32_t nc, const double mh[3],
                                               const double vh[3], int32_t nh, int32_t max_history, double m[3], double v[3],
                                               int32_t& n) {
    int32_t nh1 = nh < max_history ? nh : max_history;
    const int32_t room = 2147483647 - nc;
    if (nh1 > room) nh1 = room;
    if (nh1 <= 0) {
        for (int k = 0; k < 3; k++) {
            m[k] = mc[k];
            v[k] = vc[k];
        }
        n = nc;
        return;
    }
    n = nc + nh1;
    const double scale = nh >= 2 ? ((double)nh1 - 1.0) / ((double)nh - 1.0) : 1.0;
    const double wm = (double)nh1 / (double)n;
    const double wv = ((double)nc * (double)nh1) / (double)n;
    for (int k = 0; k < 3; k++) {
        const double vh1 = nh >= 2 ? vh[k] * scale : vh[k];
        const double delta = mh[k] - mc[k];
        m[k] = mc[k] + delta * wm;
        v[k] = (vc[k] + vh1) + (delta * delta) * wv;
    }
}

}  // namespace pt
