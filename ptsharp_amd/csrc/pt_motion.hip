// pt_motion.hip — motion vectors and temporal accumulation (pt_motion_snapshot, pt_render_motion,
// pt_accumulate_temporal).  The arithmetic is pt_motion.h's.
//
// k_motion_snapshot_tris: one lane per BVH position (the world BVH's, or every BLAS's): its record {v1, e1, e2}
// as three 16-byte loads, stored as three 16-byte stores at the record's source triangle, so that a later
// rebuild's re-sort does not matter.  A source outside [0, num_src) is skipped.  The analytic records, the
// DevXform array and the ext_recs are nothing re-sorts: they are copied as they lie (keyed by record position).
//
// k_motion<FULL>: k_features' frame (one lane per pixel, a wave an 8x8 tile, 256 lanes with the 64 KiB LDS
// stack, a lane outside the image returns before the trace), Camera.CastRay(x, y, W, H, 0.5, 0.5) with the lens
// ignored, the megakernel's trace(), then the identity lookups of k_intersect_hits (pt_query.hip: the same
// tables, every lookup guarded by its table's length) and pt_motion.h's reprojection.  The lookups are restated
// here because the reprojection needs what they pass through on the way (the BLAS position, the DevXform).
//
// k_temporal_merge: one lane per pixel, a gathered read of one history pixel, no atomics, no LDS.  The history is
// read from one set and the new one written to the other.
//
// The motion result of P = W·H pixels is one allocation (motion_bytes), in this order:
//   prev_xy [P][2] f64 | depth [P] f64 | prev_depth [P] f64 | shape [P] i32 | prim [P] i32 | prev_pixel [P] i32 | status [P] i32
// a history set (temporal_set_bytes):
//   M [P][3] f64 | V [P][3] f64 | depth [P] f64 | N [P] i32 | shape [P] i32 | prim [P] i32
// Every offset is formed in 64 bits.
#include <hip/hip_runtime.h>

#include "pt_device.h"
#include "pt_motion.h"
#include "pt_motion_dev.h"

#pragma clang fp contract(off)

namespace pt {

constexpr int kMotionBlock = 256;
using MStack = LdsStack<kMotionBlock>;

size_t motion_bytes(int32_t W, int32_t H) {
    const size_t P = (size_t)W * (size_t)H;
    return P * (4 * sizeof(double) + 4 * sizeof(int32_t));
}

MotionOut motion_of(void* base, int32_t W, int32_t H) {
    const size_t P = (size_t)W * (size_t)H;
    MotionOut m;
    m.prev_xy = (double*)base;
    m.depth = m.prev_xy + 2 * P;
    m.prev_depth = m.depth + P;
    m.shape = (int32_t*)(m.prev_depth + P);
    m.prim = m.shape + P;
    m.prev_pixel = m.prim + P;
    m.status = m.prev_pixel + P;
    return m;
}

size_t temporal_set_bytes(int32_t W, int32_t H) {
    const size_t P = (size_t)W * (size_t)H;
    return P * (7 * sizeof(double) + 3 * sizeof(int32_t));
}

TemporalSet temporal_set_of(void* base, int32_t W, int32_t H) {
    const size_t P = (size_t)W * (size_t)H;
    TemporalSet s;
    s.m = (double*)base;
    s.v = s.m + 3 * P;
    s.depth = s.v + 3 * P;
    s.n = (int32_t*)(s.depth + P);
    s.shape = s.n + P;
    s.prim = s.shape + P;
    return s;
}

__global__ __launch_bounds__(256) void k_motion_snapshot_tris(int64_t num_pos, const float4* __restrict__ recs, int32_t stride,
                                                              const int32_t* __restrict__ src_of_pos, int64_t num_src,
                                                              float4* __restrict__ snap) {
    const int64_t pos = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (pos >= num_pos) return;
    const int64_t src = (int64_t)src_of_pos[pos];
    if (src < 0 || src >= num_src) return;
    const float4* r = recs + (size_t)pos * (size_t)stride;
    const float4 a = r[0], b = r[1], c = r[2];
    float4* s = snap + 3 * (size_t)src;
    s[0] = a; s[1] = b; s[2] = c;
}

hipError_t launch_motion_snapshot_tris(int64_t num_pos, const float4* recs, int32_t stride, const int32_t* src_of_pos,
                                       int64_t num_src, float4* snap, hipStream_t stream) {
    if (num_pos <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_motion_snapshot_tris, dim3((unsigned)((num_pos + 255) / 256)), dim3(256), 0, stream, num_pos, recs, stride,
                       src_of_pos, num_src, snap);
    return hipGetLastError();
}

__device__ __forceinline__ int32_t motion_table_at(const int32_t* __restrict__ table, int64_t n, int64_t i) {
    return (table && i >= 0 && i < n) ? table[i] : -1;
}

__device__ __forceinline__ void widen(v3 a, double out[3]) { out[0] = a.x; out[1] = a.y; out[2] = a.z; }

// {v1, e1, e2} of a triangle record, widened
__device__ __forceinline__ void tri_rec(const float4* r, double v1[3], double e1[3], double e2[3]) {
    const float4 a = r[0], b = r[1], c = r[2];
    v1[0] = a.x; v1[1] = a.y; v1[2] = a.z;
    e1[0] = a.w; e1[1] = b.x; e1[2] = b.y;
    e2[0] = b.z; e2[1] = b.w; e2[2] = c.x;
}

// The previous position of the point of ray (ro, rd) on the triangle of record `cur`, from the snapshot's record
// `old` of the same source triangle
__device__ __forceinline__ void tri_previous(const float4* cur, const float4* old, v3 ro, v3 rd, double out[3]) {
    double o[3], d[3], v1[3], e1[3], e2[3], u, v;
    widen(ro, o); widen(rd, d);
    tri_rec(cur, v1, e1, e2);
    motion_bary(o, d, v1, e1, e2, u, v);
    tri_rec(old, v1, e1, e2);
    motion_tri_point(v1, e1, e2, u, v, out);
}

// index, prim and shape of hit h as k_intersect_hits' identity() gives them, and the hit point's previous
// position P1 (P where the snapshot has no record of the shape)
template <bool FULL>
__device__ __forceinline__ void motion_hit(const DevScene& S, const QueryDevTables& T, const MotionSnap& N, const HitRec& h, v3 o, v3 d,
                                           int32_t& prim, int32_t& shape, double P1[3]) {
    prim = shape = -1;
    double od[3], dd[3], P[3];
    widen(o, od); widen(d, dd);
    motion_point(od, dd, h.t, P);
    P1[0] = P[0]; P1[1] = P[1]; P1[2] = P[2];
    const int64_t pos = h.idx;
    if (h.kind == KIND_TRI) {
        const int32_t src = prim = motion_table_at(T.tri_src, T.tri_src_n, pos);
        shape = motion_table_at(T.tri_slot, T.tri_slot_n, src);
        if (N.have && N.tris && src >= 0 && (int64_t)src < N.num_src)
            tri_previous(S.tri_recs + (size_t)pos * (size_t)S.tri_rstride, N.tris + 3 * (size_t)src, o, d, P1);
        return;
    }
    if (h.kind == KIND_PLANE) {
        if (pos < 0 || pos >= (int64_t)S.num_planes) return;
        const int32_t index = (int32_t)f2u(S.planes[2 * pos + 1].w);
        shape = motion_table_at(T.plane_slot, T.plane_slot_n, index);
        return;
    }
    if (pos < 0 || pos >= (int64_t)S.ana_count) return;
    const float4* r = S.ana_recs + 3 * pos;
    int32_t index = (int32_t)f2u(r[1].w);
    int32_t off = 0, cnt = 0;
    switch (h.kind) {
        case KIND_SPHERE: off = T.ana_off[KIND_SPHERE]; cnt = T.ana_cnt[KIND_SPHERE]; break;
        case KIND_CUBE: off = T.ana_off[KIND_CUBE]; cnt = T.ana_cnt[KIND_CUBE]; break;
        case KIND_SDF: off = T.ana_off[KIND_SDF]; cnt = T.ana_cnt[KIND_SDF]; break;
        case KIND_VOLUME: off = T.ana_off[KIND_VOLUME]; cnt = T.ana_cnt[KIND_VOLUME]; break;
        case KIND_XFORM: off = T.ana_off[KIND_XFORM]; cnt = T.ana_cnt[KIND_XFORM]; break;
        default: break;
    }
    if (index < 0 || index >= cnt) return;
    shape = motion_table_at(T.ana_slot, T.ana_slot_n, (int64_t)off + index);
    const bool snap_rec = N.have && N.ana && pos < N.num_ana;
    if (h.kind == KIND_SPHERE && snap_rec) {
        const float4* q = N.ana + 3 * pos;
        const float4 a = r[0], a1 = q[0];
        const double c[3] = {a.x, a.y, a.z}, c1[3] = {a1.x, a1.y, a1.z};
        motion_sphere_point(P, c, rec_radius(r), c1, rec_radius(q), P1);
        return;
    }
    if (h.kind == KIND_CUBE && snap_rec) {
        const float4* q = N.ana + 3 * pos;
        const float4 a = r[0], b = r[1], a1 = q[0], b1 = q[1];
        const double lo[3] = {a.x, a.y, a.z}, hi[3] = {b.x, b.y, b.z}, lo1[3] = {a1.x, a1.y, a1.z}, hi1[3] = {b1.x, b1.y, b1.z};
        motion_cube_point(P, lo, hi, lo1, hi1, P1);
        return;
    }
    if (FULL && h.kind == KIND_XFORM) {
        const DevXform& X = S.xforms[index];
        const bool snap_x = N.have && N.xforms && (int64_t)index < N.num_xforms;
        if (X.kind != KIND_MESH) {
            if (snap_x) motion_xform_point(P, X.inv, N.xforms[index].m, P1);
            return;
        }
        if (X.rec < 0 || X.rec >= T.num_blas) return;
        const v3 so = mat_position(X.inv, o), sd = mat_direction(X.inv, d);   // as ext_hit_info maps the ray
        const HitRec ih = blas_hit(S, X.rec, so, sd);
        if (ih.idx < 0) return;
        const int64_t bp = (int64_t)S.blas[X.rec].rec_off + (int64_t)ih.idx;
        const int32_t src = prim = motion_table_at(T.blas_src, T.blas_src_n, bp);
        if (snap_x && N.blas && src >= 0 && (int64_t)src < N.num_src) {
            double Q[3];
            tri_previous(S.blas_recs + 3 * (size_t)bp, N.blas + 3 * (size_t)src, so, sd, Q);
            motion_mat_point(N.xforms[index].m, Q, P1);
        }
    }
}

template <bool FULL>
__global__ __launch_bounds__(kMotionBlock) void k_motion(DevScene S, QueryDevTables T, MotionSnap N, DevCamera cam, int32_t W, int32_t H,
                                                         MotionOut M) {
    __shared__ uint32_t s_stack[kStackMax * kMotionBlock];
    const MStack stack{s_stack + threadIdx.x};
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t x64 = (int64_t)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int64_t y64 = (int64_t)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x64 >= (int64_t)W || y64 >= (int64_t)H) return;
    const int x = (int)x64, y = (int)y64;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    v3 o, d;
    cast_ray(cam, x, y, W, H, 0.5, 0.5, 0ull, o, d);   // aperture_radius is 0: the key is never used
    Counters ctr{0, 0, 0, 0};
    const HitRec h = trace<false, FULL>(S, o, d, stack, ctr);
    const bool hit = h.t < kHitInf;
    int32_t prim = -1, shape = -1, pixel = -1, status = MOTION_NO_SNAPSHOT;
    double xy[2] = {-1.0, -1.0}, prev_depth = kMotionInf, P1[3];
    if (hit) motion_hit<FULL>(S, T, N, h, o, d, prim, shape, P1);
    if (N.have) {
        if (hit) {
            status = motion_project_point(N.cam, W, H, P1, xy, prev_depth, pixel);
        } else {
            double dd[3];
            widen(d, dd);
            status = motion_project(N.cam, W, H, dd, xy, pixel);
        }
    }
    M.shape[p] = shape;
    M.prim[p] = prim;
    M.depth[p] = hit ? h.t : kMotionInf;
    M.prev_xy[2 * p] = xy[0];
    M.prev_xy[2 * p + 1] = xy[1];
    M.prev_depth[p] = prev_depth;
    M.prev_pixel[p] = pixel;
    M.status[p] = status;
}

// The motion pass of the whole W x H frame on `stream`.  FULL as k_intersect_hits picks it without INFO.
hipError_t launch_motion(const DevScene& S, const QueryDevTables& T, const MotionSnap& N, const DevCamera& cam, const MotionOut& M,
                         int32_t W, int32_t H, hipStream_t stream) {
    const dim3 grid((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16)), block(kMotionBlock);
    if (S.full_geom != 0) hipLaunchKernelGGL((k_motion<true>), grid, block, 0, stream, S, T, N, cam, W, H, M);
    else hipLaunchKernelGGL((k_motion<false>), grid, block, 0, stream, S, T, N, cam, W, H, M);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_temporal_merge(uint64_t P, const double* __restrict__ bm, const double* __restrict__ bv,
                                                        const int32_t* __restrict__ bn, MotionOut M, TemporalSet hist, int have_history,
                                                        int32_t max_history, double sigma_depth, TemporalSet out,
                                                        int32_t* __restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= P) return;
    const double mc[3] = {bm[3 * p], bm[3 * p + 1], bm[3 * p + 2]};
    const double vc[3] = {bv[3 * p], bv[3 * p + 1], bv[3 * p + 2]};
    const int32_t nc = bn[p];
    const int32_t shape = M.shape[p], prim = M.prim[p];
    const int64_t q = (int64_t)M.prev_pixel[p];
    // status 0 comes with a pixel inside the image (motion_project); the history is never read through another
    const int32_t ms = (M.status[p] == MOTION_OK && (q < 0 || (uint64_t)q >= P)) ? (int32_t)MOTION_OUTSIDE : M.status[p];
    const bool tap = have_history && ms == MOTION_OK;
    double mh[3] = {0.0, 0.0, 0.0}, vh[3] = {0.0, 0.0, 0.0}, dh = 0.0;
    int32_t nh = 0, sh = -1, ph = -1;
    if (tap) {
        for (int k = 0; k < 3; k++) {
            mh[k] = hist.m[3 * (size_t)q + k];
            vh[k] = hist.v[3 * (size_t)q + k];
        }
        nh = hist.n[q]; sh = hist.shape[q]; ph = hist.prim[q]; dh = hist.depth[q];
    }
    const int32_t st = temporal_status(temporal_valid(mc, vc, nc), have_history != 0, ms,
                                       temporal_valid(mh, vh, nh), shape, prim, sh, ph, M.prev_depth[p], dh, sigma_depth);
    double m[3] = {mc[0], mc[1], mc[2]}, v[3] = {vc[0], vc[1], vc[2]};
    int32_t n = nc;
    if (st == TEMPORAL_MERGED) temporal_merge(mc, vc, nc, mh, vh, nh, max_history, m, v, n);
    for (int k = 0; k < 3; k++) {
        out.m[3 * p + k] = m[k];
        out.v[3 * p + k] = v[k];
    }
    out.n[p] = n;
    out.shape[p] = shape;
    out.prim[p] = prim;
    out.depth[p] = M.depth[p];
    status[p] = st;
}

hipError_t launch_temporal_merge(int32_t W, int32_t H, const double* m, const double* v, const int32_t* n, const MotionOut& M,
                                 const TemporalSet& hist, bool have_history, int32_t max_history, double sigma_depth,
                                 const TemporalSet& out, int32_t* status, hipStream_t stream) {
    const uint64_t P = (uint64_t)W * (uint64_t)H;
    hipLaunchKernelGGL(k_temporal_merge, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, P, m, v, n, M, hist, have_history ? 1 : 0,
                       max_history, sigma_depth, out, status);
    return hipGetLastError();
}

}  // namespace pt
