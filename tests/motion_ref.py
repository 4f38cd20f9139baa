"""An independent restatement of ptsharp_amd/csrc/pt_motion.h in Python floats (IEEE fp64, no contraction): where a
surface point was one frame ago, its projection into the previous image, and the temporal merge of Welford states.
Test infrastructure, like denoise_ref: tests/test_motion_host.py compares the header's own functions with it on the
host, tests/test_gpu_motion.py compares pt_render_motion and pt_accumulate_temporal with it.

Every sum is made in the written order: a·b + c·d + e·f is ((a·b) + (c·d)) + (e·f).

  frame(o, d, hits, cur, prev, prev_cam, w, h) -> the seven arrays of pt_read_motion, flat [w*h]
      o, d          the camera rays (query_ref.camera_rays), float32 [w*h, 3]
      hits          pt_intersect_hits' t, kind, index, prim, shape for those rays
      cur, prev     the geometry the test itself sent, now and at the snapshot (geometry())
      prev_cam      the snapshot's camera (camera()); None: no snapshot (status 2)
  merge_frame(buf, hist, motion, max_history, sigma_depth) -> (M, V, N, status)
"""
from __future__ import annotations

import math

import numpy as np

INF = 1e9
OK, OUTSIDE, NO_SNAPSHOT = 0, 1, 2
MERGED, NO_HISTORY, MOTION, HISTORY_INVALID, IDENTITY, DEPTH, INVALID = 0, 1, 2, 3, 4, 5, 7
K_SPHERE, K_CUBE, K_PLANE, K_TRI, K_MESH, K_SDF, K_VOLUME, K_XFORM = range(8)   # pt_shape_kind
DBL_MAX = 1.7976931348623157e308


def finite(x):
    return abs(x) <= DBL_MAX   # False for NaN


def fl(a):
    return [float(x) for x in a]


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def div(a, b):
    """IEEE division, as C gives it for a zero divisor."""
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def point(o, d, t):
    return [o[k] + t * d[k] for k in range(3)]


def bary(o, d, v1, e1, e2):
    pvec = cross(d, e2)
    det = dot(e1, pvec)
    tvec = [o[k] - v1[k] for k in range(3)]
    u = div(dot(tvec, pvec), det)
    qvec = cross(tvec, e1)
    v = div(dot(d, qvec), det)
    return u, v


def tri_point(v1, e1, e2, u, v):
    return [(v1[k] + u * e1[k]) + v * e2[k] for k in range(3)]


def mat_point(m, x):
    return [((m[4 * r] * x[0] + m[4 * r + 1] * x[1]) + m[4 * r + 2] * x[2]) + m[4 * r + 3] for r in range(3)]


def sphere_point(P, c, r, c1, r1):
    s = div(r1, r)
    return [c1[k] + (P[k] - c[k]) * s for k in range(3)]


def cube_point(P, lo, hi, lo1, hi1):
    out = []
    for k in range(3):
        s = 0.0 if hi[k] == lo[k] else div(P[k] - lo[k], hi[k] - lo[k])
        out.append(lo1[k] + s * (hi1[k] - lo1[k]))
    return out


def xform_point(P, inv, m1):
    return mat_point(m1, mat_point(inv, P))


def camera(c):
    """A pt_camera (Camera.to_c()) as the header's MotionCamera."""
    return dict(p=fl(c.p), u=fl(c.u), v=fl(c.v), w=fl(c.w), m=float(c.m))


def project(cam, w, h, r):
    """-> ((x', y'), pixel, status)"""
    a, b, c = dot(r, cam["u"]), dot(r, cam["v"]), dot(r, cam["w"])
    if not c > 0.0 or not (finite(a) and finite(b) and finite(c)):
        return (-1.0, -1.0), -1, OUTSIDE
    aspect = float(w) / float(h)
    px = (-(a / c) * cam["m"]) / aspect
    py = -(b / c) * cam["m"]
    x = ((px + 1.0) / 2.0) * (float(w) - 1.0)
    y = ((py + 1.0) / 2.0) * (float(h) - 1.0)
    if not (finite(x) and finite(y)):
        return (-1.0, -1.0), -1, OUTSIDE
    qx, qy = math.floor(x + 0.5), math.floor(y + 0.5)
    if qx < 0 or qy < 0 or qx >= w or qy >= h:
        return (x, y), -1, OUTSIDE
    return (x, y), int(qx) + w * int(qy), OK


def project_point(cam, w, h, P1):
    """-> ((x', y'), prev_depth, pixel, status)"""
    r = [P1[k] - cam["p"][k] for k in range(3)]
    rr = dot(r, r)
    depth = math.sqrt(rr) if rr >= 0.0 else math.nan
    if not finite(depth):
        depth = INF
    xy, pixel, status = project(cam, w, h, r)
    return xy, depth, pixel, status


def near_pixel_edge(xy, eps=1e-9):
    """Is x' + 0.5 or y' + 0.5 within eps of an integer (the nearest pixel may differ by one rounding)?"""
    return any(abs((c + 0.5) - round(c + 0.5)) <= eps for c in xy)


# ------------------------------------------------------------------ a whole frame
def geometry(v1=None, v2=None, v3=None, sphere_center=None, sphere_radius=None, cube_min=None, cube_max=None,
             xf_matrix=None, xf_inverse=None):
    """The arrays a test sent, in pt_scene_desc order: triangles as float32 [n, 3] (world space for the world BVH's,
    object space for an instanced mesh's), matrices as float64 [n, 16] row-major."""
    f32 = lambda a: None if a is None else np.array(a, np.float32).reshape(-1, 3)   # copies: the caller's arrays move on
    f64 = lambda a, c: None if a is None else np.array(a, np.float64).reshape(-1, c)
    return dict(v1=f32(v1), v2=f32(v2), v3=f32(v3), sphere_center=f32(sphere_center),
                sphere_radius=None if sphere_radius is None else np.array(sphere_radius, np.float64).reshape(-1),
                cube_min=f32(cube_min), cube_max=f32(cube_max), xf_matrix=f64(xf_matrix, 16), xf_inverse=f64(xf_inverse, 16))


def tri_record(g, s):
    """{v1, e1, e2} of source triangle s as the device holds it: e1 = v2 − v1, e2 = v3 − v1 in fp32."""
    v1, v2, v3 = g["v1"][s], g["v2"][s], g["v3"][s]
    return fl(v1), fl(v2 - v1), fl(v3 - v1)


def mat_position_f32(m, b):
    """Matrix.MulPosition as the device maps a ray's origin: fp64 rows on the fp32 vector, rounded to fp32."""
    b = fl(b)
    return np.array([m[4 * r] * b[0] + m[4 * r + 1] * b[1] + m[4 * r + 2] * b[2] + m[4 * r + 3] for r in range(3)], np.float32)


def mat_direction_f32(m, b):
    """Matrix.MulDirection, normalised as Vector.Normalize does (fp32 length, fp32 division)."""
    b = fl(b)
    v = np.array([m[4 * r] * b[0] + m[4 * r + 1] * b[1] + m[4 * r + 2] * b[2] for r in range(3)], np.float32)
    n = np.float32(np.sqrt(np.float32(np.float32(np.float32(v[0] * v[0]) + np.float32(v[1] * v[1])) + np.float32(v[2] * v[2]))))
    return (v / n).astype(np.float32)


def previous_point(o, d, t, kind, index, prim, cur, prev, xf_is_mesh, object_ray=None):
    """P' of one hit.  object_ray(matrix_inverse, o, d) -> the fp32 object-space ray of an instance hit."""
    P = point(fl(o), fl(d), float(t))
    if kind == K_TRI:
        u, v = bary(fl(o), fl(d), *tri_record(cur, prim))
        return tri_point(*tri_record(prev, prim), u, v)
    if kind == K_SPHERE:
        return sphere_point(P, fl(cur["sphere_center"][index]), float(cur["sphere_radius"][index]),
                            fl(prev["sphere_center"][index]), float(prev["sphere_radius"][index]))
    if kind == K_CUBE:
        return cube_point(P, fl(cur["cube_min"][index]), fl(cur["cube_max"][index]), fl(prev["cube_min"][index]),
                          fl(prev["cube_max"][index]))
    if kind == K_XFORM:
        inv, m1 = fl(cur["xf_inverse"][index]), fl(prev["xf_matrix"][index])
        if not xf_is_mesh[index]:
            return xform_point(P, inv, m1)
        so, sd = object_ray(inv, o, d)
        u, v = bary(fl(so), fl(sd), *tri_record(cur, prim))
        return mat_point(m1, tri_point(*tri_record(prev, prim), u, v))
    return P   # plane, top-level SDFShape and Volume


def frame(o, d, hits, cur, prev, prev_cam, w, h, xf_is_mesh=()):
    n = w * h
    out = dict(shape=np.asarray(hits["shape"], np.int32).copy(), prim=np.asarray(hits["prim"], np.int32).copy(),
               depth=np.asarray(hits["t"], np.float64).copy(), prev_xy=np.full((n, 2), -1.0), prev_depth=np.full(n, INF),
               prev_pixel=np.full(n, -1, np.int32), status=np.full(n, NO_SNAPSHOT, np.int32))
    if prev_cam is None:
        return out
    object_ray = lambda inv, ro, rd: (mat_position_f32(inv, ro), mat_direction_f32(inv, rd))
    for i in range(n):
        if hits["t"][i] < INF:
            P1 = previous_point(o[i], d[i], hits["t"][i], int(hits["kind"][i]), int(hits["index"][i]), int(hits["prim"][i]),
                                cur, prev, xf_is_mesh, object_ray)
            xy, depth, pixel, status = project_point(prev_cam, w, h, P1)
        else:
            xy, pixel, status = project(prev_cam, w, h, fl(d[i]))
            depth = INF
        out["prev_xy"][i], out["prev_depth"][i], out["prev_pixel"][i], out["status"][i] = xy, depth, pixel, status
    return out


# ------------------------------------------------------------------ the temporal merge
def valid(m3, v3, n):
    return n >= 1 and all(finite(float(x)) for x in m3) and all(finite(float(x)) for x in v3)


def merge_status(cur_valid, have_history, motion_status, hist_valid, shape_p, prim_p, shape_q, prim_q, prev_depth_p,
                 hist_depth_q, sigma_depth):
    if not cur_valid:
        return INVALID
    if not have_history:
        return NO_HISTORY
    if motion_status != OK:
        return MOTION
    if not hist_valid:
        return HISTORY_INVALID
    if shape_p != shape_q or prim_p != prim_q:
        return IDENTITY
    if sigma_depth > 0.0 and abs(prev_depth_p - hist_depth_q) > sigma_depth * prev_depth_p:
        return DEPTH
    return MERGED


def merge(mc, vc, nc, mh, vh, nh, max_history):
    nh1 = min(int(nh), int(max_history), 2147483647 - int(nc))
    if nh1 <= 0:
        return fl(mc), fl(vc), int(nc)
    n = int(nc) + nh1
    m, v = [], []
    for k in range(3):
        vh1 = float(vh[k]) * ((float(nh1) - 1.0) / (float(nh) - 1.0)) if nh >= 2 else float(vh[k])
        delta = float(mh[k]) - float(mc[k])
        m.append(float(mc[k]) + delta * (float(nh1) / float(n)))
        v.append((float(vc[k]) + vh1) + (delta * delta) * ((float(nc) * float(nh1)) / float(n)))
    return m, v, n


def merge_frame(buf, hist, motion, max_history, sigma_depth):
    """buf: (M [P,3], V [P,3], N [P]); hist: None or dict(M, V, N, shape, prim, depth) of the previous result;
    motion: the arrays of Motion(), flat.  -> (M, V, N, status)"""
    M, V, N = (np.array(a).reshape(s) for a, s in zip(buf, ((-1, 3), (-1, 3), (-1,))))
    P = len(N)
    oM, oV, oN, st = M.copy(), V.copy(), N.copy(), np.zeros(P, np.int32)
    mo = {k: np.asarray(a).reshape((P, 2) if k == "prev_xy" else (P,)) for k, a in motion.items()}
    for p in range(P):
        q = int(mo["prev_pixel"][p])
        tap = hist is not None and mo["status"][p] == OK
        hv = tap and valid(hist["M"][q], hist["V"][q], int(hist["N"][q]))
        st[p] = merge_status(valid(M[p], V[p], int(N[p])), hist is not None, int(mo["status"][p]), hv, int(mo["shape"][p]),
                             int(mo["prim"][p]), int(hist["shape"][q]) if tap else -1, int(hist["prim"][q]) if tap else -1,
                             float(mo["prev_depth"][p]), float(hist["depth"][q]) if tap else 0.0, sigma_depth)
        if st[p] == MERGED:
            oM[p], oV[p], oN[p] = merge(M[p], V[p], int(N[p]), hist["M"][q], hist["V"][q], int(hist["N"][q]), max_history)
    return oM, oV, oN, st
