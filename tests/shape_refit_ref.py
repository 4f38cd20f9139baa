"""A numpy restatement of pt_update_shapes (ptsharp_amd/csrc/pt_shape_refit.h and pt_scene_compile.cpp
shape_refit_lights) in fp32 / fp64, each operation rounded on its own: the four steps of the device kernels
(transformed shapes, records, heavy records, BVH4 levels) and the host's lights.  tests/test_shape_refit_host.py
checks it against tests/native/shapes_check.cpp's dump; the GPU tests compare the device against it word for word.

Layouts: nodes [N, 32] uint32 (pt_bvh.h: lo.x[4] hi.x[4] lo.y[4] hi.y[4] lo.z[4] hi.z[4] refs[4] 0[4]), records
[R, 12] uint32 (kind in word 3, scene index in word 7, material in word 8), heavy [H, 8] uint32 (record index in word
3), lights [L, 4] float64 (centre, radius)."""
import numpy as np

F = np.float32
SPHERE, CUBE, MESH, SDF, VOLUME, XFORM = 0, 1, 4, 5, 6, 7
EMPTY = 0x7FFFFFFF


def pad_box(lo, hi):
    """pad_box (pt_scene_compile.cpp) on float32 [..., 3] arrays."""
    with np.errstate(all="ignore"):
        m = np.maximum(np.abs(lo), np.abs(hi)).astype(F)
        e = (m * F(2.0e-6)).astype(F) + F(1e-30)
        return (lo - e).astype(F), (hi + e).astype(F)


def sphere_box(c, r):
    with np.errstate(all="ignore"):
        cc = c.astype(np.float64)
        lo = np.nextafter((cc - r[..., None]).astype(F), F(-np.inf))
        hi = np.nextafter((cc + r[..., None]).astype(F), F(np.inf))
    return pad_box(lo, hi)


def _net_min(a, b):   # Math.Min on double: -0 < +0
    return np.where(a != b, np.where(a < b, a, b), np.where(np.signbit(a), a, b))


def _net_max(a, b):
    return np.where(a != b, np.where(b < a, a, b), np.where(np.signbit(b), a, b))


def mat_box(m, mn, mx):
    """Matrix.MulBox (pt_ext.h mat_box): m [16] float64, mn / mx [3] float32."""
    m = np.asarray(m, np.float64).reshape(-1)
    col = lambda k: np.array([m[k], m[4 + k], m[8 + k]], np.float64).astype(F)
    muls = lambda v, s: (v.astype(np.float64) * float(s)).astype(F)
    lo = hi = None
    for k in range(3):
        a, b = muls(col(k), mn[k]), muls(col(k), mx[k])
        l = _net_min(a.astype(np.float64), b.astype(np.float64)).astype(F)
        h = _net_max(a.astype(np.float64), b.astype(np.float64)).astype(F)
        lo = l if lo is None else (lo + l).astype(F)
        hi = h if hi is None else (hi + h).astype(F)
    t = col(3)
    return (lo + t).astype(F), (hi + t).astype(F)


def march_pad(kind):
    return 2e-3 if kind == SDF else 4.0 / 512 if kind == VOLUME else 0.0


def inner_box(kind, index, inner_static, sphere_center, sphere_radius, cube_min, cube_max):
    if kind == SPHERE:
        c, r = sphere_center[index].astype(np.float64), sphere_radius[index]
        return (c - r).astype(F), (c + r).astype(F)
    if kind == CUBE:
        return cube_min[index], cube_max[index]
    return inner_static[:3], inner_static[3:]


def xform_boxes(m, kind, imn, imx):
    """(padded BVH box lo, hi; unpadded BoundingBox mn, mx) of a transformed shape."""
    bmn, bmx = mat_box(m, imn, imx)
    mp = march_pad(kind)
    pmn, pmx = (imn.astype(np.float64) - mp).astype(F), (imx.astype(np.float64) + mp).astype(F)
    lo, hi = mat_box(m, pmn, pmx)
    lo, hi = pad_box(lo, hi)
    return lo, hi, bmn, bmx


def box_light(mn, mx):
    """light_sphere_of_box: Box.Center and Box.OuterRadius in fp32."""
    c = (mn + ((mx - mn).astype(F) * F(0.5)).astype(F)).astype(F)
    d = (mn - c).astype(F)
    sq = (d * d).astype(F)
    return c, float(np.sqrt(((sq[0] + sq[1]).astype(F) + sq[2]).astype(F)))


def sphere_rows(c, r, index, mat):
    rb = np.array([r], np.float64).view(np.uint32)
    cw = np.ascontiguousarray(c, F).view(np.uint32)
    return np.array([cw[0], cw[1], cw[2], SPHERE, 0, 0, 0, index, mat, rb[0], rb[1], 0], np.uint32)


def cube_rows(mn, mx, index, mat):
    a, b = np.ascontiguousarray(mn, F).view(np.uint32), np.ascontiguousarray(mx, F).view(np.uint32)
    return np.array([a[0], a[1], a[2], CUBE, b[0], b[1], b[2], index, mat, 0, 0, 0], np.uint32)


def refit(nodes0, recs0, heavy0, lights0, rec_box0, xf_kind, xf_index, xf_inner_box, light_kind, light_index,
          sphere_center, sphere_radius, cube_min, cube_max, xf_matrix, xf_inverse, ext0=None):
    """The device state after an update with these (complete) parameters: nodes, records, heavy records, lights, and
    the ext records when ext0 is given."""
    sc, sr = np.asarray(sphere_center, F).reshape(-1, 3), np.asarray(sphere_radius, np.float64).reshape(-1)
    ca, cb = np.asarray(cube_min, F).reshape(-1, 3), np.asarray(cube_max, F).reshape(-1, 3)
    xm = np.asarray(xf_matrix, np.float64).reshape(-1, 16)
    nodes, recs, heavy, lights = nodes0.copy(), recs0.copy(), heavy0.copy(), np.array(lights0, np.float64).reshape(-1, 4)
    ext = None if ext0 is None else ext0.copy()
    inner_static = np.asarray(xf_inner_box, F).reshape(-1, 6)
    # 1. transformed shapes
    nx = len(xm)
    xbox = np.zeros((nx, 6), F)
    bounds = np.zeros((nx, 6), F)
    for t in range(nx):
        k, j = int(xf_kind[t]), int(xf_index[t])
        imn, imx = inner_box(k, j, inner_static[t], sc, sr, ca, cb)
        lo, hi, bmn, bmx = xform_boxes(xm[t], k, imn, imx)
        xbox[t] = np.concatenate([lo, hi])
        bounds[t] = np.concatenate([bmn, bmx])
        if ext is not None and k == SPHERE:
            ext[t] = sphere_rows(sc[j], sr[j], ext[t, 7], ext[t, 8])
        elif ext is not None and k == CUBE:
            ext[t] = cube_rows(ca[j], cb[j], ext[t, 7], ext[t, 8])
    # 2. records
    rec_box = np.array(rec_box0, F).reshape(-1, 6).copy()
    for i in range(len(recs)):
        k, j = int(recs[i, 3]), int(recs[i, 7])
        if k == SPHERE:
            recs[i] = sphere_rows(sc[j], sr[j], recs[i, 7], recs[i, 8])
            lo, hi = sphere_box(sc[j], sr[j:j + 1].reshape(()))
        elif k == CUBE:
            recs[i] = cube_rows(ca[j], cb[j], recs[i, 7], recs[i, 8])
            lo, hi = pad_box(ca[j], cb[j])
        elif k == XFORM:
            lo, hi = xbox[j, :3], xbox[j, 3:]
        else:
            continue
        rec_box[i] = np.concatenate([lo, hi])
    # 3. heavy records
    for h in range(len(heavy)):
        i = int(heavy[h, 3])
        heavy[h, 0:3] = rec_box[i, :3].view(np.uint32)
        heavy[h, 4:7] = rec_box[i, 3:].view(np.uint32)
        heavy[h, 7] = 0
    # 4. the BVH4, children before parents (a child's index is greater than its parent's)
    node_box = np.zeros((len(nodes), 6), F)
    for n in range(len(nodes) - 1, -1, -1):
        lo_all, hi_all = np.full(3, np.inf, F), np.full(3, -np.inf, F)
        for k in range(4):
            ref = int(nodes[n, 24 + k])
            if ref == EMPTY:
                continue
            if ref & 0x80000000:
                first, cnt = ref & 0x1FFFFFFF, ((ref >> 29) & 3) + 1
                lo, hi = rec_box[first:first + cnt, :3].min(axis=0), rec_box[first:first + cnt, 3:].max(axis=0)
            else:
                lo, hi = node_box[ref, :3], node_box[ref, 3:]
            for ax in range(3):
                nodes[n, 8 * ax + k] = lo[ax:ax + 1].view(np.uint32)[0]
                nodes[n, 8 * ax + 4 + k] = hi[ax:ax + 1].view(np.uint32)[0]
            lo_all, hi_all = np.minimum(lo_all, lo), np.maximum(hi_all, hi)
        node_box[n] = np.concatenate([lo_all, hi_all])
    # the lights, on the host
    for i in range(len(lights)):
        k, j = int(light_kind[i]), int(light_index[i])
        if k == SPHERE:
            lights[i] = [*sc[j].astype(np.float64), sr[j]]
        elif k == CUBE:
            c, r = box_light(ca[j], cb[j])
            lights[i] = [*c.astype(np.float64), r]
        elif k == XFORM:
            c, r = box_light(bounds[j, :3].copy(), bounds[j, 3:].copy())
            lights[i] = [*c.astype(np.float64), r]
    if ext is not None:
        return nodes, recs, heavy, lights, ext
    return nodes, recs, heavy, lights


def tables_from_flat(flat, recs0, heavy0):
    """The host tables of a compiled FlatScene that `refit` needs, recomputed from the scene and from the device's
    words at the upload: (rec_box0, xf_kind, xf_index, xf_inner_box, light_kind, light_index).  Inner shapes: spheres,
    cubes, Volumes and meshes; lights: spheres, cubes, transformed spheres and cubes (others are left where they
    are: light_kind -1)."""
    nrec = len(recs0)
    rec_box0 = np.zeros((nrec, 6), F)
    for h in range(len(heavy0)):   # SDF, Volume and transformed records: their upload box is the heavy record's
        i = int(heavy0[h, 3])
        rec_box0[i, :3] = heavy0[h, 0:3].view(F)
        rec_box0[i, 3:] = heavy0[h, 4:7].view(F)
    nx = flat.counts_ext[3]
    xf_kind, xf_index = np.zeros(nx, np.int32), np.zeros(nx, np.int32)
    xf_inner = np.zeros((nx, 6), F)
    for t in range(nx):
        x = flat.transformed[t]
        xf_kind[t], xf_index[t] = x.shape_kind, x.shape_index
        if x.shape_kind == VOLUME:
            v = flat.volumes[x.shape_index]
            xf_inner[t] = [*v.box_min, *v.box_max]
        elif x.shape_kind == MESH:
            f, n = int(flat.mesh_first[x.shape_index]), int(flat.mesh_count[x.shape_index])
            pts = np.concatenate([flat.tri_v1[f:f + n], flat.tri_v2[f:f + n], flat.tri_v3[f:f + n]])
            xf_inner[t] = [*pts.min(axis=0), *pts.max(axis=0)]
        elif x.shape_kind not in (SPHERE, CUBE):
            raise NotImplementedError(f"inner kind {x.shape_kind}")
    light_kind, light_index = [], []
    emits = lambda mat: flat.materials[int(mat)].emittance > 0
    for k, j in zip(flat.shape_kind, flat.shape_index):
        k, j = int(k), int(j)
        if k == SPHERE:
            mat = flat.sphere_material[j]
        elif k == CUBE:
            mat = flat.cube_material[j]
        elif k == 2:
            mat = flat.plane_material[j]
        elif k == 3:
            mat = flat.tri_material[j]
        elif k == SDF:
            mat = flat.sdf_shapes[j].material
        elif k == XFORM:
            ik, ij = flat.transformed[j].shape_kind, flat.transformed[j].shape_index
            if ik == SPHERE:
                mat = flat.sphere_material[ij]
            elif ik == CUBE:
                mat = flat.cube_material[ij]
            else:
                continue   # a transformed Volume's or mesh's light is not restated here (the test scenes have none)
        else:
            continue       # a mesh never registers; a Volume light is not restated here
        if emits(mat):
            moves = k in (SPHERE, CUBE, XFORM)
            light_kind.append(k if moves else -1)
            light_index.append(j if moves else -1)
    return rec_box0, xf_kind, xf_index, xf_inner, np.array(light_kind, np.int32), np.array(light_index, np.int32)
