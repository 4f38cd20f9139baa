"""The expected answers of pt_intersect_hits, built ray by ray with the CPU oracle's exported pieces: test
infrastructure, like features_ref.

Per ray:
  or_intersect(brute=1)   t, the shape kind and the index in the host's own numbering (a triangle: its tri_v1 row)
  or_hit_info             Hit.Info's position, the normal after the flip, inside, the material id
  or_hit_surface          the Material.MaterialAt colour and gloss
  or_environment          the albedo of a miss
  shape                   derived here from the scene description (slots): the Scene.Shapes slot of the hit
  prim                    index for a triangle; for a hit through an instanced mesh the triangle of that mesh whose
                          material is the hit's, where the mesh's materials differ per triangle (else PRIM_UNKNOWN:
                          nothing the oracle exports names it); -1 otherwise

  expected(oscene, o, d, brute=True) -> dict of arrays named as _abi.HIT_ARRAYS
A miss: t 1e9; kind, index, prim, shape, material -1; position, normal 0; inside, gloss 0; albedo the environment.
or_hit_info and or_hit_surface describe the hit of the oracle's k-d walk.  With brute=True, a ray at which the walk's
(t, kind, index) is not the loop's (degenerate rays) has no exported Hit.Info of the loop's hit: its
material is INFO_UNKNOWN, prim of an instance hit PRIM_UNKNOWN and the other Hit.Info fields 0.  The camera-ray cases
have no such ray (tests/test_query_host.py).

camera_rays(camera, w, h): or_cast_ray at (0.5, 0.5) with no lens, pixel by pixel in row-major order.
prim_t(flat, kind, index, o, d): or_prim_intersect of a sphere, cube, plane or triangle of the description itself,
the definition of a valid `index`: the reported primitive's own intersect gives the reported t.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import features_ref as F
import oracle_lib as O
from ptsharp_amd import _abi

HIT_INF = 1e9
PRIM_UNKNOWN = -2
INFO_UNKNOWN = -2   # material of a hit whose Hit.Info the oracle does not export: see expected()
f32 = np.float32


def slots(flat):
    """The slot tables of the description, as the compile makes them (pt_scene_compile.h QueryTables), restated:
    (tri_slot [num_triangles], {kind: slot per index} for the analytic kinds and the planes).  -1: in no slot; the
    first slot wins.  A triangle: its PT_SHAPE_TRIANGLE slot, else the slot of the last mesh range that holds it,
    else the first slot of a mesh that holds it."""
    kinds, idxs = np.asarray(flat.shape_kind), np.asarray(flat.shape_index)
    d = flat.desc
    counts = {_abi.SHAPE_SPHERE: d.num_spheres, _abi.SHAPE_CUBE: d.num_cubes, _abi.SHAPE_PLANE: d.num_planes,
              _abi.SHAPE_SDF: d.num_sdf_shapes, _abi.SHAPE_VOLUME: d.num_volumes, _abi.SHAPE_TRANSFORMED: d.num_transformed}
    by_kind = {k: np.full(n, -1, np.int32) for k, n in counts.items()}
    nt, nm = d.num_triangles, d.num_meshes
    loose, mesh_slot = np.full(nt, -1, np.int32), np.full(nm, -1, np.int32)
    for i in range(d.num_shapes):
        k, j = int(kinds[i]), int(idxs[i])
        table = loose if k == _abi.SHAPE_TRIANGLE else mesh_slot if k == _abi.SHAPE_MESH else by_kind[k]
        if table[j] < 0:
            table[j] = i
    first, count = np.asarray(flat.mesh_first)[:nm], np.asarray(flat.mesh_count)[:nm]
    group = np.full(nt, -1, np.int32)
    for m in range(nm):
        group[first[m]:first[m] + count[m]] = m
    tri_slot = loose.copy()
    for t in np.flatnonzero(tri_slot < 0):
        if group[t] >= 0 and mesh_slot[group[t]] >= 0:
            tri_slot[t] = mesh_slot[group[t]]
            continue
        holds = [mesh_slot[m] for m in range(nm) if mesh_slot[m] >= 0 and first[m] <= t < first[m] + count[m]]
        tri_slot[t] = min(holds) if holds else -1
    return tri_slot, by_kind


def camera_rays(camera, w, h):
    L = F._lib()
    cam = camera.to_c()
    cam.aperture_radius = 0.0
    o, d = np.zeros((h * w, 3), f32), np.zeros((h * w, 3), f32)
    co, cd = (C.c_float * 3)(), (C.c_float * 3)()
    for y in range(h):
        for x in range(w):
            L.or_cast_ray(C.byref(cam), x, y, w, h, 0.5, 0.5, 0, co, cd)
            o[y * w + x], d[y * w + x] = co[:], cd[:]
    return o, d


def expected(oscene, o, d, brute=True, info=True):
    L = F._lib()
    flat = oscene.flat
    n = len(o)
    out = {name: np.zeros((n, c) if c > 1 else n, dt) for name, (dt, c) in _abi.HIT_ARRAYS.items()}
    out["t"][:] = HIT_INF
    for name in ("kind", "index", "prim", "shape", "material"):
        out[name][:] = -1
    tri_slot, by_kind = slots(flat)
    tri_material = np.asarray(flat.tri_material)
    first, count = np.asarray(flat.mesh_first), np.asarray(flat.mesh_count)
    xf = flat.desc.transformed
    fo, fd, pos, nrm = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)()
    k, idx, inside, mat = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    col, gloss = (C.c_double * 3)(), C.c_double()
    for i in range(n):
        fo[:], fd[:] = o[i].tolist(), d[i].tolist()
        t = L.or_intersect(oscene.h, fo, fd, int(brute), C.byref(k), C.byref(idx))
        if not t < HIT_INF:
            if info:
                L.or_environment(oscene.h, fd, col)
                out["albedo"][i] = col[:]
            continue
        out["t"][i], out["kind"][i], out["index"][i] = t, k.value, idx.value
        if k.value == _abi.SHAPE_TRIANGLE:
            out["prim"][i], out["shape"][i] = idx.value, tri_slot[idx.value]
        else:
            out["shape"][i] = by_kind[k.value][idx.value]
        if not info:
            continue
        if brute:
            wk, wi = C.c_int32(), C.c_int32()
            wt = L.or_intersect(oscene.h, fo, fd, 0, C.byref(wk), C.byref(wi))
            if (np.float64(wt).view(np.int64), wk.value, wi.value) != (np.float64(t).view(np.int64), k.value, idx.value):
                out["material"][i] = INFO_UNKNOWN
                if k.value == _abi.SHAPE_TRANSFORMED and xf[idx.value].shape_kind == _abi.SHAPE_MESH:
                    out["prim"][i] = PRIM_UNKNOWN
                continue
        assert L.or_hit_info(oscene.h, fo, fd, pos, nrm, C.byref(inside), C.byref(mat)) == 1
        assert L.or_hit_surface(oscene.h, fo, fd, col, C.byref(gloss)) == 1
        out["position"][i], out["normal"][i] = pos[:], nrm[:]
        out["inside"][i], out["material"][i] = inside.value, mat.value
        out["albedo"][i], out["gloss"][i] = col[:], gloss.value
        if k.value == _abi.SHAPE_TRANSFORMED and xf[idx.value].shape_kind == _abi.SHAPE_MESH:
            m = xf[idx.value].shape_index
            mats = tri_material[first[m]:first[m] + count[m]]
            at = np.flatnonzero(mats == mat.value)
            out["prim"][i] = first[m] + at[0] if len(at) == 1 and len(set(mats.tolist())) == len(mats) else PRIM_UNKNOWN
    return out


def prim_t(flat, kind, index, o, d, tris=None):
    """or_prim_intersect of primitive `index` of `kind` (sphere, cube, plane, triangle) with its own parameters from
    the description (tris: (v1, v2, v3) to take a triangle's vertices from instead, e.g. after an update)."""
    L = O.lib()
    z = O.f3((0, 0, 0))
    fo, fd = O.f3(o), O.f3(d)
    if kind == _abi.SHAPE_SPHERE:
        return L.or_prim_intersect(kind, O.f3(flat.sphere_center[index]), z, z, float(flat.sphere_radius[index]), fo, fd)
    if kind == _abi.SHAPE_CUBE:
        return L.or_prim_intersect(kind, O.f3(flat.cube_min[index]), O.f3(flat.cube_max[index]), z, 0.0, fo, fd)
    if kind == _abi.SHAPE_PLANE:
        return L.or_prim_intersect(kind, O.f3(flat.plane_point[index]), O.f3(flat.plane_normal[index]), z, 0.0, fo, fd)
    assert kind == _abi.SHAPE_TRIANGLE
    v1, v2, v3 = tris if tris is not None else (flat.tri_v1, flat.tri_v2, flat.tri_v3)
    return L.or_prim_intersect(kind, O.f3(v1[index]), O.f3(v2[index]), O.f3(v3[index]), 0.0, fo, fd)


def valid_index_failures(flat, hits, o, d, tris=None):
    """The rays whose reported primitive (kind sphere, cube, plane or triangle) does not give the reported t, bit for
    bit, by its own or_prim_intersect: [(ray, kind, index, reported t, own t)]."""
    bad = []
    for i in np.flatnonzero(np.isin(hits["kind"], (0, 1, 2, 3))):
        own = prim_t(flat, int(hits["kind"][i]), int(hits["index"][i]), o[i], d[i], tris)
        if np.float64(own).view(np.int64) != hits["t"][i:i + 1].view(np.int64)[0]:
            bad.append((int(i), int(hits["kind"][i]), int(hits["index"][i]), float(hits["t"][i]), own))
    return bad


CAMERA_CASES = [(name, w, h) for name in F.SCENES for w, h in F.SIZES]


@functools.lru_cache(maxsize=None)
def camera_case(name, w, h):
    """(o, d, expected arrays) of features_ref.SCENES[name] at w x h, computed once and read-only."""
    s, c, _ = F.scene_of(name)
    o, d = camera_rays(c, w, h)
    want = expected(F.oracle_of(name), o, d)
    for a in (o, d, *want.values()):
        a.setflags(write=False)
    return o, d, want
