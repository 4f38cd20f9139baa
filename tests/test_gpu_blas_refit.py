"""pt_update_meshes on the GPU: every triangle of a scene moved, instanced meshes' included; their BLASes, the meshes'
boxes, the instances' world boxes and the analytic BVH refitted on the device.

  1. identity: an update with the upload's own arrays leaves every BLAS, triangle BVH and analytic BVH word as it was
     (the meshes' boxes as values), and a render after it is the render before it, bit for bit;
  2. after a pose the words are those of tests/blas_refit_ref.py, refit_ref.py and shape_refit_ref.py, the numpy
     restatements (each checked on the CPU against its native check): normals kept, given and FACE;
  3. SMOOTH: the BLAS shade rows are normals_ref.py's normals gathered by position;
  4. rays: pt_intersect / pt_occluded after an update against the oracle on the moved scene and against a context that
     uploaded the moved scene fresh, t bits and kinds;
  5. renders and features after an update against the oracle and the fresh upload; the pose makes the instances cover
     pixels they did not cover before (checked on the CPU), so a stale BLAS or world box fails;
  6. a scene without instanced mesh: UpdateMeshes is UpdateTriangles, word for word;
  7. sequences: pose A then B, both orders of UpdateMeshes and UpdateShapes, an upload between updates;
  8. the error cases leave the scene untouched; pt_update_triangles still refuses an instanced scene.
Scenes (the smallest that reach each path): R routed (an instanced 8-triangle mesh beside a 3200-triangle grid, an SDF,
a transformed Volume and sphere: heavy boxes), T two (a 1-triangle mesh, the lone-leaf root, and a 288-triangle mesh,
at least 3 BLAS levels, each instanced twice under a rotation and a non-uniform scale; the larger one a top-level shape
too), O only (the only triangles are instanced: no world triangle BVH), N none (no instanced mesh).  Frames are 64x48
at 2 spp.
"""
import ctypes as C

import numpy as np
import pytest

import blas_refit_ref as B
import features_ref as F
import normals_ref
import oracle_lib as O
import refit_ref
import shape_refit_ref as R
from parity import check, same_buffer, within
from ptsharp_amd import Renderer, TransformedShape, Vector, _abi
from ptsharp_amd.geometry import Box, Colour, Matrix
from ptsharp_amd.renderer import Buffer
from ptsharp_amd.scene import (Camera, Cube, DefaultSampler, Material, Mesh, Scene, SDFShape, Sphere, TorusSDF, Volume,
                               VolumeWindow, fix_normals_arrays)
from ptsharp_amd.scenes import volume_slices

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 48, 2
ENGINES = pytest.mark.parametrize("engine", [_abi.ENGINE_MEGAKERNEL, _abi.ENGINE_WAVEFRONT], ids=["mega", "wavefront"])
f32 = np.float32
GREY = lambda: Material.DiffuseMaterial(Colour(0.7, 0.7, 0.7))
BLUE = lambda: Material.DiffuseMaterial(Colour(0.2, 0.3, 0.8))
RED = lambda: Material.DiffuseMaterial(Colour(0.8, 0.3, 0.2))
LIGHT = lambda e=40: Material.LightMaterial(Colour.White, e)


def mesh_of(v1, v2, v3, material):
    z3 = np.zeros_like(v1)
    n1, n2, n3 = fix_normals_arrays(v1, v2, v3, z3, z3, z3)
    m = Mesh(*[np.ascontiguousarray(q, f32) for q in (v1, v2, v3, n1, n2, n3)])
    m.SetMaterial(material)
    return m


def grid_mesh(n, size, y, material):
    """2 n^2 triangles over [-size/2, size/2]^2 at height y, face normals."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="xy")
    x = (f32(size) * (i.astype(f32) / f32(n) - f32(0.5))).astype(f32)
    z = (f32(size) * (j.astype(f32) / f32(n) - f32(0.5))).astype(f32)
    yy = (f32(y) + f32(0.1) * np.sin(f32(3) * x) * np.cos(f32(2) * z)).astype(f32)
    p = np.stack([x, yy, z], axis=2)
    a, b, c, e = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]
    v1 = np.stack([a, b], axis=2).reshape(-1, 3)
    v2 = np.stack([c, c], axis=2).reshape(-1, 3)   # (a, c, b) and (b, c, e): normals up
    v3 = np.stack([b, e], axis=2).reshape(-1, 3)
    return mesh_of(v1, v2, v3, material)


def one_triangle(a, b, c, material):
    return mesh_of(*[np.array([p], f32) for p in (a, b, c)], material)


def placed(angle, scale, at):
    return Matrix.TranslateM(Vector(*at)).Mul(Matrix.RotateM(Vector(1, 1, 1), angle)).Mul(Matrix.ScaleM(Vector(*scale)))


CAMERA = lambda: Camera.LookAt(Vector(7, 6, 7), Vector(0, 1, 0), Vector(0, 1, 0), 45)


def scene_r():
    s = Scene()
    s.Add(grid_mesh(40, 6, 1.0, BLUE()))
    s.Add(Cube.NewCube(Vector(-8, -1, -8), Vector(8, 0, 8), GREY()))
    s.Add(Sphere.NewSphere(Vector(5, 5, 2), 0.75, LIGHT()))
    s.Add(SDFShape.NewSDFShape(TorusSDF.NewTorusSDF(f32(0.6), f32(0.2)), GREY()))
    win = [VolumeWindow(f32(0.2), f32(0.5), BLUE())]
    vol = Volume.NewVolume(Box(Vector(-0.5, -0.5, -0.5), Vector(0.5, 0.5, 0.5)), volume_slices(6, 6, 4, 3), f32(1), win)
    s.Add(TransformedShape.NewTransformedShape(vol, Matrix.TranslateM(Vector(2.5, 2, 1))))
    s.Add(TransformedShape.NewTransformedShape(Sphere.NewSphere(Vector(), 0.5, GREY()), Matrix.TranslateM(Vector(-2, 2, 2))))
    s.Add(TransformedShape.NewTransformedShape(grid_mesh(2, 1, 0, RED()), Matrix.TranslateM(Vector(-1, 2.5, -2))))
    return s, CAMERA(), DefaultSampler.NewSampler(4, 3)


def scene_t():
    s = Scene()
    s.Add(Cube.NewCube(Vector(-8, -1, -8), Vector(8, 0, 8), GREY()))
    s.Add(Sphere.NewSphere(Vector(5, 6, 2), 0.75, LIGHT()))
    big = grid_mesh(12, 2, 0.75, BLUE())
    s.Add(big)
    lone = one_triangle((-0.5, 0, -0.25), (0, 0.25, 0.75), (0.5, 0.125, 0), RED())
    stand_in = one_triangle((9, 9, 9), (9, 9.5, 9), (9.5, 9, 9), GREY())   # replaced by the top-level mesh below
    s.Add(TransformedShape.NewTransformedShape(lone, placed(0.4, (1.5, 0.75, 2.0), (-3, 2.5, 1))))
    s.Add(TransformedShape.NewTransformedShape(stand_in, placed(0.7, (1.25, 0.5, 0.8), (3, 2, -1))))
    s.Add(TransformedShape.NewTransformedShape(lone, placed(-1.1, (0.5, 2.0, 1.0), (1, 4, 3))))
    s.Add(TransformedShape.NewTransformedShape(stand_in, placed(2.1, (0.6, 1.5, 1.1), (-2, 3.5, -3))))
    flat = s.Compile()
    top = [int(j) for k, j in zip(flat.shape_kind, flat.shape_index) if k == _abi.SHAPE_MESH]
    assert len(top) == 1 and flat.mesh_count[top[0]] == 288
    for t in (1, 3):   # the larger mesh is a top-level shape and the inner mesh of two instances
        assert flat.transformed[t].shape_kind == _abi.SHAPE_MESH and flat.mesh_count[flat.transformed[t].shape_index] == 1
        flat.transformed[t].shape_index = top[0]
    return s, CAMERA(), DefaultSampler.NewSampler(4, 3)


def scene_o():
    s = Scene()
    s.Add(Cube.NewCube(Vector(-8, -1, -8), Vector(8, 0, 8), GREY()))
    s.Add(Sphere.NewSphere(Vector(5, 5, 2), 0.75, LIGHT()))
    s.Add(TransformedShape.NewTransformedShape(grid_mesh(3, 1.5, 0, RED()), placed(0.3, (1.0, 2.0, 1.0), (0.5, 2, 0.25))))
    return s, CAMERA(), DefaultSampler.NewSampler(4, 3)


def scene_n():
    s = Scene()
    s.Add(Cube.NewCube(Vector(-8, -1, -8), Vector(8, 0, 8), GREY()))
    s.Add(Sphere.NewSphere(Vector(5, 4, 2), 0.5, LIGHT()))
    s.Add(grid_mesh(10, 4, 0.5, BLUE()))
    s.Add(TransformedShape.NewTransformedShape(Sphere.NewSphere(Vector(), 0.5, GREY()), Matrix.TranslateM(Vector(-2, 2, 2))))
    return s, Camera.LookAt(Vector(7, 6, 7), Vector(0, 0.5, 0), Vector(0, 1, 0), 45), DefaultSampler.NewSampler(4, 3)


SCENES = {"R": scene_r, "T": scene_t, "O": scene_o, "N": scene_n}


def blas_meshes(flat):
    """The mesh of every BLAS, in the compile's order (first use by a transformed shape), and each transformed shape's BLAS."""
    meshes, xf_blas = [], []
    for t in range(flat.counts_ext[3]):
        x = flat.transformed[t]
        if x.shape_kind == _abi.SHAPE_MESH:
            if x.shape_index not in meshes:
                meshes.append(int(x.shape_index))
            xf_blas.append(meshes.index(x.shape_index))
        else:
            xf_blas.append(-1)
    return meshes, np.array(xf_blas, np.int32)


def instanced(flat):
    """Which source triangles belong to an instanced mesh."""
    on = np.zeros(len(flat.tri_material), bool)
    for j in blas_meshes(flat)[0]:
        on[int(flat.mesh_first[j]):int(flat.mesh_first[j]) + int(flat.mesh_count[j])] = True
    return on


def verts(flat):
    return [a.copy() for a in (flat.tri_v1, flat.tri_v2, flat.tri_v3)]


def pose(name, flat):
    """UpdateMeshes' arguments for a named pose of the scene as it stands: (v1, v2, v3), keywords."""
    v = verts(flat)
    inst = instanced(flat)
    kw = {}
    if name == "identity":
        pass
    elif name == "sine":      # every vertex displaced, the normals kept
        for a in v:
            a[:, 1] += (f32(0.3) * np.sin(f32(2.5) * a[:, 0] + f32(0.5)) * np.cos(f32(1.5) * a[:, 2])).astype(f32)
            a[:, 0] += (f32(0.1) * np.cos(f32(3) * a[:, 2])).astype(f32)
    elif name == "grow":      # the instanced meshes grown 2.5 times and lifted, the others displaced; normals given
        for a in v:
            a[inst] = (a[inst] * f32(2.5) + np.array([0.25, 0.5, -0.25], f32)).astype(f32)
            a[~inst, 1] += (f32(0.2) * np.sin(f32(2) * a[~inst, 0])).astype(f32)
        n = len(v[0])
        ang = (f32(0.01) * np.arange(n, dtype=f32)).astype(f32)
        kw = {"n1": np.stack([np.sin(ang), np.cos(ang), np.zeros(n, f32)], axis=1).astype(f32),
              "n2": np.stack([np.zeros(n, f32), np.cos(ang), np.sin(ang)], axis=1).astype(f32),
              "n3": np.broadcast_to(np.array([0.6, 0.8, 0.0], f32), (n, 3)).copy()}
    elif name in ("twist", "twist_smooth"):   # turned about y and widened; normals derived
        c, s_ = f32(np.cos(0.8) * 1.5), f32(np.sin(0.8) * 1.5)
        for a in v:
            x, z = a[:, 0].copy(), a[:, 2].copy()
            a[:, 0], a[:, 2] = (c * x - s_ * z).astype(f32), (s_ * x + c * z).astype(f32)
            a[inst, 1] += (f32(0.25) * np.sin(f32(2) * x[inst])).astype(f32)
        kw = {"normals": "face" if name == "twist" else "smooth"}
    else:
        raise KeyError(name)
    return [np.ascontiguousarray(a, f32) for a in v], kw


def apply_to_flat(flat, v, kw):
    """An update's arrays substituted into a FlatScene before it is uploaded: the fresh upload of the moved scene."""
    for dst, a in zip((flat.tri_v1, flat.tri_v2, flat.tri_v3), v):
        dst[...] = a
    if "n1" in kw:
        for dst, a in zip((flat.tri_n1, flat.tri_n2, flat.tri_n3), (kw["n1"], kw["n2"], kw["n3"])):
            dst[...] = a
    elif "normals" in kw:
        n = normals_ref.normals(*v, flat.mesh_first, flat.mesh_count, kw["normals"])
        for dst, a in zip((flat.tri_n1, flat.tri_n2, flat.tri_n3), n):
            dst[...] = a


def renderer(scene_tuple, engine=_abi.ENGINE_WAVEFRONT, seed=23):
    s, c, smp = scene_tuple
    r = Renderer.NewRenderer(s, c, smp, W, H, True, device=0)
    r.SamplesPerPixel, r.Seed, r.Engine = SPP, seed, engine
    return r


def frame(r):
    r.ResetBuffer()
    r.RenderParallel()
    b = r.ReadBuffer()
    out = Buffer(W, H)
    out.M, out.V, out.N = b.M.copy(), b.V.copy(), b.N.copy()
    return out, r.Stats().rays


def state(r):
    """Every word an update may touch: the BLASes, the triangle BVH, the analytic BVH and the lights."""
    return {"blas": r.ReadBlas(), "tri": r.ReadTriBvh(), "shape": r.ReadShapeBvh()}


def same_state(a, b, what="", boxes_as_values=True):
    for part in ("blas", "tri", "shape"):
        for i, (x, y) in enumerate(zip(a[part], b[part])):
            x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
            assert x.shape == y.shape, f"{what} {part}[{i}]: shape {x.shape} vs {y.shape}"
            if part == "blas" and i == 4 and boxes_as_values:   # the meshes' unpadded boxes: -0 == +0
                assert np.array_equal(x, y), f"{what} inner boxes differ: {x} vs {y}"
                continue
            wx = x.view(np.uint64 if x.dtype == np.float64 else np.uint32)
            wy = y.view(np.uint64 if y.dtype == np.float64 else np.uint32)
            bad = np.argwhere(wx != wy)
            assert not bad.size, f"{what} {part}[{i}]: {len(bad)} words differ, first at {bad[0]}"


def levels(nodes, n0=0):
    depth, level = 0, [0]
    while level:
        depth += 1
        level = [int(x) for n in level for x in nodes[n0 + n, 24:28] if x != R.EMPTY and not x & 0x80000000]
    return depth


def params(flat):
    nx = flat.counts_ext[3]
    return {"sphere_center": flat.sphere_center.copy(), "sphere_radius": flat.sphere_radius.copy(),
            "cube_min": flat.cube_min.copy(), "cube_max": flat.cube_max.copy(),
            "matrices": np.array([list(flat.transformed[i].matrix) for i in range(nx)], np.float64).reshape(-1, 4, 4),
            "inverses": np.array([list(flat.transformed[i].inverse) for i in range(nx)], np.float64).reshape(-1, 4, 4)}


class Upload:
    """What the references need from a context right after its upload, before an update writes into the FlatScene."""

    def __init__(self, r, flat):
        self.before = state(r)
        self.meshes, self.xf_blas = blas_meshes(flat)
        blas, _, recs, _, _ = self.before["blas"]
        self.blas_src = B.source_of_positions(blas, recs, flat.mesh_first, flat.mesh_count, self.meshes, *verts(flat))
        self.tri_src = refit_ref.src_of_pos_from(self.before["tri"][2], flat) if len(self.before["tri"][2]) else np.zeros(0, np.int32)
        tables = R.tables_from_flat(flat, self.before["shape"][1], self.before["shape"][2])
        self.tables = list(tables)

    def reference(self, flat, v, normals):
        """The state the numpy restatements expect after an update with v and normals (None: kept), the shape
        parameters being the FlatScene's."""
        b0, t0, s0 = self.before["blas"], self.before["tri"], self.before["shape"]
        nodes, recs, shade, boxes = B.refit(b0[0], b0[1], b0[2], b0[3], self.blas_src, *v, normals=normals)
        if len(t0[0]):
            tri = refit_ref.refit(t0[0], t0[1], t0[2], self.tri_src, *v, *(normals or ()))
        else:
            tri = t0
        tables = list(self.tables)
        tables[3] = B.inner_boxes(tables[3], self.xf_blas, boxes)
        p = params(flat)
        shape = R.refit(s0[0], s0[1], s0[2], s0[3], *tables, p["sphere_center"], p["sphere_radius"], p["cube_min"], p["cube_max"],
                        p["matrices"], p["inverses"])
        return {"blas": (b0[0], nodes, recs, shade, boxes), "tri": tri, "shape": shape}


# ------------------------------------------------------------------ 1. identity
@ENGINES
@pytest.mark.parametrize("name", ["R", "T", "O"])
def test_identity_on_the_device(gpu, engine, name):
    st = SCENES[name]()
    r = renderer(st, engine)
    try:
        flat = st[0].Compile()
        before = state(r)
        blas, nodes = before["blas"][0], before["blas"][1]
        if name == "R":
            assert len(blas) == 1 and len(before["blas"][2]) == 8 and len(before["shape"][2]) >= 3 and len(before["tri"][0]) > 64
        elif name == "T":
            assert len(blas) == 2 and blas[0, 1] == 1 and blas[1, 0] == 1 and blas[1, 2] == 1 and len(before["blas"][2]) == 289
            assert levels(nodes, int(blas[1, 0])) >= 3 and len(before["tri"][1]) > 0
        else:
            assert len(blas) == 1 and len(before["tri"][0]) == 0 and len(before["tri"][1]) == 0
        img0, rays0 = frame(r)
        ms = r.UpdateMeshes(*verts(flat), flat.tri_n1.copy(), flat.tri_n2.copy(), flat.tri_n3.copy())
        assert ms > 0
        same_state(state(r), before, "identity, normals given")
        r.UpdateMeshes(*verts(flat))
        same_state(state(r), before, "identity, normals kept")
        img1, rays1 = frame(r)
        assert rays0 == rays1
        same_buffer(img1, img0)
    finally:
        r.close()


# ------------------------------------------------------------------ 2. bytes after a pose
BYTES = [(s, p) for s in ("R", "T", "O") for p in ("sine", "grow", "twist")]


@pytest.mark.parametrize("name,pname", BYTES, ids=[f"{a}-{b}" for a, b in BYTES])
def test_bytes_after_a_pose(gpu, name, pname):
    st = SCENES[name]()
    r = renderer(st)
    try:
        flat = st[0].Compile()
        up = Upload(r, flat)
        v, kw = pose(pname, flat)
        r.UpdateMeshes(*v, **kw)
        assert np.array_equal(flat.tri_v2, v[1])   # written into the FlatScene in place
        normals = None
        if "n1" in kw:
            normals = (kw["n1"], kw["n2"], kw["n3"])
        elif "normals" in kw:
            normals = tuple(normals_ref.normals(*v, flat.mesh_first, flat.mesh_count, kw["normals"]))
            inst = instanced(flat)
            for got, want in zip((flat.tri_n1, flat.tri_n2, flat.tri_n3), normals):   # the derived normals, read back
                normals_ref.same_bits(got[inst], want[inst], "normals of instanced triangles in the FlatScene")
        got = state(r)
        same_state(got, up.reference(flat, v, normals), f"{name} {pname}")
        b0 = up.before["blas"]
        assert not np.array_equal(got["blas"][1], b0[1]) and np.array_equal(got["blas"][1][:, 24:], b0[1][:, 24:])
        assert np.array_equal(got["blas"][3][:, 9], b0[3][:, 9])   # the material word
        if normals is None:
            assert np.array_equal(got["blas"][3], b0[3])
        assert not np.array_equal(got["shape"][0], up.before["shape"][0])   # the instances' world boxes moved
    finally:
        r.close()


# ------------------------------------------------------------------ 3. SMOOTH
@pytest.mark.parametrize("name", ["T", "O"])
def test_smooth_normals_in_the_blas(gpu, name):
    st = SCENES[name]()
    r = renderer(st)
    try:
        flat = st[0].Compile()
        up = Upload(r, flat)
        v, kw = pose("twist_smooth", flat)
        r.UpdateMeshes(*v, **kw)
        want = normals_ref.normals(*v, flat.mesh_first, flat.mesh_count, "smooth")
        face = normals_ref.normals(*v, flat.mesh_first, flat.mesh_count, "face")
        shade = r.ReadBlas()[3]
        for k in range(3):
            normals_ref.same_bits(shade[:, 3 * k:3 * k + 3].view(f32), want[k][up.blas_src], f"{name} smooth n{k + 1}")
        big = up.blas_src[-1]   # a triangle of the grid: its smooth normals are not its face normals
        assert not np.array_equal(want[0][big], face[0][big]) or not np.array_equal(want[1][big], face[1][big])
        got = state(r)
        ref = up.reference(flat, v, tuple(want))
        same_state(got, ref, f"{name} smooth")   # and every other word, the smooth normals given
    finally:
        r.close()


# ------------------------------------------------------------------ 4. rays
def moved_box(flat):
    """The world box of the instances after the pose: their meshes' vertices through their matrices."""
    pts = []
    for t in range(flat.counts_ext[3]):
        x = flat.transformed[t]
        if x.shape_kind != _abi.SHAPE_MESH:
            continue
        f, n = int(flat.mesh_first[x.shape_index]), int(flat.mesh_count[x.shape_index])
        p = np.concatenate([flat.tri_v1[f:f + n], flat.tri_v2[f:f + n], flat.tri_v3[f:f + n]]).astype(np.float64)
        m = np.array(list(x.matrix)).reshape(4, 4)
        pts.append(p @ m[:3, :3].T + m[:3, 3])
    pts = np.concatenate(pts)
    return pts.min(axis=0), pts.max(axis=0)


def rays_at(lo, hi, n, seed):
    """Rays from a shell around the box [lo, hi] to points inside it."""
    rng = np.random.default_rng(seed)
    c, ext = (lo + hi) / 2, np.maximum((hi - lo) / 2, 0.5)
    u = rng.standard_normal((n, 3))
    o = c + 4.0 * np.abs(ext).max() * u / np.linalg.norm(u, axis=1, keepdims=True)
    t = (c - ext) + 2 * ext * rng.random((n, 3))
    o, t = o.astype(f32), t.astype(f32)
    d = (t - o).astype(f32)
    d = (d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(f32)
    return o, d


def oracle_rays(oscene, o, d):
    ot, ok = np.empty(len(o), np.float64), np.empty(len(o), np.int32)
    for i in range(len(o)):
        ot[i], ok[i], _ = oscene.intersect(o[i], d[i])
    return ot, ok


# the floors: the oracle's own counts of rays that hit an instance (kind TRANSFORMED), measured on the CPU with these
# scenes, poses and seeds (R 2,151, T 741, O 1,733 of 4,096; most of the rest hit the floor cube under them), less a tenth
RAYS = [("R", "grow", 1935), ("T", "grow", 666), ("O", "grow", 1559)]


@pytest.mark.parametrize("name,pname,floor", RAYS, ids=[f"{a}-{b}" for a, b, _ in RAYS])
def test_rays_after_an_update(gpu, name, pname, floor):
    st, st2 = SCENES[name](), SCENES[name]()
    flat2 = st2[0].Compile()
    v2, kw2 = pose(pname, flat2)
    apply_to_flat(flat2, v2, kw2)   # the moved scene, uploaded fresh
    r, fresh = renderer(st), renderer(st2)
    try:
        flat = st[0].Compile()
        v, kw = pose(pname, flat)
        r.UpdateMeshes(*v, **kw)
        o, d = rays_at(*moved_box(flat), 4096, 31)
        t, k = r.Intersect(o, d)
        os_ = O.OracleScene(st[0])   # the FlatScene the update wrote into
        ot, ok = oracle_rays(os_, o, d)
        bad = np.flatnonzero((t.view(np.int64) != ot.view(np.int64)) | (k != ok))
        assert bad.size == 0, (f"{bad.size} of {len(o)} rays differ from the oracle, first {bad[:5]}: gpu t {t[bad[:3]]} "
                               f"kind {k[bad[:3]]}, oracle t {ot[bad[:3]]} kind {ok[bad[:3]]}")
        hits = int((ok == _abi.SHAPE_TRANSFORMED).sum())
        print(f"{name} {pname}: {hits} rays hit an instance")
        assert hits >= floor, f"only {hits} rays hit an instance"
        ft, fk = fresh.Intersect(o, d)
        assert np.array_equal(t.view(np.int64), ft.view(np.int64)) and np.array_equal(k, fk), "against the fresh upload"
        rng = np.random.default_rng(7)
        tl = np.where(ot < 1e9, ot, 5.0)
        for what, tm in {"at_hit": tl, "past_hit": np.nextafter(tl, np.inf), "random": tl * rng.uniform(0.0, 1.6, len(tl))}.items():
            want = np.array([os_.any_nearer(o[i], d[i], tm[i]) for i in range(len(o))], np.int32)
            got = r.Occluded(o, d, tm)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, f"occluded {what}: {bad.size} rays differ, first {bad[:5]}"
    finally:
        r.close()
        fresh.close()


# ------------------------------------------------------------------ 5. renders and features
@ENGINES
@pytest.mark.parametrize("name", ["R", "T", "O"])
def test_render_parity_after_an_update(gpu, engine, name):
    st, st2 = SCENES[name](), SCENES[name]()
    flat2 = st2[0].Compile()
    v2, kw2 = pose("grow", flat2)
    apply_to_flat(flat2, v2, kw2)   # the moved scene, uploaded fresh
    r, fresh = renderer(st, engine), renderer(st2, engine)
    try:
        rest_kind = F.features(st[0], st[1], W, H)[3].copy()
        frame(r)                        # a pass at the rest pose first: the update comes between passes
        v, kw = pose("grow", st[0].Compile())
        r.UpdateMeshes(*v, **kw)
        want = F.features(st[0], st[1], W, H)
        # on the CPU: the grown instances cover pixels they did not cover at rest, so a stale BLAS or box shows
        newly = (want[3] == _abi.SHAPE_TRANSFORMED) & (rest_kind != _abi.SHAPE_TRANSFORMED)
        assert newly.sum() >= 20, f"the pose uncovers only {int(newly.sum())} pixels"
        g, grays = frame(r)
        o, orays = O.render(O.OracleScene(st[0]), st[1], st[2], W, H, SPP, seed=23)
        check(g, grays, o, orays)
        f, frays = frame(fresh)
        assert grays == frays
        assert np.array_equal(g.N, f.N)
        for a, b, what in ((g.M, f.M, "M"), (g.V, f.V, "V")):
            frac, err = within(a, b)
            assert frac >= 0.999, f"{what} against the fresh upload: {frac:.5f} within 1e-9, max err {err:.3g}"
        lit = g.M.sum(axis=2) > 0
        assert lit.mean() > 0.5
        if engine == _abi.ENGINE_WAVEFRONT:
            r.RenderFeatures()
            got = r.Features()
            for a, b, what in zip(got, want, ("albedo", "normal", "depth", "kind", "material")):
                if what == "albedo":
                    assert (np.abs(a - b) <= 1e-9 * np.maximum(1.0, np.abs(b))).all(), what
                else:
                    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"features after the update: {what} differs"
    finally:
        r.close()
        fresh.close()


# ------------------------------------------------------------------ 6. no instanced mesh
@pytest.mark.parametrize("pname", ["sine", "grow", "twist", "twist_smooth"])
def test_without_instanced_mesh_is_update_triangles(gpu, pname):
    sa, sb = scene_n(), scene_n()
    r, r2 = renderer(sa), renderer(sb)
    try:
        assert len(r.ReadBlas()[0]) == 0
        v, kw = pose(pname, sa[0].Compile())
        ms = r.UpdateMeshes(*v, **kw)
        r2.UpdateTriangles(*v, **kw)
        assert ms > 0
        same_state(state(r), state(r2), f"UpdateMeshes against UpdateTriangles, {pname}", boxes_as_values=False)
        for x, y in zip(r.ReadTriNormals(), r2.ReadTriNormals()):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        for x, y in zip((sa[0].Compile().tri_n1, sa[0].Compile().tri_v3), (sb[0].Compile().tri_n1, sb[0].Compile().tri_v3)):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        same_buffer(frame(r)[0], frame(r2)[0])
    finally:
        r.close()
        r2.close()


# ------------------------------------------------------------------ 7. sequences and lifecycle
def spun(flat):
    spin = Matrix.TranslateM(Vector(0.5, 0.75, -0.25)).Mul(Matrix.RotateM(Vector(1, 1, 1), 0.7))
    return {"matrices": [spin.Mul(Matrix(m)).m for m in params(flat)["matrices"]]}


def test_pose_a_then_pose_b_is_pose_b(gpu):
    sa, sb = scene_t(), scene_t()
    r, r2 = renderer(sa), renderer(sb)
    try:
        va, kwa = pose("twist", sa[0].Compile())
        r.UpdateMeshes(*va, **kwa)
        vb, kwb = pose("grow", sb[0].Compile())   # from the rest pose, normals given: nothing of pose A stays
        r.UpdateMeshes(*vb, **kwb)
        r2.UpdateMeshes(*vb, **kwb)
        same_state(state(r), state(r2), "A then B against B")
        same_buffer(frame(r)[0], frame(r2)[0])
    finally:
        r.close()
        r2.close()


def test_meshes_then_shapes_is_shapes_then_meshes_is_the_fresh_upload(gpu):
    sa, sb, sc = scene_t(), scene_t(), scene_t()
    fc = sc[0].Compile()
    vc, kwc = pose("grow", fc)
    apply_to_flat(fc, vc, kwc)
    for i, m in enumerate(spun(fc)["matrices"]):
        fc.transformed[i].matrix[:] = np.asarray(m, np.float64).reshape(-1).tolist()
        fc.transformed[i].inverse[:] = Matrix(m).Inverse().m.reshape(-1).tolist()
    r, r2, fresh = renderer(sa), renderer(sb), renderer(sc)
    try:
        fa, fb = sa[0].Compile(), sb[0].Compile()
        v, kw = pose("grow", fa)
        r.UpdateMeshes(*v, **kw)
        r.UpdateShapes(**spun(fa))    # sees the new inner boxes, on the device and in the host's tables
        r2.UpdateShapes(**spun(fb))
        r2.UpdateMeshes(*v, **kw)     # refits the shapes from the current matrices
        same_state(state(r), state(r2), "either order")
        img, rays = frame(r)
        same_buffer(img, frame(r2)[0])
        o, d = rays_at(*moved_box(fa), 2048, 5)
        t, k = r.Intersect(o, d)
        ft, fk = fresh.Intersect(o, d)
        assert np.array_equal(t.view(np.int64), ft.view(np.int64)) and np.array_equal(k, fk)
        assert (k == _abi.SHAPE_TRANSFORMED).sum() > 0
        f, frays = frame(fresh)
        assert rays == frays and np.array_equal(img.N, f.N)
        for a, b, what in ((img.M, f.M, "M"), (img.V, f.V, "V")):
            frac, err = within(a, b)
            assert frac >= 0.999, f"{what} against the fresh upload: {frac:.5f} within 1e-9, max err {err:.3g}"
    finally:
        r.close()
        r2.close()
        fresh.close()


def test_update_upload_update(gpu):
    """An update, an upload of another scene (other counts, other BLASes), an update of that one: the second update
    uses the second upload's tables."""
    st = scene_r()
    r = renderer(st)
    try:
        v, kw = pose("grow", st[0].Compile())
        r.UpdateMeshes(*v, **kw)
        s2, _, _ = scene_t()
        r.Scene = s2
        flat = s2.Compile()
        up = Upload(r, flat)          # uploads the new scene
        assert len(up.before["blas"][0]) == 2
        v2, kw2 = pose("sine", flat)
        r.UpdateMeshes(*v2, **kw2)
        same_state(state(r), up.reference(flat, v2, None), "after the second upload")
        with pytest.raises(ValueError):
            r.UpdateMeshes(*v)        # the first scene's count
    finally:
        r.close()


def test_every_entry_point_then_an_upload_of_another_size(gpu):
    """One context through the entry points that move an instanced scene (so the shape, BLAS, refit and pose workspaces
    exist and their kept layouts were used), then an upload of a scene with other counts on the same context: an
    update of that scene leaves the device bit for bit as it leaves a fresh context."""
    from ptsharp_amd import scenes
    st, st2, st3 = scenes.instances(copies=2, mesh_tris=200), scenes.instances(copies=3, mesh_tris=120), scenes.instances(copies=3, mesh_tris=120)
    r, fresh = renderer(st), renderer(st3)
    try:
        flat = st[0].Compile()
        v, kw = pose("grow", flat)
        r.UpdateMeshes(*v, **kw)
        r.UpdateShapes(**spun(flat))
        r.SetRestPose()
        r.PoseMeshes([Matrix.TranslateM(Vector(0.5, -0.25, 1)).Mul(Matrix.RotateM(Vector(1, 2, 3), 1.1))], mirror=False)
        r.Scene = st2[0]   # uploaded by the next call
        v2, kw2 = pose("twist_smooth", st3[0].Compile())
        r.UpdateMeshes(*v2, **kw2)
        fresh.UpdateMeshes(*v2, **kw2)
        assert len(r.ReadBlas()[0]) == 1
        same_state(state(r), state(fresh), "after the second upload", boxes_as_values=False)
    finally:
        r.close()
        fresh.close()


# ------------------------------------------------------------------ 8. errors and the refusal
def test_errors_leave_the_scene_untouched(gpu):
    st = scene_t()
    r = renderer(st)
    fp = C.POINTER(C.c_float)
    try:
        assert r._lib.pt_get_version() == 10
        flat = st[0].Compile()
        before = state(r)
        img0, _ = frame(r)
        v, kw = pose("grow", flat)
        keep = v + [kw["n1"], kw["n2"], kw["n3"]]
        a, b, c, n1, n2, n3 = [x.ctypes.data_as(fp) for x in keep]
        n = len(v[0])
        U, two = _abi.pt_mesh_update, (C.c_int32 * 2)
        ms = C.c_double(-1.0)
        call = lambda ctx, u: r._lib.pt_update_meshes(ctx, None if u is None else C.byref(u), C.byref(ms))
        cases = {
            "NULL ctx": lambda: call(None, U(n, 0, two(0, 0), a, b, c, n1, n2, n3)),
            "NULL u": lambda: call(r._ctx, None),
            "NULL v1": lambda: call(r._ctx, U(n, 0, two(0, 0), None, b, c)),
            "NULL v2": lambda: call(r._ctx, U(n, 0, two(0, 0), a, None, c)),
            "NULL v3": lambda: call(r._ctx, U(n, 0, two(0, 0), a, b, None)),
            "reserved[0]": lambda: call(r._ctx, U(n, 0, two(1, 0), a, b, c)),
            "reserved[1]": lambda: call(r._ctx, U(n, 0, two(0, 7), a, b, c)),
            "mode 3": lambda: call(r._ctx, U(n, 3, two(0, 0), a, b, c)),
            "mode -1": lambda: call(r._ctx, U(n, -1, two(0, 0), a, b, c)),
            "n2 missing": lambda: call(r._ctx, U(n, 0, two(0, 0), a, b, c, n1, None, n3)),
            "n1 only": lambda: call(r._ctx, U(n, 0, two(0, 0), a, b, c, n1, None, None)),
            "normals with FACE": lambda: call(r._ctx, U(n, _abi.NORMALS_FACE, two(0, 0), a, b, c, n1, n2, n3)),
            "normals with SMOOTH": lambda: call(r._ctx, U(n, _abi.NORMALS_SMOOTH, two(0, 0), a, b, c, n1, n2, n3)),
            "one triangle fewer": lambda: call(r._ctx, U(n - 1, 0, two(0, 0), a, b, c)),
            "one triangle more": lambda: call(r._ctx, U(n + 1, _abi.NORMALS_FACE, two(0, 0), a, b, c)),
        }
        for what, fn in cases.items():
            assert fn() == _abi.PT_ERR_INVALID_ARG, what
            same_state(state(r), before, what, boxes_as_values=False)
            same_buffer(frame(r)[0], img0)
        # the refusal stays: pt_update_triangles and pt_update_triangles_normals on an instanced scene
        with pytest.raises(_abi.PTError) as e:
            r.UpdateTriangles(*v)
        assert e.value.code == _abi.PT_ERR_UNSUPPORTED and "instanced mesh" in str(e.value)
        assert r._lib.pt_update_triangles_normals(r._ctx, n, a, b, c, _abi.NORMALS_FACE, None) == _abi.PT_ERR_UNSUPPORTED
        same_state(state(r), before, "refused", boxes_as_values=False)
        same_buffer(frame(r)[0], img0)
        # a refused call between two updates changes nothing
        r.UpdateMeshes(*v, **kw)
        mid = state(r)
        with pytest.raises(_abi.PTError):
            r.UpdateTriangles(*verts(flat))
        same_state(state(r), mid, "refused between updates", boxes_as_values=False)
        r.UpdateMeshes(*v, **kw)
        same_state(state(r), mid, "the same update again", boxes_as_values=False)
    finally:
        r.close()
    # no scene
    r = Renderer.NewRenderer(None, None, None, W, H, True, device=0)
    try:
        z = np.zeros((1, 3), f32).ctypes.data_as(fp)
        u = _abi.pt_mesh_update(1, 0, (C.c_int32 * 2)(0, 0), z, z, z)
        assert r._lib.pt_update_meshes(r._ctx, C.byref(u), None) == _abi.PT_ERR_NO_SCENE
        assert r._lib.pt_read_blas(r._ctx, None, None, None, None, None, None) == _abi.PT_ERR_NO_SCENE
    finally:
        r.close()
