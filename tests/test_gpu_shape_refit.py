"""pt_update_shapes on the GPU: spheres, cubes and transformed shapes moved, the analytic BVH4 refitted on the device.

  1. identity: an update with the upload's own parameters leaves every node, record, heavy record and light word
     as it was, and a render after it is the render before it, bit for bit;
  2. after each pose the words are those of tests/shape_refit_ref.py, the numpy restatement (itself checked on the
     CPU against the native check, tests/test_shape_refit_host.py);
  3. rays: pt_intersect / pt_occluded after an update against the oracle on the moved scene, t bits and kinds;
  4. renders and features after an update against the oracle and against a context that uploaded the moved scene
     fresh (the light moves to the far side of the floor: a stale DevLight fails);
  5. sequences of updates, an upload between updates, both orders of UpdateTriangles and UpdateShapes, one group given;
  6. the error cases leave the scene untouched.
Scenes (the smallest that reach each path): A beads (302 records, at least 3 BVH4 levels), B few (3 records: the
kernels test them linearly), C routed (6 records, heavy boxes, a triangle BVH above 64 nodes), D instances (the FULL
BVH path with transformed leaves; four transforms share an inner sphere that is a top-level shape too).  Frames are
64x48 at 2 spp.
"""
import ctypes as C
import math

import numpy as np
import pytest

import features_ref as F
import oracle_lib as O
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
LIGHT = lambda e=40: Material.LightMaterial(Colour.White, e)


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
    z3 = np.zeros_like(v1)
    n1, n2, n3 = fix_normals_arrays(v1, v2, v3, z3, z3, z3)
    m = Mesh(*[np.ascontiguousarray(q, f32) for q in (v1, v2, v3, n1, n2, n3)])
    m.SetMaterial(material)
    return m


def scene_a():
    s = Scene()
    s.Add(Cube.NewCube(Vector(-8, -1, -8), Vector(8, 0, 8), GREY()))
    for k in range(5):
        for i in range(60):
            a = 0.21 * i + 1.3 * k
            s.Add(Sphere.NewSphere(Vector(3 * math.cos(a) + 0.4 * k, 0.3 + 0.05 * i, 3 * math.sin(a)), 0.1, BLUE() if i % 7 == 0 else GREY()))
    s.Add(Sphere.NewSphere(Vector(5, 4, 2), 0.75, LIGHT()))
    return s, Camera.LookAt(Vector(7, 6, 7), Vector(0, 1, 0), Vector(0, 1, 0), 45), DefaultSampler.NewSampler(4, 3)


def scene_b():
    s = Scene()
    s.Add(Cube.NewCube(Vector(-8, -1, -8), Vector(8, 0, 8), GREY()))
    s.Add(Sphere.NewSphere(Vector(5, 4, 2), 0.5, LIGHT()))
    s.Add(Sphere.NewSphere(Vector(4, 5, -3), 0.25, LIGHT(80)))
    s.Add(grid_mesh(10, 4, 0.5, BLUE()))
    return s, Camera.LookAt(Vector(7, 6, 7), Vector(0, 0.5, 0), Vector(0, 1, 0), 45), DefaultSampler.NewSampler(4, 3)


def scene_c():
    s = Scene()
    s.Add(grid_mesh(40, 6, 1.0, BLUE()))
    s.Add(Cube.NewCube(Vector(-8, -1, -8), Vector(8, 0, 8), GREY()))
    s.Add(Sphere.NewSphere(Vector(5, 5, 2), 0.75, LIGHT()))
    s.Add(SDFShape.NewSDFShape(TorusSDF.NewTorusSDF(f32(0.6), f32(0.2)), GREY()))
    win = [VolumeWindow(f32(0.2), f32(0.5), BLUE())]
    vol = Volume.NewVolume(Box(Vector(-0.5, -0.5, -0.5), Vector(0.5, 0.5, 0.5)), volume_slices(6, 6, 4, 3), f32(1), win)
    s.Add(TransformedShape.NewTransformedShape(vol, Matrix.TranslateM(Vector(2.5, 2, 1))))
    s.Add(TransformedShape.NewTransformedShape(Sphere.NewSphere(Vector(), 0.5, GREY()), Matrix.TranslateM(Vector(-2, 2, 2))))
    s.Add(TransformedShape.NewTransformedShape(grid_mesh(2, 1, 0, GREY()), Matrix.TranslateM(Vector(-1, 2.5, -2))))
    return s, Camera.LookAt(Vector(7, 6, 7), Vector(0, 1, 0), Vector(0, 1, 0), 45), DefaultSampler.NewSampler(4, 3)


SHARED = 1   # scene D: the sphere index four transforms share with a top-level shape


def scene_d():
    s = Scene()
    s.Add(Cube.NewCube(Vector(-10, -1, -10), Vector(10, 0, 10), GREY()))
    s.Add(Sphere.NewSphere(Vector(0.25, 0.5, -0.125), 0.3, BLUE()))
    for i in range(49):
        s.Add(Sphere.NewSphere(Vector(0.37 * (i % 10) - 4, 0.4 + 0.3 * (i // 10), 0.5 * (i % 7) - 3), 0.15 + 0.01 * i, GREY()))
    s.Add(Sphere.NewSphere(Vector(4, 7, 3), 0.6, LIGHT()))   # the fiftieth sphere lights the frame
    for i in range(60):
        m = Matrix.TranslateM(Vector(0.9 * (i % 8) - 3, 1 + 0.5 * (i // 8) + (3 if i < 4 else 0), 0.7 * (i % 5) + 1))
        if i < 4 or i % 2:
            inner = Sphere.NewSphere(Vector(), 0.2, BLUE())
        else:
            inner = Cube.NewCube(Vector(-0.2, -0.1, -0.15), Vector(0.2, 0.1, 0.15), LIGHT(60) if i == 10 else GREY())
        s.Add(TransformedShape.NewTransformedShape(inner, m))
    flat = s.Compile()
    assert flat.shape_kind[SHARED] == _abi.SHAPE_SPHERE and flat.shape_index[SHARED] == 0
    for t in range(4):   # the first four transforms take the top-level sphere 0 as their inner shape
        assert flat.transformed[t].shape_kind == _abi.SHAPE_SPHERE
        flat.transformed[t].shape_index = 0
    return s, Camera.LookAt(Vector(6, 7, 9), Vector(0, 1.5, 1), Vector(0, 1, 0), 45), DefaultSampler.NewSampler(4, 3)


SCENES = {"A": scene_a, "B": scene_b, "C": scene_c, "D": scene_d}


def params(flat):
    """The scene's parameters now: the six arrays of an update (copies)."""
    nx = flat.counts_ext[3]
    return {"sphere_center": flat.sphere_center.copy(), "sphere_radius": flat.sphere_radius.copy(),
            "cube_min": flat.cube_min.copy(), "cube_max": flat.cube_max.copy(),
            "matrices": np.array([list(flat.transformed[i].matrix) for i in range(nx)], np.float64).reshape(-1, 4, 4),
            "inverses": np.array([list(flat.transformed[i].inverse) for i in range(nx)], np.float64).reshape(-1, 4, 4)}


def spin():
    return Matrix.TranslateM(Vector(0.5, 0.75, -0.25)).Mul(Matrix.RotateM(Vector(1, 1, 1), 0.7))


def pose(name, flat):
    """An update's arguments (UpdateShapes keywords) for a named pose of the scene as it stands."""
    p = params(flat)
    out = {}
    lights = np.array([flat.materials[int(m)].emittance > 0 for m in flat.sphere_material], bool)
    if name == "identity":
        out = p
    elif name == "translate":
        t = np.array([1000, -2000, 3000], f32)
        out = {"sphere_center": p["sphere_center"] + t, "cube_min": p["cube_min"] + t, "cube_max": p["cube_max"] + t,
               "matrices": [Matrix.TranslateM(Vector(1000, -2000, 3000)).Mul(Matrix(m)).m for m in p["matrices"]]}
    elif name == "swap":
        out = {"sphere_center": p["sphere_center"][::-1]}
    elif name == "point":
        out = {"sphere_center": np.broadcast_to(np.array([0.5, 1.5, -0.5], f32), p["sphere_center"].shape)}
    elif name in ("huge", "tiny"):
        f = 1e6 if name == "huge" else 1e-6
        out = {"sphere_center": p["sphere_center"] * f32(f), "sphere_radius": p["sphere_radius"] * f,
               "cube_min": p["cube_min"] * f32(f), "cube_max": p["cube_max"] * f32(f),
               "matrices": [Matrix.ScaleM(Vector(f, f, f)).Mul(Matrix(m)).m for m in p["matrices"]]}
    elif name == "lit":   # the lights to the far side of the floor
        c = p["sphere_center"]
        c[lights] = c[lights] * np.array([-1, 1, -1], f32)
        out = {"sphere_center": c}
    elif name == "spin":
        out = {"matrices": [spin().Mul(Matrix(m)).m for m in p["matrices"]]}
    elif name == "spin_shared":   # scene D: every transform spun, the shared inner sphere moved and grown
        c, r = p["sphere_center"], p["sphere_radius"]
        c[0] += np.array([0.5, -0.25, 0.125], f32)
        r[0] *= 1.75
        out = {"sphere_center": c, "sphere_radius": r, "matrices": [spin().Mul(Matrix(m)).m for m in p["matrices"]]}
    else:
        raise KeyError(name)
    if "matrices" in out and not len(p["matrices"]):
        del out["matrices"]
        out.pop("inverses", None)
    if "cube_min" in out and not len(p["cube_min"]):
        del out["cube_min"], out["cube_max"]
    return out


def apply_to_flat(flat, kw):
    """The arrays of an update substituted into a FlatScene before it is uploaded: the fresh upload of the moved scene."""
    for k in ("sphere_center", "sphere_radius", "cube_min", "cube_max"):
        if k in kw:
            getattr(flat, k)[...] = kw[k]
    for i, m in enumerate(kw.get("matrices", [])):
        flat.transformed[i].matrix[:] = np.asarray(m, np.float64).reshape(-1).tolist()
        inv = kw["inverses"][i] if "inverses" in kw else Matrix(m).Inverse().m
        flat.transformed[i].inverse[:] = np.asarray(inv, np.float64).reshape(-1).tolist()


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


def same_words(a, b, what=""):
    for name, x, y in zip(("nodes", "records", "heavy", "lights"), a, b):
        x = np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint32)
        y = np.ascontiguousarray(y).view(np.uint64 if y.dtype == np.float64 else np.uint32)
        assert x.shape == y.shape, f"{what} {name}: shape {x.shape} vs {y.shape}"
        bad = np.argwhere(x != y)
        assert not bad.size, f"{what} {name}: {len(bad)} words differ, first at {bad[0]}: {x[tuple(bad[0])]:#x} vs {y[tuple(bad[0])]:#x}"


def reference(flat, before):
    """tests/shape_refit_ref.py on the words of the upload and the parameters the FlatScene holds now."""
    tables = R.tables_from_flat(flat, before[1], before[2])
    p = params(flat)
    return R.refit(before[0], before[1], before[2], before[3], *tables, p["sphere_center"], p["sphere_radius"], p["cube_min"],
                   p["cube_max"], p["matrices"], p["inverses"])


def levels(nodes):
    depth, level = 0, [0]
    while level:
        depth += 1
        level = [int(r) for n in level for r in nodes[n, 24:28] if r != R.EMPTY and not r & 0x80000000]
    return depth


# ------------------------------------------------------------------ 1. identity
@ENGINES
@pytest.mark.parametrize("name", ["A", "C"])
def test_identity_on_the_device(gpu, engine, name):
    st = SCENES[name]()
    r = renderer(st, engine)
    try:
        before = r.ReadShapeBvh()
        if name == "A":
            assert len(before[1]) == 302 and levels(before[0]) >= 3
        else:
            assert len(before[1]) <= 8 and len(before[2]) >= 3 and len(r.ReadTriBvh()[0]) > 64
        img0, rays0 = frame(r)
        ms = r.UpdateShapes(**pose("identity", st[0].Compile()))
        assert ms > 0
        same_words(r.ReadShapeBvh(), before, "identity")
        img1, rays1 = frame(r)
        assert rays0 == rays1
        same_buffer(img1, img0)
    finally:
        r.close()


# ------------------------------------------------------------------ 2. bytes after each pose
BYTES = [("A", p) for p in ("translate", "swap", "point", "huge", "tiny", "lit")] + \
        [("B", p) for p in ("translate", "lit")] + [("C", p) for p in ("translate", "spin", "lit", "tiny")] + \
        [("D", p) for p in ("translate", "swap", "spin", "spin_shared", "huge")]


@pytest.mark.parametrize("name,pname", BYTES, ids=[f"{a}-{b}" for a, b in BYTES])
def test_bytes_after_a_pose(gpu, name, pname):
    st = SCENES[name]()
    r = renderer(st)
    try:
        flat = st[0].Compile()
        before = r.ReadShapeBvh()
        kw = pose(pname, flat)
        r.UpdateShapes(**kw)
        for k in ("sphere_center", "cube_max"):
            if k in kw:
                assert np.array_equal(getattr(flat, k), np.asarray(kw[k], f32))   # written into the FlatScene in place
        got = r.ReadShapeBvh()
        same_words(got, reference(flat, before), f"{name} {pname}")
        assert not np.array_equal(got[0], before[0]) and np.array_equal(got[0][:, 24:], before[0][:, 24:])
    finally:
        r.close()


# ------------------------------------------------------------------ 3. rays
def moved_box(flat):
    """The box of the shapes an update moves: top-level spheres and the transformed shapes' origins, padded."""
    pts = []
    for k, j in zip(flat.shape_kind, flat.shape_index):
        if k == _abi.SHAPE_SPHERE and not flat.materials[int(flat.sphere_material[j])].emittance > 0:
            pts += [flat.sphere_center[j] - f32(flat.sphere_radius[j]), flat.sphere_center[j] + f32(flat.sphere_radius[j])]
        elif k == _abi.SHAPE_TRANSFORMED:
            m = np.array(list(flat.transformed[j].matrix)).reshape(4, 4)
            pts += [m[:3, 3] - 0.5, m[:3, 3] + 0.5]
    pts = np.array(pts, np.float64)
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


def root_box(nodes):
    used = nodes[0, 24:28] != R.EMPTY
    b = nodes[0, :24].view(f32).reshape(3, 2, 4)[:, :, used]
    return b[:, 0].min(axis=1), b[:, 1].max(axis=1)


def oracle_rays(oscene, o, d):
    ot, ok = np.empty(len(o), np.float64), np.empty(len(o), np.int32)
    for i in range(len(o)):
        ot[i], ok[i], _ = oscene.intersect(o[i], d[i])
    return ot, ok


# the floors: the oracle's own counts of rays that hit a moved shape (a sphere or a transformed shape), measured on
# the CPU with these scenes, poses and seeds (A swap 594, A translate 597, C spin 235, D spin_shared 712 of 4,096; most
# of the rest hit the floor cube under them), less a tenth
RAYS = [("A", "swap", 534), ("A", "translate", 537), ("C", "spin", 211), ("D", "spin_shared", 640)]


@pytest.mark.parametrize("name,pname,floor", RAYS, ids=[f"{a}-{b}" for a, b, _ in RAYS])
def test_rays_after_an_update(gpu, name, pname, floor):
    st = SCENES[name]()
    r = renderer(st)
    try:
        flat = st[0].Compile()
        old_lo, old_hi = root_box(r.ReadShapeBvh()[0])
        r.UpdateShapes(**pose(pname, flat))
        o, d = rays_at(*moved_box(flat), 4096, 31)
        outside_old = ((o < old_lo) | (o > old_hi)).any(axis=1)
        assert outside_old.sum() > 1000
        t, k = r.Intersect(o, d)
        os_ = O.OracleScene(st[0])   # the FlatScene the update wrote into
        ot, ok = oracle_rays(os_, o, d)
        bad = np.flatnonzero((t.view(np.int64) != ot.view(np.int64)) | (k != ok))
        assert bad.size == 0, (f"{bad.size} of {len(o)} rays differ from the oracle, first {bad[:5]}: gpu t {t[bad[:3]]} "
                               f"kind {k[bad[:3]]}, oracle t {ot[bad[:3]]} kind {ok[bad[:3]]}")
        hits = int(((ok == _abi.SHAPE_SPHERE) | (ok == _abi.SHAPE_TRANSFORMED)).sum())
        print(f"{name} {pname}: {hits} rays hit a moved shape, {int(outside_old.sum())} from outside the old root box")
        assert hits >= floor, f"only {hits} rays hit a moved shape"
        rng = np.random.default_rng(7)
        tl = np.where(ot < 1e9, ot, 5.0)
        for what, tm in {"at_hit": tl, "past_hit": np.nextafter(tl, np.inf), "random": tl * rng.uniform(0.0, 1.6, len(tl))}.items():
            want = np.array([os_.any_nearer(o[i], d[i], tm[i]) for i in range(len(o))], np.int32)
            got = r.Occluded(o, d, tm)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, f"occluded {what}: {bad.size} rays differ, first {bad[:5]}"
    finally:
        r.close()


# ------------------------------------------------------------------ 4. renders and features
RENDERS = [("A", "lit"), ("B", "lit"), ("C", "spin"), ("D", "spin")]


@ENGINES
@pytest.mark.parametrize("name,pname", RENDERS, ids=[f"{a}-{b}" for a, b in RENDERS])
def test_render_parity_after_an_update(gpu, engine, name, pname):
    st, st2 = SCENES[name](), SCENES[name]()
    apply_to_flat(st2[0].Compile(), pose(pname, st2[0].Compile()))   # the moved scene, uploaded fresh
    r, fresh = renderer(st, engine), renderer(st2, engine)
    try:
        frame(r)                        # a pass at the rest pose first: the update comes between passes
        r.UpdateShapes(**pose(pname, st[0].Compile()))
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
            want = F.features(st[0], st[1], W, H)
            for a, b, what in zip(got, want, ("albedo", "normal", "depth", "kind", "material")):
                if what == "albedo":
                    assert (np.abs(a - b) <= 1e-9 * np.maximum(1.0, np.abs(b))).all(), what
                else:
                    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"features after the update: {what} differs"
    finally:
        r.close()
        fresh.close()


# ------------------------------------------------------------------ 5. sequences and lifecycle
def test_pose_a_then_pose_b_is_pose_b(gpu):
    sa, sb = scene_d(), scene_d()
    r, r2 = renderer(sa), renderer(sb)
    try:
        rest = {k: v for k, v in params(sb[0].Compile()).items() if k != "inverses"}
        b = {**rest, **pose("spin_shared", sb[0].Compile())}   # every group: what pose A moved and B leaves comes back
        r.UpdateShapes(**pose("translate", sa[0].Compile()))
        r.UpdateShapes(**b)
        r2.UpdateShapes(**b)
        same_words(r.ReadShapeBvh(), r2.ReadShapeBvh(), "A then B against B")
        same_buffer(frame(r)[0], frame(r2)[0])
    finally:
        r.close()
        r2.close()


def test_update_upload_update(gpu):
    """An update, an upload of another scene (other counts, another BVH), an update of that one: the second update
    uses the second upload's tables."""
    st = scene_a()
    r = renderer(st)
    try:
        r.UpdateShapes(**pose("swap", st[0].Compile()))
        s2, _, _ = scene_d()
        r.Scene = s2
        before = r.ReadShapeBvh()      # uploads the new scene
        flat = s2.Compile()
        assert len(before[1]) == 112
        r.UpdateShapes(**pose("spin", flat))
        same_words(r.ReadShapeBvh(), reference(flat, before), "after the second upload")
        with pytest.raises(ValueError):
            r.UpdateShapes(sphere_center=st[0].Compile().sphere_center)      # the first scene's count
    finally:
        r.close()


def test_triangles_then_shapes_is_shapes_then_triangles(gpu):
    sa, sb = scene_b(), scene_b()
    r, r2 = renderer(sa), renderer(sb)
    try:
        fa, fb = sa[0].Compile(), sb[0].Compile()
        v = [np.ascontiguousarray(a + np.array([0.25, 0.5, -0.25], f32)) for a in (fa.tri_v1, fa.tri_v2, fa.tri_v3)]
        r.UpdateTriangles(*v)
        r.UpdateShapes(**pose("lit", fa))
        r2.UpdateShapes(**pose("lit", fb))
        r2.UpdateTriangles(*v)
        same_words(r.ReadShapeBvh(), r2.ReadShapeBvh(), "either order")
        for x, y in zip(r.ReadTriBvh(), r2.ReadTriBvh()):
            assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
        same_buffer(frame(r)[0], frame(r2)[0])
    finally:
        r.close()
        r2.close()


def test_one_group_given_leaves_the_others(gpu):
    st = scene_d()
    r = renderer(st)
    try:
        flat = st[0].Compile()
        before = r.ReadShapeBvh()
        r.UpdateShapes(**pose("spin_shared", flat))
        radii, cubes, mats = flat.sphere_radius.copy(), flat.cube_min.copy(), params(flat)["matrices"]
        r.UpdateShapes(sphere_center=flat.sphere_center[::-1].copy())
        assert np.array_equal(flat.sphere_radius, radii) and np.array_equal(flat.cube_min, cubes)
        assert np.array_equal(params(flat)["matrices"], mats)
        same_words(r.ReadShapeBvh(), reference(flat, before), "only sphere_center")
    finally:
        r.close()


# ------------------------------------------------------------------ 6. errors
def test_errors_leave_the_scene_untouched(gpu):
    st = scene_d()
    r = renderer(st)
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    try:
        assert r._lib.pt_get_version() == 10
        flat = st[0].Compile()
        before = r.ReadShapeBvh()
        img0, _ = frame(r)
        p = pose("spin_shared", flat)
        p["cube_min"], p["cube_max"] = flat.cube_min + f32(1), flat.cube_max + f32(1)
        m = np.ascontiguousarray(p["matrices"], np.float64)
        keep = [np.ascontiguousarray(p["sphere_center"], f32), np.ascontiguousarray(p["sphere_radius"], np.float64),
                np.ascontiguousarray(p["cube_min"], f32), np.ascontiguousarray(p["cube_max"], f32), m, m.copy()]
        sc, sr, ca, cb, xm, xi = [a.ctypes.data_as(fp if a.dtype == f32 else dp) for a in keep]
        ns, nc, nx = len(keep[0]), len(keep[2]), len(m)
        U = _abi.pt_shape_update
        call = lambda ctx, u: r._lib.pt_update_shapes(ctx, None if u is None else C.byref(u), None)
        cases = {
            "NULL ctx": lambda: call(None, U(ns, nc, nx, 0, sc, sr, ca, cb, xm, xi)),
            "NULL u": lambda: call(r._ctx, None),
            "reserved": lambda: call(r._ctx, U(ns, nc, nx, 1, sc, sr, ca, cb, xm, xi)),
            "cube_min only": lambda: call(r._ctx, U(ns, nc, nx, 0, sc, sr, ca, None, xm, xi)),
            "cube_max only": lambda: call(r._ctx, U(ns, nc, nx, 0, sc, sr, None, cb, xm, xi)),
            "matrix only": lambda: call(r._ctx, U(ns, nc, nx, 0, sc, sr, ca, cb, xm, None)),
            "inverse only": lambda: call(r._ctx, U(ns, nc, nx, 0, sc, sr, ca, cb, None, xi)),
            "radius without centre": lambda: call(r._ctx, U(ns, nc, nx, 0, None, sr, ca, cb, xm, xi)),
            "one sphere fewer": lambda: call(r._ctx, U(ns - 1, nc, nx, 0, sc, sr, ca, cb, xm, xi)),
            "one cube more": lambda: call(r._ctx, U(ns, nc + 1, nx, 0, sc, sr, ca, cb, xm, xi)),
            "no transformed": lambda: call(r._ctx, U(ns, nc, 0, 0, sc, sr, ca, cb, xm, xi)),
        }
        for what, fn in cases.items():
            assert fn() == _abi.PT_ERR_INVALID_ARG, what
            same_words(r.ReadShapeBvh(), before, what)
            same_buffer(frame(r)[0], img0)
        # no group given: nothing to do (the counts of groups that are not given are not looked at)
        ms = C.c_double(-1.0)
        assert r._lib.pt_update_shapes(r._ctx, C.byref(U(7, 7, 7, 0)), C.byref(ms)) == _abi.PT_OK and ms.value == 0.0
        same_words(r.ReadShapeBvh(), before, "no group")
        same_buffer(frame(r)[0], img0)
    finally:
        r.close()
    # no scene
    r = Renderer.NewRenderer(None, None, None, W, H, True, device=0)
    try:
        assert r._lib.pt_update_shapes(r._ctx, C.byref(_abi.pt_shape_update()), None) == _abi.PT_ERR_NO_SCENE
        assert r._lib.pt_read_shape_bvh(r._ctx, None, None, None, None, None) == _abi.PT_ERR_NO_SCENE
    finally:
        r.close()
    # a scene without analytic record: nothing to do
    s = Scene()
    s.Add(grid_mesh(4, 2, 0, LIGHT(5)))
    r = renderer((s, *scene_b()[1:]))
    try:
        img0, _ = frame(r)
        ms = C.c_double(-1.0)
        c3 = np.zeros((1, 3), f32)
        u = _abi.pt_shape_update(0, 0, 0, 0, c3.ctypes.data_as(fp))
        assert r._lib.pt_update_shapes(r._ctx, C.byref(u), C.byref(ms)) == _abi.PT_OK and ms.value == 0.0
        nodes, recs, heavy, lights = r.ReadShapeBvh()
        assert len(nodes) == len(recs) == len(heavy) == 0
        same_buffer(frame(r)[0], img0)
    finally:
        r.close()
