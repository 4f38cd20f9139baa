"""pt_motion_snapshot, pt_render_motion, pt_accumulate_temporal, pt_denoise_temporal and pt_reset_temporal on the GPU,
against tests/motion_ref.py (the independent restatement tests/test_motion_host.py holds pt_motion.h to on the host).

Motion: the reference is fed the rays of query_ref.camera_rays, pt_intersect_hits' t, kind, index, prim and shape for them,
and the current and previous arrays the test itself sent (the uploaded FlatScene mirrors every update).  prev_xy and
prev_depth are compared at the project's fp64 bar (rtol 1e-11, atol 1e-13); shape, prim, depth and status exactly;
prev_pixel exactly but for the pixels whose x' + 0.5 or y' + 0.5 lies within 1e-9 of an integer, which the reference
alone must show to be at most 1 % of the frame.
Merge: motion_ref.merge_frame is fed the Buffer, the history and the motion arrays read back from the device; M and V at
the fp64 bar, N and the status exactly.
Every case is 64x48 at 2 spp, and one 37x29 for ragged edge waves."""
import ctypes as C

import numpy as np
import pytest

import motion_ref as R
import query_ref as Q
from ptsharp_amd import Renderer, TransformedShape, Vector, _abi
from ptsharp_amd.geometry import Colour, Matrix
from ptsharp_amd.renderer import Buffer
from ptsharp_amd.scene import Camera, Cube, DefaultSampler, Material, Mesh, Plane, Scene, Sphere, Triangle, fix_normals_arrays

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 48, 2
RTOL, ATOL = 1e-11, 1e-13
f32 = np.float32
MOTION_INTS = ("shape", "prim", "status")


# ------------------------------------------------------------------ scenes
def grid_mesh(n, origin, du, dv):
    """n x n quads (2 n² triangles) spanning origin + s·du + t·dv, with face normals."""
    s, t = np.meshgrid(np.arange(n + 1) / n, np.arange(n + 1) / n, indexing="ij")
    p = (np.asarray(origin)[None, None] + s[..., None] * np.asarray(du) + t[..., None] * np.asarray(dv)).astype(f32)
    a, b, c, e = p[:-1, :-1], p[1:, :-1], p[:-1, 1:], p[1:, 1:]
    v = [np.concatenate([x.reshape(-1, 3), y.reshape(-1, 3)]) for x, y in ((a, b), (b, e), (c, c))]
    z3 = np.zeros_like(v[0])
    nrm = fix_normals_arrays(v[0], v[1], v[2], z3, z3, z3)
    return Mesh(*[np.ascontiguousarray(q, f32) for q in v + list(nrm)])


def instance_matrices(shift=0.0):
    return [Matrix.TranslateM(Vector(-0.2 + shift, 0.3, 0.1)).Mul(Matrix.RotateM(Vector(0, 0, 1), 0.3)),
            Matrix.TranslateM(Vector(1.3, 0.6 - shift, 1.0)).Mul(Matrix.ScaleM(Vector(0.7, 0.7, 0.7)))]


def camera_at(eye=(0.0, -6.0, 1.5), centre=(0.0, 0.0, 0.5)):
    return Camera.LookAt(Vector(*eye), Vector(*centre), Vector(0, 0, 1), 40)


def mixed_scene():
    """A world mesh, two loose triangles, an instanced mesh used twice, a sphere, a cube, a transformed sphere, a plane,
    an environment, and a camera that sees the sky above the plane's horizon."""
    s = Scene()
    s.Color = Colour(0.2, 0.3, 0.5)
    world = grid_mesh(8, (-2.4, 0.2, 0.0), (1.6, 0.0, 0.0), (0.0, 0.3, 1.6))
    world.SetMaterial(Material.DiffuseMaterial(Colour(0.9, 0.6, 0.3)))
    s.Add(world)
    grey = Material.DiffuseMaterial(Colour(0.7, 0.7, 0.7))
    vec = lambda *q: Vector(*[float(x) for x in q])
    up = vec(0, -1, 0)
    s.Add(Triangle(vec(-2.2, -0.5, 1.8), vec(-1.4, -0.5, 1.8), vec(-1.8, -0.4, 2.4), up, up, up, grey))
    s.Add(Triangle(vec(1.6, -1.0, -0.3), vec(2.3, -1.0, -0.3), vec(1.9, -0.8, 0.4), up, up, up, Material.DiffuseMaterial(Colour(0.3, 0.8, 0.4))))
    inst = grid_mesh(6, (-0.5, 0.0, -0.5), (1.0, 0.0, 0.0), (0.0, 0.1, 1.0))
    inst.SetMaterial(Material.DiffuseMaterial(Colour(0.4, 0.5, 0.9)))
    for m in instance_matrices():
        s.Add(TransformedShape.NewTransformedShape(inst, m))
    s.Add(Sphere.NewSphere(vec(0.3, -1.6, -0.1), 0.4, Material.DiffuseMaterial(Colour(0.9, 0.3, 0.3))))
    s.Add(Cube.NewCube(vec(-1.4, -2.2, -0.6), vec(-0.8, -1.6, 0.1), grey))
    ball = Sphere.NewSphere(vec(0, 0, 0), 0.35, Material.DiffuseMaterial(Colour(0.8, 0.8, 0.2)))
    s.Add(TransformedShape.NewTransformedShape(ball, Matrix.TranslateM(vec(-0.4, -1.0, 1.9)).Mul(Matrix.ScaleM(vec(1.0, 1.0, 0.6)))))
    s.Add(Plane.NewPlane(vec(0, 0, -0.6), vec(0, 0, 1), Material.DiffuseMaterial(Colour(0.5, 0.5, 0.5))))
    s.Add(Sphere.NewSphere(vec(0.0, -2.0, 6.0), 0.5, Material.LightMaterial(Colour.White, 30)))
    return s, camera_at(), DefaultSampler.NewSampler(4, 3)


def world_scene():
    """A world mesh alone over a cube floor (no instanced mesh): pt_rebuild_meshes' kind of scene."""
    s = Scene()
    s.Color = Colour(0.3, 0.3, 0.4)
    m = grid_mesh(10, (-1.5, 0.0, -0.2), (3.0, 0.0, 0.0), (0.0, 0.5, 2.0))
    m.SetMaterial(Material.DiffuseMaterial(Colour(0.9, 0.6, 0.3)))
    s.Add(m)
    s.Add(Cube.NewCube(Vector(-6, -4, -1.0), Vector(6, 6, -0.6), Material.DiffuseMaterial(Colour(0.6, 0.6, 0.6))))
    s.Add(Sphere.NewSphere(Vector(0.0, -2.0, 6.0), 0.5, Material.LightMaterial(Colour.White, 30)))
    return s, camera_at(), DefaultSampler.NewSampler(4, 3)


def renderer(st, w=W, h=H, engine=_abi.ENGINE_WAVEFRONT, seed=11):
    s, c, smp = st
    r = Renderer.NewRenderer(s, c, smp, w, h, True, device=0)
    r.SamplesPerPixel, r.Seed, r.Engine = SPP, seed, engine
    r._ensure_scene()
    return r


def geom(r):
    flat = r._uploaded
    n = flat.desc.num_transformed
    return R.geometry(flat.tri_v1, flat.tri_v2, flat.tri_v3, flat.sphere_center, flat.sphere_radius, flat.cube_min, flat.cube_max,
                      [list(flat.transformed[i].matrix) for i in range(n)], [list(flat.transformed[i].inverse) for i in range(n)])


def xf_is_mesh(r):
    flat = r._uploaded
    return [flat.transformed[i].shape_kind == _abi.SHAPE_MESH for i in range(flat.desc.num_transformed)]


def snapshot(r):
    """MotionSnapshot, and what the reference takes for the previous frame."""
    r.MotionSnapshot()
    return geom(r), R.camera(r.Camera.to_c())


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a == b) | (np.abs(a - b) <= ATOL + RTOL * np.abs(b))


def check_motion(r, prev, what, w=W, h=H):
    """RenderMotion against the reference; returns (got, want)."""
    o, d = Q.camera_rays(r.Camera, w, h)
    hits = r.IntersectHits(o, d, want=("t", "kind", "index", "prim", "shape"))
    want = R.frame(o, d, hits, geom(r), prev[0] if prev else None, prev[1] if prev else None, w, h, xf_is_mesh(r))
    r.RenderMotion()
    got = {k: a.reshape((w * h, 2) if k == "prev_xy" else (w * h,)) for k, a in r.Motion().items()}
    for k in MOTION_INTS:
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(got[k] != want[k])[:8])
    assert np.array_equal(got["depth"].view(np.int64), want["depth"].view(np.int64)), (what, "depth")
    for k in ("prev_xy", "prev_depth"):
        bad = ~close(got[k], want[k])
        assert not bad.any(), (what, k, got[k][bad][:4], want[k][bad][:4])
    edge = np.array([want["status"][i] == R.OK and R.near_pixel_edge(want["prev_xy"][i]) for i in range(w * h)])
    assert edge.sum() <= w * h // 100, (what, "pixels on a rounding boundary", int(edge.sum()))
    assert np.array_equal(got["prev_pixel"][~edge], want["prev_pixel"][~edge]), (what, "prev_pixel")
    return got, want


def moved_pixels(got, w=W):
    """Status-0 pixels whose previous pixel is another one."""
    ok = got["status"] == R.OK
    return int((ok & (got["prev_pixel"] != np.arange(len(ok)))).sum())


# ------------------------------------------------------------------ motion
@pytest.mark.parametrize("w,h", [(W, H), (37, 29)], ids=["64x48", "37x29"])
def test_frame_zero_then_a_static_scene(gpu, w, h):
    r = renderer(mixed_scene(), w, h)
    try:
        got, _ = check_motion(r, None, "frame 0", w, h)
        assert (got["status"] == R.NO_SNAPSHOT).all() and (got["prev_pixel"] == -1).all() and (got["prev_depth"] == R.INF).all()
        hit = got["shape"] >= 0
        assert 0.5 < hit.mean() < 0.95 and (got["depth"][~hit] == R.INF).all() and (got["prim"][~hit] == -1).all()
        flat = r._uploaded
        kinds = set(np.asarray(flat.shape_kind)[np.unique(got["shape"][hit])].tolist())
        assert kinds >= {_abi.SHAPE_MESH, _abi.SHAPE_TRIANGLE, _abi.SHAPE_TRANSFORMED, _abi.SHAPE_SPHERE, _abi.SHAPE_CUBE, _abi.SHAPE_PLANE}
        prev = snapshot(r)
        got, _ = check_motion(r, prev, "static", w, h)
        ok = got["status"] == R.OK
        assert ok.all(), "a static scene under the same camera projects every pixel into the image"
        assert np.array_equal(got["prev_pixel"], np.arange(w * h))
        # the distance of the hit point from the camera is the ray's t, up to the fp32 rounding of the intersect
        assert np.abs(got["prev_depth"][hit] / got["depth"][hit] - 1).max() < 1e-4
    finally:
        r.close()


def test_motion_follows_every_update(gpu):
    r = renderer(mixed_scene())
    try:
        flat = r._uploaded
        n = len(flat.tri_material)
        first, count = np.asarray(flat.mesh_first), np.asarray(flat.mesh_count)
        assert len(first) == 2 and sorted(count.tolist()) == [72, 128]
        rest = [np.array(a) for a in (flat.tri_v1, flat.tri_v2, flat.tri_v3)]
        # UpdateMeshes: every vertex moves by a smooth field (world mesh, loose triangles and the instanced mesh's object space)
        prev = snapshot(r)
        wave = lambda p: (p + np.stack([0.15 * np.sin(2 * p[:, 2]), 0.05 * np.cos(3 * p[:, 0]), 0.1 * np.sin(2 * p[:, 0])], 1)).astype(f32)
        r.UpdateMeshes(*[wave(a) for a in rest])
        got, _ = check_motion(r, prev, "UpdateMeshes")
        assert moved_pixels(got) > 100
        # pt_rebuild_blas between the snapshot and the motion pass: the records are re-sorted, the identity holds
        prev = snapshot(r)
        r.RebuildBlas(*[wave(wave(a)) for a in rest], what=_abi.REBUILD_WORLD | _abi.REBUILD_BLAS)
        got, _ = check_motion(r, prev, "RebuildBlas")
        assert moved_pixels(got) > 100
        # PoseMeshes: a translation of several pixels, then a rotation
        r.UpdateMeshes(*rest)
        prev = snapshot(r)
        big = int(np.argmax(count))
        mats = [Matrix.TranslateM(Vector(0.4, 0.0, 0.15)) if j == big else Matrix.TranslateM(Vector(0.0, 0.0, -0.1)) for j in range(2)]
        r.PoseMeshes(mats)
        got, _ = check_motion(r, prev, "PoseMeshes, translation")
        world = np.isin(got["prim"], np.arange(first[big], first[big] + count[big])) & (got["status"] == R.OK)
        shift = np.abs(got["prev_xy"][world, 0] - (np.flatnonzero(world) % W))
        assert world.sum() > 50 and 2.0 < shift.min() and shift.max() < 8.0, "the world mesh moved by several pixels"
        prev = snapshot(r)
        r.PoseMeshes([Matrix.RotateM(Vector(0, 1, 0.2), 0.25), Matrix.RotateM(Vector(0, 0, 1), -0.4)])
        got, _ = check_motion(r, prev, "PoseMeshes, rotation")
        assert moved_pixels(got) > 100
        # SkinMeshes: two bones blended per corner
        bones = np.zeros((n, 3, 4), np.int32)
        bones[:, :, 1] = 1
        wts = np.zeros((n, 3, 4), f32)
        wts[:, :, 0] = np.linspace(0.1, 0.9, n * 3, dtype=f32).reshape(n, 3)
        wts[:, :, 1] = f32(1) - wts[:, :, 0]
        r.SetSkin(bones, wts, 2)
        prev = snapshot(r)
        r.SkinMeshes([Matrix.TranslateM(Vector(0.2, 0, 0.1)), Matrix.RotateM(Vector(0, 1, 0), 0.15)])
        got, _ = check_motion(r, prev, "SkinMeshes")
        assert moved_pixels(got) > 100
        # MorphMeshes: one target over every corner of the meshes
        tri = np.sort(np.concatenate([np.arange(f, f + c) for f, c in zip(first, count)]))
        corners = (3 * tri[:, None] + np.arange(3)).reshape(-1).astype(np.int32)
        rng = np.random.default_rng(3)
        r.SetMorph([(corners, (0.2 * rng.standard_normal((len(corners), 3))).astype(f32))])
        prev = snapshot(r)
        r.MorphMeshes([0.6])
        got, _ = check_motion(r, prev, "MorphMeshes")
        assert moved_pixels(got) > 100
        # UpdateShapes: the sphere moved and resized, the cube, the instance matrices
        prev = snapshot(r)
        sc, sr = np.array(flat.sphere_center), np.array(flat.sphere_radius)
        ground = int(np.flatnonzero(np.isclose(sr, 0.4))[0])
        sc[ground] += f32([0.3, 0.1, 0.2])
        sr[ground] = 0.55
        ca, cb = np.array(flat.cube_min), np.array(flat.cube_max)
        ca[0] += f32([-0.2, 0.0, 0.0])
        cb[0] += f32([0.1, 0.2, 0.3])
        ms = [m.m for m in instance_matrices(0.25)] + [Matrix.TranslateM(Vector(-0.2, -1.0, 1.7)).Mul(Matrix.ScaleM(Vector(1.2, 1.0, 0.7))).m]
        r.UpdateShapes(sphere_center=sc, sphere_radius=sr, cube_min=ca, cube_max=cb, matrices=ms)
        got, _ = check_motion(r, prev, "UpdateShapes")
        for kind in (_abi.SHAPE_SPHERE, _abi.SHAPE_CUBE, _abi.SHAPE_TRANSFORMED):
            of_kind = (got["shape"] >= 0) & (np.asarray(flat.shape_kind)[np.maximum(got["shape"], 0)] == kind) & (got["status"] == R.OK)
            assert (of_kind & (got["prev_pixel"] != np.arange(W * H))).sum() > 10, kind
        # a moved camera, then a camera turned so that part of what it sees lay behind the snapshot's
        prev = snapshot(r)
        r.Camera = camera_at((0.8, -5.6, 1.9), (0.1, 0.0, 0.4))
        got, _ = check_motion(r, prev, "moved camera")
        assert moved_pixels(got) > 1000 and (got["status"] == R.OUTSIDE).any()
        r.Camera = camera_at()
        prev = snapshot(r)
        r.Camera = camera_at((0.0, -6.0, 1.5), (6.0, -6.6, 1.0))
        got, _ = check_motion(r, prev, "turned camera")
        behind = (got["status"] == R.OUTSIDE) & (got["prev_xy"] == -1.0).all(axis=1)
        assert behind.sum() > 100 and (got["prev_pixel"][got["status"] != R.OK] == -1).all()
    finally:
        r.close()


def test_identity_keying_across_pt_rebuild_meshes(gpu):
    st = world_scene()
    r = renderer(st)
    try:
        flat = r._uploaded
        rest = [np.array(a) for a in (flat.tri_v1, flat.tri_v2, flat.tri_v3)]
        before = r.ReadTriBvh()
        prev = snapshot(r)
        bend = lambda p: (p + np.stack([0.2 * np.sin(3 * p[:, 2]), 0.3 * p[:, 0] ** 2, 0.1 * p[:, 0]], 1)).astype(f32)
        r.RebuildMeshes(*[bend(a) for a in rest])
        after = r.ReadTriBvh()
        assert not np.array_equal(before[2], after[2]), "the rebuild re-sorted the records"
        got, _ = check_motion(r, prev, "RebuildMeshes")
        assert moved_pixels(got) > 100
    finally:
        r.close()


# ------------------------------------------------------------------ merge
def read_all(r):
    b = r.ReadBuffer()
    return b.M.reshape(-1, 3).copy(), b.V.reshape(-1, 3).copy(), b.N.reshape(-1).copy()


def render_frame(r, passes=1):
    r.ResetBuffer()
    for _ in range(passes):
        r.RenderParallel()


def history_of(r):
    t, st = r.Temporal()
    mo = r.Motion()
    return dict(M=t.M.reshape(-1, 3).copy(), V=t.V.reshape(-1, 3).copy(), N=t.N.reshape(-1).copy(), shape=mo["shape"].reshape(-1).copy(),
                prim=mo["prim"].reshape(-1).copy(), depth=mo["depth"].reshape(-1).copy())


def check_merge(r, hist, what):
    """AccumulateTemporal against the reference, from what the device holds; returns the status."""
    buf, mo = read_all(r), {k: a.copy() for k, a in r.Motion().items()}
    p = r.TemporalParams
    want = R.merge_frame(buf, hist, mo, p.max_history, p.sigma_depth)
    r.AccumulateTemporal()
    t, st = r.Temporal()
    assert np.array_equal(st.reshape(-1), want[3]), (what, "status", np.flatnonzero(st.reshape(-1) != want[3])[:8])
    assert np.array_equal(t.N.reshape(-1), want[2]), (what, "N")
    for got, w, name in ((t.M, want[0], "M"), (t.V, want[1], "V")):
        bad = ~close(got.reshape(-1, 3), w)
        assert not bad.any(), (what, name, got.reshape(-1, 3)[bad][:4], w[bad][:4])
    after = read_all(r)
    assert all(np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)
               for a, b in zip(buf, after)), (what, "the Buffer changed")
    return st.reshape(-1)


def test_merge_matches_the_reference_with_every_status(gpu):
    r = renderer(mixed_scene())
    seen = set()
    try:
        flat = r._uploaded
        count = np.asarray(flat.mesh_count)
        big = int(np.argmax(count))
        # frame 0: no history
        render_frame(r)
        r.RenderMotion()
        st = check_merge(r, None, "frame 0")
        assert (st == R.NO_HISTORY).all()
        seen |= set(st.tolist())
        hist = history_of(r)
        r.MotionSnapshot()
        # frame 1: the world mesh translated by several pixels: q != p over overlapping regions, the case an in-place
        # history update gets wrong; the edge of the frame's content gives 2 (outside) and 4 (another surface)
        r.PoseMeshes([Matrix.TranslateM(Vector(0.4, 0.0, 0.15)) if j == big else Matrix.Identity() for j in range(2)])
        r.Camera = camera_at((0.5, -6.0, 1.5), (0.5, 0.0, 0.5))
        render_frame(r)
        r.RenderMotion()
        mo = r.Motion()
        ok = mo["status"].reshape(-1) == R.OK
        q = mo["prev_pixel"].reshape(-1)
        chain = ok & (q != np.arange(W * H)) & np.isin(q, np.flatnonzero(ok))
        assert chain.sum() > 500, "many pixels read a history pixel that another pixel's merge writes"
        st = check_merge(r, hist, "translated frame")
        seen |= set(st.tolist())
        assert (st == R.MERGED).sum() > 1000 and (st == R.MOTION).any() and (st == R.IDENTITY).any()
        hist = history_of(r)
        r.MotionSnapshot()
        # frame 2: a sphere passes in front (4), and a shrunk sigma_depth turns slanted surfaces away (5)
        sc, sr = np.array(flat.sphere_center), np.array(flat.sphere_radius)
        ground = int(np.flatnonzero(np.isclose(sr, 0.4))[0])
        sc[ground] = f32([-0.3, -2.5, 0.9])
        r.UpdateShapes(sphere_center=sc, sphere_radius=sr)
        r.Camera = camera_at((0.5, -5.0, 1.5), (0.5, 0.0, 0.5))
        r.TemporalParams.sigma_depth = 1e-3
        render_frame(r)
        r.RenderMotion()
        st = check_merge(r, hist, "sphere in front, shrunk sigma_depth")
        seen |= set(st.tolist())
        assert (st == R.IDENTITY).sum() > 20 and (st == R.DEPTH).sum() > 100
        hist = history_of(r)
        r.MotionSnapshot()
        # frame 3: a tile-sharded context merges what it holds: foreign pixels have N = 0 and give 7; the history they
        # leave is invalid, which frame 4 meets as 3
        r.TemporalParams.sigma_depth = 0.1
        r.Tiles = np.array([0], np.int32)
        render_frame(r)
        r.RenderMotion()
        st = check_merge(r, hist, "one tile of two")
        seen |= set(st.tolist())
        n = r.ReadBuffer().N.reshape(-1)
        assert (n == 0).sum() == W * H - 32 * 32 and (st[n == 0] == R.INVALID).all() and (st[n > 0] != R.INVALID).all()
        hist = history_of(r)
        r.MotionSnapshot()
        r.Tiles = None
        r.TemporalParams.max_history = 0
        render_frame(r)
        r.RenderMotion()
        st = check_merge(r, hist, "after the sharded frame, max_history = 0")
        seen |= set(st.tolist())
        assert (st == R.HISTORY_INVALID).sum() == W * H - 32 * 32
        t, _ = r.Temporal()
        buf = read_all(r)
        assert np.array_equal(t.N.reshape(-1), buf[2]) and np.array_equal(t.M.reshape(-1, 3).view(np.int64), buf[0].view(np.int64))
        assert np.array_equal(t.V.reshape(-1, 3).view(np.int64), buf[1].view(np.int64)), "max_history = 0: the result is the Buffer"
        assert seen == {0, 1, 2, 3, 4, 5, 7}
    finally:
        r.close()


def test_static_frames_pool_to_the_uninterrupted_render(gpu):
    """K = 4 frames of one 2-spp pass each, pass numbers continuing: the temporal state is the 4-pass render's."""
    st = mixed_scene()
    r, ref = renderer(st), renderer(st)
    try:
        r.TemporalParams.max_history = 8
        for k in range(4):
            r.LoadBuffer(Buffer(W, H), k)
            r.RenderParallel()
            r.TemporalFrame()
        t, status = r.Temporal()
        for _ in range(4):
            ref.RenderParallel()
        b = ref.ReadBuffer()
        ok = status == R.MERGED
        assert ok.all(), "a static scene under one camera merges every pixel"
        assert np.array_equal(t.N[ok], b.N[ok]) and (b.N[ok] == 4).all()   # N counts passes (Pixel.AddSample per pass)
        assert close(t.M[ok], b.M[ok]).all()
        bound = 1e-11 * (b.V[ok] + b.N[ok][:, None] * np.abs(b.M[ok]) ** 2)
        assert (np.abs(t.V[ok] - b.V[ok]) <= bound).all(), float((np.abs(t.V[ok] - b.V[ok]) / np.maximum(bound, 1e-300)).max())
    finally:
        r.close()
        ref.close()


def test_history_lowers_the_error_of_a_moving_frame(gpu):
    """A posed mesh translates over 6 frames at 2 spp: the last frame's temporal M is nearer a 256-spp render of that
    frame than the frame's own 2-spp M."""
    st = world_scene()
    r, ref = renderer(st), renderer(st, seed=977)
    try:
        pose = lambda k: [Matrix.TranslateM(Vector(0.12 * k, 0.0, 0.03 * k))]
        for k in range(6):
            r.PoseMeshes(pose(k), mirror=False)
            r.LoadBuffer(Buffer(W, H), k)
            r.RenderParallel()
            r.TemporalFrame()
        t, status = r.Temporal()
        own = r.ReadBuffer().M.copy()
        ref.PoseMeshes(pose(5), mirror=False)
        ref.SamplesPerPixel = 16
        ref.RenderPasses(16)
        truth = ref.ReadBuffer().M
        rmse = lambda a: float(np.sqrt(np.mean((a - truth) ** 2)))
        e_temporal, e_own = rmse(t.M), rmse(own)
        print(f"RMSE against 256 spp: temporal {e_temporal:.6g}, the frame's own 2 spp {e_own:.6g}; merged pixels {float((status == 0).mean()):.3f}")
        assert (status == R.MERGED).mean() > 0.8
        assert e_temporal < e_own
    finally:
        r.close()
        ref.close()


# ------------------------------------------------------------------ denoise, state rules, leaks
@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
def test_denoise_temporal_is_denoise_of_the_temporal_state(gpu, guided):
    st = mixed_scene()
    r, other = renderer(st), renderer(st)
    try:
        for k in range(2):
            r.LoadBuffer(Buffer(W, H), k)
            r.RenderParallel()
            r.TemporalFrame()
        if guided:
            r.RenderFeatures()
            other.RenderFeatures()
        before = read_all(r)
        r.DenoiseTemporal(guided=guided)
        t, _ = r.Temporal()
        other.LoadBuffer(t, 2)
        other.DenoiseBuffer(guided=guided)
        for a, b in ((r.DenoisedColour(), other.DenoisedColour()), (r.DenoisedVariance(), other.DenoisedVariance())):
            assert np.array_equal(a.view(np.int64), b.view(np.int64))
        assert np.array_equal(r.Denoised(), other.Denoised())
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, read_all(r)))
        assert (t.N > r.ReadBuffer().N).mean() > 0.9, "the filter ran on the merged state, not the Buffer"
    finally:
        r.close()
        other.close()


def state_of(r):
    b = r.ReadBuffer()
    s = r.Stats()
    out = [b.M.copy(), b.V.copy(), b.N.copy(), *[np.array(a) for a in r.ReadTriBvh()], *[np.array(a) for a in r.Features()]]
    out.append(np.array([s.rays, s.rays_total, s.passes, s.shadow_rays, s.bvh_nodes, s.bvh_bytes, s.traversal_bytes], np.uint64))
    return out


def same_state(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_state_rules_and_errors(gpu):
    st = world_scene()
    r = renderer(st)
    lib, ctx = r._lib, r._ctx
    bad = _abi.PT_ERR_INVALID_ARG
    ms = C.c_double(-1.0)
    P = W * H
    try:
        r.RenderParallel()
        r.RenderFeatures()
        out = (C.c_double * (2 * P))()
        # nothing yet: every read and the accumulate are refused
        assert lib.pt_read_motion(ctx, 0, out) == bad and lib.pt_read_temporal(ctx, out, None, None, None) == bad
        assert lib.pt_accumulate_temporal(ctx, None, C.byref(ms)) == bad and lib.pt_denoise_temporal(ctx, None, None, C.byref(ms)) == bad
        r.TemporalFrame()
        # accumulate without a fresh motion result
        with pytest.raises(_abi.PTError) as e:
            r.AccumulateTemporal()
        assert e.value.code == bad
        t0, s0 = r.Temporal()
        before = state_of(r)
        cam = r.Camera.to_c()
        T = _abi.pt_temporal_params
        r.RenderMotion()
        for p in (T(-1, 0, 0.1), T((1 << 20) + 1, 0, 0.1), T(32, 7, 0.1), T(32, 0, -1.0), T(32, 0, float("nan"))):
            assert lib.pt_accumulate_temporal(ctx, C.byref(p), C.byref(ms)) == bad
        assert lib.pt_read_motion(ctx, 7, out) == bad and lib.pt_read_motion(ctx, -1, out) == bad and lib.pt_read_motion(ctx, 0, None) == bad
        assert lib.pt_motion_snapshot(ctx, None) == bad and lib.pt_render_motion(ctx, None, C.byref(ms)) == bad
        dp, gp = _abi.pt_denoise_params(5, 0, 4.0), _abi.pt_denoise_guided_params(5, 0, 4.0, 0.3, 0.3, 0.1)
        assert lib.pt_denoise_temporal(ctx, C.byref(dp), C.byref(gp), C.byref(ms)) == bad
        assert lib.pt_denoise_temporal(ctx, C.byref(_abi.pt_denoise_params(0, 0, 4.0)), None, C.byref(ms)) == bad
        assert ms.value == -1.0
        t1, s1 = r.Temporal()
        assert same_state(before, state_of(r)) and same_state([t0.M, t0.V, t0.N, s0], [t1.M, t1.V, t1.N, s1])
        # the refused calls left the fresh motion result: the accumulate still goes through, and merges
        r.AccumulateTemporal()
        assert (r.Temporal()[1] == R.MERGED).mean() > 0.99
        assert same_state(before, state_of(r)), "a temporal frame changes no Buffer, BVH, feature or counter"
        # ResetTemporal: status 1 everywhere, the snapshot kept
        r.ResetTemporal()
        assert lib.pt_read_motion(ctx, 0, out) == bad and lib.pt_read_temporal(ctx, out, None, None, None) == bad
        assert lib.pt_accumulate_temporal(ctx, None, C.byref(ms)) == bad
        r.RenderMotion()
        assert (r.Motion()["status"] == R.OK).all(), "the snapshot is kept"
        r.AccumulateTemporal()
        assert (r.Temporal()[1] == R.NO_HISTORY).all()
        # an upload drops everything
        s2, c2, smp2 = world_scene()
        r.Scene = s2
        r._ensure_scene()
        assert lib.pt_read_motion(ctx, 0, out) == bad and lib.pt_read_temporal(ctx, out, None, None, None) == bad
        assert lib.pt_accumulate_temporal(ctx, None, C.byref(ms)) == bad and lib.pt_denoise_temporal(ctx, None, None, C.byref(ms)) == bad
        r.RenderMotion()
        assert (r.Motion()["status"] == R.NO_SNAPSHOT).all()
    finally:
        r.close()
    # no scene
    s, c, smp = world_scene()
    r = Renderer.NewRenderer(s, c, smp, W, H, True, device=0)
    try:
        cam = c.to_c()
        assert r._lib.pt_motion_snapshot(r._ctx, C.byref(cam)) == _abi.PT_ERR_NO_SCENE
        assert r._lib.pt_render_motion(r._ctx, C.byref(cam), C.byref(ms)) == _abi.PT_ERR_NO_SCENE
        assert r._lib.pt_reset_temporal(r._ctx) == _abi.PT_OK
    finally:
        r.close()


@pytest.mark.parametrize("engine", [_abi.ENGINE_MEGAKERNEL, _abi.ENGINE_WAVEFRONT], ids=["mega", "wavefront"])
def test_a_temporal_frame_leaks_into_no_render(gpu, engine):
    st = mixed_scene()
    r = renderer(st, engine=engine)
    try:
        def picture():
            r.LoadBuffer(Buffer(W, H), 0)
            r.RenderParallel()
            return [a.copy() for a in read_all(r)]
        before = picture()
        r.TemporalFrame()
        r.RenderMotion()
        r.AccumulateTemporal()
        r.DenoiseTemporal()
        after = picture()
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, after))
    finally:
        r.close()
