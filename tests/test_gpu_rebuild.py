"""pt_rebuild_meshes and pt_tri_bvh_cost on the GPU: the world triangle BVH re-sorted on the device.

  1. words: after RebuildMeshes at the rest, sine, twist and offset poses, for P in {1, 2, 3, 4, 24, 25, 192, 193, 1537,
     6400}, pt_read_tri_bvh's nodes, chunks, records, counts and root box are tests/rebuild_ref.py's word for word (the
     numpy restatement, itself checked against the native check by tests/test_rebuild_host.py), pt_read_tri_normals
     returns the normals in source order (given, face, smooth: one mode per pose, kept at the rest pose), and
     pt_tri_bvh_cost matches the reference within 1e-9 relative (the fp64 summation bound for at most 10^6 positive
     terms is about 1.1e-10);
  2. rays: pt_intersect t and kind and pt_occluded against a context that uploaded the deformed scene fresh, bit for
     bit, on 4,096 seeded rays that include tests/degenerate_rays.py's families; renders on both engines against the
     oracle on the deformed scene (rays and N exact);
  3. composition: a later pt_update_triangles refits the rebuilt topology; RebuildMeshes() from a staged pose equals
     RebuildMeshes(the pose's arrays) and leaves the pose readable; PT_NORMALS_SMOOTH after a rebuild; a rebuild with
     the upload's own vertices renders what the upload rendered, within the oracle bar;
  4. the cost gates of the CPU model on the device's own numbers: after the offset pose cost(rebuilt) <= cost(refit) / 3,
     after the twist cost(rebuilt) <= 0.8 cost(refit);
  5. every error leaves pt_read_tri_bvh's bytes unchanged.
The scene of P triangles: the first P - 1 triangles of a displaced sphere (40 x 80 quads) as one mesh and one loose
emissive triangle, over a floor cube under a sphere light.  Frames are 64x48 at 2 spp.
"""
import ctypes as C

import numpy as np
import pytest

import degenerate_rays as DR
import normals_ref
import oracle_lib as O
import rebuild_ref
import refit_ref
from parity import check
from ptsharp_amd import Renderer, Vector, _abi, scenes
from ptsharp_amd.geometry import Colour, Matrix
from ptsharp_amd.renderer import Buffer
from ptsharp_amd.scene import Camera, Cube, DefaultSampler, Material, Mesh, Scene, Sphere, Triangle, fix_normals_arrays

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 48, 2
ENGINES = pytest.mark.parametrize("engine", [_abi.ENGINE_MEGAKERNEL, _abi.ENGINE_WAVEFRONT], ids=["mega", "wavefront"])
SIZES = [1, 2, 3, 4, 24, 25, 192, 193, 1537, 6400]
POSES = ["rest", "sine", "twist", "offset"]
NTH, NPH = 40, 80
f32 = np.float32


def sphere_arrays(P):
    """v1, v2, v3, n1, n2, n3 of the scene of P triangles, in the compiled scene's order: the mesh's P - 1 triangles,
    then the loose emissive one.  r = 1 + 0.05 sin 7θ cos 5φ + 0.02 sin(23φ + 3θ); face normals."""
    i, j = np.meshgrid(np.arange(NTH + 1), np.arange(NPH + 1), indexing="ij")
    th = (np.pi * (0.02 + 0.96 * i / NTH))
    ph = (2 * np.pi * j / NPH)
    r = 1 + 0.05 * np.sin(7 * th) * np.cos(5 * ph) + 0.02 * np.sin(23 * ph + 3 * th)
    p = np.stack([r * np.sin(th) * np.cos(ph), r * np.cos(th), r * np.sin(th) * np.sin(ph)], axis=2).astype(f32)
    a, b, c, e = p[:-1, :-1], p[1:, :-1], p[:-1, 1:], p[1:, 1:]
    g = [np.stack(q, axis=2).reshape(-1, 3)[:P - 1] for q in ((a, b), (b, e), (c, c))]
    loose = np.array([[0, 2, 0], [0.5, 2, 0], [0, 2, 0.5]], f32)
    v = [np.concatenate([g[k], loose[k:k + 1]]).astype(f32) for k in range(3)]
    z3 = np.zeros_like(v[0])
    n = fix_normals_arrays(v[0], v[1], v[2], z3, z3, z3)
    return [np.ascontiguousarray(q, f32) for q in v + list(n)]


def make_scene(arrs):
    v1, v2, v3, n1, n2, n3 = arrs
    P = len(v1)
    s = Scene()
    grey = Material.DiffuseMaterial(Colour(0.7, 0.7, 0.7))
    vec = lambda r: Vector(*[float(q) for q in r])
    if P > 1:
        g = slice(0, P - 1)
        mesh = Mesh(v1[g], v2[g], v3[g], n1[g], n2[g], n3[g])
        mesh.SetMaterial(Material.DiffuseMaterial(Colour(0.9, 0.6, 0.3)))
        s.Add(mesh)
    k = P - 1
    s.Add(Triangle(vec(v1[k]), vec(v2[k]), vec(v3[k]), vec(n1[k]), vec(n2[k]), vec(n3[k]), Material.LightMaterial(Colour.White, 40)))
    s.Add(Cube.NewCube(Vector(-10, -3, -10), Vector(10, -2, 10), grey))
    s.Add(Sphere.NewSphere(Vector(0, 6, 0), 1, Material.LightMaterial(Colour.White, 20)))
    camera = Camera.LookAt(Vector(3, 3, 3), Vector(0, 0, 0), Vector(0, 1, 0), 45)
    sampler = DefaultSampler.NewSampler(4, 3)
    return s, camera, sampler


def pose(name, arrs):
    """The CPU check's poses in fp32: positions only (out[3:] are the rest normals)."""
    out = [a.copy() for a in arrs]
    rng = np.random.default_rng(12345)
    off = (rng.random((len(arrs[0]), 3)) - 0.5).astype(f32)
    for k in range(3):
        p = arrs[k]
        x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
        if name == "rest":
            q = p.copy()
        elif name == "sine":
            q = np.stack([x, y, z + (f32(0.3) * np.sin(f32(5) * x) * np.cos(f32(3) * y)).astype(f32)], 1)
        elif name == "twist":
            a = (f32(3) * y).astype(f32)
            c, s = np.cos(a).astype(f32), np.sin(a).astype(f32)
            q = np.stack([c * x + s * z, y, c * z - s * x], 1)
        elif name == "offset":
            q = p + off
        else:
            raise KeyError(name)
        out[k] = np.ascontiguousarray(q, f32)
    return out


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


def same_bvh(a, b, what=""):
    for name, x, y in zip(("nodes", "chunks", "records", "box"), a, b):
        x, y = np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)
        assert x.shape == y.shape, f"{what} {name}: shape {x.shape} vs {y.shape}"
        bad = np.argwhere(x != y)
        assert not bad.size, f"{what} {name}: {len(bad)} words differ, first at {bad[0]}: {x[tuple(bad[0])]:#x} vs {y[tuple(bad[0])]:#x}"


def same_cost(got, nodes, what=""):
    want = rebuild_ref.cost(nodes)
    print(what, "pt_tri_bvh_cost", got, "reference", want)
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-9 * abs(w), f"{what}: cost {got} vs {want}"


def total_cost(c):
    return c[0] + c[1]


# ------------------------------------------------------------------ 1. words
MODE_OF_POSE = {"rest": "kept", "sine": "given", "twist": "face", "offset": "smooth"}


@pytest.mark.parametrize("name", POSES)
@pytest.mark.parametrize("P", SIZES)
def test_words_after_a_rebuild(gpu, P, name):
    arrs = sphere_arrays(P)
    st = make_scene(arrs)
    r = renderer(st)
    try:
        before = r.ReadTriBvh()
        assert len(before[2]) == P
        flat = st[0].Compile()
        assert np.array_equal(flat.tri_v1, arrs[0]) and np.array_equal(flat.tri_n3, arrs[5])
        src = refit_ref.src_of_pos_from(before[2], flat)
        same_cost(r.TriBvhCost(), before[0], "upload")
        moved = pose(name, arrs)
        mode = MODE_OF_POSE[name]
        mf, mc = ([0], [P - 1]) if P > 1 else ([], [])
        if mode == "kept":
            normals, kw, want_n = [], {}, arrs[3:]
        elif mode == "given":
            rng = np.random.default_rng(3)
            normals = [rng.standard_normal(a.shape).astype(f32) for a in arrs[3:]]
            kw, want_n = {}, normals
        else:
            normals, kw = [], {"normals": mode}
            want_n = normals_ref.normals(*moved[:3], mf, mc, mode)
        ref_n = want_n if mode != "kept" else [None] * 3
        want, new_src = rebuild_ref.rebuild(before[2], src, *moved[:3], *ref_n)
        ms = r.RebuildMeshes(*moved[:3], *normals, **kw)
        assert ms > 0
        got = r.ReadTriBvh()
        same_bvh(got, want, f"P {P} {name}")
        h, L, counts = rebuild_ref.plan(P)
        assert len(got[0]) == sum(counts) and len(got[1]) == L and len(got[2]) == P
        for a, b, what in zip(r.ReadTriNormals(), want_n, ("n1", "n2", "n3")):
            normals_ref.same_bits(a, b, f"P {P} {name} {what}")
        same_cost(r.TriBvhCost(), got[0], f"P {P} {name}")
        assert np.array_equal(flat.tri_v1, moved[0]) and np.array_equal(flat.tri_v3, moved[2])
        assert np.array_equal(flat.tri_n2, want_n[1], equal_nan=True)
        # a second rebuild with the same arrays: a fixed point
        r.RebuildMeshes(*moved[:3])
        same_bvh(r.ReadTriBvh(), got, f"P {P} {name} again")
        if P > 24:
            assert not np.array_equal(np.sort(new_src), new_src)
    finally:
        r.close()


# ------------------------------------------------------------------ 2. rays and renders
def rays_for(moved, total, seed):
    """tests/degenerate_rays.py's mesh families at the moved triangles, filled up to `total` with rays from a shell
    around the geometry to points inside its box."""
    o, d, _ = DR.mesh_rays(*moved[:3], n=200, seed=seed)
    n_random = total - len(o)
    assert n_random > 1000
    allv = np.concatenate(moved[:3]).astype(np.float64)
    lo, hi = allv.min(axis=0), allv.max(axis=0)
    rng = np.random.default_rng(seed + 1)
    c, ext = (lo + hi) / 2, np.maximum((hi - lo) / 2, 0.5)
    u = rng.standard_normal((n_random, 3))
    ro = (c + 4.0 * ext.max() * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(f32)
    t = ((c - ext) + 2 * ext * rng.random((n_random, 3))).astype(f32)
    rd = (t - ro).astype(np.float64)
    rd = (rd / np.linalg.norm(rd, axis=1, keepdims=True)).astype(f32)
    return np.ascontiguousarray(np.concatenate([o, ro]), f32), np.ascontiguousarray(np.concatenate([d, rd]), f32)


@pytest.mark.parametrize("name", ["twist", "offset"])
def test_rays_equal_a_fresh_upload(gpu, name):
    arrs = sphere_arrays(6400)
    moved = pose(name, arrs)
    r = renderer(make_scene(arrs))
    fresh = renderer(make_scene(moved[:3] + arrs[3:]))
    try:
        r.Intersect(np.zeros((1, 3), f32), np.array([[0, 0, 1]], f32))   # uploads
        r.RebuildMeshes(*moved[:3])
        o, d = rays_for(moved, 4096, 31)
        assert len(o) == 4096
        t, k = r.Intersect(o, d)
        ft, fk = fresh.Intersect(o, d)
        bad = np.flatnonzero((t.view(np.int64) != ft.view(np.int64)) | (k != fk))
        assert bad.size == 0, (f"{bad.size} of {len(o)} rays differ from the fresh upload, first {bad[:5]}: t {t[bad[:3]]} kind "
                               f"{k[bad[:3]]}, fresh t {ft[bad[:3]]} kind {fk[bad[:3]]}")
        assert int((fk == _abi.SHAPE_TRIANGLE).sum()) > 1000
        rng = np.random.default_rng(7)
        tl = np.where(ft < 1e9, ft, 5.0)
        for what, tm in {"at_hit": tl, "past_hit": np.nextafter(tl, np.inf), "random": tl * rng.uniform(0.0, 1.6, len(tl))}.items():
            got, want = r.Occluded(o, d, tm), fresh.Occluded(o, d, tm)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, f"occluded {what}: {bad.size} rays differ, first {bad[:5]}"
    finally:
        r.close()
        fresh.close()


@ENGINES
def test_render_parity_after_a_rebuild(gpu, engine):
    arrs = sphere_arrays(6400)
    st = make_scene(arrs)
    moved = pose("twist", arrs)
    r = renderer(st, engine)
    try:
        frame(r)                        # a pass at the rest pose first: the rebuild comes between passes
        r.RebuildMeshes(*moved[:3])
        g, grays = frame(r)
        o, orays = O.render(O.OracleScene(st[0]), st[1], st[2], W, H, SPP, seed=23)
        check(g, grays, o, orays)
        assert (g.M.sum(axis=2) > 0).mean() > 0.5
    finally:
        r.close()


# ------------------------------------------------------------------ 3. composition
def test_update_after_a_rebuild_refits_the_new_topology(gpu):
    arrs = sphere_arrays(1537)
    st = make_scene(arrs)
    r = renderer(st)
    try:
        before = r.ReadTriBvh()
        src = refit_ref.src_of_pos_from(before[2], st[0].Compile())
        a, b = pose("offset", arrs), pose("sine", arrs)
        want_a, new_src = rebuild_ref.rebuild(before[2], src, *a[:3])
        r.RebuildMeshes(*a[:3])
        same_bvh(r.ReadTriBvh(), want_a, "pose A")
        r.UpdateTriangles(*b[:3])
        same_bvh(r.ReadTriBvh(), refit_ref.refit(want_a[0], want_a[1], want_a[2], new_src, *b[:3]), "pose B on A's topology")
        for got, want, what in zip(r.ReadTriNormals(), arrs[3:], ("n1", "n2", "n3")):
            normals_ref.same_bits(got, want, what)
    finally:
        r.close()


def test_rebuild_from_the_staged_pose(gpu):
    arrs = sphere_arrays(1537)
    r, r2 = renderer(make_scene(arrs)), renderer(make_scene(arrs))
    try:
        m = Matrix.TranslateM(Vector(0.5, -0.25, 1)).Mul(Matrix.RotateM(Vector(1, 2, 3), 1.1)).Mul(Matrix.ScaleM(Vector(1.5, 0.5, 1)))
        r.SetRestPose()
        r.PoseMeshes([m], mirror=False)
        staged = [a.copy() for a in r.ReadPose()]
        assert r.RebuildMeshes() > 0
        again = r.ReadPose()          # the pose stays readable
        for a, b in zip(staged, again):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        r2.RebuildMeshes(*staged)
        same_bvh(r.ReadTriBvh(), r2.ReadTriBvh(), "staged pose against its arrays")
        assert not np.array_equal(staged[0], arrs[0])
        # without a staged pose: refused, nothing changed
        before = r2.ReadTriBvh()
        assert r2._lib.pt_rebuild_meshes(r2._ctx, None, None) == _abi.PT_ERR_INVALID_ARG
        same_bvh(r2.ReadTriBvh(), before, "no staged pose")
    finally:
        r.close()
        r2.close()


@pytest.mark.parametrize("first,second", [(1537, 193), (193, 1537)])
def test_every_entry_point_then_an_upload_of_another_size(gpu, first, second):
    """One context through every moving-triangle entry point (so every per-scene workspace exists and its kept layout
    was used), then an upload of a scene of another size on the same context: a rebuild and an update of that scene
    leave the device bit for bit as they leave a fresh context.  At 1537 triangles the balanced tree and the uploaded
    one differ in node count."""
    arrs, arrs2 = sphere_arrays(first), sphere_arrays(second)
    a, b = pose("offset", arrs2), pose("sine", arrs2)
    r, fresh = renderer(make_scene(arrs)), renderer(make_scene(arrs2))
    try:
        r.UpdateTriangles(*pose("sine", arrs)[:3], normals="smooth")
        m = Matrix.TranslateM(Vector(0.5, -0.25, 1)).Mul(Matrix.RotateM(Vector(1, 2, 3), 1.1)).Mul(Matrix.ScaleM(Vector(1.5, 0.5, 1)))
        r.SetRestPose()
        r.PoseMeshes([m], mirror=False)
        assert r.RebuildMeshes() > 0
        r.UpdateTriangles(*pose("twist", arrs)[:3])
        r.ReadTriNormals()
        r.Scene = make_scene(arrs2)[0]   # uploaded by the next call
        for q in (r, fresh):
            q.RebuildMeshes(*a)
            q.UpdateTriangles(*b[:3])
        same_bvh(r.ReadTriBvh(), fresh.ReadTriBvh(), f"{first} then {second}")
        assert len(r.ReadTriBvh()[2]) == second
        for got, want, what in zip(r.ReadTriNormals(), fresh.ReadTriNormals(), ("n1", "n2", "n3")):
            normals_ref.same_bits(got, want, what)
        assert r.TriBvhCost() == fresh.TriBvhCost()
    finally:
        r.close()
        fresh.close()


def test_smooth_normals_after_a_rebuild(gpu):
    P = 1537
    arrs = sphere_arrays(P)
    r = renderer(make_scene(arrs))
    try:
        a, b = pose("twist", arrs), pose("sine", arrs)
        r.RebuildMeshes(*a[:3])
        r.UpdateTriangles(*b[:3], normals="smooth")
        want = normals_ref.normals(*b[:3], [0], [P - 1], "smooth")
        for got, w, what in zip(r.ReadTriNormals(), want, ("n1", "n2", "n3")):
            normals_ref.same_bits(got, w, what)
    finally:
        r.close()


@ENGINES
def test_rebuild_at_the_upload_pose_renders_the_same(gpu, engine):
    arrs = sphere_arrays(6400)
    st = make_scene(arrs)
    r = renderer(st, engine)
    try:
        g0, rays0 = frame(r)
        o, orays = O.render(O.OracleScene(st[0]), st[1], st[2], W, H, SPP, seed=23)
        check(g0, rays0, o, orays)
        r.RebuildMeshes(*arrs[:3])
        g1, rays1 = frame(r)
        check(g1, rays1, o, orays)
        assert rays0 == rays1 and np.array_equal(g0.N, g1.N)
    finally:
        r.close()


# ------------------------------------------------------------------ 4. the cost gates on the device's numbers
@pytest.mark.parametrize("name,bound", [("offset", 1 / 3), ("twist", 0.8)])
def test_cost_gates(gpu, name, bound):
    arrs = sphere_arrays(6400)
    r = renderer(make_scene(arrs))
    try:
        moved = pose(name, arrs)
        r.UpdateTriangles(*moved[:3])
        refit = r.TriBvhCost()
        same_cost(refit, r.ReadTriBvh()[0], f"{name} refit")
        r.RebuildMeshes(*moved[:3])
        rebuilt = r.TriBvhCost()
        same_cost(rebuilt, r.ReadTriBvh()[0], f"{name} rebuilt")
        print(name, "cost refit", total_cost(refit), "rebuilt", total_cost(rebuilt))
        assert total_cost(rebuilt) <= bound * total_cost(refit)
        assert refit[2] > 0 and rebuilt[2] > 0
    finally:
        r.close()


# ------------------------------------------------------------------ 5. errors
def test_errors_leave_the_scene_untouched(gpu):
    arrs = sphere_arrays(193)
    r = renderer(make_scene(arrs))
    fp = C.POINTER(C.c_float)
    try:
        assert r._lib.pt_get_version() == 10
        before = r.ReadTriBvh()
        moved = pose("twist", arrs)
        n = len(moved[0])

        def upd(count=n, mode=0, reserved=0, skip=(), with_normals=False):
            u = _abi.pt_mesh_update()
            u.num_triangles, u.normals_mode = count, mode
            u.reserved[0] = reserved
            names = ("v1", "v2", "v3") + (("n1", "n2", "n3") if with_normals else ())
            for name, a in zip(names, moved):
                if name not in skip:
                    setattr(u, name, a.ctypes.data_as(fp))
            return u

        cases = {
            "NULL ctx": lambda: r._lib.pt_rebuild_meshes(None, C.byref(upd()), None),
            "NULL u, no staged pose": lambda: r._lib.pt_rebuild_meshes(r._ctx, None, None),
            "NULL v1": lambda: r._lib.pt_rebuild_meshes(r._ctx, C.byref(upd(skip=("v1",))), None),
            "NULL v3": lambda: r._lib.pt_rebuild_meshes(r._ctx, C.byref(upd(skip=("v3",))), None),
            "reserved": lambda: r._lib.pt_rebuild_meshes(r._ctx, C.byref(upd(reserved=1)), None),
            "normals_mode 3": lambda: r._lib.pt_rebuild_meshes(r._ctx, C.byref(upd(mode=3)), None),
            "normals and a mode": lambda: r._lib.pt_rebuild_meshes(r._ctx, C.byref(upd(mode=1, with_normals=True)), None),
            "n2 missing": lambda: r._lib.pt_rebuild_meshes(r._ctx, C.byref(upd(with_normals=True, skip=("n2",))), None),
            "one triangle fewer": lambda: r._lib.pt_rebuild_meshes(r._ctx, C.byref(upd(count=n - 1)), None),
            "one triangle more": lambda: r._lib.pt_rebuild_meshes(r._ctx, C.byref(upd(count=n + 1)), None),
            "cost: NULL out": lambda: r._lib.pt_tri_bvh_cost(r._ctx, None),
        }
        for what, call in cases.items():
            assert call() == _abi.PT_ERR_INVALID_ARG, what
            assert r._lib.pt_last_error()
            same_bvh(r.ReadTriBvh(), before, what)
    finally:
        r.close()
    # no scene
    r = Renderer.NewRenderer(None, None, None, W, H, True, device=0)
    try:
        u = _abi.pt_mesh_update()
        u.num_triangles = len(arrs[0])
        for name, a in zip(("v1", "v2", "v3"), arrs):
            setattr(u, name, a.ctypes.data_as(fp))
        assert r._lib.pt_rebuild_meshes(r._ctx, C.byref(u), None) == _abi.PT_ERR_NO_SCENE
        assert r._lib.pt_tri_bvh_cost(r._ctx, (C.c_double * 3)()) == _abi.PT_ERR_NO_SCENE
    finally:
        r.close()
    # an instanced mesh: BLASes are not rebuilt
    s, cam, smp = scenes.instances(copies=2, mesh_tris=200)
    r = renderer((s, cam, smp))
    try:
        before = r.ReadTriBvh()
        blas = r.ReadBlas()
        flat = s.Compile()
        v = [np.ascontiguousarray(a + f32(1)) for a in (flat.tri_v1, flat.tri_v2, flat.tri_v3)]
        with pytest.raises(_abi.PTError) as e:
            r.RebuildMeshes(*v)
        assert e.value.code == _abi.PT_ERR_UNSUPPORTED and "instanced mesh" in str(e.value)
        same_bvh(r.ReadTriBvh(), before, "instanced mesh")
        for a, b in zip(r.ReadBlas(), blas):
            assert np.array_equal(a, b)
        assert r.TriBvhCost() == (0.0, 0.0, 0.0)      # no triangle in the world BVH
    finally:
        r.close()
    # a scene without triangles: nothing to do
    s = Scene()
    s.Add(Sphere.NewSphere(Vector(0, 0, 6), 1, Material.LightMaterial(Colour.White, 20)))
    r = renderer((s, *make_scene(arrs)[1:]))
    try:
        r.Intersect(np.zeros((1, 3), f32), np.array([[0, 0, 1]], f32))   # uploads
        empty = np.zeros((1, 3), f32)
        u = _abi.pt_mesh_update()
        u.v1 = u.v2 = u.v3 = empty.ctypes.data_as(fp)
        ms = C.c_double(-1.0)
        assert r._lib.pt_rebuild_meshes(r._ctx, C.byref(u), C.byref(ms)) == _abi.PT_OK
        assert ms.value == 0.0
        assert r.TriBvhCost() == (0.0, 0.0, 0.0)
        nodes, chunks, recs, _ = r.ReadTriBvh()
        assert len(nodes) == len(chunks) == len(recs) == 0
    finally:
        r.close()
