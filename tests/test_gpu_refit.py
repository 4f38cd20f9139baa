"""pt_update_triangles on the GPU: the triangle BVH refitted on the device from new vertices.

  1. identity: an update with the upload's own arrays leaves every node, chunk and record word and the root
     box as they were, and a render after it is the render before it, bit for bit;
  2. after each deformed pose the words and the box are those of tests/refit_ref.py, the numpy restatement
     (itself checked on the CPU against the native check, tests/test_refit_host.py);
  3. rays: pt_intersect / pt_occluded after an update against the oracle on the deformed scene, t bits and kinds;
  4. renders and features after an update against the oracle and against a context that uploaded the
     deformed scene fresh (the emissive loose triangle moves to the other side of the mesh: a stale light fails);
  5. sequences of updates, an upload between updates, normals kept or replaced;
  6. the error cases leave the scene untouched.
The scene is tests/native/refit_check.cpp's grid: a 40x40 grid mesh (3,200 triangles) and three loose triangles,
one of them emissive, over a floor cube under a sphere light.  Frames are 64x48 at 2 spp.
"""
import ctypes as C

import numpy as np
import pytest

import features_ref as F
import oracle_lib as O
import refit_ref
from parity import check, same_buffer, within
from ptsharp_amd import Renderer, TransformedShape, Vector, _abi
from ptsharp_amd.geometry import Colour, Matrix
from ptsharp_amd.renderer import Buffer
from ptsharp_amd.scene import Camera, Cube, DefaultSampler, Material, Mesh, Scene, Sphere, Triangle, fix_normals_arrays

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 48, 2
ENGINES = pytest.mark.parametrize("engine", [_abi.ENGINE_MEGAKERNEL, _abi.ENGINE_WAVEFRONT], ids=["mega", "wavefront"])
GRID = 40
f32 = np.float32


def rest_arrays():
    """v1, v2, v3, n1, n2, n3 in the compiled scene's order: loose triangle 0, the grid, loose triangles 1 (emissive)
    and 2.  Face normals."""
    i, j = np.meshgrid(np.arange(GRID + 1), np.arange(GRID + 1), indexing="xy")
    x = (i.astype(f32) * f32(0.1) - f32(2)).astype(f32)
    y = (j.astype(f32) * f32(0.1) - f32(2)).astype(f32)
    z = (f32(0.25) * np.cos(f32(1.5) * x) * np.sin(f32(2) * y)).astype(f32)
    p = np.stack([x, y, z], axis=2)   # [j, i, 3]
    a, b, c, e = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]
    g1 = np.stack([a, b], axis=2).reshape(-1, 3)
    g2 = np.stack([b, e], axis=2).reshape(-1, 3)
    g3 = np.stack([c, c], axis=2).reshape(-1, 3)
    loose = np.array([[[-3, 0, 1], [-2.5, 0, 1], [-3, 0.5, 1.2]],
                      [[0, 0, 2], [0.5, 0, 2], [0, 0.5, 2]],
                      [[3, 3, -0.5], [3.5, 3, -0.5], [3, 3.5, -0.75]]], f32)
    v = [np.concatenate([loose[0:1, k], g, loose[1:3, k]]).astype(f32) for k, g in enumerate((g1, g2, g3))]
    z3 = np.zeros_like(v[0])
    n = fix_normals_arrays(v[0], v[1], v[2], z3, z3, z3)
    return [np.ascontiguousarray(q, f32) for q in v + list(n)]


EMISSIVE = 2 * GRID * GRID + 1   # the emissive loose triangle's index


def make_scene(arrs, instanced=False):
    v1, v2, v3, n1, n2, n3 = arrs
    s = Scene()
    grey = Material.DiffuseMaterial(Colour(0.7, 0.7, 0.7))
    vec = lambda r: Vector(*[float(q) for q in r])

    def tri(k, m):
        return Triangle(vec(v1[k]), vec(v2[k]), vec(v3[k]), vec(n1[k]), vec(n2[k]), vec(n3[k]), m)
    g = slice(1, 1 + 2 * GRID * GRID)
    mesh = Mesh(v1[g], v2[g], v3[g], n1[g], n2[g], n3[g])
    mesh.SetMaterial(Material.DiffuseMaterial(Colour(0.9, 0.6, 0.3)))
    s.Add(tri(0, grey))
    s.Add(mesh)
    s.Add(tri(EMISSIVE, Material.LightMaterial(Colour.White, 40)))
    s.Add(tri(EMISSIVE + 1, grey))
    s.Add(Cube.NewCube(Vector(-10, -10, -2), Vector(10, 10, -1), grey))
    s.Add(Sphere.NewSphere(Vector(0, 0, 6), 1, Material.LightMaterial(Colour.White, 20)))
    if instanced:
        small = Mesh(v1[1:9] * f32(0.2), v2[1:9] * f32(0.2), v3[1:9] * f32(0.2), n1[1:9], n2[1:9], n3[1:9])
        small.SetMaterial(grey)
        s.Add(TransformedShape.NewTransformedShape(small, Matrix.TranslateM(Vector(0, 0, 3))))
    camera = Camera.LookAt(Vector(4, 4, 4), Vector(0, 0, 0), Vector(0, 0, 1), 45)
    sampler = DefaultSampler.NewSampler(4, 3)
    return s, camera, sampler


def pose(name, arrs):
    """The CPU check's poses, in fp32; `lit` is the sine pose with the emissive triangle under the mesh."""
    out = [a.copy() for a in arrs]
    for k in range(3):
        p = arrs[k]
        x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
        if name == "translate":
            q = np.stack([x + f32(1000), y - f32(2000), z + f32(3000)], 1)
        elif name == "scale":
            q = np.stack([x * f32(37), y * f32(0.01), z], 1)
        elif name in ("sine", "lit"):
            q = np.stack([x, y, z + (f32(0.3) * np.sin(f32(5) * x) * np.cos(f32(3) * y)).astype(f32)], 1)
            if name == "lit":
                q[EMISSIVE, 2] = f32(-0.7) - (z[EMISSIVE] - f32(2))
        elif name == "flat":
            q = np.stack([x, y, np.zeros_like(z)], 1)
        elif name == "point":
            q = np.broadcast_to(np.array([0.5, -0.25, 2.0], f32), p.shape)
        elif name == "huge":
            q = p * f32(1e6)
        elif name == "tiny":
            q = p * f32(1e-6)
        else:
            raise KeyError(name)
        out[k] = np.ascontiguousarray(q, f32)
    return out


POSES = ["translate", "scale", "sine", "flat", "point", "huge", "tiny"]


def renderer(scene_tuple, engine=_abi.ENGINE_WAVEFRONT, seed=23):
    s, c, smp = scene_tuple
    r = Renderer.NewRenderer(s, c, smp, W, H, True, device=0)
    r.SamplesPerPixel, r.Seed, r.Engine = SPP, seed, engine
    return r


def frame(r):
    """One pass from an empty Buffer: (Buffer copy, rays)."""
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


# ------------------------------------------------------------------ 1. identity
@ENGINES
def test_identity_on_the_device(gpu, engine):
    arrs = rest_arrays()
    r = renderer(make_scene(arrs), engine)
    try:
        before = r.ReadTriBvh()
        assert len(before[0]) > 100 and len(before[2]) == 2 * GRID * GRID + 3
        img0, rays0 = frame(r)
        ms = r.UpdateTriangles(*arrs[:3])
        assert ms > 0
        same_bvh(r.ReadTriBvh(), before, "identity")
        img1, rays1 = frame(r)
        assert rays0 == rays1
        same_buffer(img1, img0)
        r.UpdateTriangles(*arrs)   # and with the normals given
        same_bvh(r.ReadTriBvh(), before, "identity with normals")
    finally:
        r.close()


# ------------------------------------------------------------------ 2. bytes after each pose
@pytest.mark.parametrize("name", POSES)
def test_bytes_after_a_pose(gpu, name):
    arrs = rest_arrays()
    st = make_scene(arrs)
    r = renderer(st)
    try:
        before = r.ReadTriBvh()
        src = refit_ref.src_of_pos_from(before[2], st[0].Compile())
        moved = pose(name, arrs)
        want = refit_ref.refit(before[0], before[1], before[2], src, *moved[:3])
        r.UpdateTriangles(*moved[:3])
        got = r.ReadTriBvh()
        same_bvh(got, want, name)
        assert not np.array_equal(got[0], before[0])
        flat = st[0].Compile()
        assert np.array_equal(flat.tri_v1, moved[0]) and np.array_equal(flat.tri_v3, moved[2])
    finally:
        r.close()


# ------------------------------------------------------------------ 3. rays
def rays_at(lo, hi, n, seed):
    """Rays from a shell around the box [lo, hi] to points inside it (rays along the axes, in the boxes' planes and
    through vertices are tests/degenerate_rays.py's)."""
    rng = np.random.default_rng(seed)
    c, ext = (lo + hi) / 2, np.maximum((hi - lo) / 2, 0.5)
    u = rng.standard_normal((n, 3))
    o = c + 4.0 * np.abs(ext).max() * u / np.linalg.norm(u, axis=1, keepdims=True)
    t = (c - ext) + 2 * ext * rng.random((n, 3))
    o, t = o.astype(f32), t.astype(f32)
    d = (t - o).astype(f32)
    d = (d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(f32)
    return o, d


@pytest.mark.parametrize("name", ["sine", "translate"])
def test_rays_after_an_update(gpu, name):
    arrs = rest_arrays()
    st = make_scene(arrs)
    r = renderer(st)
    try:
        r.Intersect(np.zeros((1, 3), f32), np.array([[0, 0, 1]], f32))   # uploads
        old_box = r.ReadTriBvh()[3].copy()
        moved = pose(name, arrs)
        r.UpdateTriangles(*moved[:3])
        allv = np.concatenate(moved[:3])
        lo, hi = allv.min(axis=0).astype(np.float64), allv.max(axis=0).astype(np.float64)
        o, d = rays_at(lo, hi, 4096, 31)
        outside_old = ((o < old_box[:3]) | (o > old_box[3:])).any(axis=1)
        assert outside_old.sum() > 1000
        t, k = r.Intersect(o, d)
        os_ = O.OracleScene(st[0])   # the FlatScene the update wrote into
        ot = np.empty(len(o), np.float64)
        ok = np.empty(len(o), np.int32)
        for i in range(len(o)):
            ot[i], ok[i], _ = os_.intersect(o[i], d[i])
        bad = np.flatnonzero((t.view(np.int64) != ot.view(np.int64)) | (k != ok))
        assert bad.size == 0, (f"{bad.size} of {len(o)} rays differ from the oracle, first {bad[:5]}: gpu t {t[bad[:3]]} "
                               f"kind {k[bad[:3]]}, oracle t {ot[bad[:3]]} kind {ok[bad[:3]]}")
        tri_hits = int(((ok == _abi.SHAPE_TRIANGLE) & outside_old).sum())
        assert tri_hits > 300, f"only {tri_hits} triangle hits from outside the old box"
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
@ENGINES
def test_render_parity_after_an_update(gpu, engine):
    arrs = rest_arrays()
    st = make_scene(arrs)
    moved = pose("lit", arrs)
    r = renderer(st, engine)
    fresh = renderer(make_scene(moved[:3] + arrs[3:]), engine)
    try:
        frame(r)                        # a pass at the rest pose first: the update comes between passes
        r.UpdateTriangles(*moved[:3])
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
            assert (got[3] == _abi.SHAPE_TRIANGLE).sum() > 200
    finally:
        r.close()
        fresh.close()


# ------------------------------------------------------------------ 5. sequences and lifecycle
def test_pose_a_then_pose_b_is_pose_b(gpu):
    arrs = rest_arrays()
    r, r2 = renderer(make_scene(arrs)), renderer(make_scene(arrs))
    try:
        a, b = pose("scale", arrs), pose("sine", arrs)
        r.UpdateTriangles(*a[:3])
        r.UpdateTriangles(*b[:3])
        r2.UpdateTriangles(*b[:3])
        same_bvh(r.ReadTriBvh(), r2.ReadTriBvh(), "A then B against B")
        same_buffer(frame(r)[0], frame(r2)[0])
    finally:
        r.close()
        r2.close()


def test_update_upload_update(gpu):
    """An update, an upload of another scene (fewer triangles, another order), an update of that one: the
    second update uses the second upload's tables."""
    arrs = rest_arrays()
    r = renderer(make_scene(arrs))
    try:
        r.UpdateTriangles(*pose("sine", arrs)[:3])
        keep = np.r_[0:1601, 3201:3203]
        small = [np.ascontiguousarray(a[keep][::-1]) for a in arrs]
        s = Scene()
        m = Mesh(*small)
        m.SetMaterial(Material.DiffuseMaterial(Colour(0.5, 0.5, 0.5)))
        s.Add(m)
        s.Add(Sphere.NewSphere(Vector(0, 0, 6), 1, Material.LightMaterial(Colour.White, 20)))
        r.Scene = s
        before = r.ReadTriBvh()      # uploads the new scene
        assert len(before[2]) == len(keep)
        src = refit_ref.src_of_pos_from(before[2], s.Compile())
        moved = pose("scale", small)
        want = refit_ref.refit(before[0], before[1], before[2], src, *moved[:3])
        r.UpdateTriangles(*moved[:3])
        same_bvh(r.ReadTriBvh(), want, "after the second upload")
        with pytest.raises(ValueError):
            r.UpdateTriangles(*arrs[:3])      # the first scene's count
    finally:
        r.close()


def test_normals_kept_or_replaced(gpu):
    arrs = rest_arrays()
    st = make_scene(arrs)
    r = renderer(st)
    try:
        before = r.ReadTriBvh()
        src = refit_ref.src_of_pos_from(before[2], st[0].Compile())
        moved = pose("sine", arrs)
        r.UpdateTriangles(*moved[:3])
        kept = r.ReadTriBvh()
        assert np.array_equal(kept[2][:, 12:32], before[2][:, 12:32])      # normals, material and uv rows stay
        rng = np.random.default_rng(3)
        normals = [rng.standard_normal(a.shape).astype(f32) for a in arrs[3:]]
        r.UpdateTriangles(*moved[:3], *normals)
        got = r.ReadTriBvh()
        same_bvh(got, refit_ref.refit(before[0], before[1], before[2], src, *moved[:3], *normals), "normals given")
        assert np.array_equal(got[0], kept[0]) and np.array_equal(got[1], kept[1])
        assert np.array_equal(got[2][:, :12], kept[2][:, :12]) and np.array_equal(got[2][:, 21:], kept[2][:, 21:])
        assert not np.array_equal(got[2][:, 12:21], kept[2][:, 12:21])
        assert np.array_equal(st[0].Compile().tri_n2, normals[1])
    finally:
        r.close()


# ------------------------------------------------------------------ 6. errors
def _raw_update(r, n, ptrs, ms=None):
    return r._lib.pt_update_triangles(r._ctx, n, *ptrs, ms)


def test_errors_leave_the_scene_untouched(gpu):
    arrs = rest_arrays()
    r = renderer(make_scene(arrs))
    fp = C.POINTER(C.c_float)
    null = fp()
    try:
        assert r._lib.pt_get_version() == 10
        before = r.ReadTriBvh()
        img0, _ = frame(r)
        moved = pose("sine", arrs)
        p = [a.ctypes.data_as(fp) for a in moved]
        n = len(moved[0])
        cases = {
            "NULL ctx": lambda: r._lib.pt_update_triangles(None, n, *p, None),
            "NULL v1": lambda: _raw_update(r, n, [null] + p[1:]),
            "NULL v2": lambda: _raw_update(r, n, [p[0], null] + p[2:]),
            "NULL v3": lambda: _raw_update(r, n, p[:2] + [null] + p[3:]),
            "n1 only": lambda: _raw_update(r, n, p[:4] + [null, null]),
            "n2 missing": lambda: _raw_update(r, n, p[:4] + [null, p[5]]),
            "n3 only": lambda: _raw_update(r, n, p[:3] + [null, null, p[5]]),
            "one triangle fewer": lambda: _raw_update(r, n - 1, p),
            "one triangle more": lambda: _raw_update(r, n + 1, p),
            "no triangles": lambda: _raw_update(r, 0, p),
        }
        for what, call in cases.items():
            assert call() == _abi.PT_ERR_INVALID_ARG, what
            same_bvh(r.ReadTriBvh(), before, what)
            same_buffer(frame(r)[0], img0)
    finally:
        r.close()
    # no scene
    r = Renderer.NewRenderer(None, None, None, W, H, True, device=0)
    try:
        p = [a.ctypes.data_as(fp) for a in arrs]
        assert _raw_update(r, len(arrs[0]), p) == _abi.PT_ERR_NO_SCENE
        assert r._lib.pt_read_tri_bvh(r._ctx, None, None, None, None, None) == _abi.PT_ERR_NO_SCENE
    finally:
        r.close()
    # an instanced mesh
    st = make_scene(arrs, instanced=True)
    r = renderer(st)
    try:
        before = r.ReadTriBvh()
        img0, _ = frame(r)
        flat = st[0].Compile()
        n = len(flat.tri_material)
        assert n == len(arrs[0]) + 8
        v = [np.ascontiguousarray(a + f32(1)) for a in (flat.tri_v1, flat.tri_v2, flat.tri_v3)]
        p = [a.ctypes.data_as(fp) for a in v] + [null] * 3
        assert _raw_update(r, n, p) == _abi.PT_ERR_UNSUPPORTED
        assert b"instanced mesh" in r._lib.pt_last_error()
        same_bvh(r.ReadTriBvh(), before, "instanced mesh")
        same_buffer(frame(r)[0], img0)
    finally:
        r.close()
    # a scene without triangles: nothing to do
    s = Scene()
    s.Add(Sphere.NewSphere(Vector(0, 0, 6), 1, Material.LightMaterial(Colour.White, 20)))
    r = renderer((s, *make_scene(arrs)[1:]))
    try:
        img0, _ = frame(r)
        empty = np.zeros((1, 3), f32)
        ms = C.c_double(-1.0)
        assert _raw_update(r, 0, [empty.ctypes.data_as(fp)] * 3 + [null] * 3, C.byref(ms)) == _abi.PT_OK
        assert ms.value == 0.0
        nodes, chunks, recs, _ = r.ReadTriBvh()
        assert len(nodes) == len(chunks) == len(recs) == 0
        same_buffer(frame(r)[0], img0)
    finally:
        r.close()
