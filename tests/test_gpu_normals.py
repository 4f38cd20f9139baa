"""pt_update_triangles_normals on the GPU: the normals of moved triangles derived on the device, face and smooth.

  1. FACE: Renderer.ReadTriNormals() after the update equals tests/normals_ref.py bit for bit, every pose;
  2. SMOOTH: the same (NaNs compared by position), after the reference alone has shown that the scene can tell a
     right answer from a wrong one;
  3. records: the triangle BVH after either mode is tests/refit_ref.py's with the reference normals given;
  4. renders and features after a SMOOTH update against the oracle on the written-back FlatScene and against a
     context that uploaded the posed, host-smoothed scene fresh;
  5. sequences: pose A then B, a plain update after a SMOOTH one, an upload between two SMOOTH calls, the reader
     right after an upload;
  6. the error cases leave the scene untouched.
normals_ref.py is checked on the CPU against tests/native/normals_check.cpp (tests/test_normals_host.py).
The scene: tests/test_gpu_refit.py's 40x40 grid as two meshes (rows 0-19 and 20-39) that share the seam's positions,
a fan of 300 triangles around one hub as a third mesh (a run of equal keys longer than a wave and than a block; two
turns over 150 rim points, the second joining every rim point to the next but one, so that the mesh has fewer
distinct positions than a third of its corners, which a single turn misses by one), three loose triangles, one of
them emissive, over a floor cube under a sphere light.  Frames are 64x48 at 2 spp.
"""
import ctypes as C

import numpy as np
import pytest

import features_ref as F
import normals_ref
import oracle_lib as O
import refit_ref
from parity import check, same_buffer
from ptsharp_amd import Renderer, TransformedShape, Vector, _abi
from ptsharp_amd.geometry import Colour, Matrix
from ptsharp_amd.renderer import Buffer
from ptsharp_amd.scene import Camera, Cube, DefaultSampler, Material, Mesh, Scene, Sphere, Triangle

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 48, 2
ENGINES = pytest.mark.parametrize("engine", [_abi.ENGINE_MEGAKERNEL, _abi.ENGINE_WAVEFRONT], ids=["mega", "wavefront"])
GRID, FAN, RIM = 40, 300, 150
HALF = GRID * GRID                  # triangles of one grid mesh
A0, L1, B0, F0, L2 = 1, 1 + HALF, 2 + HALF, 2 + 2 * HALF, 2 + 2 * HALF + FAN   # source order: loose 0 | mesh A | loose 1 | mesh B | fan | loose 2
NTRI = L2 + 1
MESH_FIRST, MESH_COUNT = [A0, B0, F0], [HALF, HALF, FAN]
EMISSIVE = L1
f32 = np.float32
POSES = ["sine", "scale", "huge", "tiny", "translate", "zero-sign", "degenerate"]
DEGENERATE = [A0 + 100, A0 + 101, B0 + 400, B0 + 401]


def rest_positions():
    i, j = np.meshgrid(np.arange(GRID + 1), np.arange(GRID + 1), indexing="xy")
    x = (i.astype(f32) * f32(0.1) - f32(2)).astype(f32)
    y = (j.astype(f32) * f32(0.1) - f32(2)).astype(f32)
    z = (f32(0.25) * np.cos(f32(1.5) * x) * np.sin(f32(2) * y)).astype(f32)
    p = np.stack([x, y, z], axis=2)   # [j, i, 3]
    a, b, c, e = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]
    grid = [np.stack(q, axis=2).reshape(-1, 3) for q in ((a, b), (b, e), (c, c))]   # rows of cells, two triangles per cell
    th = (np.arange(RIM).astype(f32) * f32(2 * np.pi / RIM)).astype(f32)
    rim = np.stack([f32(3) + np.cos(th), f32(-3) + np.sin(th), f32(0.2) + f32(0.2) * np.sin(f32(3) * th)], axis=1).astype(f32)
    hub = np.broadcast_to(np.array([3, -3, 0.5], f32), (FAN, 3))
    k = np.arange(RIM)
    fan = [hub, rim[np.r_[k, k]], rim[np.r_[(k + 1) % RIM, (k + 2) % RIM]]]   # two turns: to the next rim point, to the one after
    loose = np.array([[[-3, 0, 1], [-2.5, 0, 1], [-3, 0.5, 1.2]],
                      [[0, 0, 2], [0.5, 0, 2], [0, 0.5, 2]],
                      [[3, 3, -0.5], [3.5, 3, -0.5], [3, 3.5, -0.75]]], f32)
    return [np.ascontiguousarray(np.concatenate([loose[0:1, k], grid[k][:HALF], loose[1:2, k], grid[k][HALF:], fan[k], loose[2:3, k]]), f32)
            for k in range(3)]


def rest_arrays():
    """v1, v2, v3, n1, n2, n3 in the compiled scene's order, face normals."""
    v = rest_positions()
    assert len(v[0]) == NTRI
    return v + normals_ref.normals(*v, MESH_FIRST, MESH_COUNT, "face")


def make_scene(arrs, instanced=False):
    v1, v2, v3, n1, n2, n3 = arrs
    s = Scene()
    grey = Material.DiffuseMaterial(Colour(0.7, 0.7, 0.7))
    vec = lambda r: Vector(*[float(q) for q in r])

    def tri(k, m):
        return Triangle(vec(v1[k]), vec(v2[k]), vec(v3[k]), vec(n1[k]), vec(n2[k]), vec(n3[k]), m)

    def mesh(first, count, colour):
        g = slice(first, first + count)
        m = Mesh(v1[g], v2[g], v3[g], n1[g], n2[g], n3[g])
        m.SetMaterial(Material.DiffuseMaterial(colour))
        return m
    s.Add(tri(0, grey))
    s.Add(mesh(A0, HALF, Colour(0.9, 0.6, 0.3)))
    s.Add(tri(L1, Material.LightMaterial(Colour.White, 40)))
    s.Add(mesh(B0, HALF, Colour(0.3, 0.6, 0.9)))
    s.Add(mesh(F0, FAN, Colour(0.4, 0.8, 0.4)))
    s.Add(tri(L2, grey))
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
    """New v1, v2, v3.  `lit` is the sine pose with the emissive triangle under the mesh; `zero-sign` and
    `degenerate` are the sine pose with the grid vertex at x = 0, y = 0 (on the seam, three triangles of either mesh)
    written as -0 in its even triangles, and with four grid triangles collapsed to their first vertex."""
    out = []
    for k in range(3):
        p = arrs[k]
        x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
        if name == "translate":
            q = np.stack([x + f32(1000), y - f32(2000), z + f32(3000)], 1)
        elif name == "scale":
            q = np.stack([x * f32(37), y * f32(0.01), z], 1)
        elif name in ("sine", "lit", "zero-sign", "degenerate"):
            q = np.stack([x, y, z + (f32(0.3) * np.sin(f32(5) * x) * np.cos(f32(3) * y)).astype(f32)], 1)
            if name == "lit":
                q[EMISSIVE, 2] = f32(-0.7) - (z[EMISSIVE] - f32(2))
            if name == "zero-sign":
                at = np.flatnonzero((x == 0) & (y == 0) & (z < 1))
                q[at[at % 2 == 0], 0] = f32(-0.0)
        elif name == "huge":
            q = p * f32(1e6)
        elif name == "tiny":
            q = p * f32(1e-6)
        else:
            raise KeyError(name)
        out.append(np.ascontiguousarray(q, f32))
    if name == "degenerate":
        out[1][DEGENERATE] = out[0][DEGENERATE]
        out[2][DEGENERATE] = out[0][DEGENERATE]
    return out


_REF = {}


def reference(name, mode):
    """(v1, v2, v3), (n1, n2, n3) of a pose, computed once and left unchanged."""
    if (name, mode) not in _REF:
        v = pose(name, rest_arrays())
        n = normals_ref.normals(*v, MESH_FIRST, MESH_COUNT, mode)
        for a in v + n:
            a.setflags(write=False)
        _REF[(name, mode)] = (v, n)
    return _REF[(name, mode)]


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


def same_normals(got, want, what):
    for k in range(3):
        normals_ref.same_bits(got[k], want[k], f"{what} n{k + 1}")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ------------------------------------------------------------------ 1. FACE
@pytest.mark.parametrize("name", POSES)
def test_face_normals(gpu, name):
    v, want = reference(name, "face")
    st = make_scene(rest_arrays())
    r = renderer(st)
    try:
        ms = r.UpdateTriangles(*v, normals="face")
        assert ms > 0
        same_normals(r.ReadTriNormals(), want, f"face {name}")
        flat = st[0].Compile()
        same_normals((flat.tri_n1, flat.tri_n2, flat.tri_n3), want, f"face {name}, the FlatScene")
        assert np.array_equal(flat.tri_v2, v[1])
    finally:
        r.close()


# ------------------------------------------------------------------ 2. SMOOTH
def corner_keys(v, first, count):
    """[3 count, 3] uint32: the position words of a mesh's corners after + 0.0, triangle-major."""
    c = np.stack([a[first:first + count] for a in v], axis=1).reshape(-1, 3)
    return bits(c + f32(0))


def check_reference_can_tell(name):
    """On the reference alone: the input separates a right answer from a wrong one."""
    v, smooth = reference(name, "smooth")
    _, face = reference(name, "face")
    sm = np.stack(smooth, axis=1)   # [n, corner, 3]
    fc = np.stack(face, axis=1)
    for first, count in zip(MESH_FIRST, MESH_COUNT):
        keys = corner_keys(v, first, count)
        distinct = len(np.unique(keys, axis=0))
        assert distinct < 3 * count / 3, f"{name}: mesh at {first}: {distinct} distinct positions of {3 * count} corners"
    grid = np.r_[A0:A0 + HALF, B0:B0 + HALF]
    differ = (bits(sm[grid]) != bits(fc[grid])).any(axis=2)
    assert differ.mean() > 0.5, f"{name}: smooth differs from face on {differ.mean():.2f} of the grid's corners"
    # the seam: positions that both grid meshes hold; their corners differ between the meshes, and from the grid smoothed as one mesh
    ka, kb = corner_keys(v, A0, HALF), corner_keys(v, B0, HALF)
    na, nb = bits(sm[A0:A0 + HALF]).reshape(-1, 3), bits(sm[B0:B0 + HALF]).reshape(-1, 3)
    of_a = {k.tobytes(): n for k, n in zip(ka, na)}
    shared = [(of_a[k.tobytes()], n) for k, n in zip(kb, nb) if k.tobytes() in of_a]
    assert len(shared) >= 3 * (GRID - 1)
    across = np.mean([(a != b).any() for a, b in shared])
    assert across > 0.9, f"{name}: the seam's corners differ between the meshes on {across:.2f}"
    gv = [np.concatenate([a[A0:A0 + HALF], a[B0:B0 + HALF]]) for a in v]
    one = np.stack(normals_ref.smooth_range(*gv, *[np.concatenate([a[A0:A0 + HALF], a[B0:B0 + HALF]]) for a in face]), axis=1)
    in_b = {q.tobytes() for q in kb}
    seam_a = np.array([k.tobytes() in in_b for k in ka]).reshape(HALF, 3)
    merged = (bits(one[:HALF])[seam_a] != bits(sm[A0:A0 + HALF])[seam_a]).any(axis=1)
    assert merged.mean() > 0.9, f"{name}: the seam differs from the grid smoothed as one mesh on {merged.mean():.2f}"
    # the hub's 300 corners hold one value
    hub = bits(smooth[0][F0:F0 + FAN])
    assert (hub == hub[0]).all() and not np.isnan(smooth[0][F0]).any()
    assert (bits(face[0][F0:F0 + FAN]) != hub[0]).any(axis=1).mean() > 0.9
    nan_corners = int(np.isnan(sm).any(axis=2).sum())
    if name == "degenerate":
        assert 12 <= nan_corners <= 0.02 * 3 * NTRI, nan_corners
    else:
        assert nan_corners == 0
    if name == "zero-sign":
        for first in (A0, B0):
            x = np.stack([a[first:first + HALF, 0] for a in v], axis=1)
            zero = x == 0
            assert (np.signbit(x) & zero).sum() >= 1 and (~np.signbit(x) & zero).sum() >= 1
            at = zero & (np.stack([a[first:first + HALF, 1] for a in v], axis=1) == 0)
            assert at.sum() == 3 and len(np.unique(bits(sm[first:first + HALF])[at], axis=0)) == 1
    # loose triangles keep the face normal
    for t in (0, L1, L2):
        assert np.array_equal(bits(sm[t]), bits(fc[t]))


@pytest.mark.parametrize("name", POSES)
def test_smooth_normals(gpu, name):
    check_reference_can_tell(name)
    v, want = reference(name, "smooth")
    st = make_scene(rest_arrays())
    r = renderer(st)
    try:
        ms = r.UpdateTriangles(*v, normals="smooth")
        assert ms > 0
        same_normals(r.ReadTriNormals(), want, f"smooth {name}")
        flat = st[0].Compile()
        same_normals((flat.tri_n1, flat.tri_n2, flat.tri_n3), want, f"smooth {name}, the FlatScene")
    finally:
        r.close()


# ------------------------------------------------------------------ 3. records
@pytest.mark.parametrize("mode", ["face", "smooth"])
@pytest.mark.parametrize("name", ["sine", "zero-sign"])
def test_records_after_an_update(gpu, mode, name):
    arrs = rest_arrays()
    st = make_scene(arrs)
    r = renderer(st)
    try:
        before = r.ReadTriBvh()
        assert len(before[2]) == NTRI
        src = refit_ref.src_of_pos_from(before[2], st[0].Compile())
        v, n = reference(name, mode)
        want = refit_ref.refit(before[0], before[1], before[2], src, *v, *n)
        r.UpdateTriangles(*v, normals=mode)
        got = r.ReadTriBvh()
        same_bvh(got, want, f"{mode} {name}")
        assert np.array_equal(got[2][:, 21], before[2][:, 21]) and np.array_equal(got[2][:, 24:], before[2][:, 24:])   # material, uv
        assert not np.array_equal(got[2][:, 12:21], before[2][:, 12:21]) and not np.array_equal(got[0], before[0])
    finally:
        r.close()


# ------------------------------------------------------------------ 4. renders and features
@ENGINES
def test_render_parity_after_a_smooth_update(gpu, engine):
    arrs = rest_arrays()
    st = make_scene(arrs)
    v, n = reference("lit", "smooth")
    r = renderer(st, engine)
    fresh = renderer(make_scene(list(v) + list(n)), engine)
    try:
        frame(r)                        # a pass at the rest pose first: the update comes between passes
        r.UpdateTriangles(*v, normals="smooth")
        g, grays = frame(r)
        o, orays = O.render(O.OracleScene(st[0]), st[1], st[2], W, H, SPP, seed=23)   # the FlatScene the update wrote into
        check(g, grays, o, orays)
        _, frays = frame(fresh)
        assert grays == frays
        assert (g.M.sum(axis=2) > 0).mean() > 0.5
        if engine == _abi.ENGINE_WAVEFRONT:
            r.RenderFeatures()
            got = r.Features()
            want = F.features(st[0], st[1], W, H)
            assert np.array_equal(got[1].view(np.uint8), want[1].view(np.uint8)), "the features' normal after the update"
            assert (got[3] == _abi.SHAPE_TRIANGLE).sum() > 200
    finally:
        r.close()
        fresh.close()


# ------------------------------------------------------------------ 5. sequences and lifecycle
def test_pose_a_then_pose_b_is_pose_b(gpu):
    arrs = rest_arrays()
    r, r2 = renderer(make_scene(arrs)), renderer(make_scene(arrs))
    try:
        a, _ = reference("scale", "smooth")
        b, nb = reference("sine", "smooth")
        r.UpdateTriangles(*a, normals="smooth")
        r.UpdateTriangles(*b, normals="smooth")
        r2.UpdateTriangles(*b, normals="smooth")
        same_bvh(r.ReadTriBvh(), r2.ReadTriBvh(), "A then B against B")
        same_normals(r.ReadTriNormals(), nb, "A then B")
        same_normals(r2.ReadTriNormals(), nb, "B")
    finally:
        r.close()
        r2.close()


def test_plain_update_keeps_the_smooth_normals(gpu):
    arrs = rest_arrays()
    st = make_scene(arrs)
    r = renderer(st)
    try:
        v, n = reference("sine", "smooth")
        r.UpdateTriangles(*v, normals="smooth")
        recs = r.ReadTriBvh()[2]
        moved, _ = reference("scale", "smooth")
        r.UpdateTriangles(*moved)
        same_normals(r.ReadTriNormals(), n, "kept")
        after = r.ReadTriBvh()[2]
        assert np.array_equal(after[:, 12:], recs[:, 12:]) and not np.array_equal(after[:, :9], recs[:, :9])
        flat = st[0].Compile()
        same_normals((flat.tri_n1, flat.tri_n2, flat.tri_n3), n, "kept, the FlatScene")
        # and given normals replace them
        given = [np.ascontiguousarray(a[::-1]) for a in n]
        r.UpdateTriangles(*moved, *given)
        same_normals(r.ReadTriNormals(), given, "given")
    finally:
        r.close()


def test_upload_between_two_smooth_updates(gpu):
    """A SMOOTH update, an upload of another scene (fewer triangles, another order, one mesh), a SMOOTH update of that
    one: the second uses the second upload's tables."""
    arrs = rest_arrays()
    r = renderer(make_scene(arrs))
    try:
        r.UpdateTriangles(*reference("sine", "smooth")[0], normals="smooth")
        keep = np.r_[A0:A0 + HALF, F0:F0 + FAN]
        small = [np.ascontiguousarray(a[keep][::-1]) for a in arrs]
        s = Scene()
        m = Mesh(*small)
        m.SetMaterial(Material.DiffuseMaterial(Colour(0.5, 0.5, 0.5)))
        s.Add(m)
        s.Add(Sphere.NewSphere(Vector(0, 0, 6), 1, Material.LightMaterial(Colour.White, 20)))
        r.Scene = s
        same_normals(r.ReadTriNormals(), small[3:], "right after the second upload")   # uploads the new scene
        before = r.ReadTriBvh()
        assert len(before[2]) == len(keep)
        src = refit_ref.src_of_pos_from(before[2], s.Compile())
        moved = pose("scale", small)
        n = normals_ref.normals(*moved, [0], [len(keep)], "smooth")
        r.UpdateTriangles(*moved, normals="smooth")
        same_normals(r.ReadTriNormals(), n, "after the second upload")
        same_bvh(r.ReadTriBvh(), refit_ref.refit(before[0], before[1], before[2], src, *moved, *n), "after the second upload")
        with pytest.raises(ValueError):
            r.UpdateTriangles(*arrs[:3], normals="smooth")      # the first scene's count
    finally:
        r.close()


def test_read_normals_right_after_an_upload(gpu):
    rng = np.random.default_rng(5)
    arrs = rest_arrays()
    arrs[3:] = [rng.standard_normal(a.shape).astype(f32) for a in arrs[3:]]
    r = renderer(make_scene(arrs))
    try:
        before = r.ReadTriBvh()
        same_normals(r.ReadTriNormals(), arrs[3:], "uploaded")
        same_normals(r.ReadTriNormals(), arrs[3:], "uploaded, read twice")
        same_bvh(r.ReadTriBvh(), before, "the reader changes nothing")
    finally:
        r.close()


# ------------------------------------------------------------------ 6. errors
def test_errors_leave_the_scene_untouched(gpu):
    arrs = rest_arrays()
    r = renderer(make_scene(arrs))
    fp = C.POINTER(C.c_float)
    null = fp()
    up = lambda ctx, n, p, mode, ms=None: r._lib.pt_update_triangles_normals(ctx, n, *p, mode, ms)
    try:
        assert r._lib.pt_get_version() == 10
        before = r.ReadTriBvh()
        normals0 = r.ReadTriNormals()
        img0, _ = frame(r)
        moved = reference("sine", "smooth")[0]
        p = [a.ctypes.data_as(fp) for a in moved]
        out = [np.zeros((NTRI, 3), f32) for _ in range(3)]
        q = [a.ctypes.data_as(fp) for a in out]
        n = NTRI
        SM = _abi.NORMALS_SMOOTH
        cases = {
            "NULL ctx": lambda: up(None, n, p, SM),
            "NULL v1": lambda: up(r._ctx, n, [null] + p[1:], SM),
            "NULL v2": lambda: up(r._ctx, n, [p[0], null, p[2]], SM),
            "NULL v3": lambda: up(r._ctx, n, p[:2] + [null], _abi.NORMALS_FACE),
            "mode 0": lambda: up(r._ctx, n, p, 0),
            "mode 3": lambda: up(r._ctx, n, p, 3),
            "mode -1": lambda: up(r._ctx, n, p, -1),
            "one triangle fewer": lambda: up(r._ctx, n - 1, p, SM),
            "one triangle more": lambda: up(r._ctx, n + 1, p, _abi.NORMALS_FACE),
            "no triangles": lambda: up(r._ctx, 0, p, SM),
            "reader: NULL ctx": lambda: r._lib.pt_read_tri_normals(None, *q),
            "reader: NULL n1": lambda: r._lib.pt_read_tri_normals(r._ctx, null, q[1], q[2]),
            "reader: NULL n3": lambda: r._lib.pt_read_tri_normals(r._ctx, q[0], q[1], null),
        }
        for what, call in cases.items():
            assert call() == _abi.PT_ERR_INVALID_ARG, what
            same_bvh(r.ReadTriBvh(), before, what)
            same_normals(r.ReadTriNormals(), normals0, what)
            same_buffer(frame(r)[0], img0)
        with pytest.raises(ValueError):
            r.UpdateTriangles(*moved, *normals0, normals="smooth")   # the keyword is exclusive with n1..n3
        with pytest.raises(ValueError):
            r.UpdateTriangles(*moved, normals="flat")
        same_bvh(r.ReadTriBvh(), before, "the wrapper's own checks")
    finally:
        r.close()
    # no scene
    r = Renderer.NewRenderer(None, None, None, W, H, True, device=0)
    try:
        p = [a.ctypes.data_as(fp) for a in arrs[:3]]
        out = [np.zeros((NTRI, 3), f32) for _ in range(3)]
        assert r._lib.pt_update_triangles_normals(r._ctx, NTRI, *p, _abi.NORMALS_SMOOTH, None) == _abi.PT_ERR_NO_SCENE
        assert r._lib.pt_read_tri_normals(r._ctx, *[a.ctypes.data_as(fp) for a in out]) == _abi.PT_ERR_NO_SCENE
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
        assert n == NTRI + 8
        v = [np.ascontiguousarray(a + f32(1)) for a in (flat.tri_v1, flat.tri_v2, flat.tri_v3)]
        p = [a.ctypes.data_as(fp) for a in v]
        for mode in (_abi.NORMALS_FACE, _abi.NORMALS_SMOOTH):
            assert r._lib.pt_update_triangles_normals(r._ctx, n, *p, mode, None) == _abi.PT_ERR_UNSUPPORTED
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
        e = empty.ctypes.data_as(fp)
        assert r._lib.pt_update_triangles_normals(r._ctx, 0, e, e, e, _abi.NORMALS_SMOOTH, C.byref(ms)) == _abi.PT_OK
        assert ms.value == 0.0
        assert r._lib.pt_read_tri_normals(r._ctx, e, e, e) == _abi.PT_OK
        assert not empty.any()
        same_buffer(frame(r)[0], img0)
    finally:
        r.close()
