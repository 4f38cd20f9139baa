"""pt_pose_meshes on the GPU: the rest pose kept on the device posed by one matrix per mesh (Mesh.Transform), then the
refits of pt_update_meshes.  Every comparison is bit equality, or the project's parity bar through `check`.

  1. words: after PoseMeshes every word on the device (triangle BVH, BLASes, analytic BVH, lights, normals) is what
     UpdateMeshes leaves with the arrays Mesh.Transform's numpy arithmetic gives, normals given; ReadPose is those
     arrays; the same with the normals derived ("face", "smooth") against UpdateMeshes(normals=...);
  2. mask: a masked mesh and the loose triangles read back as the rest values verbatim, an unmasked neighbour moves;
     mirror=False leaves the FlatScene behind until ReadPose;
  3. no drift, and rest wins: pose P1 then P2 is P2 alone; UpdateMeshes(sine) then P2 is P2 alone, the loose light
     back at its rest record;
  4. pictures: renders and features after the pose equal UpdateMeshes' bit for bit on both engines, and equal a fresh
     upload of the posed scene within the parity bar; the pose moves an instance onto pixels it did not cover;
  5. PoseMeshes and UpdateShapes in both orders give the same words;
  6. the error cases leave the scene untouched; an upload drops the rest pose.
Scenes: T, R, O and N of tests/test_gpu_blas_refit.py (the 1-triangle lone-leaf mesh, a 288-triangle mesh that is both
top-level and instanced, R's 3,208 triangles: more than one block and a ragged tail, instanced-only triangles, no
instance at all) and L: a loose emissive triangle that is a light, two meshes whose ranges overlap (the last wins) and
one-triangle meshes up to exactly the kernel's LDS matrix table (kPoseLdsMeshes) and one more, so both matrix paths
and the boundary run.  Matrices per mesh, in turn: placed() (a rotation, a non-uniform scale, a translation), a far
translation, the identity.  Frames are 64x48 at 2 spp.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import features_ref as F
import normals_ref
import test_gpu_blas_refit as G
from parity import check, same_buffer
from ptsharp_amd import Renderer, Vector, _abi
from ptsharp_amd.geometry import Matrix
from ptsharp_amd.scene import Cube, DefaultSampler, Scene, Sphere, Triangle

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MESHES = int(re.search(r"kPoseLdsMeshes = (\d+);", open(os.path.join(ROOT, "ptsharp_amd", "csrc", "pt_pose.hip")).read()).group(1))


def scene_l(total):
    """`total` meshes: two 18-triangle grids, the second's range reaching back over the first's last four triangles,
    and one-triangle meshes; before them a loose emissive triangle (a light)."""
    s = Scene()
    s.Add(Cube.NewCube(Vector(-8, -1, -8), Vector(8, 0, 8), G.GREY()))
    s.Add(Sphere.NewSphere(Vector(5, 5, 2), 0.75, G.LIGHT()))
    s.Add(Triangle.NewTriangle(Vector(-1, 3, -1), Vector(1, 3, -1), Vector(0, 3.5, 1), material=G.LIGHT(30)))
    s.Add(G.grid_mesh(3, 1.5, 1.0, G.BLUE()))
    s.Add(G.grid_mesh(3, 1.5, 1.75, G.RED()))
    for i in range(total - 2):
        x, z = -3.0 + 0.25 * (i % 24), 2.0 + 0.5 * (i // 24)
        s.Add(G.one_triangle((x, 0.25, z), (x + 0.2, 0.25, z), (x + 0.1, 0.6, z + 0.1), G.GREY()))
    flat = s.Compile()
    assert len(flat.mesh_first) == total and list(flat.mesh_count[:2]) == [18, 18] and flat.mesh_first[0] == 1
    flat.mesh_first[1] -= 4
    flat.mesh_count[1] += 4
    return s, G.CAMERA(), DefaultSampler.NewSampler(4, 3)


SCENES = dict(G.SCENES, L=lambda: scene_l(LDS_MESHES), L1=lambda: scene_l(LDS_MESHES + 1))


def tri_group(flat):
    """RefitTables::tri_group: the last mesh range that contains a triangle, -1 for a loose one."""
    g = np.full(len(flat.tri_material), -1, np.int32)
    for j, (f, n) in enumerate(zip(flat.mesh_first, flat.mesh_count)):
        g[int(f):int(f) + int(n)] = j
    return g


def rest_of(flat):
    return [a.copy() for a in (flat.tri_v1, flat.tri_v2, flat.tri_v3, flat.tri_n1, flat.tri_n2, flat.tri_n3)]


FAR = Matrix.TranslateM(Vector(40000, -25000, 30000))


def matrices(flat, off=0):
    """One matrix per mesh: placed(), a far translation, the identity, in turn from `off`."""
    out = []
    for j in range(len(flat.mesh_first)):
        kind = (j + off) % 3
        if kind == 0:
            out.append(G.placed(0.4 + 0.05 * (j % 7) + off, (1.5, 0.75, 1.25), (0.3, 0.5 + 0.1 * off, -0.2)))
        else:
            out.append(FAR if kind == 1 else Matrix.Identity())
    return out


def grown(flat):
    """The instanced meshes grown 2.5 times and lifted (they come to cover new pixels), the others placed."""
    inst = set(G.blas_meshes(flat)[0])
    big = Matrix.TranslateM(Vector(0.25, 0.5, -0.25)).Mul(Matrix.ScaleM(Vector(2.5, 2.5, 2.5)))
    return [big if j in inst else G.placed(0.2, (1.0, 1.1, 1.0), (0.0, 0.3, 0.0)) for j in range(len(flat.mesh_first))]


def posed(flat, rest, mats, mask=None):
    """Mesh.Transform's numpy arithmetic on the rest arrays, mesh by mesh: the six arrays pt_pose_meshes stages."""
    out = [a.copy() for a in rest]
    g = tri_group(flat)
    with np.errstate(all="ignore"):
        for j, m in enumerate(mats):
            sel = g == j
            if (mask is not None and not mask[j]) or not sel.any():
                continue
            for k in range(3):
                out[k][sel] = m.MulPosition_arrays(np.ascontiguousarray(rest[k][sel]))
            for k in range(3, 6):
                out[k][sel] = m.MulDirection_arrays(np.ascontiguousarray(rest[k][sel]))
    return out


def same_arrays(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        normals_ref.same_bits(np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32), f"{what} array {k}")


def same_normals(r, r2, what):
    for x, y in zip(r.ReadTriNormals(), r2.ReadTriNormals()):
        normals_ref.same_bits(x, y, f"{what}: pt_read_tri_normals")


def pair(name):
    sa, sb = SCENES[name](), SCENES[name]()
    return sa, sb, G.renderer(sa), G.renderer(sb)


# ------------------------------------------------------------------ 1. words
@pytest.mark.parametrize("name", ["T", "R", "O", "N", "L", "L1"])
def test_words_are_update_meshes_words(gpu, name):
    sa, sb, r, r2 = pair(name)
    try:
        fa, fb = sa[0].Compile(), sb[0].Compile()
        rest = rest_of(fa)
        n = len(rest[0])
        assert len(fa.mesh_first) == {"L": LDS_MESHES, "L1": LDS_MESHES + 1}.get(name, len(fa.mesh_first))
        if name == "R":
            assert n == 3208 and n % 256 != 0
        before = G.state(r)
        mats = matrices(fa)
        want = posed(fa, rest, mats)
        moved = (want[0].view(np.uint32) != rest[0].view(np.uint32)).any(axis=1)
        assert moved.any()
        # normals=None: Mesh.Transform's
        ms = r.PoseMeshes(mats)
        assert ms > 0
        same_arrays(r.ReadPose(), want, f"{name} ReadPose")
        same_arrays(rest_of(fa), want, f"{name} the FlatScene after the pose")
        r2.UpdateMeshes(*want)
        got = G.state(r)
        G.same_state(got, G.state(r2), f"{name} posed against UpdateMeshes", boxes_as_values=False)
        same_normals(r, r2, name)
        changed = any(not np.array_equal(x, y) for part in ("blas", "tri") for x, y in zip(got[part], before[part]))
        assert changed, "the pose left every BVH word as it was"
        # the normals derived from the posed positions
        for mode in ("face", "smooth"):
            r.PoseMeshes(mats, normals=mode)
            pose_arrays = r.ReadPose()
            same_arrays(pose_arrays[:3], want[:3], f"{name} {mode} ReadPose positions")
            r2.UpdateMeshes(*want[:3], normals=mode)
            G.same_state(G.state(r), G.state(r2), f"{name} posed against UpdateMeshes, {mode}", boxes_as_values=False)
            if not name.startswith("L"):   # (normals_ref takes disjoint mesh ranges)
                same_arrays(pose_arrays[3:], normals_ref.normals(*want[:3], fa.mesh_first, fa.mesh_count, mode),
                            f"{name} {mode} ReadPose normals")
            same_normals(r, r2, f"{name} {mode}")
    finally:
        r.close()
        r2.close()


# ------------------------------------------------------------------ 2. mask, mirror
def test_mask_and_mirror(gpu):
    sa, sb, r, r2 = pair("L1")
    try:
        fa = sa[0].Compile()
        rest = rest_of(fa)
        g = tri_group(fa)
        mats = matrices(fa)
        mask = np.ones(len(mats), np.int32)
        mask[[1, 3, LDS_MESHES]] = 0          # the overlapping mesh, a placed one-triangle mesh, the one past the LDS table
        assert g[0] == -1 and (g[15:19] == 1).all() and (g[1:15] == 0).all()   # the last range wins
        want = posed(fa, rest, mats, mask)
        r.PoseMeshes(mats, mask=mask, mirror=False)
        same_arrays(rest_of(fa), rest, "the FlatScene before the mirror is refreshed")
        got = r.ReadPose()
        same_arrays(got, want, "masked ReadPose")
        same_arrays(rest_of(fa), want, "the FlatScene after ReadPose")
        kept = (g == -1) | np.isin(g, [1, 3, LDS_MESHES])
        assert kept.sum() == 1 + 22 + 2
        for k in range(6):
            assert np.array_equal(got[k][kept].view(np.uint32), rest[k][kept].view(np.uint32)), "a kept triangle changed"
        neighbour = g == 0                      # shares vertices with the masked mesh 1, placed
        assert not np.array_equal(got[0][neighbour], rest[0][neighbour])
        r2.UpdateMeshes(*want)
        G.same_state(G.state(r), G.state(r2), "masked pose against UpdateMeshes", boxes_as_values=False)
        # derived normals: the mask governs positions only
        r.PoseMeshes(mats, normals="face", mask=mask)
        r2.UpdateMeshes(*want[:3], normals="face")
        G.same_state(G.state(r), G.state(r2), "masked pose, face normals", boxes_as_values=False)
        same_normals(r, r2, "masked, face")
    finally:
        r.close()
        r2.close()


# ------------------------------------------------------------------ 3. no drift, and rest wins
def test_no_drift_and_rest_wins(gpu):
    sa, sb, r, r2 = pair("L")
    try:
        fa, fb = sa[0].Compile(), sb[0].Compile()
        rest_lights = G.state(r)["shape"][3].copy()
        p1, p2 = matrices(fa, 0), matrices(fa, 1)
        r2.PoseMeshes(p2)
        alone = G.state(r2)
        r.PoseMeshes(p1)
        assert not np.array_equal(G.state(r)["tri"][2], alone["tri"][2])
        r.PoseMeshes(p2)
        G.same_state(G.state(r), alone, "P1 then P2 against P2", boxes_as_values=False)
        for _ in range(3):
            r.PoseMeshes(p2)
        G.same_state(G.state(r), alone, "P2 repeated", boxes_as_values=False)
        # an update moves everything, the loose light included; the next pose starts from the rest pose all the same
        v, kw = G.pose("sine", fa)
        r.UpdateMeshes(*v, **kw)
        lights = G.state(r)["shape"][3]
        moved = (lights != rest_lights).any(axis=1)
        assert moved.sum() == 1, "the sine pose moves the loose emissive triangle's light, and only it"
        r.PoseMeshes(p2)
        after = G.state(r)
        G.same_state(after, alone, "UpdateMeshes then P2 against P2", boxes_as_values=False)
        assert np.array_equal(after["shape"][3].view(np.uint64), rest_lights.view(np.uint64)), "the loose light is back at rest"
        same_arrays(rest_of(fa), rest_of(fb), "the FlatScenes")
        same_buffer(G.frame(r)[0], G.frame(r2)[0])
    finally:
        r.close()
        r2.close()


# ------------------------------------------------------------------ 4. pictures
@G.ENGINES
def test_pictures(gpu, engine):
    sa, sb, sc = G.scene_t(), G.scene_t(), G.scene_t()
    fa, fc = sa[0].Compile(), sc[0].Compile()
    rest = rest_of(fa)
    mats = grown(fa)
    want = posed(fa, rest, mats)
    for dst, a in zip((fc.tri_v1, fc.tri_v2, fc.tri_v3, fc.tri_n1, fc.tri_n2, fc.tri_n3), want):
        dst[...] = a                          # the posed scene, uploaded fresh
    r, r2, fresh = G.renderer(sa, engine), G.renderer(sb, engine), G.renderer(sc, engine)
    try:
        rest_kind = F.features(sa[0], sa[1], G.W, G.H)[3].copy()
        G.frame(r)                            # a pass at the rest pose first: the pose comes between passes
        G.frame(r2)
        r.PoseMeshes(mats)
        r2.UpdateMeshes(*want)
        # on the CPU: the grown instances cover pixels they did not cover at rest, so a no-op or a stale box shows
        kind = F.features(sa[0], sa[1], G.W, G.H)[3]
        newly = (kind == _abi.SHAPE_TRANSFORMED) & (rest_kind != _abi.SHAPE_TRANSFORMED)
        assert newly.sum() >= 20, f"the pose uncovers only {int(newly.sum())} pixels"
        g, grays = G.frame(r)
        g2, grays2 = G.frame(r2)
        assert grays == grays2
        same_buffer(g, g2)
        r.RenderFeatures()
        r2.RenderFeatures()
        for a, b, what in zip(r.Features(), r2.Features(), ("albedo", "normal", "depth", "kind", "material")):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"features after the pose: {what} differs"
        assert (r.Features()[3] == _abi.SHAPE_TRANSFORMED)[newly].all()
        f, frays = G.frame(fresh)
        check(g, grays, f, frays)
        assert (g.M.sum(axis=2) > 0).mean() > 0.5
    finally:
        r.close()
        r2.close()
        fresh.close()


# ------------------------------------------------------------------ 5. composition
def test_pose_then_shapes_is_shapes_then_pose(gpu):
    sa, sb, r, r2 = pair("T")
    try:
        fa, fb = sa[0].Compile(), sb[0].Compile()
        mats = grown(fa)
        before = G.state(r)
        r.PoseMeshes(mats)
        r.UpdateShapes(**G.spun(fa))      # sees the posed meshes' inner boxes
        r2.UpdateShapes(**G.spun(fb))
        r2.PoseMeshes(mats)               # refits the shapes from the current matrices
        got = G.state(r)
        G.same_state(got, G.state(r2), "either order", boxes_as_values=False)
        assert not np.array_equal(got["shape"][0], before["shape"][0])
        same_buffer(G.frame(r)[0], G.frame(r2)[0])
    finally:
        r.close()
        r2.close()


# ------------------------------------------------------------------ 6. errors
def test_errors_leave_the_scene_untouched(gpu):
    st = G.scene_t()
    r = G.renderer(st)
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    try:
        flat = st[0].Compile()
        before = G.state(r)
        img0, _ = G.frame(r)
        rest = rest_of(flat)
        n, nm = len(rest[0]), len(flat.mesh_first)
        ptrs = [a.ctypes.data_as(fp) for a in rest]
        m = np.ascontiguousarray([k.m for k in grown(flat)], np.float64).reshape(-1, 16)
        U, two = _abi.pt_mesh_pose, (C.c_int32 * 2)
        ms = C.c_double(-1.0)
        lib = r._lib
        pose = lambda count, mode=0: lib.pt_pose_meshes(r._ctx, C.byref(U(count, mode, two(0, 0), m.ctypes.data_as(dp))), C.byref(ms))
        out = [np.zeros((n, 3), f32) for _ in range(6)]
        read = lambda: lib.pt_read_pose(r._ctx, *[a.ctypes.data_as(fp) for a in out])

        def untouched(what):
            G.same_state(G.state(r), before, what, boxes_as_values=False)
            same_buffer(G.frame(r)[0], img0)

        assert pose(nm) == _abi.PT_ERR_INVALID_ARG and b"rest pose" in lib.pt_last_error()
        untouched("a pose before any rest pose")
        assert read() == _abi.PT_ERR_INVALID_ARG
        for bad in (n - 1, n + 1, 0):
            assert lib.pt_set_rest_pose(r._ctx, bad, *ptrs) == _abi.PT_ERR_INVALID_ARG, bad
        assert pose(nm) == _abi.PT_ERR_INVALID_ARG   # a refused rest pose installed nothing
        assert lib.pt_set_rest_pose(r._ctx, n, *ptrs) == _abi.PT_OK
        untouched("the rest pose installed")
        assert read() == _abi.PT_ERR_INVALID_ARG     # a rest pose is not a pose
        for bad in (nm - 1, nm + 1, 0):
            assert pose(bad) == _abi.PT_ERR_INVALID_ARG, bad
        assert pose(nm, 3) == _abi.PT_ERR_INVALID_ARG
        assert ms.value == -1.0
        untouched("refused poses")
        assert all((a == 0).all() for a in out)
        assert pose(nm) == _abi.PT_OK and ms.value > 0 and read() == _abi.PT_OK
        same_arrays(out, posed(flat, rest, grown(flat)), "the raw pose")
        # an upload drops the rest pose
        r.Scene = G.scene_t()[0]
        G.state(r)                                   # uploads
        assert pose(nm) == _abi.PT_ERR_INVALID_ARG and b"rest pose" in lib.pt_last_error()
        assert read() == _abi.PT_ERR_INVALID_ARG
        G.same_state(G.state(r), before, "after the upload", boxes_as_values=False)
    finally:
        r.close()
    r = Renderer.NewRenderer(None, None, None, G.W, G.H, True, device=0)
    try:
        z = np.zeros((1, 3), f32).ctypes.data_as(fp)
        eye = np.eye(4).reshape(-1)
        u = _abi.pt_mesh_pose(1, 0, (C.c_int32 * 2)(0, 0), eye.ctypes.data_as(dp))
        assert r._lib.pt_pose_meshes(r._ctx, C.byref(u), None) == _abi.PT_ERR_NO_SCENE
        assert r._lib.pt_set_rest_pose(r._ctx, 1, z, z, z, z, z, z) == _abi.PT_ERR_NO_SCENE
        assert r._lib.pt_read_pose(r._ctx, z, z, z, z, z, z) == _abi.PT_ERR_NO_SCENE
    finally:
        r.close()
