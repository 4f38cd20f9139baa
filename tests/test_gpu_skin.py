"""pt_set_skin / pt_skin_meshes on the GPU: the rest pose kept on the device blended by four (bone, weight) influences
per corner and one matrix per bone, then the refits of pt_update_meshes.  Every comparison is bit equality, or the
project's parity bar through `check`; the reference arrays come from tests/skin_ref.py.

  1. words: after SkinMeshes every word on the device (triangle BVH, BLASes, analytic BVH, normals, the lights through
     ReadMaterials) is what UpdateMeshes leaves with skin_ref's arrays, normals given, "face" and "smooth"; ReadPose is
     those arrays; ReadSkin is what was set;
  2. degenerate skins: one bone per mesh with weight 1 gives PoseMeshes' words; all-zero weights give the rest pose
     verbatim; the loose light triangle stays at rest although its weights are not zero;
  3. no drift: S1 then S2, UpdateMeshes then S2 and PoseMeshes then S2 are S2 alone; a new SetRestPose keeps the skin, an
     upload drops it until SetSkin is called again;
  4. pictures: renders and features after the skin equal UpdateMeshes' bit for bit on both engines, and a fresh upload
     of the skinned scene within the parity bar; the skin bends an instanced mesh onto pixels it did not cover;
  5. composition: SkinMeshes and UpdateShapes in both orders; RebuildMeshes() and RebuildBlas() with no arrays after a
     skin against the same rebuild given skin_ref's arrays, the IntersectHits identities unchanged;
  6. the error cases leave the scene untouched.
Scenes: T, R, O and N of tests/test_gpu_blas_refit.py and L of tests/test_gpu_pose.py (the 1-triangle lone-leaf mesh, a
mesh both top-level and instanced, R's 3,208 triangles: more than one block and a ragged tail, instanced-only
triangles, no instance at all, a loose emissive light triangle, overlapping mesh ranges).  Bone counts: 1, exactly the
kernel's LDS matrix table (kSkinLdsBones) and one more, so both matrix paths and the boundary run.  Weights:
skin_ref.seeded_skin (1 to 4 live influences, some corners all zero, some a single 1).  Frames are 64x48 at 2 spp.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import features_ref as F
import normals_ref
import skin_ref
import test_gpu_blas_refit as G
import test_gpu_pose as P
from parity import check, same_buffer
from ptsharp_amd import Renderer, Vector, _abi
from ptsharp_amd.geometry import Matrix

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_BONES = int(re.search(r"kSkinLdsBones = (\d+);", open(os.path.join(ROOT, "ptsharp_amd", "csrc", "pt_skin.hip")).read()).group(1))
SCENES = dict(G.SCENES, L=lambda: P.scene_l(4))


def bone_matrices(count, seed):
    """`count` matrices near the identity: a rotation, a non-uniform scale and a translation each, seeded."""
    rng = np.random.default_rng(seed)
    return [G.placed(float(rng.uniform(-0.6, 0.6)), tuple(rng.uniform(0.8, 1.3, 3)), tuple(rng.uniform(-0.4, 0.4, 3)))
            for _ in range(count)]


def skinned(flat, rest, bones, weights, mats, normals=True):
    return skin_ref.skin(rest, skin_ref.tri_group(flat), bones, weights, mats, normals=normals)


def lights(r):
    m = r.ReadMaterials()
    return m["light_rows"].copy(), m["light_spheres"].copy()


def same_lights(r, r2, what):
    (ra, sa), (rb, sb) = lights(r), lights(r2)
    assert np.array_equal(ra, rb) and np.array_equal(sa.view(np.uint64), sb.view(np.uint64)), f"{what}: the lights differ"


def pair(name):
    sa, sb = SCENES[name](), SCENES[name]()
    return sa, sb, G.renderer(sa), G.renderer(sb)


# ------------------------------------------------------------------ 1. words
WORDS = [("T", 1), ("T", LDS_BONES), ("R", LDS_BONES), ("R", LDS_BONES + 1), ("O", LDS_BONES + 1), ("N", 1), ("N", LDS_BONES),
         ("L", LDS_BONES), ("L", LDS_BONES + 1)]


@pytest.mark.parametrize("name,nb", WORDS, ids=[f"{a}-{b}" for a, b in WORDS])
def test_words_are_update_meshes_words(gpu, name, nb):
    sa, sb, r, r2 = pair(name)
    try:
        fa = sa[0].Compile()
        rest = P.rest_of(fa)
        n = len(rest[0])
        if name == "R":
            assert n == 3208 and n % 256 != 0
        bones, weights = skin_ref.seeded_skin(n, nb, 7 + nb)
        live = (weights != 0).sum(axis=-1)
        assert (live == 0).any() and ((live == 1) & (weights == 1).any(axis=-1)).any() and (n < 8 or live.max() == 4)
        mats = bone_matrices(nb, nb)
        want = skinned(fa, rest, bones, weights, mats)
        assert (want[0].view(np.uint32) != rest[0].view(np.uint32)).any()
        before = G.state(r)
        r.SetSkin(bones, weights, nb)
        G.same_state(G.state(r), before, f"{name} SetSkin changes nothing a ray sees", boxes_as_values=False)
        got_b, got_w = r.ReadSkin()
        assert np.array_equal(got_b, bones) and np.array_equal(got_w.view(np.uint32), weights.view(np.uint32))
        # normals=None: the blended rest normals
        ms = r.SkinMeshes(mats)
        assert ms > 0
        P.same_arrays(r.ReadPose(), want, f"{name} ReadPose")
        P.same_arrays(P.rest_of(fa), want, f"{name} the FlatScene after the skin")
        r2.UpdateMeshes(*want)
        got = G.state(r)
        G.same_state(got, G.state(r2), f"{name} skinned against UpdateMeshes", boxes_as_values=False)
        P.same_normals(r, r2, name)
        same_lights(r, r2, name)
        changed = any(not np.array_equal(x, y) for part in ("blas", "tri") for x, y in zip(got[part], before[part]))
        assert changed, "the skin left every BVH word as it was"
        # the normals derived from the skinned positions
        for mode in ("face", "smooth"):
            r.SkinMeshes(mats, normals=mode)
            arrays = r.ReadPose()
            P.same_arrays(arrays[:3], want[:3], f"{name} {mode} ReadPose positions")
            r2.UpdateMeshes(*want[:3], normals=mode)
            G.same_state(G.state(r), G.state(r2), f"{name} skinned against UpdateMeshes, {mode}", boxes_as_values=False)
            if name != "L":   # (normals_ref takes disjoint mesh ranges)
                P.same_arrays(arrays[3:], normals_ref.normals(*want[:3], fa.mesh_first, fa.mesh_count, mode),
                              f"{name} {mode} ReadPose normals")
            P.same_normals(r, r2, f"{name} {mode}")
            same_lights(r, r2, f"{name} {mode}")
        got_b, got_w = r.ReadSkin()
        assert np.array_equal(got_b, bones) and np.array_equal(got_w.view(np.uint32), weights.view(np.uint32))
    finally:
        r.close()
        r2.close()


# ------------------------------------------------------------------ 2. degenerate skins
def test_degenerate_skins(gpu):
    sa, sb, r, r2 = pair("L")
    try:
        fa = sa[0].Compile()
        rest = P.rest_of(fa)
        n, nm = len(rest[0]), len(fa.mesh_first)
        g = skin_ref.tri_group(fa)
        loose = g < 0
        assert loose.sum() == 1 and nm == 4
        rest_lights = lights(r)
        # one bone per mesh, weight 1 (in a different slot per corner): PoseMeshes with the same matrices
        mats = P.matrices(fa)
        bones = np.zeros((n, 3, 4), np.int32)
        weights = np.zeros((n, 3, 4), f32)
        for c in range(3):
            bones[:, c, c + 1] = np.maximum(g, 0)
            weights[:, c, c + 1] = 1.0
        assert (weights[loose] != 0).any()
        r.SetSkin(bones, weights, nm)
        r.SkinMeshes(mats)
        r2.PoseMeshes(mats)
        G.same_state(G.state(r), G.state(r2), "one bone per mesh against PoseMeshes", boxes_as_values=False)
        got = r.ReadPose()
        P.same_arrays(got, r2.ReadPose(), "one bone per mesh: ReadPose")
        P.same_arrays(got, P.posed(fa, rest, mats), "one bone per mesh: Mesh.Transform")
        P.same_normals(r, r2, "one bone per mesh")   # (reuses the staged arrays: the pose is read before)
        same_lights(r, r2, "one bone per mesh")
        # the loose light triangle stays at rest although its weights are not zero
        for k in range(6):
            assert np.array_equal(got[k][loose].view(np.uint32), rest[k][loose].view(np.uint32)), "the loose triangle moved"
        assert np.array_equal(lights(r)[1].view(np.uint64), rest_lights[1].view(np.uint64))
        assert not np.array_equal(got[0][~loose], rest[0][~loose])
        # all-zero weights (+0 and -0): the rest pose verbatim
        zero = np.zeros((n, 3, 4), f32)
        zero[:, :, 1::2] = -0.0
        r.SetSkin(bones, zero, nm)
        r.SkinMeshes(mats)
        got = r.ReadPose()
        for k in range(6):
            assert np.array_equal(got[k].view(np.uint32), rest[k].view(np.uint32)), "all-zero weights changed the rest pose"
        r2.UpdateMeshes(*rest)
        G.same_state(G.state(r), G.state(r2), "all-zero weights against UpdateMeshes(rest)", boxes_as_values=False)
    finally:
        r.close()
        r2.close()


# ------------------------------------------------------------------ 3. no drift
def test_no_drift_and_the_skin_lives_until_an_upload(gpu):
    sa, sb, r, r2 = pair("L")
    try:
        fa = sa[0].Compile()
        rest = P.rest_of(fa)
        n, nb = len(rest[0]), 5
        rest_lights = lights(r)
        bones, weights = skin_ref.seeded_skin(n, nb, 3)
        s1, s2 = bone_matrices(nb, 1), bone_matrices(nb, 2)
        r2.SetSkin(bones, weights, nb)
        r2.SkinMeshes(s2)
        alone = G.state(r2)
        r.SetSkin(bones, weights, nb)
        r.SkinMeshes(s1)
        assert not np.array_equal(G.state(r)["tri"][2], alone["tri"][2])
        r.SkinMeshes(s2)
        G.same_state(G.state(r), alone, "S1 then S2 against S2", boxes_as_values=False)
        for _ in range(3):
            r.SkinMeshes(s2)
        G.same_state(G.state(r), alone, "S2 repeated", boxes_as_values=False)
        # an update moves everything, the loose light included; the next skin starts from the rest pose all the same
        v, kw = G.pose("sine", fa)
        r.UpdateMeshes(*v, **kw)
        assert not np.array_equal(lights(r)[1], rest_lights[1])
        r.SkinMeshes(s2)
        G.same_state(G.state(r), alone, "UpdateMeshes then S2 against S2", boxes_as_values=False)
        assert np.array_equal(lights(r)[1].view(np.uint64), rest_lights[1].view(np.uint64)), "the loose light is back at rest"
        r.PoseMeshes(P.matrices(fa))
        assert not np.array_equal(G.state(r)["tri"][2], alone["tri"][2])
        r.SkinMeshes(s2)
        G.same_state(G.state(r), alone, "PoseMeshes then S2 against S2", boxes_as_values=False)
        # and the other way round: a pose overwrites the skin
        r.PoseMeshes(P.matrices(fa))
        r2.PoseMeshes(P.matrices(fa))
        G.same_state(G.state(r), G.state(r2), "S2 then a pose against the pose", boxes_as_values=False)
        # a new rest pose keeps the skin
        r.SetRestPose(*rest)
        r.SkinMeshes(s2)
        G.same_state(G.state(r), alone, "SetRestPose then S2 against S2", boxes_as_values=False)
        r2.SkinMeshes(s2)
        same_buffer(G.frame(r)[0], G.frame(r2)[0])
        # an upload drops it
        r.Scene = SCENES["L"]()[0]
        G.state(r)                                   # uploads
        r.SetRestPose()
        m = np.ascontiguousarray([k.m for k in s2], np.float64).reshape(-1, 16)
        u = _abi.pt_mesh_skin(nb, 0, (C.c_int32 * 2)(0, 0), m.ctypes.data_as(C.POINTER(C.c_double)))
        assert r._lib.pt_skin_meshes(r._ctx, C.byref(u), None) == _abi.PT_ERR_INVALID_ARG and b"no skin" in r._lib.pt_last_error()
        z = np.zeros((n, 4), np.int32).ctypes.data_as(C.POINTER(C.c_int32))
        assert r._lib.pt_read_skin(r._ctx, z, None, None, None, None, None) == _abi.PT_ERR_INVALID_ARG
        with pytest.raises(_abi.PTError):
            r.SkinMeshes(s2)
        r.SetSkin(bones, weights, nb)
        r.SkinMeshes(s2)
        G.same_state(G.state(r), alone, "after the upload and a new SetSkin", boxes_as_values=False)
    finally:
        r.close()
        r2.close()


# ------------------------------------------------------------------ 4. pictures
def bend(flat):
    """Two bones and a skin that bends scene T's instanced meshes: the corners blend a gentle placement with one grown
    2.5 times and lifted, by their height and depth in the mesh; the other triangles follow the gentle bone alone."""
    mats = [G.placed(0.2, (1.0, 1.1, 1.0), (0.0, 0.3, 0.0)),
            Matrix.TranslateM(Vector(0.25, 0.5, -0.25)).Mul(Matrix.ScaleM(Vector(2.5, 2.5, 2.5)))]
    n = len(flat.tri_material)
    inst = G.instanced(flat)
    bones = np.zeros((n, 3, 4), np.int32)
    bones[:, :, 2] = 1
    weights = np.zeros((n, 3, 4), f32)
    for c, v in enumerate((flat.tri_v1, flat.tri_v2, flat.tri_v3)):
        t = np.clip(0.75 + 0.25 * np.sin(3.0 * v[:, 2].astype(np.float64)), 0.5, 1.0).astype(f32)
        weights[:, c, 2] = np.where(inst, t, f32(0))
        weights[:, c, 0] = np.where(inst, f32(1) - t, f32(1))
    return mats, bones, weights


@G.ENGINES
def test_pictures(gpu, engine):
    sa, sb, sc = G.scene_t(), G.scene_t(), G.scene_t()
    fa, fc = sa[0].Compile(), sc[0].Compile()
    rest = P.rest_of(fa)
    mats, bones, weights = bend(fa)
    want = skinned(fa, rest, bones, weights, mats)
    for dst, a in zip((fc.tri_v1, fc.tri_v2, fc.tri_v3, fc.tri_n1, fc.tri_n2, fc.tri_n3), want):
        dst[...] = a                          # the skinned scene, uploaded fresh
    r, r2, fresh = G.renderer(sa, engine), G.renderer(sb, engine), G.renderer(sc, engine)
    try:
        rest_kind = F.features(sa[0], sa[1], G.W, G.H)[3].copy()
        G.frame(r)                            # a pass at the rest pose first: the skin comes between passes
        G.frame(r2)
        r.SetSkin(bones, weights, len(mats))
        r.SkinMeshes(mats)
        r2.UpdateMeshes(*want)
        # on the CPU: the bent instances cover pixels they did not cover at rest, so a no-op or a stale box shows
        kind = F.features(sa[0], sa[1], G.W, G.H)[3]
        newly = (kind == _abi.SHAPE_TRANSFORMED) & (rest_kind != _abi.SHAPE_TRANSFORMED)
        assert newly.sum() >= 20, f"the skin uncovers only {int(newly.sum())} pixels"
        g, grays = G.frame(r)
        g2, grays2 = G.frame(r2)
        assert grays == grays2
        same_buffer(g, g2)
        r.RenderFeatures()
        r2.RenderFeatures()
        for a, b, what in zip(r.Features(), r2.Features(), ("albedo", "normal", "depth", "kind", "material")):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"features after the skin: {what} differs"
        assert (r.Features()[3] == _abi.SHAPE_TRANSFORMED)[newly].all()
        f, frays = G.frame(fresh)
        check(g, grays, f, frays)
        assert (g.M.sum(axis=2) > 0).mean() > 0.5
    finally:
        r.close()
        r2.close()
        fresh.close()


# ------------------------------------------------------------------ 5. composition
def test_skin_then_shapes_is_shapes_then_skin(gpu):
    sa, sb, r, r2 = pair("T")
    try:
        fa, fb = sa[0].Compile(), sb[0].Compile()
        mats, bones, weights = bend(fa)
        before = G.state(r)
        r.SetSkin(bones, weights, len(mats))
        r2.SetSkin(bones, weights, len(mats))
        r.SkinMeshes(mats)
        r.UpdateShapes(**G.spun(fa))      # sees the skinned meshes' inner boxes
        r2.UpdateShapes(**G.spun(fb))
        r2.SkinMeshes(mats)               # refits the shapes from the current matrices
        got = G.state(r)
        G.same_state(got, G.state(r2), "either order", boxes_as_values=False)
        assert not np.array_equal(got["shape"][0], before["shape"][0])
        same_buffer(G.frame(r)[0], G.frame(r2)[0])
    finally:
        r.close()
        r2.close()


def hits(r, flat):
    o, d = G.rays_at(*G.moved_box(flat), 2048, 5) if G.instanced(flat).any() else G.rays_at(np.array([-2, 0, -2.0]), np.array([2, 1.5, 2.0]), 2048, 5)
    return r.IntersectHits(o, d, want={"t", "kind", "index", "prim", "shape"})


def same_hits(a, b, what):
    assert np.array_equal(a["t"].view(np.int64), b["t"].view(np.int64)), f"{what}: t"
    for key in ("kind", "index", "prim", "shape"):
        assert np.array_equal(a[key], b[key]), f"{what}: {key}"


def test_rebuilds_take_the_staged_skin(gpu):
    # the world tree, on a scene without an instance
    sa, sb, r, r2 = pair("N")
    try:
        fa = sa[0].Compile()
        rest = P.rest_of(fa)
        bones, weights = skin_ref.seeded_skin(len(rest[0]), 3, 11)
        mats = bone_matrices(3, 4)
        want = skinned(fa, rest, bones, weights, mats)
        r.SetSkin(bones, weights, 3)
        r.SkinMeshes(mats)
        refitted = hits(r, fa)
        assert (refitted["kind"] == _abi.SHAPE_TRIANGLE).sum() >= 200
        r.RebuildMeshes()
        r2.RebuildMeshes(*want)
        G.same_state(G.state(r), G.state(r2), "RebuildMeshes() after a skin against the arrays", boxes_as_values=False)
        P.same_arrays(r.ReadPose(), want, "the skin stays readable")
        same_hits(hits(r, fa), hits(r2, fa), "RebuildMeshes() against the arrays")
        same_hits(hits(r, fa), refitted, "the identities after RebuildMeshes()")
    finally:
        r.close()
        r2.close()
    # the BLASes and the world tree
    sa, sb, r, r2 = pair("T")
    try:
        fa = sa[0].Compile()
        rest = P.rest_of(fa)
        mats, bones, weights = bend(fa)
        want = skinned(fa, rest, bones, weights, mats)
        r.SetSkin(bones, weights, len(mats))
        r.SkinMeshes(mats)
        refitted = hits(r, fa)
        assert (refitted["kind"] == _abi.SHAPE_TRANSFORMED).sum() >= 200
        r.RebuildBlas()
        r2.RebuildBlas(*want)
        a, b = G.state(r), G.state(r2)
        for stt in (a, b):   # lines past a BLAS's new count are left as they are: the skin's refit wrote r's, the upload r2's
            blas, nodes = stt["blas"][0], stt["blas"][1]
            for n0, nn, _, _ in blas:
                end = int(blas[blas[:, 0] > n0, 0].min()) if (blas[:, 0] > n0).any() else len(nodes)
                nodes[n0 + nn:end] = 0
        G.same_state(a, b, "RebuildBlas() after a skin against the arrays", boxes_as_values=False)
        same_hits(hits(r, fa), hits(r2, fa), "RebuildBlas() against the arrays")
        same_hits(hits(r, fa), refitted, "the identities after RebuildBlas()")
    finally:
        r.close()
        r2.close()


# ------------------------------------------------------------------ 6. errors
def test_errors_leave_the_scene_untouched(gpu):
    st = G.scene_t()
    r = G.renderer(st)
    ip, fp, dp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)
    try:
        flat = st[0].Compile()
        before = G.state(r)
        img0, _ = G.frame(r)
        rest = P.rest_of(flat)
        n, nb = len(rest[0]), 6
        bones, weights = skin_ref.seeded_skin(n, nb, 5)
        mats = bone_matrices(nb, 9)
        m = np.ascontiguousarray([k.m for k in mats], np.float64).reshape(-1, 16)
        D, U, two = _abi.pt_skin_desc, _abi.pt_mesh_skin, (C.c_int32 * 2)
        ms = C.c_double(-1.0)
        lib = r._lib

        def set_skin(b, w=weights, count=n, num_bones=nb, reserved=(0, 0), drop=None):
            b = [np.ascontiguousarray(b[:, k]) for k in range(3)]
            w = [np.ascontiguousarray(w[:, k]) for k in range(3)]
            args = [x.ctypes.data_as(ip) for x in b] + [x.ctypes.data_as(fp) for x in w]
            if drop is not None:
                args[drop] = None
            return lib.pt_set_skin(r._ctx, C.byref(D(count, num_bones, two(*reserved), *args)))
        skin = lambda count, mode=0: lib.pt_skin_meshes(r._ctx, C.byref(U(count, mode, two(0, 0), m.ctypes.data_as(dp))), C.byref(ms))
        out_b = [np.full((n, 4), -7, np.int32) for _ in range(3)]
        out_w = [np.full((n, 4), -7, f32) for _ in range(3)]
        read = lambda: lib.pt_read_skin(r._ctx, *[a.ctypes.data_as(ip) for a in out_b], *[a.ctypes.data_as(fp) for a in out_w])

        def untouched(what):
            G.same_state(G.state(r), before, what, boxes_as_values=False)
            same_buffer(G.frame(r)[0], img0)

        # nothing installed yet
        assert lib.pt_set_rest_pose(r._ctx, n, *[a.ctypes.data_as(fp) for a in rest]) == _abi.PT_OK
        assert skin(nb) == _abi.PT_ERR_INVALID_ARG and b"no skin" in lib.pt_last_error()
        assert read() == _abi.PT_ERR_INVALID_ARG
        # refused skins install nothing
        for bad in (n - 1, n + 1, 0):
            assert set_skin(bones, count=bad) == _abi.PT_ERR_INVALID_ARG, bad
        for bad in (0, -1, 65537):
            assert set_skin(bones, num_bones=bad) == _abi.PT_ERR_INVALID_ARG, bad
        assert set_skin(bones, reserved=(0, 1)) == _abi.PT_ERR_INVALID_ARG
        for k in range(6):
            assert set_skin(bones, drop=k) == _abi.PT_ERR_INVALID_ARG, k
        for at, value in (((0, 0, 0), nb), ((0, 0, 0), -1), ((n - 1, 2, 3), nb), ((n - 1, 2, 3), 1 << 16), ((n // 2, 1, 2), nb)):
            wrong = bones.copy()
            wrong[at] = value
            zero_there = weights.copy()
            zero_there[at] = 0.0                   # checked whatever its weight
            assert set_skin(wrong, zero_there) == _abi.PT_ERR_INVALID_ARG, (at, value)
            assert b"outside" in lib.pt_last_error()
        assert skin(nb) == _abi.PT_ERR_INVALID_ARG and b"no skin" in lib.pt_last_error()
        assert read() == _abi.PT_ERR_INVALID_ARG
        untouched("refused skins")
        # installed: a later refused one keeps it
        assert set_skin(bones) == _abi.PT_OK
        untouched("the skin installed")
        wrong = bones.copy()
        wrong[n - 1, 2, 3] = nb
        assert set_skin(wrong) == _abi.PT_ERR_INVALID_ARG
        assert read() == _abi.PT_OK
        assert np.array_equal(np.stack(out_b, axis=1), bones)
        assert np.array_equal(np.stack(out_w, axis=1).view(np.uint32), weights.view(np.uint32))
        # refused calls launch nothing
        for bad in (nb - 1, nb + 1, 0):
            assert skin(bad) == _abi.PT_ERR_INVALID_ARG, bad
        assert skin(nb, 3) == _abi.PT_ERR_INVALID_ARG and skin(nb, -1) == _abi.PT_ERR_INVALID_ARG
        assert lib.pt_skin_meshes(r._ctx, C.byref(U(nb, 0, two(1, 0), m.ctypes.data_as(dp))), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
        assert lib.pt_skin_meshes(r._ctx, C.byref(U(nb, 0, two(0, 0), None)), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
        assert lib.pt_skin_meshes(r._ctx, None, C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
        assert ms.value == -1.0
        untouched("refused calls")
        # no rest pose: a second context on the same scene
        r3 = G.renderer(G.scene_t())
        try:
            G.state(r3)
            b3 = [np.ascontiguousarray(bones[:, k]) for k in range(3)]
            w3 = [np.ascontiguousarray(weights[:, k]) for k in range(3)]
            d = D(n, nb, two(0, 0), *[x.ctypes.data_as(ip) for x in b3], *[x.ctypes.data_as(fp) for x in w3])
            assert lib.pt_set_skin(r3._ctx, C.byref(d)) == _abi.PT_OK     # a skin needs no rest pose
            u = U(nb, 0, two(0, 0), m.ctypes.data_as(dp))
            assert lib.pt_skin_meshes(r3._ctx, C.byref(u), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG and b"rest pose" in lib.pt_last_error()
            assert ms.value == -1.0
            G.same_state(G.state(r3), before, "a skin before any rest pose", boxes_as_values=False)
        finally:
            r3.close()
        # and the call itself
        assert skin(nb) == _abi.PT_OK and ms.value > 0
        pose = [np.zeros((n, 3), f32) for _ in range(6)]
        assert lib.pt_read_pose(r._ctx, *[a.ctypes.data_as(fp) for a in pose]) == _abi.PT_OK
        P.same_arrays(pose, skinned(flat, rest, bones, weights, mats), "the raw skin")
        # more bones than the workspace was made for: it grows, and the old skin is replaced
        nb2 = LDS_BONES + 40
        bones2, weights2 = skin_ref.seeded_skin(n, nb2, 6)
        mats2 = bone_matrices(nb2, 10)
        assert set_skin(bones2, weights2, num_bones=nb2) == _abi.PT_OK
        assert skin(nb) == _abi.PT_ERR_INVALID_ARG
        m = np.ascontiguousarray([k.m for k in mats2], np.float64).reshape(-1, 16)
        assert skin(nb2) == _abi.PT_OK
        assert lib.pt_read_pose(r._ctx, *[a.ctypes.data_as(fp) for a in pose]) == _abi.PT_OK
        P.same_arrays(pose, skinned(flat, rest, bones2, weights2, mats2), "the larger skin")
    finally:
        r.close()
    r = Renderer.NewRenderer(None, None, None, G.W, G.H, True, device=0)
    try:
        zi, zf = np.zeros((1, 4), np.int32).ctypes.data_as(ip), np.ones((1, 4), f32).ctypes.data_as(fp)
        eye = np.eye(4).reshape(-1)
        d = _abi.pt_skin_desc(1, 1, (C.c_int32 * 2)(0, 0), zi, zi, zi, zf, zf, zf)
        u = _abi.pt_mesh_skin(1, 0, (C.c_int32 * 2)(0, 0), eye.ctypes.data_as(dp))
        assert r._lib.pt_set_skin(r._ctx, C.byref(d)) == _abi.PT_ERR_NO_SCENE
        assert r._lib.pt_skin_meshes(r._ctx, C.byref(u), None) == _abi.PT_ERR_NO_SCENE
        assert r._lib.pt_read_skin(r._ctx, zi, zi, zi, zf, zf, zf) == _abi.PT_ERR_NO_SCENE
    finally:
        r.close()
