"""pt_set_morph / pt_morph_meshes on the GPU: sparse per-corner deltas, packed by wave-sized slices, scaled by one weight
per target and added to the rest pose kept on the device, optionally skinned, then the refits of pt_update_meshes.
Every comparison is bit equality, or the project's parity bar through `check`; the reference arrays come from
tests/morph_ref.py (and tests/skin_ref.py for the composed call).

  1. words: after MorphMeshes every word on the device (triangle BVH, BLASes, analytic BVH, normals, the lights through
     ReadMaterials) is what UpdateMeshes leaves with morph_ref's arrays, normals given, "face" and "smooth", for morphs
     with and without normal deltas; ReadPose is those arrays; ReadMorph is what was set;
  2. degenerates: all-zero weights give the rest pose verbatim; the loose light triangle stays at rest although deltas
     name it; one target of weight 1 with power-of-two deltas on exactly representable positions gives p + d exactly;
  3. no drift: M1 then M2, UpdateMeshes then M2, PoseMeshes then M2 and SkinMeshes then M2 are M2 alone; a new
     SetRestPose keeps the morph, an upload drops it, a second SetMorph replaces it;
  4. composition: MorphMeshes(w, skin=mats) is UpdateMeshes(skin(morph(rest))) with 1 and 129 bones; MorphMeshes and
     UpdateShapes in both orders; RebuildMeshes() and RebuildBlas() with no arrays after a morph against the same
     rebuild given the arrays, the IntersectHits identities unchanged;
  5. pictures: renders and features after the morph equal UpdateMeshes' bit for bit on both engines, and a fresh upload
     of the morphed scene within the parity bar; the morph pushes an instanced mesh onto pixels it did not cover;
  6. the error cases leave every device word as it was.
Scenes: T, R, O and N of tests/test_gpu_blas_refit.py and L of tests/test_gpu_pose.py.  Target counts: 1, exactly the
kernel's LDS weight table (kMorphLdsTargets) and one more, so both weight paths and the boundary run.  Delta patterns:
morph_ref.seeded_morph (a target on every corner, empty targets, a single corner named by 40 targets, seeded windows,
the last corner of R's ragged last slice, and from 257 triangles on three slices with no delta).  Frames are 64x48 at
2 spp.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import features_ref as F
import morph_ref
import normals_ref
import skin_ref
import test_gpu_blas_refit as G
import test_gpu_pose as P
import test_gpu_skin as S
from parity import check, same_buffer
from ptsharp_amd import Renderer, _abi

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_TARGETS = int(re.search(r"kMorphLdsTargets = (\d+);", open(os.path.join(ROOT, "ptsharp_amd", "csrc", "pt_morph.hip")).read()).group(1))
SCENES = S.SCENES
pair, lights, same_lights = S.pair, S.lights, S.same_lights


def morphed(flat, rest, targets, weights, normals=True):
    return morph_ref.morph(rest, morph_ref.tri_group(flat), targets, weights, normals=normals)


def same_morph(got, targets, what):
    want = morph_ref.packed(targets)
    assert np.array_equal(got["target_first"], want["target_first"]), f"{what}: target_first"
    assert np.array_equal(got["corner"], want["corner"]), f"{what}: corner"
    assert np.array_equal(got["dpos"].view(np.uint32), want["dpos"].view(np.uint32)), f"{what}: dpos"
    assert (got["dnrm"] is None) == (want["dnrm"] is None), f"{what}: dnrm"
    if want["dnrm"] is not None:
        assert np.array_equal(got["dnrm"].view(np.uint32), want["dnrm"].view(np.uint32)), f"{what}: dnrm"


def padded_entries(n, targets):
    """64 per step: per slice of 64 triangles of one corner array, the deltas of its busiest corner."""
    per = np.bincount(np.concatenate([np.asarray(t[0], np.int64) for t in targets]), minlength=3 * n).reshape(n, 3)
    return 64 * sum(int(per[j:j + 64, c].max()) for c in range(3) for j in range(0, n, 64))


# ------------------------------------------------------------------ 1. words
WORDS = [("T", 1, True), ("T", LDS_TARGETS, True), ("R", LDS_TARGETS, True), ("R", LDS_TARGETS + 1, True), ("R", 50, False),
         ("O", LDS_TARGETS + 1, False), ("N", 1, False), ("N", LDS_TARGETS, True), ("L", LDS_TARGETS, False),
         ("L", LDS_TARGETS + 1, True)]


@pytest.mark.parametrize("name,nt,dnrm", WORDS, ids=[f"{a}-{b}-{'dnrm' if c else 'pos'}" for a, b, c in WORDS])
def test_words_are_update_meshes_words(gpu, name, nt, dnrm):
    sa, sb, r, r2 = pair(name)
    try:
        fa = sa[0].Compile()
        rest = P.rest_of(fa)
        n = len(rest[0])
        if name == "R":
            assert n == 3208 and n % 64 != 0      # 51 slices per corner array, the last of 8 triangles
        targets = morph_ref.seeded_morph(n, nt, 7 + nt, normal_deltas=dnrm)
        weights = morph_ref.seeded_weights(nt, nt)
        per = np.bincount(np.concatenate([t[0] for t in targets]), minlength=3 * n)
        assert per[3 * n - 1] >= 1 and (nt < 42 or per.max() >= 40) and (n <= 256 or (per[3 * 128:3 * 192] == 0).all())
        assert nt < 3 or ((weights == 0).any() and any(len(t[0]) == 0 for t in targets))
        want = morphed(fa, rest, targets, weights)
        assert (want[0].view(np.uint32) != rest[0].view(np.uint32)).any()
        assert (want[3].view(np.uint32) != rest[3].view(np.uint32)).any() == dnrm
        before = G.state(r)
        r.SetMorph(targets)
        G.same_state(G.state(r), before, f"{name} SetMorph changes nothing a ray sees", boxes_as_values=False)
        got = r.ReadMorph()
        same_morph(got, targets, f"{name} ReadMorph")
        assert got["padded"] == padded_entries(n, targets)
        # normals=None: the rest normals with the normal deltas, or the rest normals
        ms = r.MorphMeshes(weights)
        assert ms > 0
        P.same_arrays(r.ReadPose(), want, f"{name} ReadPose")
        P.same_arrays(P.rest_of(fa), want, f"{name} the FlatScene after the morph")
        r2.UpdateMeshes(*want)
        got = G.state(r)
        G.same_state(got, G.state(r2), f"{name} morphed against UpdateMeshes", boxes_as_values=False)
        P.same_normals(r, r2, name)
        same_lights(r, r2, name)
        changed = any(not np.array_equal(x, y) for part in ("blas", "tri") for x, y in zip(got[part], before[part]))
        assert changed, "the morph left every BVH word as it was"
        # the normals derived from the morphed positions
        for mode in ("face", "smooth"):
            r.MorphMeshes(weights, normals=mode)
            arrays = r.ReadPose()
            P.same_arrays(arrays[:3], want[:3], f"{name} {mode} ReadPose positions")
            r2.UpdateMeshes(*want[:3], normals=mode)
            G.same_state(G.state(r), G.state(r2), f"{name} morphed against UpdateMeshes, {mode}", boxes_as_values=False)
            if name != "L":   # (normals_ref takes disjoint mesh ranges)
                P.same_arrays(arrays[3:], normals_ref.normals(*want[:3], fa.mesh_first, fa.mesh_count, mode),
                              f"{name} {mode} ReadPose normals")
            P.same_normals(r, r2, f"{name} {mode}")
            same_lights(r, r2, f"{name} {mode}")
        same_morph(r.ReadMorph(), targets, f"{name} ReadMorph after the calls")
    finally:
        r.close()
        r2.close()


# ------------------------------------------------------------------ 2. degenerates
def test_degenerate_morphs(gpu):
    sa, sb, r, r2 = pair("L")
    try:
        fa = sa[0].Compile()
        rest = P.rest_of(fa)
        n = len(rest[0])
        loose = morph_ref.tri_group(fa) < 0
        assert loose.sum() == 1
        rest_lights = lights(r)
        targets = morph_ref.seeded_morph(n, 6, 2)
        assert np.isin(np.flatnonzero(np.repeat(loose, 3)), targets[0][0]).all()    # deltas name the loose triangle
        # all-zero weights (+0 and -0): the rest pose verbatim
        zero = np.zeros(6, f32)
        zero[1::2] = -0.0
        r.SetMorph(targets)
        r.MorphMeshes(zero)
        got = r.ReadPose()
        for k in range(6):
            assert np.array_equal(got[k].view(np.uint32), rest[k].view(np.uint32)), "all-zero weights changed the rest pose"
        r2.UpdateMeshes(*rest)
        G.same_state(G.state(r), G.state(r2), "all-zero weights against UpdateMeshes(rest)", boxes_as_values=False)
        # the loose light triangle stays at rest although deltas name it and its target is live
        r.MorphMeshes(np.ones(6, f32))
        got = r.ReadPose()
        for k in range(6):
            assert np.array_equal(got[k][loose].view(np.uint32), rest[k][loose].view(np.uint32)), "the loose triangle moved"
        assert np.array_equal(lights(r)[1].view(np.uint64), rest_lights[1].view(np.uint64))
        assert (got[0][~loose].view(np.uint32) != rest[0][~loose].view(np.uint32)).any()
        # one target, weight 1, power-of-two deltas, positions on a 2^-10 grid: p + d exactly
        grid = [np.round(a.astype(np.float64) * 1024) / 1024 for a in rest[:3]]
        exact = [g.astype(f32) for g in grid] + rest[3:]
        assert all(np.array_equal(e.astype(np.float64), g) for e, g in zip(exact, grid))
        r.SetRestPose(*exact)
        q = np.arange(3, 3 * n, 2, dtype=np.int32)                     # every other corner from triangle 1 on
        d = np.stack([np.where(q % 4 < 2, 0.25, -0.5), np.full(len(q), 2.0), np.where(q % 3 == 0, 0.0, -0.125)], axis=1).astype(f32)
        r.SetMorph([(q, d)])
        r.MorphMeshes([1.0])
        got = r.ReadPose()
        total = np.stack(grid, axis=1).reshape(3 * n, 3)
        total[q] += d.astype(np.float64)
        total = total.reshape(n, 3, 3)
        total[loose] = np.stack(grid, axis=1)[loose]
        for c in range(3):
            assert np.array_equal(total[:, c].astype(f32).astype(np.float64), total[:, c]), "p + d is not representable"
            assert np.array_equal(got[c].view(np.uint32), total[:, c].astype(f32).view(np.uint32)), f"v{c + 1} is not p + d"
        P.same_arrays(got[3:], rest[3:], "the normals of a morph without normal deltas")
    finally:
        r.close()
        r2.close()


# ------------------------------------------------------------------ 3. no drift
def test_no_drift_and_the_morph_lives_until_an_upload(gpu):
    sa, sb, r, r2 = pair("L")
    try:
        fa = sa[0].Compile()
        rest = P.rest_of(fa)
        n, nt, nb = len(rest[0]), 9, 5
        rest_lights = lights(r)
        targets = morph_ref.seeded_morph(n, nt, 3)
        m1, m2 = morph_ref.seeded_weights(nt, 1), morph_ref.seeded_weights(nt, 2)
        assert not np.array_equal(m1, m2)
        r2.SetMorph(targets)
        r2.MorphMeshes(m2)
        alone = G.state(r2)
        r.SetMorph(targets)
        r.MorphMeshes(m1)
        assert not np.array_equal(G.state(r)["tri"][2], alone["tri"][2])
        r.MorphMeshes(m2)
        G.same_state(G.state(r), alone, "M1 then M2 against M2", boxes_as_values=False)
        for _ in range(3):
            r.MorphMeshes(m2)
        G.same_state(G.state(r), alone, "M2 repeated", boxes_as_values=False)
        # an update moves everything, the loose light included; the next morph starts from the rest pose all the same
        v, kw = G.pose("sine", fa)
        r.UpdateMeshes(*v, **kw)
        assert not np.array_equal(lights(r)[1], rest_lights[1])
        r.MorphMeshes(m2)
        G.same_state(G.state(r), alone, "UpdateMeshes then M2 against M2", boxes_as_values=False)
        assert np.array_equal(lights(r)[1].view(np.uint64), rest_lights[1].view(np.uint64)), "the loose light is back at rest"
        r.PoseMeshes(P.matrices(fa))
        assert not np.array_equal(G.state(r)["tri"][2], alone["tri"][2])
        r.MorphMeshes(m2)
        G.same_state(G.state(r), alone, "PoseMeshes then M2 against M2", boxes_as_values=False)
        bones, sw = skin_ref.seeded_skin(n, nb, 3)
        r.SetSkin(bones, sw, nb)
        r.SkinMeshes(S.bone_matrices(nb, 1))
        assert not np.array_equal(G.state(r)["tri"][2], alone["tri"][2])
        r.MorphMeshes(m2)
        G.same_state(G.state(r), alone, "SkinMeshes then M2 against M2", boxes_as_values=False)
        # and the other way round: a pose overwrites the morph
        r.PoseMeshes(P.matrices(fa))
        r2.PoseMeshes(P.matrices(fa))
        G.same_state(G.state(r), G.state(r2), "M2 then a pose against the pose", boxes_as_values=False)
        # a new rest pose keeps the morph
        r.SetRestPose(*rest)
        r.MorphMeshes(m2)
        G.same_state(G.state(r), alone, "SetRestPose then M2 against M2", boxes_as_values=False)
        r2.MorphMeshes(m2)
        same_buffer(G.frame(r)[0], G.frame(r2)[0])
        # a second SetMorph replaces it: other targets, another count, no normal deltas
        other = morph_ref.seeded_morph(n, 4, 8, normal_deltas=False)
        w4 = morph_ref.seeded_weights(4, 5)
        r.SetMorph(other)
        same_morph(r.ReadMorph(), other, "the second morph")
        with pytest.raises(_abi.PTError):
            r.MorphMeshes(m2)                        # nine weights for four targets
        r.MorphMeshes(w4)
        P.same_arrays(r.ReadPose(), morphed(fa, rest, other, w4), "the second morph")
        # an upload drops it
        r.Scene = SCENES["L"]()[0]
        G.state(r)                                   # uploads
        r.SetRestPose()
        w = np.ascontiguousarray(w4)
        u = _abi.pt_mesh_morph(4, 0, 0, 0, w.ctypes.data_as(C.POINTER(C.c_float)), None)
        assert r._lib.pt_morph_meshes(r._ctx, C.byref(u), None) == _abi.PT_ERR_INVALID_ARG and b"no morph" in r._lib.pt_last_error()
        assert r._lib.pt_read_morph(r._ctx, (C.c_int64 * 3)(), None, None, None, None) == _abi.PT_ERR_INVALID_ARG
        with pytest.raises(_abi.PTError):
            r.MorphMeshes(w4)
        r.SetMorph(targets)
        r.MorphMeshes(m2)
        G.same_state(G.state(r), alone, "after the upload and a new SetMorph", boxes_as_values=False)
    finally:
        r.close()
        r2.close()


# ------------------------------------------------------------------ 4. composition
@pytest.mark.parametrize("name,nb", [("R", 1), ("T", S.LDS_BONES + 1), ("L", S.LDS_BONES + 1)], ids=["R-1", "T-129", "L-129"])
def test_morph_then_skin_in_one_call(gpu, name, nb):
    sa, sb, r, r2 = pair(name)
    try:
        fa = sa[0].Compile()
        rest = P.rest_of(fa)
        n, nt = len(rest[0]), 60
        group = morph_ref.tri_group(fa)
        bones, sw = skin_ref.seeded_skin(n, nb, 11 + nb)
        mats = S.bone_matrices(nb, nb)
        r.SetSkin(bones, sw, nb)
        for dnrm in (True, False):
            targets = morph_ref.seeded_morph(n, nt, 5, normal_deltas=dnrm)
            weights = morph_ref.seeded_weights(nt, 6)
            r.SetMorph(targets)
            mid = morphed(fa, rest, targets, weights)
            want = skin_ref.skin(mid, group, bones, sw, mats)
            alone = skin_ref.skin(rest, group, bones, sw, mats)
            assert (want[0].view(np.uint32) != alone[0].view(np.uint32)).any() and (want[0].view(np.uint32) != mid[0].view(np.uint32)).any()
            ms = r.MorphMeshes(weights, skin=mats)
            assert ms > 0
            P.same_arrays(r.ReadPose(), want, f"{name} dnrm={dnrm} ReadPose")
            r2.UpdateMeshes(*want)
            G.same_state(G.state(r), G.state(r2), f"{name} dnrm={dnrm} skin(morph(rest)) against UpdateMeshes", boxes_as_values=False)
            P.same_normals(r, r2, name)
            same_lights(r, r2, name)
            for mode in ("face", "smooth"):
                r.MorphMeshes(weights, normals=mode, skin=mats)
                P.same_arrays(r.ReadPose()[:3], want[:3], f"{name} {mode} ReadPose positions")
                r2.UpdateMeshes(*want[:3], normals=mode)
                G.same_state(G.state(r), G.state(r2), f"{name} dnrm={dnrm} {mode} against UpdateMeshes", boxes_as_values=False)
                P.same_normals(r, r2, f"{name} {mode}")
        # the skin alone and the morph alone still give their own results afterwards
        r.SkinMeshes(mats)
        P.same_arrays(r.ReadPose(), alone, f"{name} the skin alone")
        r.MorphMeshes(weights)
        P.same_arrays(r.ReadPose(), mid, f"{name} the morph alone")
    finally:
        r.close()
        r2.close()


def bulge(flat):
    """One live target (and a dead one with huge deltas) that grows scene T's instanced meshes 2.5 times and lifts
    them, p + d = 2.5 p + (0.25, 0.5, -0.25), and moves every other mesh corner a little; normal deltas on all."""
    n = len(flat.tri_material)
    inst = np.repeat(G.instanced(flat), 3)
    p = np.stack([flat.tri_v1, flat.tri_v2, flat.tri_v3], axis=1).reshape(3 * n, 3).astype(np.float64)
    d = np.where(inst[:, None], 1.5 * p + np.array([0.25, 0.5, -0.25]), 0.1 * np.sin(3.0 * p[:, ::-1])).astype(f32)
    dn = (0.2 * np.cos(2.0 * p)).astype(f32)
    q = np.arange(3 * n, dtype=np.int32)
    return [(q, d, dn), (q[::5], np.full((len(q[::5]), 3), 1e30, f32), np.full((len(q[::5]), 3), np.inf, f32))], np.array([1.0, 0.0], f32)


def test_morph_then_shapes_is_shapes_then_morph(gpu):
    sa, sb, r, r2 = pair("T")
    try:
        fa, fb = sa[0].Compile(), sb[0].Compile()
        targets, weights = bulge(fa)
        before = G.state(r)
        r.SetMorph(targets)
        r2.SetMorph(targets)
        r.MorphMeshes(weights)
        r.UpdateShapes(**G.spun(fa))      # sees the morphed meshes' inner boxes
        r2.UpdateShapes(**G.spun(fb))
        r2.MorphMeshes(weights)           # refits the shapes from the current matrices
        got = G.state(r)
        G.same_state(got, G.state(r2), "either order", boxes_as_values=False)
        assert not np.array_equal(got["shape"][0], before["shape"][0])
        same_buffer(G.frame(r)[0], G.frame(r2)[0])
    finally:
        r.close()
        r2.close()


def test_rebuilds_take_the_staged_morph(gpu):
    # the world tree, on a scene without an instance
    sa, sb, r, r2 = pair("N")
    try:
        fa = sa[0].Compile()
        rest = P.rest_of(fa)
        targets = morph_ref.seeded_morph(len(rest[0]), 12, 11)
        weights = morph_ref.seeded_weights(12, 4)
        want = morphed(fa, rest, targets, weights)
        r.SetMorph(targets)
        r.MorphMeshes(weights)
        refitted = S.hits(r, fa)
        assert (refitted["kind"] == _abi.SHAPE_TRIANGLE).sum() >= 200
        r.RebuildMeshes()
        r2.RebuildMeshes(*want)
        G.same_state(G.state(r), G.state(r2), "RebuildMeshes() after a morph against the arrays", boxes_as_values=False)
        P.same_arrays(r.ReadPose(), want, "the morph stays readable")
        S.same_hits(S.hits(r, fa), S.hits(r2, fa), "RebuildMeshes() against the arrays")
        S.same_hits(S.hits(r, fa), refitted, "the identities after RebuildMeshes()")
    finally:
        r.close()
        r2.close()
    # the BLASes and the world tree
    sa, sb, r, r2 = pair("T")
    try:
        fa = sa[0].Compile()
        rest = P.rest_of(fa)
        targets, weights = bulge(fa)
        want = morphed(fa, rest, targets, weights)
        r.SetMorph(targets)
        r.MorphMeshes(weights)
        refitted = S.hits(r, fa)
        assert (refitted["kind"] == _abi.SHAPE_TRANSFORMED).sum() >= 200
        r.RebuildBlas()
        r2.RebuildBlas(*want)
        a, b = G.state(r), G.state(r2)
        for stt in (a, b):   # lines past a BLAS's new count are left as they are: the morph's refit wrote r's, the upload r2's
            blas, nodes = stt["blas"][0], stt["blas"][1]
            for n0, nn, _, _ in blas:
                end = int(blas[blas[:, 0] > n0, 0].min()) if (blas[:, 0] > n0).any() else len(nodes)
                nodes[n0 + nn:end] = 0
        G.same_state(a, b, "RebuildBlas() after a morph against the arrays", boxes_as_values=False)
        S.same_hits(S.hits(r, fa), S.hits(r2, fa), "RebuildBlas() against the arrays")
        S.same_hits(S.hits(r, fa), refitted, "the identities after RebuildBlas()")
    finally:
        r.close()
        r2.close()


# ------------------------------------------------------------------ 5. pictures
@G.ENGINES
def test_pictures(gpu, engine):
    sa, sb, sc = G.scene_t(), G.scene_t(), G.scene_t()
    fa, fc = sa[0].Compile(), sc[0].Compile()
    rest = P.rest_of(fa)
    targets, weights = bulge(fa)
    want = morphed(fa, rest, targets, weights)
    assert all(np.isfinite(a).all() for a in want)          # the dead target's 1e30 and inf never enter
    for dst, a in zip((fc.tri_v1, fc.tri_v2, fc.tri_v3, fc.tri_n1, fc.tri_n2, fc.tri_n3), want):
        dst[...] = a                          # the morphed scene, uploaded fresh
    r, r2, fresh = G.renderer(sa, engine), G.renderer(sb, engine), G.renderer(sc, engine)
    try:
        rest_kind = F.features(sa[0], sa[1], G.W, G.H)[3].copy()
        G.frame(r)                            # a pass at the rest pose first: the morph comes between passes
        G.frame(r2)
        r.SetMorph(targets)
        r.MorphMeshes(weights)
        r2.UpdateMeshes(*want)
        # on the CPU: the grown instances cover pixels they did not cover at rest, so a no-op or a stale box shows
        kind = F.features(sa[0], sa[1], G.W, G.H)[3]
        newly = (kind == _abi.SHAPE_TRANSFORMED) & (rest_kind != _abi.SHAPE_TRANSFORMED)
        assert newly.sum() >= 20, f"the morph uncovers only {int(newly.sum())} pixels"
        g, grays = G.frame(r)
        g2, grays2 = G.frame(r2)
        assert grays == grays2
        same_buffer(g, g2)
        r.RenderFeatures()
        r2.RenderFeatures()
        for a, b, what in zip(r.Features(), r2.Features(), ("albedo", "normal", "depth", "kind", "material")):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"features after the morph: {what} differs"
        assert (r.Features()[3] == _abi.SHAPE_TRANSFORMED)[newly].all()
        f, frays = G.frame(fresh)
        check(g, grays, f, frays)
        assert (g.M.sum(axis=2) > 0).mean() > 0.5
    finally:
        r.close()
        r2.close()
        fresh.close()


# ------------------------------------------------------------------ 6. errors
def test_errors_leave_the_scene_untouched(gpu):
    st = G.scene_t()
    r = G.renderer(st)
    lp, ip, fp, dp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)
    try:
        flat = st[0].Compile()
        before = G.state(r)
        img0, _ = G.frame(r)
        rest = P.rest_of(flat)
        n, nt, nb = len(rest[0]), 7, 6
        targets = morph_ref.seeded_morph(n, nt, 5)
        weights = morph_ref.seeded_weights(nt, 9)
        pk = morph_ref.packed(targets)
        deltas = len(pk["corner"])
        D, U, two = _abi.pt_morph_desc, _abi.pt_mesh_morph, (C.c_int32 * 2)
        ms = C.c_double(-1.0)
        lib = r._lib
        mats = np.ascontiguousarray([k.m for k in S.bone_matrices(nb, 9)], np.float64).reshape(-1, 16)

        def set_morph(first=pk["target_first"], corner=pk["corner"], count=n, num_targets=nt, reserved=(0, 0), drop=None, dnrm=pk["dnrm"]):
            keep = [np.ascontiguousarray(first, np.int64), np.ascontiguousarray(corner, np.int32), pk["dpos"], dnrm]
            args = [keep[0].ctypes.data_as(lp), keep[1].ctypes.data_as(ip), keep[2].ctypes.data_as(fp),
                    None if dnrm is None else keep[3].ctypes.data_as(fp)]
            if drop is not None:
                args[drop] = None
            return lib.pt_set_morph(r._ctx, C.byref(D(count, num_targets, two(*reserved), *args)))

        def morph(count=nt, mode=0, bones=0, reserved=0, w=weights, m=None):
            w = None if w is None else np.ascontiguousarray(w, f32)
            u = U(count, mode, bones, reserved, None if w is None else w.ctypes.data_as(fp), None if m is None else m.ctypes.data_as(dp))
            return lib.pt_morph_meshes(r._ctx, C.byref(u), C.byref(ms))
        counts = (C.c_int64 * 3)(-7, -7, -7)
        read = lambda: lib.pt_read_morph(r._ctx, counts, None, None, None, None)

        def untouched(what):
            G.same_state(G.state(r), before, what, boxes_as_values=False)
            same_buffer(G.frame(r)[0], img0)

        # nothing installed yet
        assert lib.pt_set_rest_pose(r._ctx, n, *[a.ctypes.data_as(fp) for a in rest]) == _abi.PT_OK
        assert morph() == _abi.PT_ERR_INVALID_ARG and b"no morph" in lib.pt_last_error()
        assert read() == _abi.PT_ERR_INVALID_ARG and list(counts) == [-7, -7, -7]
        # refused morphs install nothing
        for bad in (n - 1, n + 1, 0):
            assert set_morph(count=bad) == _abi.PT_ERR_INVALID_ARG, bad
        for bad in (0, -1, 65536):
            assert set_morph(num_targets=bad) == _abi.PT_ERR_INVALID_ARG, bad
        assert set_morph(reserved=(0, 1)) == _abi.PT_ERR_INVALID_ARG and set_morph(reserved=(1, 0)) == _abi.PT_ERR_INVALID_ARG
        for k in range(3):
            assert set_morph(drop=k) == _abi.PT_ERR_INVALID_ARG, k
        wrong = pk["target_first"].copy()
        wrong[0] = 1
        assert set_morph(first=wrong) == _abi.PT_ERR_INVALID_ARG and b"target_first[0]" in lib.pt_last_error()
        wrong = pk["target_first"].copy()
        wrong[3] = wrong[2] - 1
        assert set_morph(first=wrong) == _abi.PT_ERR_INVALID_ARG and b"below" in lib.pt_last_error()
        for at, value in ((0, -1), (0, 3 * n), (deltas - 1, 3 * n), (deltas - 1, -2), (deltas // 2, 1 << 30)):
            wrong = pk["corner"].copy()
            wrong[at] = value
            assert set_morph(corner=wrong) == _abi.PT_ERR_INVALID_ARG, (at, value)
            assert b"outside" in lib.pt_last_error()
        wrong = pk["corner"].copy()
        wrong[1] = wrong[0]                           # a corner twice in target 0
        assert set_morph(corner=wrong) == _abi.PT_ERR_INVALID_ARG and b"not above" in lib.pt_last_error()
        assert morph() == _abi.PT_ERR_INVALID_ARG and b"no morph" in lib.pt_last_error()
        assert read() == _abi.PT_ERR_INVALID_ARG
        untouched("refused morphs")
        # installed: a later refused one keeps it
        r.SetMorph(targets)
        untouched("the morph installed")
        wrong = pk["corner"].copy()
        wrong[deltas - 1] = 3 * n
        assert set_morph(corner=wrong) == _abi.PT_ERR_INVALID_ARG
        assert read() == _abi.PT_OK and list(counts)[:2] == [nt, deltas] and counts[2] == padded_entries(n, targets)
        same_morph(r.ReadMorph(), targets, "the installed morph after a refused one")
        # refused calls launch nothing and copy nothing
        for bad in (nt - 1, nt + 1, 0):
            assert morph(count=bad) == _abi.PT_ERR_INVALID_ARG, bad
        assert morph(mode=3) == _abi.PT_ERR_INVALID_ARG and morph(mode=-1) == _abi.PT_ERR_INVALID_ARG
        assert morph(reserved=1) == _abi.PT_ERR_INVALID_ARG
        assert morph(w=None) == _abi.PT_ERR_INVALID_ARG
        assert morph(bones=nb) == _abi.PT_ERR_INVALID_ARG                       # bones without matrices
        assert morph(bones=nb, m=mats) == _abi.PT_ERR_INVALID_ARG and b"no skin" in lib.pt_last_error()
        assert lib.pt_morph_meshes(r._ctx, None, C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
        bones, sw = skin_ref.seeded_skin(n, nb, 5)
        r.SetSkin(bones, sw, nb)
        for bad in (nb - 1, nb + 1, 0):
            assert morph(bones=bad, m=mats) == _abi.PT_ERR_INVALID_ARG, bad
        assert ms.value == -1.0
        untouched("refused calls")
        # no rest pose: a second context on the same scene
        r3 = G.renderer(G.scene_t())
        try:
            G.state(r3)
            r3.SetMorph(targets)                       # a morph needs no rest pose
            w = np.ascontiguousarray(weights)
            u = U(nt, 0, 0, 0, w.ctypes.data_as(fp), None)
            assert lib.pt_morph_meshes(r3._ctx, C.byref(u), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG and b"rest pose" in lib.pt_last_error()
            assert ms.value == -1.0
            G.same_state(G.state(r3), before, "a morph before any rest pose", boxes_as_values=False)
        finally:
            r3.close()
        # and the calls themselves
        assert morph() == _abi.PT_OK and ms.value > 0
        pose = [np.zeros((n, 3), f32) for _ in range(6)]
        assert lib.pt_read_pose(r._ctx, *[a.ctypes.data_as(fp) for a in pose]) == _abi.PT_OK
        mid = morphed(flat, rest, targets, weights)
        P.same_arrays(pose, mid, "the raw morph")
        assert morph(bones=nb, m=mats) == _abi.PT_OK and ms.value > 0
        assert lib.pt_read_pose(r._ctx, *[a.ctypes.data_as(fp) for a in pose]) == _abi.PT_OK
        P.same_arrays(pose, skin_ref.skin(mid, morph_ref.tri_group(flat), bones, sw, mats), "the raw morph and skin")
    finally:
        r.close()
    r = Renderer.NewRenderer(None, None, None, G.W, G.H, True, device=0)
    try:
        first, corner, d3, w = np.array([0, 1], np.int64), np.zeros(1, np.int32), np.ones((1, 3), f32), np.ones(1, f32)
        d = _abi.pt_morph_desc(1, 1, (C.c_int32 * 2)(0, 0), first.ctypes.data_as(lp), corner.ctypes.data_as(ip), d3.ctypes.data_as(fp), None)
        u = _abi.pt_mesh_morph(1, 0, 0, 0, w.ctypes.data_as(fp), None)
        assert r._lib.pt_set_morph(r._ctx, C.byref(d)) == _abi.PT_ERR_NO_SCENE
        assert r._lib.pt_morph_meshes(r._ctx, C.byref(u), None) == _abi.PT_ERR_NO_SCENE
        assert r._lib.pt_read_morph(r._ctx, (C.c_int64 * 3)(), None, None, None, None) == _abi.PT_ERR_NO_SCENE
    finally:
        r.close()
