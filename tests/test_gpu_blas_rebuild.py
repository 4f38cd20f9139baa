"""pt_rebuild_blas and pt_blas_cost on the GPU: every instanced mesh's BLAS re-sorted on the device into the balanced
tree of pt_blas_rebuild.h, then refitted.

  1. words: after RebuildBlas, ReadBlas() equals tests/blas_rebuild_ref.py (checked on the CPU against the native check)
     for BLASes of 1 .. 6,400 triangles, two per scene, at four poses, normals kept, given, FACE and SMOOTH; with the
     default LDS tail, with PT_BLAS_TAIL=64 and with PT_BLAS_TAIL=0 (every round a device sort), all three identical;
  2. rays: pt_intersect / pt_occluded / pt_intersect_hits after a rebuild against a context that uploaded the deformed
     scene fresh, degenerate_rays.py's families at an instance among them;
     a textured instance, whose blas_uv rows must move with their triangles;
  3. renders and features on both engines against the oracle and the fresh upload;
  4. what: PT_REBUILD_WORLD on a scene without instanced mesh is RebuildMeshes word for word; PT_REBUILD_BLAS leaves the
     world triangle BVH as UpdateMeshes leaves it;
  5. sequences: a rebuild then UpdateMeshes (the reference's refit of the rebuilt topology), a rebuild from the staged
     pose against one from its arrays, UpdateShapes before and after, upload / rebuild / upload;
  6. cost: BlasCost() against the numpy value, and the CPU check's gates on the device's numbers;
  7. the error cases leave the scene untouched; RebuildMeshes still refuses an instanced scene.
The fallback (a BLAS whose balanced tree needs more nodes than the upload gave it) is not tested here: the native
check's table of such n is empty, no upload produces one.  Frames are 64x48 at 2 spp."""
import ctypes as C
import os

import numpy as np
import pytest

import blas_rebuild_ref as RB
import blas_refit_ref as B
import degenerate_rays as D
import features_ref as F
import normals_ref
import oracle_lib as O
import test_gpu_blas_refit as TB
from parity import check, same_buffer, within
from ptsharp_amd import TransformedShape, Vector, _abi, scenes
from ptsharp_amd.geometry import Matrix
from ptsharp_amd.scene import Cube, DefaultSampler, Scene, Sphere

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = TB.W, TB.H
PAIRS = ((1, 288), (4, 5), (16, 17), (64, 65), (288, 65), (1025, 17), (4097, 5), (6400, 64))
POSES = ("rest", "sine", "twist", "offset")
NORMALS = ("kept", "given", "face", "smooth")
TAILS = (None, "64", "0")


class tail:
    """PT_BLAS_TAIL for the calls inside (the library reads it at each call)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.pop("PT_BLAS_TAIL", None)
        if self.value is not None:
            os.environ["PT_BLAS_TAIL"] = self.value

    def __exit__(self, *exc):
        os.environ.pop("PT_BLAS_TAIL", None)
        if self.old is not None:
            os.environ["PT_BLAS_TAIL"] = self.old


# ------------------------------------------------------------------ scenes and poses
def part_grid(n, size, y, material):
    """The first n triangles of the wavy grid of side ceil(sqrt(n / 2))."""
    side = 1
    while 2 * side * side < n:
        side += 1
    m = TB.grid_mesh(side, size, y, material)
    return TB.mesh_of(m.v1[:n].copy(), m.v2[:n].copy(), m.v3[:n].copy(), material)


def sphere_mesh(slices, stacks, radius, material):
    """A latitude-longitude sphere of 2 * slices * stacks triangles, as tests/native/blas_rebuild_check.cpp builds it."""
    i, j = np.meshgrid(np.arange(slices + 1), np.arange(stacks + 1), indexing="xy")
    th = (f32(3.14159265) * j.astype(f32) / f32(stacks)).astype(f32)
    ph = (f32(6.2831853) * i.astype(f32) / f32(slices)).astype(f32)
    p = np.stack([f32(radius) * np.sin(th) * np.cos(ph), f32(radius) * np.cos(th), f32(radius) * np.sin(th) * np.sin(ph)], axis=2).astype(f32)
    a, b, c, e = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]
    v1 = np.stack([a, b], axis=2).reshape(-1, 3)
    v2 = np.stack([b, e], axis=2).reshape(-1, 3)
    v3 = np.stack([c, c], axis=2).reshape(-1, 3)
    return TB.mesh_of(v1, v2, v3, material)


def scene_pair(na, nb):
    """Two BLASes of na and nb triangles: the first instanced twice under a rotation and a non-uniform scale, the second
    once; a floor and a light."""
    s = Scene()
    s.Add(Cube.NewCube(Vector(-8, -1, -8), Vector(8, 0, 8), TB.GREY()))
    s.Add(Sphere.NewSphere(Vector(5, 6, 2), 0.75, TB.LIGHT()))
    ma = sphere_mesh(80, 40, 1.0, TB.BLUE()) if na == 6400 else part_grid(na, 2, 0.75, TB.BLUE())
    mb = part_grid(nb, 2, 0.75, TB.RED())
    s.Add(TransformedShape.NewTransformedShape(ma, TB.placed(0.4, (1.5, 0.75, 2.0), (-3, 2.5, 1))))
    s.Add(TransformedShape.NewTransformedShape(mb, TB.placed(0.7, (1.25, 0.5, 0.8), (3, 2, -1))))
    s.Add(TransformedShape.NewTransformedShape(ma, TB.placed(-1.1, (0.5, 2.0, 1.0), (1, 4, 3))))
    return s, TB.CAMERA(), DefaultSampler.NewSampler(4, 3)


def move(name, flat):
    """The vertex arrays of a named pose of the scene as it stands."""
    v = TB.verts(flat)
    if name == "rest":
        pass
    elif name == "sine":
        v = TB.pose("sine", flat)[0]
    elif name == "twist":   # turned about y by an angle that grows with the height and the radius
        for a in v:
            x, y, z = a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()
            ang = (f32(2.5) * y + f32(1.5) * np.sqrt(x * x + z * z)).astype(f32)
            c, s_ = np.cos(ang).astype(f32), np.sin(ang).astype(f32)
            a[:, 0], a[:, 2] = (c * x - s_ * z).astype(f32), (s_ * x + c * z).astype(f32)
    elif name == "offset":   # every triangle moved as a whole by its own vector
        h = (np.arange(len(v[0]), dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
        off = np.zeros((len(v[0]), 3), f32)
        for k in range(3):
            h = (h * np.uint64(1664525) + np.uint64(1013904223)) & np.uint64(0xFFFFFFFF)
            off[:, k] = f32(1.5) * ((h >> np.uint64(8)).astype(f32) * f32(1.0 / 16777216.0) - f32(0.5))
        v = [(a + off).astype(f32) for a in v]
    else:
        raise KeyError(name)
    return [np.ascontiguousarray(a, f32) for a in v]


def normals_kw(mode, n):
    if mode == "kept":
        return {}
    if mode == "given":
        ang = (f32(0.01) * np.arange(n, dtype=f32)).astype(f32)
        return {"n1": np.stack([np.sin(ang), np.cos(ang), np.zeros(n, f32)], axis=1).astype(f32),
                "n2": np.stack([np.zeros(n, f32), np.cos(ang), np.sin(ang)], axis=1).astype(f32),
                "n3": np.broadcast_to(np.array([0.6, 0.8, 0.0], f32), (n, 3)).copy()}
    return {"normals": mode}


def normals_of(kw, v, flat):
    if "n1" in kw:
        return kw["n1"], kw["n2"], kw["n3"]
    if "normals" in kw:
        return tuple(normals_ref.normals(*v, flat.mesh_first, flat.mesh_count, kw["normals"]))
    return None


def same_blas(got, want, what):
    """ReadBlas() against the reference: the per-BLAS rows, nodes up to each BLAS's count, recs, shade, inner boxes."""
    gb, gn, gr, gs, gx = got
    wb, wn, wr, ws, wx = want
    assert np.array_equal(gb[:, :3], np.asarray(wb)[:, :3]), f"{what}: blas rows {gb} vs {wb}"
    for name, a, b in (("nodes", gn, wn), ("recs", gr, wr), ("shade", gs, ws)):
        bad = np.argwhere(a != b)
        assert not bad.size, f"{what}: {name}: {len(bad)} words differ, first at {bad[0]}"
    assert np.array_equal(gx, wx), f"{what}: inner boxes {gx} vs {wx}"


# ------------------------------------------------------------------ 1. words
CASES = [(p, q) for p in PAIRS for q in POSES]


@pytest.mark.parametrize("pair,pname", CASES, ids=[f"{a}+{b}-{q}" for (a, b), q in CASES])
def test_words_after_a_rebuild(gpu, pair, pname):
    st = scene_pair(*pair)
    flat0 = st[0].Compile()
    rest = [a.copy() for a in (flat0.tri_v1, flat0.tri_v2, flat0.tri_v3, flat0.tri_n1, flat0.tri_n2, flat0.tri_n3)]
    up = None
    for mode in NORMALS:
        want = None
        for t in TAILS:
            for dst, a in zip((flat0.tri_v1, flat0.tri_v2, flat0.tri_v3, flat0.tri_n1, flat0.tri_n2, flat0.tri_n3), rest):
                dst[...] = a    # the FlatScene an earlier rebuild wrote into, back at rest
            r = TB.renderer(st)
            try:
                flat = st[0].Compile()
                if up is None:
                    up = TB.Upload(r, flat)
                    assert list(B.tri_counts(up.before["blas"][0], len(up.before["blas"][2]))) == list(pair)
                v = move(pname, flat)
                kw = normals_kw(mode, len(v[0]))
                with tail(t):
                    ms = r.RebuildBlas(*v, what=_abi.REBUILD_BLAS, **kw)
                assert ms > 0
                got = r.ReadBlas()
                if want is None:
                    b0 = up.before["blas"]
                    ref = RB.rebuild(b0[0], b0[1], b0[2], b0[3], up.blas_src, *v, normals=normals_of(kw, v, flat))
                    want = ref[:5]
                    for b, nt in enumerate(pair):
                        assert want[0][b, 1] == sum(RB.plan(nt)[2]) <= b0[0][b, 1]
                    if max(pair) > 16 and pname != "rest":
                        assert not np.array_equal(ref[5], up.blas_src)   # the order changed: the sort is not idle
                same_blas(got, want, f"{pair} {pname} {mode} tail {t}")
            finally:
                r.close()


# ------------------------------------------------------------------ 2. rays
def fresh_of(make, pname, mode):
    """A scene tuple whose FlatScene holds the moved arrays: uploaded fresh, it is the reference context."""
    st = make()
    flat = st[0].Compile()
    v = move(pname, flat)
    kw = normals_kw(mode, len(v[0]))
    TB.apply_to_flat(flat, v, kw)
    return st


def instance_mesh(flat, t):
    x = flat.transformed[t]
    f, n = int(flat.mesh_first[x.shape_index]), int(flat.mesh_count[x.shape_index])
    return flat.tri_v1[f:f + n], flat.tri_v2[f:f + n], flat.tri_v3[f:f + n], np.array(list(x.matrix)).reshape(4, 4)


RAY_SCENES = {"pair": lambda: scene_pair(288, 65), "T": TB.scene_t, "big": lambda: scene_pair(6400, 64),
              "instances": lambda: scenes.instances(copies=3, mesh_tris=1200)}
RAY_CASES = [("pair", "twist"), ("T", "offset"), ("big", "offset"), ("instances", "twist")]


@pytest.mark.parametrize("name,pname", RAY_CASES, ids=[f"{a}-{b}" for a, b in RAY_CASES])
def test_rays_after_a_rebuild(gpu, name, pname):
    make = RAY_SCENES[name]
    st, st2 = make(), fresh_of(make, pname, "face")
    r, fresh = TB.renderer(st), TB.renderer(st2)
    try:
        flat = st[0].Compile()
        v = move(pname, flat)
        r.RebuildBlas(*v, normals="face")
        t0 = next(t for t in range(flat.counts_ext[3]) if flat.transformed[t].shape_kind == _abi.SHAPE_MESH)
        od, dd, _ = D.instance_rays(*instance_mesh(flat, t0), n=100, seed=9)
        lo, hi = TB.moved_box(flat)
        o2, d2 = TB.rays_at(lo, hi, 4096 - len(od), 31)
        o, d = np.ascontiguousarray(np.concatenate([od, o2]), f32), np.ascontiguousarray(np.concatenate([dd, d2]), f32)
        assert len(o) == 4096 and len(od) >= 1000
        t, k = r.Intersect(o, d)
        ft, fk = fresh.Intersect(o, d)
        bad = np.flatnonzero((t.view(np.int64) != ft.view(np.int64)) | (k != fk))
        assert bad.size == 0, f"{bad.size} rays differ from the fresh upload, first {bad[:5]}: t {t[bad[:3]]} vs {ft[bad[:3]]}, kind {k[bad[:3]]} vs {fk[bad[:3]]}"
        hits = int((k == _abi.SHAPE_TRANSFORMED).sum())
        print(f"{name} {pname}: {hits} rays hit an instance")
        assert hits >= 400
        rng = np.random.default_rng(7)
        tl = np.where(t < 1e9, t, 5.0)
        for what, tm in {"at_hit": tl, "past_hit": np.nextafter(tl, np.inf), "random": tl * rng.uniform(0.0, 1.6, len(tl))}.items():
            assert np.array_equal(r.Occluded(o, d, tm), fresh.Occluded(o, d, tm)), f"occluded {what}"
        want_names = {"t", "kind", "index", "prim", "shape"}
        got, want = r.IntersectHits(o, d, want=want_names), fresh.IntersectHits(o, d, want=want_names)
        assert np.array_equal(got["t"].view(np.int64), t.view(np.int64)) and np.array_equal(got["kind"], k)
        for key in ("kind", "index", "shape"):
            assert np.array_equal(got[key], want[key]), key
        assert np.array_equal(got["prim"], want["prim"]), f"prim differs on rays {np.flatnonzero(got['prim'] != want['prim'])[:5]}"
        inst = instanced_prims(flat)
        hit = k == _abi.SHAPE_TRANSFORMED
        assert np.isin(got["prim"][hit], inst).all()
    finally:
        r.close()
        fresh.close()


def instanced_prims(flat):
    return np.flatnonzero(TB.instanced(flat))


def scene_textured():
    """An instanced 288-triangle grid whose material has a texture and whose triangles carry their own uv: blas_uv rows
    that stay behind when the triangles are re-sorted show as another albedo."""
    from ptsharp_amd.scene import ColorTexture, Material, Mesh
    from ptsharp_amd.geometry import Colour
    g = part_grid(288, 2, 0.75, TB.BLUE())
    rng = np.random.default_rng(3)
    uv = [np.concatenate([rng.random((288, 2)), np.zeros((288, 1))], axis=1).astype(f32) for _ in range(3)]
    import dataclasses
    mat = dataclasses.replace(Material.DiffuseMaterial(Colour(1, 1, 1)),
                              Texture=ColorTexture.NewTexture(rng.integers(0, 256, (16, 16, 3)).astype(np.uint8)))
    m = Mesh(g.v1, g.v2, g.v3, g.n1, g.n2, g.n3, materials=[mat], t1=uv[0], t2=uv[1], t3=uv[2])
    s = Scene()
    s.Add(Cube.NewCube(Vector(-8, -1, -8), Vector(8, 0, 8), TB.GREY()))
    s.Add(Sphere.NewSphere(Vector(5, 6, 2), 0.75, TB.LIGHT()))
    s.Add(TransformedShape.NewTransformedShape(m, TB.placed(0.4, (1.5, 0.75, 2.0), (-1, 2.5, 1))))
    return s, TB.CAMERA(), DefaultSampler.NewSampler(4, 3)


def test_uv_rows_move_with_their_triangles(gpu):
    st, st2 = scene_textured(), fresh_of(scene_textured, "twist", "face")
    r, fresh = TB.renderer(st), TB.renderer(st2)
    try:
        flat = st[0].Compile()
        r.RebuildBlas(*move("twist", flat), normals="face")
        o, d = TB.rays_at(*TB.moved_box(flat), 2048, 11)
        names = {"t", "kind", "prim", "albedo", "material"}
        got, want = r.IntersectHits(o, d, want=names), fresh.IntersectHits(o, d, want=names)
        hit = got["kind"] == _abi.SHAPE_TRANSFORMED
        assert hit.sum() >= 300 and len(np.unique(got["albedo"][hit], axis=0)) >= 100   # the texture is seen, texel by texel
        for key in names:
            assert np.array_equal(np.ascontiguousarray(got[key]).view(np.uint8), np.ascontiguousarray(want[key]).view(np.uint8)), key
    finally:
        r.close()
        fresh.close()


# ------------------------------------------------------------------ 3. renders and features
@TB.ENGINES
@pytest.mark.parametrize("name", ["R", "T", "O"])
def test_render_parity_after_a_rebuild(gpu, engine, name):
    make = TB.SCENES[name]
    st, st2 = make(), fresh_of(make, "twist", "face")
    r, fresh = TB.renderer(st, engine), TB.renderer(st2, engine)
    try:
        TB.frame(r)                        # a pass at the rest pose first: the rebuild comes between passes
        v = move("twist", st[0].Compile())
        r.RebuildBlas(*v, normals="face")
        g, grays = TB.frame(r)
        o, orays = O.render(O.OracleScene(st[0]), st[1], st[2], W, H, TB.SPP, seed=23)
        check(g, grays, o, orays)
        f, frays = TB.frame(fresh)
        assert grays == frays
        assert np.array_equal(g.N, f.N)
        for a, b, what in ((g.M, f.M, "M"), (g.V, f.V, "V")):
            frac, err = within(a, b)
            assert frac >= 0.999, f"{what} against the fresh upload: {frac:.5f} within 1e-9, max err {err:.3g}"
        if engine == _abi.ENGINE_WAVEFRONT:
            want = F.features(st[0], st[1], W, H)
            assert (want[3] == _abi.SHAPE_TRANSFORMED).sum() >= 20
            r.RenderFeatures()
            fresh.RenderFeatures()
            for a, b, c, what in zip(r.Features(), fresh.Features(), want, ("albedo", "normal", "depth", "kind", "material")):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"features against the fresh upload: {what} differs"
                if what == "albedo":
                    assert (np.abs(a - c) <= 1e-9 * np.maximum(1.0, np.abs(c))).all(), what
                else:
                    assert np.array_equal(a.view(np.uint8), c.view(np.uint8)), f"features against the reference: {what} differs"
    finally:
        r.close()
        fresh.close()


# ------------------------------------------------------------------ 4. what
@pytest.mark.parametrize("what", [_abi.REBUILD_WORLD, 0, _abi.REBUILD_BLAS])
def test_without_instanced_mesh(gpu, what):
    sa, sb = TB.scene_n(), TB.scene_n()
    r, r2 = TB.renderer(sa), TB.renderer(sb)
    try:
        v = move("twist", sa[0].Compile())
        r.RebuildBlas(*v, normals="smooth", what=what)
        if what == _abi.REBUILD_BLAS:   # nothing to re-sort: the refit alone
            r2.UpdateMeshes(*v, normals="smooth")
        else:
            r2.RebuildMeshes(*v, normals="smooth")
        TB.same_state(TB.state(r), TB.state(r2), f"what {what}", boxes_as_values=False)
        same_buffer(TB.frame(r)[0], TB.frame(r2)[0])
    finally:
        r.close()
        r2.close()


def test_blas_only_leaves_the_world_tree_to_the_refit(gpu):
    sa, sb, sc = TB.scene_t(), TB.scene_t(), TB.scene_t()
    r, r2, r3 = TB.renderer(sa), TB.renderer(sb), TB.renderer(sc)
    try:
        v = move("twist", sa[0].Compile())
        r.RebuildBlas(*v, what=_abi.REBUILD_BLAS)
        r2.UpdateMeshes(*v)
        for x, y in zip(r.ReadTriBvh(), r2.ReadTriBvh()):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        r3.RebuildBlas(*v)   # both: the world tree re-sorted too, the BLASes as with PT_REBUILD_BLAS alone
        assert not np.array_equal(r3.ReadTriBvh()[0][:, 3:8], r.ReadTriBvh()[0][:len(r3.ReadTriBvh()[0]), 3:8])
        for x, y in zip(r3.ReadBlas(), r.ReadBlas()):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        o, d = TB.rays_at(*TB.moved_box(sa[0].Compile()), 2048, 5)
        t, k = r.Intersect(o, d)
        t3, k3 = r3.Intersect(o, d)
        assert np.array_equal(t.view(np.int64), t3.view(np.int64)) and np.array_equal(k, k3)
    finally:
        r.close()
        r2.close()
        r3.close()


def test_only_instanced_triangles(gpu):
    st = TB.scene_o()
    r = TB.renderer(st)
    try:
        flat = st[0].Compile()
        up = TB.Upload(r, flat)
        v = move("twist", flat)
        r.RebuildBlas(*v)   # both: nothing is launched for the world
        assert len(r.ReadTriBvh()[0]) == 0
        b0 = up.before["blas"]
        same_blas(r.ReadBlas(), RB.rebuild(b0[0], b0[1], b0[2], b0[3], up.blas_src, *v)[:5], "only")
    finally:
        r.close()


# ------------------------------------------------------------------ 5. sequences
def test_rebuild_then_update_meshes(gpu):
    st = scene_pair(288, 65)
    r = TB.renderer(st)
    try:
        flat = st[0].Compile()
        up = TB.Upload(r, flat)
        v = move("twist", flat)
        r.RebuildBlas(*v)
        b0 = up.before["blas"]
        blas1, nodes1, recs1, shade1, _, src1 = RB.rebuild(b0[0], b0[1], b0[2], b0[3], up.blas_src, *v)
        v2 = move("sine", flat)   # of the twisted scene
        kw = normals_kw("given", len(v2[0]))
        r.UpdateMeshes(*v2, **kw)
        nodes2, recs2, shade2, boxes2 = B.refit(blas1, nodes1, recs1, shade1, src1, *v2, normals=normals_of(kw, v2, flat))
        same_blas(r.ReadBlas(), (blas1, nodes2, recs2, shade2, boxes2), "rebuild then update")
        assert np.array_equal(r.ReadBlas()[1][:, 24:], nodes1[:, 24:])
        # a second rebuild at the pose the tree was sorted for changes no word
        r.RebuildBlas(*v)
        first = r.ReadBlas()
        r.RebuildBlas(*v)
        same_blas(r.ReadBlas(), first, "fixed point")
    finally:
        r.close()


def test_rebuild_from_the_staged_pose(gpu):
    sa, sb = TB.scene_t(), TB.scene_t()
    r, r2 = TB.renderer(sa), TB.renderer(sb)
    try:
        m = Matrix.TranslateM(Vector(0.5, -0.25, 1)).Mul(Matrix.RotateM(Vector(1, 2, 3), 1.1)).Mul(Matrix.ScaleM(Vector(3, 0.3, 1)))
        flat = sa[0].Compile()
        r.SetRestPose()
        r.PoseMeshes([m] * len(flat.mesh_first))
        r.RebuildBlas()
        posed = [a.copy() for a in (flat.tri_v1, flat.tri_v2, flat.tri_v3, flat.tri_n1, flat.tri_n2, flat.tri_n3)]
        r2.RebuildBlas(*posed)
        sa_, sb_ = TB.state(r), TB.state(r2)
        for stt in (sa_, sb_):   # lines past a BLAS's new count are left as they are: the pose's refit wrote r's, the upload r2's
            blas, nodes = stt["blas"][0], stt["blas"][1]
            for n0, nn, _, _ in blas:
                end = int(blas[blas[:, 0] > n0, 0].min()) if (blas[:, 0] > n0).any() else len(nodes)
                nodes[n0 + nn:end] = 0
        TB.same_state(sa_, sb_, "staged against arrays", boxes_as_values=False)
        assert r.ReadBlas()[0][1, 1] == sum(RB.plan(288)[2])   # rebuilt, not only refitted
    finally:
        r.close()
        r2.close()


def test_update_shapes_before_and_after(gpu):
    sa, sb, sc = TB.scene_t(), TB.scene_t(), TB.scene_t()
    fc = sc[0].Compile()
    vc = move("twist", fc)
    TB.apply_to_flat(fc, vc, {"normals": "face"})
    for i, mm in enumerate(TB.spun(fc)["matrices"]):
        fc.transformed[i].matrix[:] = np.asarray(mm, np.float64).reshape(-1).tolist()
        fc.transformed[i].inverse[:] = Matrix(mm).Inverse().m.reshape(-1).tolist()
    r, r2, fresh = TB.renderer(sa), TB.renderer(sb), TB.renderer(sc)
    try:
        fa, fb = sa[0].Compile(), sb[0].Compile()
        v = move("twist", fa)
        r.RebuildBlas(*v, normals="face")
        r.UpdateShapes(**TB.spun(fa))
        r2.UpdateShapes(**TB.spun(fb))
        r2.RebuildBlas(*v, normals="face")
        TB.same_state(TB.state(r), TB.state(r2), "either order")
        o, d = TB.rays_at(*TB.moved_box(fa), 2048, 5)
        t, k = r.Intersect(o, d)
        ft, fk = fresh.Intersect(o, d)
        assert np.array_equal(t.view(np.int64), ft.view(np.int64)) and np.array_equal(k, fk)
        assert (k == _abi.SHAPE_TRANSFORMED).sum() > 0
    finally:
        r.close()
        r2.close()
        fresh.close()


def test_upload_rebuild_upload(gpu):
    st = scene_pair(288, 65)
    r = TB.renderer(st)
    try:
        r.RebuildBlas(*move("twist", st[0].Compile()))
        r.IntersectHits(*TB.rays_at(np.zeros(3), np.ones(3), 16, 1), want={"prim"})   # the query's copy of the order exists
        s2 = TB.scene_t()[0]
        r.Scene = s2
        flat = s2.Compile()
        up = TB.Upload(r, flat)          # uploads the new scene
        assert list(up.before["blas"][0][:, 1]) != [26, 8]
        v = move("offset", flat)
        r.RebuildBlas(*v, what=_abi.REBUILD_BLAS)
        b0 = up.before["blas"]
        same_blas(r.ReadBlas(), RB.rebuild(b0[0], b0[1], b0[2], b0[3], up.blas_src, *v)[:5], "after the second upload")
        fresh = TB.renderer(fresh_of(TB.scene_t, "offset", "kept"))
        try:
            o, d = TB.rays_at(*TB.moved_box(flat), 2048, 5)
            got, want = r.IntersectHits(o, d, want={"t", "prim"}), fresh.IntersectHits(o, d, want={"t", "prim"})
            assert np.array_equal(got["t"].view(np.int64), want["t"].view(np.int64))
            assert np.array_equal(got["prim"], want["prim"])
        finally:
            fresh.close()
    finally:
        r.close()


# ------------------------------------------------------------------ 6. cost
# tests/native/blas_rebuild_check.cpp's gates, on the device's numbers: the rebuilt tree M costs less than the refitted
# one R, and at most the measured M / F (twist 0.9613, offset 1.1129) + 10 % of the fresh build's F
COST_RATIO = {"twist": 0.9613, "offset": 1.1129}


@pytest.mark.parametrize("pname", ["twist", "offset"])
def test_cost(gpu, pname):
    make = lambda: scene_pair(6400, 64)
    st, st2 = make(), fresh_of(make, pname, "kept")
    r, fresh = TB.renderer(st), TB.renderer(st2)
    try:
        v = move(pname, st[0].Compile())
        for step in ("upload", "refit", "rebuilt"):
            if step == "refit":
                r.UpdateMeshes(*v)
            elif step == "rebuilt":
                r.RebuildBlas(*v, what=_abi.REBUILD_BLAS)
            blas, nodes = r.ReadBlas()[:2]
            got, want = r.BlasCost(), RB.cost(blas, nodes)
            assert got.shape == want.shape == (2, 3) and (want[:, 2] > 0).all()
            assert (np.abs(got - want) <= 1e-9 * np.abs(want)).all(), f"{step}: {got} vs {want}"
            if step == "refit":
                R = got[0, 0] + got[0, 1]
        M = got[0, 0] + got[0, 1]
        f = fresh.BlasCost()
        Fc = f[0, 0] + f[0, 1]
        print(f"cost {pname}: fresh {Fc:.4f} refit {R:.4f} rebuilt {M:.4f} M/F {M / Fc:.4f}")
        assert M < R
        assert M <= (COST_RATIO[pname] + 0.10) * Fc
    finally:
        r.close()
        fresh.close()


# ------------------------------------------------------------------ 7. errors and the refusal
def test_errors_leave_the_scene_untouched(gpu):
    st = TB.scene_t()
    r = TB.renderer(st)
    fp = C.POINTER(C.c_float)
    try:
        assert r._lib.pt_get_version() == 10
        flat = st[0].Compile()
        before = TB.state(r)
        v, kw = TB.pose("grow", flat)
        keep = v + [kw["n1"], kw["n2"], kw["n3"]]
        a, b, c, n1, n2, n3 = [x.ctypes.data_as(fp) for x in keep]
        n = len(v[0])
        U, two = _abi.pt_mesh_update, (C.c_int32 * 2)
        ms = C.c_double(-1.0)
        call = lambda ctx, u, what=0: r._lib.pt_rebuild_blas(ctx, None if u is None else C.byref(u), what, C.byref(ms))
        cases = {
            "NULL ctx": lambda: call(None, U(n, 0, two(0, 0), a, b, c, n1, n2, n3)),
            "NULL u, no staged pose": lambda: call(r._ctx, None),
            "NULL v1": lambda: call(r._ctx, U(n, 0, two(0, 0), None, b, c)),
            "NULL v3": lambda: call(r._ctx, U(n, 0, two(0, 0), a, b, None)),
            "reserved[0]": lambda: call(r._ctx, U(n, 0, two(1, 0), a, b, c)),
            "mode 3": lambda: call(r._ctx, U(n, 3, two(0, 0), a, b, c)),
            "n2 missing": lambda: call(r._ctx, U(n, 0, two(0, 0), a, b, c, n1, None, n3)),
            "normals with FACE": lambda: call(r._ctx, U(n, _abi.NORMALS_FACE, two(0, 0), a, b, c, n1, n2, n3)),
            "one triangle fewer": lambda: call(r._ctx, U(n - 1, 0, two(0, 0), a, b, c)),
            "what 4": lambda: call(r._ctx, U(n, 0, two(0, 0), a, b, c), 4),
            "what -1": lambda: call(r._ctx, U(n, 0, two(0, 0), a, b, c), -1),
            "cost: wrong count": lambda: r._lib.pt_blas_cost(r._ctx, 3, (C.c_double * 9)()),
            "cost: NULL out": lambda: r._lib.pt_blas_cost(r._ctx, 2, None),
            "cost: NULL ctx": lambda: r._lib.pt_blas_cost(None, 2, (C.c_double * 6)()),
        }
        for what, fn in cases.items():
            assert fn() == _abi.PT_ERR_INVALID_ARG, what
            TB.same_state(TB.state(r), before, what, boxes_as_values=False)
        # the refusal stays: pt_rebuild_meshes on an instanced scene, byte for byte
        with pytest.raises(_abi.PTError) as e:
            r.RebuildMeshes(*v)
        assert e.value.code == _abi.PT_ERR_UNSUPPORTED
        assert ("rebuild meshes: the scene holds an instanced mesh (a transformed shape over PT_SHAPE_MESH); "
                "BLASes are not rebuilt") in str(e.value)
        TB.same_state(TB.state(r), before, "refused", boxes_as_values=False)
        # a refused call between two rebuilds changes nothing
        r.RebuildBlas(*v, **kw)
        mid = TB.state(r)
        assert call(r._ctx, U(n, 0, two(0, 0), a, b, c), 7) == _abi.PT_ERR_INVALID_ARG
        TB.same_state(TB.state(r), mid, "refused between rebuilds", boxes_as_values=False)
    finally:
        r.close()
    from ptsharp_amd import Renderer
    r = Renderer.NewRenderer(None, None, None, W, H, True, device=0)
    try:
        z = np.zeros((1, 3), f32).ctypes.data_as(fp)
        u = _abi.pt_mesh_update(1, 0, (C.c_int32 * 2)(0, 0), z, z, z)
        assert r._lib.pt_rebuild_blas(r._ctx, C.byref(u), 0, None) == _abi.PT_ERR_NO_SCENE
        assert r._lib.pt_blas_cost(r._ctx, 0, (C.c_double * 3)()) == _abi.PT_ERR_NO_SCENE
    finally:
        r.close()
