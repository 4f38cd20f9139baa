"""pt_intersect_hits on the GPU: what a host's rays hit and where.

  1. camera rays of the seven features_ref.SCENES at 67x45 and 9x2 against tests/query_ref.py (the oracle's loop for t,
     kind and index, its Hit.Info, its slots): t, kind, material, inside, the normal's and the position's bits equal,
     albedo and gloss within 1e-9 max(1, |want|), index, prim and shape equal; a ray whose index differs is accepted only
     when the reported primitive's own intersect gives the reported t (a tie), such rays at most 1 % of the hits; t and
     kind are Renderer.Intersect's bit for bit;
  2. identity at degenerate rays (tests/degenerate_rays.py: lattice, the rest pose of the grid mesh, instanced; every
     generated family, rays at edges and vertices tie by construction): t and kind are pt_intersect's; for every hit of a
     sphere, cube, plane or triangle or_prim_intersect of the reported primitive's own parameters returns t bit for bit,
     the definition of a valid index; where t, kind and index equal those of the oracle's walk (whose hit or_hit_info
     describes), material and slot equal or_hit_info's, and normal and inside where the primitive is the oracle's too (for
     a hit through an instanced mesh the index names the instance, and which of two tying triangles the oracle took is
     known only where the mesh has a material per triangle: case 3);
  3. prim through an instance: a 200-triangle mesh with a material per triangle, instanced twice and not top-level:
     kind TRANSFORMED, index the instance, shape its slot, material or_hit_info's, prim == material; with the same mesh
     range top-level as well, world hits give kind TRIANGLE and index == prim == material;
  4. after the scene moved: the 6,400-triangle sphere of tests/test_gpu_rebuild.py with a material per triangle, after
     UpdateMeshes (twist), RebuildMeshes and PoseMeshes, 4,096 rays each: the valid-index rule on the new vertices, index
     == material, and every array against a context that uploaded the moved scene fresh (t, kind, shape everywhere; the
     rest where the index agrees; a differing index is a tie by the rule above, at most 1 % of the hits); UpdateShapes
     moving a sphere keeps index and shape, and the position follows;
  5. sizes and options: n in {0, 1, 63, 64, 65, 255, 256, 257, 3015} equal the prefix of one large call, PT_QUERY_CHUNK=64
     equals the default, every single-output call equals that array of the all-outputs call, PT_MARCH_LANE / _WAVE give
     the same bits, on gopher3 (not FULL) and mixed (FULL);
  6. a query changes neither the Buffer, Stats() nor Features(), nor what the next pass renders;
  7. errors on a live context leave the outputs' sentinel in place.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import degenerate_rays as D
import features_ref as F
import oracle_lib as O
import query_ref as Q
import test_gpu_rebuild as RB
import test_gpu_refit as RF
from ptsharp_amd import Renderer, TransformedShape, Vector, _abi, scenes
from ptsharp_amd.geometry import Colour, Matrix
from ptsharp_amd.scene import Camera, Cube, DefaultSampler, Material, Mesh, Scene, Sphere, Triangle

pytestmark = pytest.mark.gpu
f32 = np.float32
INTS = ("kind", "index", "prim", "shape", "inside", "material")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same_arrays(got, want, what, names=None):
    for name in names or want:
        g, w = bits(got[name]), bits(want[name])
        assert g.shape == w.shape, f"{what}: {name} shape {g.shape} vs {w.shape}"
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1)) if len(g) else np.zeros(0, int)
        assert not bad.size, f"{what}: {name} differs on {bad.size} rays, first {bad[:5]}: {got[name][bad[:3]]} vs {want[name][bad[:3]]}"


def tie_rays(flat, got, want_index, o, d, what, tris=None):
    """The rays whose index differs from want_index: each must be a tie (the reported primitive's own intersect gives
    the reported t), and they are at most 1 % of the hits.  Returns the mask of rays whose index agrees."""
    differ = np.flatnonzero(got["index"] != want_index)
    hits = int((got["kind"] >= 0).sum())
    print(f"{what}: {hits} hits of {len(o)}, index differs on {differ.size} rays")
    sub = {k: got[k][differ] for k in ("t", "kind", "index")}
    assert np.isin(sub["kind"], (0, 1, 2, 3)).all(), f"{what}: index differs on rays that hit kinds {set(sub['kind'].tolist())}"
    bad = Q.valid_index_failures(flat, sub, o[differ], d[differ], tris)
    assert not bad, f"{what}: index differs and is no tie on rays {[(int(differ[i]), k, x, t, own) for i, k, x, t, own in bad[:4]]}"
    assert differ.size <= 0.01 * hits, f"{what}: index differs on {differ.size} of {hits} hits"
    return got["index"] == want_index


# ------------------------------------------------------------------ 1. camera rays against the oracle
@pytest.mark.parametrize("name,w,h", Q.CAMERA_CASES, ids=[f"{n}-{w}x{h}" for n, w, h in Q.CAMERA_CASES])
def test_camera_rays_match_the_oracle(gpu, name, w, h):
    s, c, smp = F.scene_of(name)
    o, d, want = Q.camera_case(name, w, h)
    r = Renderer.NewRenderer(s, c, smp, w, h, True, device=0)
    try:
        got = r.IntersectHits(o, d)
        t, k = r.Intersect(o, d)
    finally:
        r.close()
    what = f"{name} {w}x{h}"
    assert np.array_equal(bits(got["t"]), bits(t)) and np.array_equal(got["kind"], k), f"{what}: t or kind differ from pt_intersect's"
    same_arrays(got, want, what, ("t", "kind", "material", "inside", "normal", "position"))
    for name_ in ("albedo", "gloss"):
        err = np.abs(got[name_] - want[name_])
        print(f"{what}: max |d {name_}| {err.max():.3g}")
        assert (err <= 1e-9 * np.maximum(1.0, np.abs(want[name_]))).all(), f"{what}: {name_} max err {err.max()}"
    agree = tie_rays(F.oracle_of(name).flat, got, want["index"], o, d, what)
    assert np.array_equal(got["shape"][agree], want["shape"][agree]), f"{what}: shape"
    known = agree & (want["prim"] != Q.PRIM_UNKNOWN)
    assert np.array_equal(got["prim"][known], want["prim"][known]), f"{what}: prim"
    differ = ~agree   # a tie between two primitives: both still belong to shapes of the scene
    assert (got["shape"][differ] >= 0).all()


# ------------------------------------------------------------------ 2. identity at degenerate rays
@functools.lru_cache(maxsize=None)
def degenerate_case(name):
    st, _, (o, d, fam) = D.case(name)
    os_ = O.OracleScene(st[0])
    walk = Q.expected(os_, o, d, brute=False)
    return st, os_, o, d, fam, walk


@pytest.mark.parametrize("name", ["lattice", "rest", "instanced"])
def test_identity_at_degenerate_rays(gpu, name):
    st, os_, o, d, fam, walk = degenerate_case(name)
    r = RF.renderer(st)
    try:
        got = r.IntersectHits(o, d)
        t, k = r.Intersect(o, d)
    finally:
        r.close()
    assert np.array_equal(bits(got["t"]), bits(t)) and np.array_equal(got["kind"], k), f"{name}: t or kind differ from pt_intersect's"
    hit = got["kind"] >= 0
    assert ((got["index"] >= 0) == hit).all() and ((got["shape"] >= 0) == hit).all() and ((got["material"] >= 0) == hit).all()
    bad = Q.valid_index_failures(os_.flat, got, o, d)
    checked = int(np.isin(got["kind"], (0, 1, 2, 3)).sum())
    print(f"{name}: {len(o)} rays, {int(hit.sum())} hits, {checked} checked by their own primitive, {len(bad)} fail")
    assert checked >= 100
    assert not bad, f"{name}: the reported primitive does not give the reported t: {[(i, fam[i], k_, x, t_, own) for i, k_, x, t_, own in bad[:4]]}"
    tri = got["kind"] == _abi.SHAPE_TRIANGLE
    assert np.array_equal(got["prim"][tri], got["index"][tri])
    same = hit & (bits(got["t"]) == bits(walk["t"])) & (got["kind"] == walk["kind"]) & (got["index"] == walk["index"])
    print(f"{name}: {int(same.sum())} hits are the oracle walk's own")
    assert same.sum() > 0
    # a hit through an instanced mesh: index names the instance, the primitive is `prim`, and at these rays two
    # triangles of the mesh tie by construction.  The oracle exports which one it took only through the material
    # (query_ref: PRIM_UNKNOWN for a mesh of one material; test_prim_through_an_instance has one per triangle), so the
    # normal and the side are compared where the primitive is known to be the oracle's; material and slot everywhere
    prim_same = same & (walk["prim"] != Q.PRIM_UNKNOWN) & (got["prim"] == walk["prim"])
    print(f"{name}: {int(prim_same.sum())} of them with the oracle's primitive known and equal")
    assert prim_same.sum() > 0
    sub = lambda a, m, names: {n: a[n][m] for n in names}
    same_arrays(sub(got, same, ("material", "shape")), sub(walk, same, ("material", "shape")), f"{name}, where the index is the oracle's")
    same_arrays(sub(got, prim_same, ("normal", "inside")), sub(walk, prim_same, ("normal", "inside")), f"{name}, where the primitive is the oracle's")


# ------------------------------------------------------------------ 3. prim through an instance
N_INST = 200


def instance_mesh():
    arrs = RB.sphere_arrays(N_INST + 1)
    v = [a[:N_INST] for a in arrs]
    mats = [Material.DiffuseMaterial(Colour((i + 1) / 256.0, 0.5, 1.0 - i / 512.0)) for i in range(N_INST)]
    return Mesh(*v, mat_index=np.arange(N_INST, dtype=np.int32), materials=mats)


def instance_scene(top_level):
    """Two instances of one mesh; top_level: the same triangle range is a top-level mesh as well (FlatScene flattens a
    top-level Mesh into a range of its own, so the slot is pointed at the instanced range in place: the copy's
    triangles are then in no shape)."""
    mesh = instance_mesh()
    s = Scene()
    mats = D.instance_matrices()
    for m in mats:
        s.Add(TransformedShape.NewTransformedShape(mesh, m))
    if top_level:
        s.Add(mesh)
    flat = s.Compile()
    assert np.array_equal(flat.tri_material[:N_INST], np.arange(N_INST)) and flat.mesh_first[0] == 0
    if top_level:
        assert flat.shape_kind[2] == _abi.SHAPE_MESH and flat.shape_index[2] == 1
        flat.shape_index[2] = 0
    camera = Camera.LookAt(Vector(4, 4, 4), Vector(0, 0, 0), Vector(0, 0, 1), 45)
    return (s, camera, DefaultSampler.NewSampler(4, 3)), mesh, mats


@pytest.mark.parametrize("top_level", [False, True], ids=["instanced", "instanced+top-level"])
def test_prim_through_an_instance(gpu, top_level):
    st, mesh, mats = instance_scene(top_level)
    parts = [D.instance_rays(mesh.v1, mesh.v2, mesh.v3, m.m, n=100, seed=9 + i)[:2] for i, m in enumerate(mats)]
    if top_level:
        parts.append(D.mesh_rays(mesh.v1, mesh.v2, mesh.v3, n=100)[:2])
    o = np.ascontiguousarray(np.concatenate([p[0] for p in parts]))
    d = np.ascontiguousarray(np.concatenate([p[1] for p in parts]))
    os_ = O.OracleScene(st[0])
    want = Q.expected(os_, o, d, brute=True)
    r = RF.renderer(st)
    try:
        got = r.IntersectHits(o, d)
    finally:
        r.close()
    same_arrays(got, want, "instances", ("t", "kind"))
    inst = got["kind"] == _abi.SHAPE_TRANSFORMED
    world = got["kind"] == _abi.SHAPE_TRIANGLE
    print(f"{len(o)} rays: {int(inst.sum())} hit an instance, {int(world.sum())} the top-level mesh")
    assert inst.sum() > 1000 and ((got["kind"] < 0) | inst | world).all()
    assert np.array_equal(got["index"][inst], want["index"][inst]) and np.isin(got["index"][inst], (0, 1)).all()
    assert np.array_equal(got["shape"][inst], got["index"][inst])       # the instances are slots 0 and 1
    told = inst & (want["material"] != Q.INFO_UNKNOWN)   # the oracle's walk found the loop's hit: or_hit_info describes it
    assert told.sum() > 0.9 * inst.sum()
    assert np.array_equal(got["material"][told], want["material"][told])
    assert np.array_equal(got["prim"][inst], got["material"][inst])
    assert (got["prim"][inst] >= 0).all() and (got["prim"][inst] < N_INST).all()
    if top_level:
        assert world.sum() > 500
        assert np.array_equal(got["index"][world], got["prim"][world]) and np.array_equal(got["index"][world], got["material"][world])
        assert (got["shape"][world] == 2).all()
    else:
        assert not world.any()


# ------------------------------------------------------------------ 4. after the scene moved
P_MOVED = 6400


def moved_scene(arrs):
    """test_gpu_rebuild's scene of 6,400 triangles with a material per triangle: the material id of a triangle is its
    index (the mesh is the first shape, the loose triangle the second)."""
    v1, v2, v3, n1, n2, n3 = arrs
    P = len(v1)
    s = Scene()
    vec = lambda r: Vector(*[float(q) for q in r])
    g = slice(0, P - 1)
    mats = [Material.DiffuseMaterial(Colour((i % 251 + 1) / 256.0, (i // 251 + 1) / 64.0, 0.5)) for i in range(P - 1)]
    s.Add(Mesh(v1[g], v2[g], v3[g], n1[g], n2[g], n3[g], mat_index=np.arange(P - 1, dtype=np.int32), materials=mats))
    k = P - 1
    s.Add(Triangle(vec(v1[k]), vec(v2[k]), vec(v3[k]), vec(n1[k]), vec(n2[k]), vec(n3[k]), Material.LightMaterial(Colour.White, 40)))
    s.Add(Cube.NewCube(Vector(-10, -3, -10), Vector(10, -2, 10), Material.DiffuseMaterial(Colour(0.7, 0.7, 0.7))))
    s.Add(Sphere.NewSphere(Vector(0, 6, 0), 1, Material.LightMaterial(Colour.White, 20)))
    camera = Camera.LookAt(Vector(3, 3, 3), Vector(0, 0, 0), Vector(0, 1, 0), 45)
    flat = s.Compile()
    assert np.array_equal(flat.tri_material, np.arange(P))
    return s, camera, DefaultSampler.NewSampler(4, 3)


def check_against_fresh(r, moved, step):
    """4,096 rays at the moved triangles: the valid-index rule on the new vertices, index == material, every array
    against a context that uploaded the moved scene fresh."""
    o, d = RB.rays_for(moved, 4096, 31)
    fresh_scene = moved_scene(moved)
    # as degenerate_rays.case drops them: a grazing hit nearer than the fp32 slab test enters the triangle's own padded
    # box is found or not by the order the tree is walked in, so two trees over the same triangles may
    # differ there in t itself; the input is changed, not the assertion
    keep = ~D.nearer_than_own_box(O.OracleScene(fresh_scene[0]), o, d)
    print(f"{step}: {int((~keep).sum())} of {len(o)} rays are grazing hits nearer than their own box and are left out")
    assert (~keep).sum() <= 8
    o, d = np.ascontiguousarray(o[keep]), np.ascontiguousarray(d[keep])
    fresh = RB.renderer(fresh_scene)
    try:
        got = r.IntersectHits(o, d)
        want = fresh.IntersectHits(o, d)
    finally:
        fresh.close()
    flat = fresh_scene[0].Compile()
    for who, a in (("moved", got), ("fresh", want)):
        bad = Q.valid_index_failures(flat, a, o, d)
        assert not bad, f"{step}, {who}: the reported primitive does not give the reported t: {bad[:4]}"
    tri = got["kind"] == _abi.SHAPE_TRIANGLE
    assert tri.sum() > 1000
    assert np.array_equal(got["index"][tri], got["material"][tri]) and np.array_equal(got["index"][tri], got["prim"][tri])
    assert (got["shape"][tri] == np.where(got["index"][tri] == P_MOVED - 1, 1, 0)).all()
    same_arrays(got, want, step, ("t", "kind", "shape"))
    agree = tie_rays(flat, got, want["index"], o, d, step)
    sub = lambda a: {n: a[n][agree] for n in _abi.HIT_ARRAYS}
    same_arrays(sub(got), sub(want), f"{step}, where the index agrees")
    return got


def test_identity_follows_the_moving_scene(gpu):
    arrs = RB.sphere_arrays(P_MOVED)
    st = moved_scene(arrs)
    r = RB.renderer(st)
    try:
        twist = RB.pose("twist", arrs)
        r.UpdateMeshes(*twist[:3])
        check_against_fresh(r, twist[:3] + arrs[3:], "after UpdateMeshes")
        r.RebuildMeshes(*twist[:3])
        before = r.ReadTriBvh()
        check_against_fresh(r, twist[:3] + arrs[3:], "after RebuildMeshes")
        m = Matrix.TranslateM(Vector(0.25, -0.125, 0.5)).Mul(Matrix.RotateM(Vector(1, 2, 3), 0.7))
        r.PoseMeshes([m])
        flat = st[0].Compile()
        posed = [np.array(a) for a in (flat.tri_v1, flat.tri_v2, flat.tri_v3, flat.tri_n1, flat.tri_n2, flat.tri_n3)]
        assert not np.array_equal(posed[0], twist[0]) and len(before[2]) == P_MOVED
        check_against_fresh(r, posed, "after PoseMeshes")
        # a sphere moves: who it is stays, where it is follows
        target = np.array([0.5, 6.0, 0.25])
        rng = np.random.default_rng(5)
        u = rng.standard_normal((512, 3))
        o = (target + 3.0 * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(f32)
        aim = target + 0.6 * rng.uniform(-1, 1, (512, 3))
        dd = aim - o
        d = (dd / np.linalg.norm(dd, axis=1, keepdims=True)).astype(f32)
        a = r.IntersectHits(o, d)
        r.UpdateShapes(sphere_center=[target.tolist()], sphere_radius=[1.0])
        b = r.IntersectHits(o, d)
        both = (a["kind"] == _abi.SHAPE_SPHERE) & (b["kind"] == _abi.SHAPE_SPHERE)
        assert both.sum() > 100 and (b["kind"] == _abi.SHAPE_SPHERE).sum() > 400
        assert (a["index"][both] == 0).all() and (b["index"][both] == 0).all() and (a["shape"][both] == 3).all() and (b["shape"][both] == 3).all()
        assert not Q.valid_index_failures(flat, b, o, d)      # the FlatScene mirrors the update
        sph = b["kind"] == _abi.SHAPE_SPHERE
        dist = np.linalg.norm(b["position"][sph].astype(np.float64) - target, axis=1)
        # fp32 rounding of the intersect and of the position at these magnitudes is about 3e-6; the sphere moved by 0.56
        assert np.abs(dist - 1.0).max() < 1e-4, "the positions lie on the moved sphere"
        assert (bits(a["position"][both]) != bits(b["position"][both])).any(axis=1).all()
    finally:
        r.close()


# ------------------------------------------------------------------ 5. sizes and options
@pytest.mark.parametrize("name", ["gopher3", "mixed"])
def test_sizes_chunks_and_single_outputs(gpu, name, monkeypatch):
    s, c, smp = F.scene_of(name)
    o, d, _ = Q.camera_case(name, 67, 45)
    assert len(o) == 3015
    monkeypatch.delenv("PT_QUERY_CHUNK", raising=False)
    r = Renderer.NewRenderer(s, c, smp, 67, 45, True, device=0)
    try:
        r._ensure_scene()
        assert (r._uploaded.counts_ext[1] + r._uploaded.counts_ext[2] + r._uploaded.counts_ext[3] > 0) == (name == "mixed")
        whole = r.IntersectHits(o, d)
        assert r.QueryKernelMs() > 0
        assert (whole["kind"] >= 0).sum() > 1000
        for n in (0, 1, 63, 64, 65, 255, 256, 257, 3015):
            part = r.IntersectHits(o[:n], d[:n])
            same_arrays(part, {k: v[:n] for k, v in whole.items()}, f"{name} n = {n}")
        monkeypatch.setenv("PT_QUERY_CHUNK", "64")
        same_arrays(r.IntersectHits(o, d), whole, f"{name} PT_QUERY_CHUNK=64")
        monkeypatch.setenv("PT_QUERY_CHUNK", "1")        # clamped to 64
        same_arrays(r.IntersectHits(o[:200], d[:200]), {k: v[:200] for k, v in whole.items()}, f"{name} PT_QUERY_CHUNK=1")
        monkeypatch.delenv("PT_QUERY_CHUNK")
        for out in _abi.HIT_ARRAYS:
            one = r.IntersectHits(o, d, want={out})
            assert list(one) == [out]
            same_arrays(one, {out: whole[out]}, f"{name} want = {out}")
        same_arrays(r.IntersectHits(o, d, want={"t", "kind", "index", "prim", "shape"}), whole, f"{name} identity only",
                    ("t", "kind", "index", "prim", "shape"))
        assert r.IntersectHits(o, d, want=set()) == {} and r.QueryKernelMs() == 0
    finally:
        r.close()


@pytest.mark.parametrize("name", ["volume", "mixed"])
def test_march_flags_give_the_same_bits(gpu, name):
    s, c, smp = F.scene_of(name)
    o, d, _ = Q.camera_case(name, 67, 45)
    r = Renderer.NewRenderer(s, c, smp, 67, 45, True, device=0)
    try:
        plain = r.IntersectHits(o, d)
        for flag in (_abi.MARCH_LANE, _abi.MARCH_WAVE):
            same_arrays(r.IntersectHits(o, d, flags=flag), plain, f"{name} flags {flag}")
            same_arrays(r.IntersectHits(o, d, flags=flag, want={"t", "index"}), plain, f"{name} flags {flag}, no info", ("t", "index"))
    finally:
        r.close()


# ------------------------------------------------------------------ 6. nothing else changes
def test_a_query_changes_nothing_else(gpu):
    def make():
        s, c, smp = scenes.gopher3()
        smp.MaxBounces = 4
        r = Renderer.NewRenderer(s, c, smp, 64, 48, True, device=0)
        r.SamplesPerPixel, r.Seed = 2, 7
        return r
    r, twin = make(), make()
    try:
        for q in (r, twin):
            q.RenderParallel()
            q.RenderFeatures()
        state = lambda q: (q.ReadBuffer().M.tobytes(), q.ReadBuffer().V.tobytes(), q.ReadBuffer().N.tobytes(), bytes(q.Stats()),
                           [a.tobytes() for a in q.Features()])
        before = state(r)
        o, d = Q.camera_rays(r.Camera, 64, 48)
        got = r.IntersectHits(o, d)
        assert (got["kind"] >= 0).sum() > 1000
        r.IntersectHits(o, d, want={"index"})
        assert state(r) == before
        assert r.Stats().rays_total == twin.Stats().rays_total
        for q in (r, twin):
            q.RenderParallel()
        assert state(r)[:3] == state(twin)[:3] and r.Stats().rays_total == twin.Stats().rays_total
    finally:
        r.close()
        twin.close()


# ------------------------------------------------------------------ 7. errors
def test_errors_on_a_live_context(gpu):
    s, c, smp = scenes.gopher3()
    r = Renderer.NewRenderer(s, c, smp, 16, 16, True, device=0)
    lib = _abi.load_library()
    o = np.zeros((4, 3), f32)
    d = np.tile(np.array([0, 0, 1], f32), (4, 1))
    fp = C.POINTER(C.c_float)
    po, pd = o.ctypes.data_as(fp), d.ctypes.data_as(fp)
    outs = {name: np.full((4, comps) if comps > 1 else 4, 77, dt) for name, (dt, comps) in _abi.HIT_ARRAYS.items()}

    def arrays(reserved=(0, 0)):
        a = _abi.pt_hit_arrays()
        a.reserved[0], a.reserved[1] = reserved
        for name, arr in outs.items():
            setattr(a, name, arr.ctypes.data_as(dict(_abi.pt_hit_arrays._fields_)[name]))
        return a

    def untouched():
        return all((a == 77).all() for a in outs.values())
    try:
        a = arrays()
        assert lib.pt_intersect_hits(r._ctx, 4, po, pd, 0, C.byref(a)) == _abi.PT_ERR_NO_SCENE and untouched()
        r._ensure_scene()
        for what, args in {"reserved[0]": (4, po, pd, 0, arrays((1, 0))), "reserved[1]": (4, po, pd, 0, arrays((0, 1))),
                           "n < 0": (-1, po, pd, 0, arrays()), "n > 2^30": ((1 << 30) + 1, po, pd, 0, arrays()),
                           "both march flags": (4, po, pd, _abi.MARCH_LANE | _abi.MARCH_WAVE, arrays()),
                           "unknown flag": (4, po, pd, 4, arrays()), "NULL origins": (4, None, pd, 0, arrays()),
                           "NULL dirs": (4, po, None, 0, arrays())}.items():
            n, oo, dd_, flags, arr = args
            assert lib.pt_intersect_hits(r._ctx, n, oo, dd_, flags, C.byref(arr)) == _abi.PT_ERR_INVALID_ARG, what
            assert lib.pt_last_error(), what
            assert untouched(), what
        assert lib.pt_intersect_hits(r._ctx, 4, po, pd, 0, None) == _abi.PT_ERR_INVALID_ARG and untouched()
        # degenerate calls: nothing launched, nothing written
        assert lib.pt_intersect_hits(r._ctx, 0, None, None, 0, C.byref(arrays())) == _abi.PT_OK and untouched()
        assert lib.pt_intersect_hits(r._ctx, 4, po, pd, 0, C.byref(_abi.pt_hit_arrays())) == _abi.PT_OK and untouched()
        assert lib.pt_intersect_hits(r._ctx, 4, po, pd, 0, C.byref(arrays())) == _abi.PT_OK and not untouched()
    finally:
        r.close()
