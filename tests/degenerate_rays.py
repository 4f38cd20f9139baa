"""Seeded generators of degenerate rays, shared by tests/test_degenerate_rays_ref.py (CPU: the generators' claims
and the reference) and tests/test_gpu_degenerate_rays.py (pt_intersect / pt_occluded against the oracle's loop
over every shape).  A helper like refit_ref.py, not a test.

Every generator returns (origins f32 [n, 3], dirs f32 [n, 3], family [n], an array of names).  Directions are
finite and non-zero; they are not all of unit length (Scene.Intersect does not ask for that, and a component
such as 1e-20 beside two general ones changes the length by nothing fp32 can hold).  Origins lie within about
twice the geometry's extent of it: far origins are another effect (the pt_occluded finding).

Mesh families (mesh_rays): what a BVH over triangles meets at its own planes.  Coordinates taken from a vertex
are copied bit for bit, never recomputed.
  axis_vertex / axis_edge / axis_centroid   two components exactly +0.0, all six signs, through a vertex, an
                                            edge midpoint, a centroid
  ..._nz                                    the same with one of the zero components -0.0
  plane_zero                                one component exactly +0.0 and the origin on that coordinate of a
                                            vertex: the ray lies in a plane that node and leaf boxes share
  plane_nz, plane_1e-20, plane_-1e-38,      that component -0.0 (1/d = -inf), 1e-20, -1e-38 (products that
  plane_1e-45                               overflow) and 1e-45 (a denormal: 1/d = inf, and 0 if flushed)
  origin_on_vertex                          the origin a vertex, the direction random
  aimed_at_vertex                           from a general direction at a vertex
  flat_in_plane (flat=True only)            inside z = 0 with d.z = 0: every triangle of the flat pose has
                                            det = 0 there and a box 2e-30 thick

Analytic families (lattice_rays) on lattice_scene(): unit cubes and spheres of radius 0.5 alternating at
spacing 2 in the plane z = 0 over the floor cube, a sphere above, and two TransformedShapes in lattice places
(a sphere translated, a cube under a quarter turn).
  axis_centre                               axis-aligned through a centre
  tangent_r / tangent_below / tangent_above axis-aligned, offset from a centre by exactly r, nextafter(r, 0),
                                            nextafter(r, inf) in a perpendicular axis
  origin_on_surface / origin_at_centre
  face_axis / face_oblique                  in a cube's face plane, axis-aligned and oblique
  cube_edge                                 along a cube edge
  cube_corner                               aimed at a cube corner
"""
from __future__ import annotations

import functools
import math

import numpy as np

from ptsharp_amd import TransformedShape, Vector
from ptsharp_amd.geometry import Colour, Matrix
from ptsharp_amd.scene import Camera, Cube, DefaultSampler, Material, Scene, Sphere

f32 = np.float32
R = f32(0.5)
PLANE_VALUES = {"plane_zero": f32(0.0), "plane_nz": f32(-0.0), "plane_1e-20": f32(1e-20), "plane_-1e-38": f32(-1e-38),
                "plane_1e-45": f32(1e-45)}
MESH_FAMILIES = (["axis_vertex", "axis_edge", "axis_centroid", "axis_vertex_nz", "axis_edge_nz", "axis_centroid_nz"]
                 + list(PLANE_VALUES) + ["origin_on_vertex", "aimed_at_vertex"])
LATTICE_FAMILIES = ["axis_centre", "tangent_r", "tangent_below", "tangent_above", "origin_on_surface",
                    "origin_at_centre", "face_axis", "face_oblique", "cube_edge", "cube_corner"]


def _unit(rng, n):
    u = rng.standard_normal((n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _finish(parts):
    o = np.ascontiguousarray(np.concatenate([p[0] for p in parts]), f32)
    d = np.ascontiguousarray(np.concatenate([p[1] for p in parts]), f32)
    fam = np.concatenate([np.full(len(p[0]), p[2], dtype=object) for p in parts])
    assert o.dtype == f32 and d.dtype == f32 and np.isfinite(o).all() and np.isfinite(d).all()
    assert (d != 0).any(axis=1).all()
    return o, d, fam


def mesh_extent(v1, v2, v3):
    """The centre and the largest half-extent of the triangles' box."""
    allv = np.concatenate([v1, v2, v3]).astype(np.float64)
    lo, hi = allv.min(axis=0), allv.max(axis=0)
    return (lo + hi) / 2, float(((hi - lo) / 2).max())


def _axis(rng, p, ext, n, negzero):
    """Axis-aligned rays through the points p [n, 3] (f32): the two other coordinates are p's own bits."""
    axis, sign = np.arange(n) % 3, np.where((np.arange(n) // 3) % 2 == 0, f32(1), f32(-1))
    d = np.zeros((n, 3), f32)
    d[np.arange(n), axis] = sign
    if negzero:
        other = (axis + 1 + (np.arange(n) // 6) % 2) % 3
        d[np.arange(n), other] = f32(-0.0)
    o = p.copy()
    dist = (ext * rng.uniform(0.25, 2.0, n)).astype(f32)
    o[np.arange(n), axis] = (p[np.arange(n), axis] - sign * dist).astype(f32)
    return o, d


def _in_plane(rng, verts, ext, n, value):
    """Rays with d[axis] = value and o[axis] the bits of a vertex's coordinate.  Half pass through that vertex,
    half through a random point of the same plane inside the geometry's box."""
    lo, hi = verts.min(axis=0).astype(np.float64), verts.max(axis=0).astype(np.float64)
    axis = np.arange(n) % 3
    v = verts[rng.integers(0, len(verts), n)]
    u = _unit(rng, n)
    u[np.arange(n), axis] = 0.0
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    d = u.astype(f32)
    d[np.arange(n), axis] = value
    through = v.astype(np.float64)
    rnd = lo + (hi - lo) * rng.random((n, 3))
    through[1::2] = rnd[1::2]
    o = (through - u * (ext * rng.uniform(0.25, 2.0, (n, 1)))).astype(f32)
    o[np.arange(n), axis] = v[np.arange(n), axis]
    return o, d


def mesh_rays(v1, v2, v3, n=200, seed=7, flat=False):
    """The mesh families at the triangles v1, v2, v3 ([T, 3] f32), n rays each."""
    rng = np.random.default_rng(seed)
    v1, v2, v3 = (np.ascontiguousarray(a, f32) for a in (v1, v2, v3))
    centre, ext = mesh_extent(v1, v2, v3)
    verts = np.concatenate([v1, v2, v3])
    T = len(v1)
    parts = []
    for negzero in (False, True):
        sfx = "_nz" if negzero else ""
        k = rng.integers(0, T, n)
        corner = rng.integers(0, 3, n)
        parts.append((*_axis(rng, np.stack([v1, v2, v3])[corner, k], ext, n, negzero), "axis_vertex" + sfx))
        k = rng.integers(0, T, n)
        a, b = np.stack([v1, v2, v3])[corner, k], np.stack([v2, v3, v1])[corner, k]
        parts.append((*_axis(rng, ((a + b) * f32(0.5)).astype(f32), ext, n, negzero), "axis_edge" + sfx))
        k = rng.integers(0, T, n)
        parts.append((*_axis(rng, ((v1[k] + v2[k] + v3[k]) / f32(3)).astype(f32), ext, n, negzero), "axis_centroid" + sfx))
    for name, value in PLANE_VALUES.items():
        parts.append((*_in_plane(rng, verts, ext, n, value), name))
    v = verts[rng.integers(0, len(verts), n)]
    parts.append((v.copy(), _unit(rng, n).astype(f32), "origin_on_vertex"))
    v = verts[rng.integers(0, len(verts), n)]
    o = (centre + ext * rng.uniform(1.0, 2.0, (n, 1)) * _unit(rng, n)).astype(f32)
    d = v.astype(np.float64) - o.astype(np.float64)
    parts.append((o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32), "aimed_at_vertex"))
    if flat:
        assert (verts[:, 2] == 0).all()
        v = verts[rng.integers(0, len(verts), n)]
        u = _unit(rng, n)
        u[:, 2] = 0.0
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        o = (v.astype(np.float64) - u * (ext * rng.uniform(0.25, 2.0, (n, 1)))).astype(f32)
        o[1::2] = (centre + ext * rng.uniform(-2, 2, (n, 3)))[1::2].astype(f32)
        o[:, 2] = v[:, 2]
        parts.append((o, u.astype(f32), "flat_in_plane"))
    return _finish(parts)


def instance_rays(v1, v2, v3, matrix, n=200, seed=9):
    """The mesh families at an instance: the object-space triangles moved by `matrix` ([4, 4] float64) in fp64
    and rounded, so a ray meets the instance's vertices and planes to within an fp32 rounding of the transform."""
    m = np.asarray(matrix, np.float64)
    move = lambda a: (a.astype(np.float64) @ m[:3, :3].T + m[:3, 3]).astype(f32)
    return mesh_rays(move(v1), move(v2), move(v3), n, seed)


# ------------------------------------------------------------------ the lattice
LIGHT = (0.0, 0.0, 6.0, 1.0)                      # the sphere above: centre and radius
FLOOR = ((-10.0, -10.0, -2.0), (10.0, 10.0, -1.0))
MOVED_SPHERE = (4.0, 2.0, 0.0)                    # a lattice sphere at the origin, translated here
TURNED_CUBE = (-4.0, 0.0, 0.0)                    # a lattice cube at (0, -4, 0) under a quarter turn about z


def lattice_shapes():
    """[(kind, centre)] of the 3x3 lattice: a cube where i + j is even, a sphere where it is odd."""
    return [("cube" if (i + j) % 2 == 0 else "sphere", (2.0 * i, 2.0 * j, 0.0)) for j in (-1, 0, 1) for i in (-1, 0, 1)]


def lattice_targets():
    """The lattice and the two TransformedShapes, by their world-space centres."""
    return lattice_shapes() + [("sphere", MOVED_SPHERE), ("cube", TURNED_CUBE)]


def lattice_scene(without=None):
    """(Scene, Camera, Sampler, names): the lattice, the floor, the light and the two TransformedShapes, in that
    order; `without` leaves the shape of that name out (the leave-one-out scenes of the near-tie check)."""
    s = Scene()
    grey = Material.DiffuseMaterial(Colour(0.7, 0.7, 0.7))
    names = []

    def add(name, shape):
        if name != without:
            s.Add(shape)
            names.append(name)

    def unit_cube(c):
        return Cube.NewCube(Vector(c[0] - 0.5, c[1] - 0.5, c[2] - 0.5), Vector(c[0] + 0.5, c[1] + 0.5, c[2] + 0.5), grey)
    for n, (kind, c) in enumerate(lattice_shapes()):
        add(f"{kind}{n}", unit_cube(c) if kind == "cube" else Sphere.NewSphere(Vector(*c), 0.5, grey))
    add("floor", Cube.NewCube(Vector(*FLOOR[0]), Vector(*FLOOR[1]), grey))
    add("light", Sphere.NewSphere(Vector(*LIGHT[:3]), LIGHT[3], Material.LightMaterial(Colour.White, 20)))
    add("moved_sphere", TransformedShape.NewTransformedShape(Sphere.NewSphere(Vector(0, 0, 0), 0.5, grey),
                                                             Matrix.TranslateM(Vector(*MOVED_SPHERE))))
    turn = Matrix.RotateM(Vector(0, 0, 1), math.pi / 2)        # cos = 6e-17, not 0
    assert np.allclose(turn.m[:3, :3] @ np.array([0.0, -4.0, 0.0]), TURNED_CUBE)
    add("turned_cube", TransformedShape.NewTransformedShape(unit_cube((0.0, -4.0, 0.0)), turn))
    camera = Camera.LookAt(Vector(8, 8, 6), Vector(0, 0, 0), Vector(0, 0, 1), 45)
    return s, camera, DefaultSampler.NewSampler(4, 3), names


def _pick(rng, kind, n):
    c = np.array([c for k, c in lattice_targets() if kind is None or k == kind], f32)
    return c[rng.integers(0, len(c), n)]


def _start(rng, n):
    """Distances from a centre to an axis-aligned ray's origin: between two lattice shapes, or outside the lattice."""
    return np.where(rng.random(n) < 0.5, rng.uniform(0.8, 0.95, n), rng.uniform(7.0, 9.0, n)).astype(f32)


def lattice_rays(n=60, seed=11):
    """The analytic families, n rays each (the tangent families n for each of the three offsets)."""
    rng = np.random.default_rng(seed)
    idx = np.arange(n)
    parts = []

    def axis_ray(c, offset_axis_shift=None, offset=None, second=None):
        axis, sign = idx % 3, np.where((idx // 3) % 2 == 0, f32(1), f32(-1))
        d = np.zeros((n, 3), f32)
        d[idx, axis] = sign
        o = c.copy()
        o[idx, axis] = (c[idx, axis] - sign * _start(rng, n)).astype(f32)
        if offset is not None:
            b = (axis + 1 + offset_axis_shift) % 3
            o[idx, b] = (c[idx, b] + offset).astype(f32)
            if second is not None:
                b2 = (axis + 2 - offset_axis_shift) % 3
                o[idx, b2] = (c[idx, b2] + second).astype(f32)
        return o, d

    parts.append((*axis_ray(_pick(rng, None, n)), "axis_centre"))
    side = lambda: np.where(rng.random(n) < 0.5, f32(1), f32(-1))
    for name, off in (("tangent_r", R), ("tangent_below", np.nextafter(R, f32(0))), ("tangent_above", np.nextafter(R, f32(np.inf)))):
        parts.append((*axis_ray(_pick(rng, "sphere", n), (idx // 6) % 2, side() * off), name))
    # origins on a surface: a sphere's (centre + r u, rounded) or a cube's face (that coordinate exact)
    c = _pick(rng, "sphere", n)
    o = (c + R * _unit(rng, n)).astype(f32)
    c2 = _pick(rng, "cube", n)
    o2 = (c2 + rng.uniform(-0.5, 0.5, (n, 3))).astype(f32)
    o2[idx, idx % 3] = (c2[idx, idx % 3] + side() * R).astype(f32)
    o[1::2] = o2[1::2]
    parts.append((o, _unit(rng, n).astype(f32), "origin_on_surface"))
    parts.append((_pick(rng, None, n), _unit(rng, n).astype(f32), "origin_at_centre"))
    # in a cube's face plane: the offset axis carries +-r exactly, the third axis a random offset inside the face
    c = _pick(rng, "cube", n)
    parts.append((*axis_ray(c, (idx // 6) % 2, side() * R, rng.uniform(-0.45, 0.45, n).astype(f32)), "face_axis"))
    c = _pick(rng, "cube", n)
    b = idx % 3
    u = _unit(rng, n)
    u[idx, b] = 0.0
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    through = c + rng.uniform(-0.45, 0.45, (n, 3))
    o = (through - u * rng.uniform(0.8, 3.0, (n, 1))).astype(f32)
    o[idx, b] = (c[idx, b] + side() * R).astype(f32)
    parts.append((o, u.astype(f32), "face_oblique"))
    c = _pick(rng, "cube", n)
    parts.append((*axis_ray(c, (idx // 6) % 2, side() * R, side() * R), "cube_edge"))
    c = _pick(rng, "cube", n)
    corner = (c + np.where(rng.random((n, 3)) < 0.5, R, -R)).astype(f32)
    out = corner - c
    w = _unit(rng, n)
    w = np.where((w * out).sum(axis=1, keepdims=True) < 0, -w, w)      # from the corner's own side
    o = (corner + w * rng.uniform(0.8, 3.0, (n, 1))).astype(f32)
    d = corner.astype(np.float64) - o.astype(np.float64)
    parts.append((o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32), "cube_corner"))
    return _finish(parts)


# ------------------------------------------------------------------ the fp32 slab test of a triangle's own box
def pad_box(v1, v2, v3):
    """pad_box of each triangle (pt_bvh.h): lo - e, hi + e with e = max(|lo|, |hi|) * 2e-6f + 1e-30f, in fp32."""
    lo = np.minimum(np.minimum(v1, v2), v3).astype(f32)
    hi = np.maximum(np.maximum(v1, v2), v3).astype(f32)
    e = (np.maximum(np.abs(lo), np.abs(hi)) * f32(2.0e-6)).astype(f32) + f32(1e-30)
    return (lo - e).astype(f32), (hi + e).astype(f32)


def slab1(lo, hi, o, d, tmax):
    """slab1 of pt_device.h in numpy float32, NaN dropped as fminf / fmaxf drop it: True where the box is entered."""
    with np.errstate(all="ignore"):
        invd = (f32(1) / d).astype(f32)
        t1, t2 = ((lo - o) * invd).astype(f32), ((hi - o) * invd).astype(f32)
        near, far = np.fmin(t1, t2), np.fmax(t1, t2)
        tn = np.fmax(np.fmax(near[:, 0], near[:, 1]), np.fmax(near[:, 2], f32(0)))
        tf = np.fmin(np.fmin(far[:, 0], far[:, 1]), np.fmin(far[:, 2], tmax.astype(f32)))
        return tn <= (tf * f32(1.0000005)).astype(f32)


def tmax_bound(t):
    """tmax_bound of pt_device.h: the hit distance rounded up to fp32."""
    f = t.astype(f32)
    return np.where(f.astype(np.float64) < t, np.nextafter(f, f32(np.inf)), f).astype(f32)


# ------------------------------------------------------------------ the scenes and the reference
MESH_POSES = ["rest", "flat", "translate", "huge", "scale", "tiny"]
SECOND_INSTANCE = (1.5, 0.0, 2.5)     # the small mesh again, a quarter turn about z and then moved here


def posed_scene(name):
    """(scene tuple, [v1, v2, v3] of all its triangles, rays) of test_gpu_refit.py's grid scene uploaded in a pose."""
    from test_gpu_refit import make_scene, pose, rest_arrays
    arrs = rest_arrays()
    tris = arrs[:3] if name == "rest" else pose(name, arrs)[:3]
    return make_scene(list(tris) + arrs[3:]), tris, mesh_rays(*tris, flat=name == "flat")


def instance_matrices():
    turn = Matrix.TranslateM(Vector(*SECOND_INSTANCE)).Mul(Matrix.RotateM(Vector(0, 0, 1), math.pi / 2))
    return [Matrix.TranslateM(Vector(0, 0, 3)), turn]


def instanced_scene(split=False):
    """The grid scene with its instanced small mesh (make_scene(instanced=True)) and a second instance of the same
    Mesh under a quarter turn; rays at the grid and at both instances.
    The oracle's loop over every shape still walks an instance's own k-d tree.  split=True gives the scene for which
    it is a loop over the instances' triangles too: every instance as two TransformedShapes of half the mesh each,
    fewer than the eight shapes a tree splits at, so each tree is one leaf; two zero-area triangles (never hit:
    det = 0) far out at opposite corners keep the tree's box test from deciding anything."""
    from ptsharp_amd.scene import Mesh
    from test_gpu_refit import make_scene, rest_arrays
    arrs = rest_arrays()
    st = make_scene(arrs, instanced=True)
    first = st[0].Shapes[-1]
    small = first.Shape
    mats = instance_matrices()
    assert np.array_equal(first.Matrix.m, mats[0].m)
    if split:
        st[0].Shapes.pop()
        far = np.repeat(np.array([[-50, -50, -50], [50, 50, 50]], f32), 1, axis=0)
        for m in mats:
            for half in (slice(0, 4), slice(4, 8)):
                v = [np.concatenate([a[half], far]) for a in (small.v1, small.v2, small.v3)]
                nrm = [np.concatenate([a[half], np.zeros((2, 3), f32)]) for a in (small.n1, small.n2, small.n3)]
                st[0].Add(TransformedShape.NewTransformedShape(Mesh(*v, *nrm), m))
    else:
        st[0].Add(TransformedShape.NewTransformedShape(small, mats[1]))
    parts = [mesh_rays(*arrs[:3], n=100)]
    for i, m in enumerate(mats):
        o, d, fam = instance_rays(small.v1, small.v2, small.v3, m.m, n=100, seed=9 + i)
        parts.append((o, d, np.array([f"instance{i}_{f}" for f in fam], dtype=object)))
    o, d, fam = (np.concatenate([p[k] for p in parts]) for k in range(3))
    return st, arrs[:3], (np.ascontiguousarray(o, f32), np.ascontiguousarray(d, f32), fam)


def oracle_hits(oscene, o, d, brute=True):
    """or_intersect of every ray: (t [n] float64, kind [n] int32, index [n] int32); brute: the loop over every
    shape, else the reference's k-d tree walk."""
    t, k, x = np.empty(len(o), np.float64), np.empty(len(o), np.int32), np.empty(len(o), np.int32)
    for i in range(len(o)):
        t[i], k[i], x[i] = oscene.intersect(o[i], d[i], brute=brute)
    return t, k, x


def oracle_any_nearer(oscene, o, d, tmax):
    return np.array([oscene.any_nearer(o[i], d[i], float(tmax[i])) for i in range(len(o))], np.int32)


def occlusion_bounds(t):
    """The t_max of the pt_occluded checks: at the hit, one ulp past it, half and twice it; 5 and 1e9 for a miss."""
    hit = t < 1e9
    return {"at_hit": np.where(hit, t, 5.0), "past_hit": np.where(hit, np.nextafter(t, np.inf), 1e9),
            "half": np.where(hit, t / 2, 5.0), "twice": np.where(hit, 2 * t, 1e9)}


SCENES = MESH_POSES + ["instanced", "lattice"]


def raw_case(name):
    """(the scene tuple a renderer uploads, the Scene whose loop over every shape is the reference, (o, d, family))
    of one of SCENES, every generated ray.  Only `instanced` has two scenes: see instanced_scene."""
    if name == "lattice":
        s, camera, sampler, _ = lattice_scene()
        return (s, camera, sampler), s, lattice_rays()
    if name == "instanced":
        st, _, rays = instanced_scene()
        return st, instanced_scene(split=True)[0][0], rays
    st, _, rays = posed_scene(name)
    return st, st[0], rays


def nearer_than_own_box(oscene, o, d):
    """True for the rays whose triangle hit in the oracle's loop lies nearer than the fp32 slab test enters the
    triangle's own padded box once boxes are culled at that hit's own t.  The t of a grazing hit carries 1e-5 of
    fp32 error, the box 2e-6 of padding: such a hit is found only if no neighbour a few ulp farther is found first,
    so the loop's answer is not one a BVH that culls by distance can promise."""
    t, k, x = oracle_hits(oscene, o, d, brute=True)
    m = np.flatnonzero(k == 3)
    flat = oscene.flat
    lo, hi = pad_box(flat.tri_v1[x[m]], flat.tri_v2[x[m]], flat.tri_v3[x[m]])
    out = np.zeros(len(o), bool)
    out[m] = ~slab1(lo, hi, o[m], d[m], tmax_bound(t[m]))
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """raw_case without the rays of nearer_than_own_box (tests/test_degenerate_rays_ref.py bounds and prints them):
    there the expected value is ill defined, and the input is changed rather than the assertion."""
    import oracle_lib
    st, ref_scene, (o, d, fam) = raw_case(name)
    keep = ~nearer_than_own_box(oracle_lib.OracleScene(ref_scene), o, d)
    return st, ref_scene, (np.ascontiguousarray(o[keep]), np.ascontiguousarray(d[keep]), fam[keep])
