"""The inputs and the reference of tests/test_gpu_degenerate_rays.py, checked on the CPU before the device is
compared with them.

  1. every family of tests/degenerate_rays.py is what it claims: exact zeros, sign bits, coordinates that are a
     vertex's own bits, origins within twice the extent;
  2. the oracle's loop over every shape (or_intersect brute=1) never answers farther than its k-d tree walk; the
     rays where the two differ are counted per family and printed (DESIGN.md §2 quotes them): they are why the
     loop, not the walk, is the expected value;
  3. every family still hits something: at least half the rays that hit when the floors below were taken;
  4. every triangle the loop hits is hit inside its own padded box by the fp32 slab test (numpy restatements of
     pad_box and slab1), so bit equality is a fair demand of a BVH; with the box culled at the hit's own t that
     fails for a few grazing hits (their t carries 1e-5 of fp32 error and lies before the box): there a BVH finds
     the hit only if it meets no neighbour first, so those rays are taken out of the input (D.case), counted here;
  5. the lattice has no near tie: with the hit shape left out, the next hit is more than 1e-2 t farther;
  6. in the mesh scenes the triangles and the analytic shapes never come within 1e-3 t on a ray that hits both;
  7. the instanced scene: the oracle's loop still walks an instance's own tree, so the reference is the same
     scene with every instance split into meshes too small for a tree; that loop never answers farther.
"""
import functools

import numpy as np
import pytest

import degenerate_rays as D
import oracle_lib as O
from ptsharp_amd import TransformedShape, _abi
from ptsharp_amd.scene import Cube, Scene, Sphere

f32 = np.float32
MISS = 1e9

# Rays of each family that hit something in the oracle's loop when this test was written, halved (check 3).
FLOORS = {'rest': {'axis_vertex': 99,
          'axis_edge': 100,
          'axis_centroid': 100,
          'axis_vertex_nz': 97,
          'axis_edge_nz': 100,
          'axis_centroid_nz': 100,
          'plane_zero': 89,
          'plane_nz': 87,
          'plane_1e-20': 82,
          'plane_-1e-38': 88,
          'plane_1e-45': 85,
          'origin_on_vertex': 56,
          'aimed_at_vertex': 98},
 'flat': {'axis_vertex': 33,
          'axis_edge': 33,
          'axis_centroid': 33,
          'axis_vertex_nz': 33,
          'axis_edge_nz': 33,
          'axis_centroid_nz': 33,
          'plane_zero': 62,
          'plane_nz': 66,
          'plane_1e-20': 63,
          'plane_-1e-38': 62,
          'plane_1e-45': 63,
          'origin_on_vertex': 41,
          'aimed_at_vertex': 99,
          'flat_in_plane': 0},
 'translate': {'axis_vertex': 100,
               'axis_edge': 99,
               'axis_centroid': 100,
               'axis_vertex_nz': 100,
               'axis_edge_nz': 100,
               'axis_centroid_nz': 100,
               'plane_zero': 80,
               'plane_nz': 79,
               'plane_1e-20': 70,
               'plane_-1e-38': 68,
               'plane_1e-45': 76,
               'origin_on_vertex': 14,
               'aimed_at_vertex': 98},
 'huge': {'axis_vertex': 98,
          'axis_edge': 100,
          'axis_centroid': 100,
          'axis_vertex_nz': 98,
          'axis_edge_nz': 99,
          'axis_centroid_nz': 100,
          'plane_zero': 79,
          'plane_nz': 78,
          'plane_1e-20': 70,
          'plane_-1e-38': 70,
          'plane_1e-45': 75,
          'origin_on_vertex': 20,
          'aimed_at_vertex': 95},
 'scale': {'axis_vertex': 98,
           'axis_edge': 99,
           'axis_centroid': 100,
           'axis_vertex_nz': 98,
           'axis_edge_nz': 100,
           'axis_centroid_nz': 100,
           'plane_zero': 70,
           'plane_nz': 73,
           'plane_1e-20': 69,
           'plane_-1e-38': 65,
           'plane_1e-45': 69,
           'origin_on_vertex': 65,
           'aimed_at_vertex': 98},
 'tiny': {'axis_vertex': 33,
          'axis_edge': 33,
          'axis_centroid': 33,
          'axis_vertex_nz': 33,
          'axis_edge_nz': 33,
          'axis_centroid_nz': 33,
          'plane_zero': 32,
          'plane_nz': 32,
          'plane_1e-20': 38,
          'plane_-1e-38': 34,
          'plane_1e-45': 35,
          'origin_on_vertex': 40,
          'aimed_at_vertex': 58},
 'instanced': {'axis_vertex': 49,
               'axis_edge': 49,
               'axis_centroid': 50,
               'axis_vertex_nz': 49,
               'axis_edge_nz': 49,
               'axis_centroid_nz': 50,
               'plane_zero': 41,
               'plane_nz': 45,
               'plane_1e-20': 36,
               'plane_-1e-38': 40,
               'plane_1e-45': 40,
               'origin_on_vertex': 26,
               'aimed_at_vertex': 49,
               'instance0_axis_vertex': 37,
               'instance0_axis_edge': 47,
               'instance0_axis_centroid': 50,
               'instance0_axis_vertex_nz': 36,
               'instance0_axis_edge_nz': 46,
               'instance0_axis_centroid_nz': 50,
               'instance0_plane_zero': 31,
               'instance0_plane_nz': 30,
               'instance0_plane_1e-20': 34,
               'instance0_plane_-1e-38': 28,
               'instance0_plane_1e-45': 30,
               'instance0_origin_on_vertex': 29,
               'instance0_aimed_at_vertex': 29,
               'instance1_axis_vertex': 37,
               'instance1_axis_edge': 47,
               'instance1_axis_centroid': 50,
               'instance1_axis_vertex_nz': 40,
               'instance1_axis_edge_nz': 45,
               'instance1_axis_centroid_nz': 50,
               'instance1_plane_zero': 38,
               'instance1_plane_nz': 35,
               'instance1_plane_1e-20': 33,
               'instance1_plane_-1e-38': 32,
               'instance1_plane_1e-45': 32,
               'instance1_origin_on_vertex': 29,
               'instance1_aimed_at_vertex': 37},
 'lattice': {'axis_centre': 30,
             'tangent_r': 19,
             'tangent_below': 22,
             'tangent_above': 17,
             'origin_on_surface': 22,
             'origin_at_centre': 20,
             'face_axis': 10,
             'face_oblique': 10,
             'cube_edge': 8,
             'cube_corner': 21}}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(o, d, family, loop t / kind / index, walk t, the reference OracleScene) of a scene, computed once."""
    st, ref_scene, (o, d, fam) = D.case(name)
    os_ = O.OracleScene(ref_scene)
    t, k, x = D.oracle_hits(os_, o, d, brute=True)
    tree_scene = os_ if name != "instanced" else O.OracleScene(st[0])   # the walk of the scene as it is uploaded
    tt, _, _ = D.oracle_hits(tree_scene, o, d, brute=False)
    return o, d, fam, t, k, x, tt, os_


def families(fam):
    return list(dict.fromkeys(fam.tolist()))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def rows(a, cols):
    """The set of the rows of a[:, cols] as bytes: membership is bit equality."""
    return {r.tobytes() for r in np.ascontiguousarray(a[:, cols], f32)}


# ------------------------------------------------------------------ 1. the generators' claims
@pytest.mark.parametrize("name", D.MESH_POSES)
def test_mesh_families_are_what_they_claim(name):
    _, tris, (o, d, fam) = D.posed_scene(name)
    verts = np.concatenate(tris)
    ext = D.mesh_extent(*tris)[1]
    assert set(families(fam)) == set(D.MESH_FAMILIES) | ({"flat_in_plane"} if name == "flat" else set())
    assert all((fam == f).sum() >= 200 for f in families(fam))
    assert np.isfinite(o).all() and np.isfinite(d).all() and (d != 0).any(axis=1).all()
    lo, hi = verts.min(axis=0).astype(np.float64), verts.max(axis=0).astype(np.float64)
    away = np.maximum(np.maximum(lo - o, o - hi), 0).max(axis=1)
    assert (away <= 2.0 * ext * (1 + 1e-6)).all(), "an origin farther than twice the extent from the geometry"
    others = {0: [1, 2], 1: [0, 2], 2: [0, 1]}
    pairs = {a: rows(verts, others[a]) for a in range(3)}
    coords = {a: set(bits(verts[:, a]).tolist()) for a in range(3)}
    tri = np.stack(tris)   # [3, T, 3]
    mids = np.concatenate([((tri[c] + tri[(c + 1) % 3]) * f32(0.5)).astype(f32) for c in range(3)])
    cents = ((tri[0] + tri[1] + tri[2]) / f32(3)).astype(f32)
    through = {"axis_vertex": pairs, "axis_edge": {a: rows(mids, others[a]) for a in range(3)},
               "axis_centroid": {a: rows(cents, others[a]) for a in range(3)}}
    for base, sets in through.items():
        for nz in (False, True):
            m = fam == base + ("_nz" if nz else "")
            oo, dd = o[m], d[m]
            axis = np.abs(dd).argmax(axis=1)
            assert (np.abs(dd[np.arange(len(dd)), axis]) == 1).all() and ((dd == 0).sum(axis=1) == 2).all()
            assert {(int(a), float(s)) for a, s in zip(axis, dd[np.arange(len(dd)), axis])} == {(a, s) for a in range(3) for s in (1.0, -1.0)}
            negzeros = (np.signbit(dd) & (dd == 0)).sum(axis=1)
            assert (negzeros == (1 if nz else 0)).all()
            for i in range(len(oo)):
                assert oo[i, others[axis[i]]].tobytes() in sets[int(axis[i])], f"{base}: ray {i} is not through one"
    for fname, value in D.PLANE_VALUES.items():
        m = np.flatnonzero(fam == fname)
        axis = np.arange(len(m)) % 3
        assert (bits(d[m, axis]) == bits(np.array([value]))[0]).all(), fname
        assert all(int(b) in coords[int(a)] for a, b in zip(axis, bits(o[m, axis]))), fname
        assert ((d[m] != 0).sum(axis=1) >= 2).all()
    with np.errstate(all="ignore"):   # the reciprocals the slab tests form: -inf, inf, and a finite one that overflows times 4
        inv = {k: f32(1) / v for k, v in D.PLANE_VALUES.items()}
        assert inv["plane_nz"] == -np.inf and inv["plane_1e-45"] == np.inf and inv["plane_zero"] == np.inf
        assert np.isfinite(inv["plane_-1e-38"]) and np.isinf(f32(4) * inv["plane_-1e-38"]) and np.isfinite(f32(1e6) * inv["plane_1e-20"])
    whole = rows(verts, [0, 1, 2])
    assert all(r.tobytes() in whole for r in o[fam == "origin_on_vertex"])
    m = fam == "aimed_at_vertex"
    to = verts[None, :, :].astype(np.float64) - o[m][:, None, :]
    sin = np.linalg.norm(np.cross(to, d[m][:, None, :].astype(np.float64)), axis=2) / np.linalg.norm(to, axis=2)
    assert (sin.min(axis=1) < 1e-6).all()
    if name == "flat":
        m = fam == "flat_in_plane"
        assert (bits(o[m, 2]) == 0).all() and (bits(d[m, 2]) == 0).all() and (verts[:, 2] == 0).all()


def test_instance_rays_aim_at_both_instances():
    xf = [s for s in D.instanced_scene()[0][0].Shapes if isinstance(s, TransformedShape)]
    assert len(xf) == 2 and xf[0].Shape is xf[1].Shape
    turn = xf[1].Matrix.m
    assert 0 < abs(turn[0, 0]) < 1e-16 and abs(turn[0, 1]) == 1.0     # a quarter turn: cos = 6e-17, not 0
    o, d, fam, t, k, x, tt, os_ = reference("instanced")
    for i in (0, 1):
        m = np.char.startswith(fam.astype(str), f"instance{i}_")
        assert m.sum() >= 1290 and (k[m] == _abi.SHAPE_TRANSFORMED).sum() > 500, f"instance {i} is hardly hit"


def test_lattice_families_are_what_they_claim():
    o, d, fam = D.lattice_rays()
    assert families(fam) == D.LATTICE_FAMILIES
    targets = D.lattice_targets()
    centres = np.array([c for _, c in targets], f32)
    spheres = np.array([c for k, c in targets if k == "sphere"], f32)
    cubes = np.array([c for k, c in targets if k == "cube"], f32)
    axis_aligned = np.isin(fam, ["axis_centre", "tangent_r", "tangent_below", "tangent_above", "face_axis", "cube_edge"])
    assert ((d[axis_aligned] == 0).sum(axis=1) == 2).all() and (np.abs(d[axis_aligned]).max(axis=1) == 1).all()
    assert not (np.signbit(d[axis_aligned]) & (d[axis_aligned] == 0)).any()

    def offsets(i, cs):
        """The two axes perpendicular to the axis-aligned ray i, and every centre of cs on them ([len(cs), 2])."""
        perp = np.flatnonzero(d[i] == 0)
        return perp, cs[:, perp]
    for i in np.flatnonzero(fam == "axis_centre"):
        perp, c = offsets(i, centres)
        assert (c == o[i, perp]).all(axis=1).any()
    for fname, off in (("tangent_r", D.R), ("tangent_below", np.nextafter(D.R, f32(0))), ("tangent_above", np.nextafter(D.R, f32(np.inf)))):
        exact = 0
        for i in np.flatnonzero(fam == fname):
            perp, c = offsets(i, spheres)
            want = [np.stack([(c[:, 0] + s * off).astype(f32), c[:, 1]], 1) for s in (1, -1)] + \
                   [np.stack([c[:, 0], (c[:, 1] + s * off).astype(f32)], 1) for s in (1, -1)]
            hit = [(bits(w) == bits(o[i, perp])).all(axis=1) for w in want]
            assert np.any(hit), f"{fname}: ray {i} is not offset from a sphere's centre by {off!r}"
            exact += int(any(abs(float(v)) == float(off) for v in o[i, perp]))
        assert exact >= 5, f"{fname}: only {exact} rays carry the offset itself (a centre coordinate of 0)"
    m = fam == "origin_at_centre"
    assert all((centres == r).all(axis=1).any() for r in o[m])
    for i in np.flatnonzero(fam == "origin_on_surface"):
        on_sphere = np.abs(np.linalg.norm(spheres.astype(np.float64) - o[i], axis=1) - 0.5).min() < 1e-6
        off = np.abs(cubes - o[i])
        on_cube = ((off == 0.5).any(axis=1) & (off <= 0.5).all(axis=1)).any()
        assert on_sphere or on_cube
    for fname, exact_axes in (("face_axis", 1), ("face_oblique", 1), ("cube_edge", 2)):
        for i in np.flatnonzero(fam == fname):
            off = np.abs(cubes - o[i])                       # exact: centres are integers, the offsets +-0.5
            in_plane = (off == 0.5) & (d[i] == 0)
            assert (in_plane.sum(axis=1) >= exact_axes).any(), f"{fname}: ray {i}"
        if fname == "face_oblique":
            assert ((d[fam == fname] == 0).sum(axis=1) == 1).all()
    m = fam == "cube_corner"
    corners = np.concatenate([cubes + (np.array(s, f32) * 2 - 1) * D.R for s in np.ndindex(2, 2, 2)])
    to = corners[None].astype(np.float64) - o[m][:, None, :]
    sin = np.linalg.norm(np.cross(to, d[m][:, None, :].astype(np.float64)), axis=2) / np.linalg.norm(to, axis=2)
    assert (sin.min(axis=1) < 1e-6).all()


# ------------------------------------------------------------------ 2, 3. the loop against the walk; hit floors
@pytest.mark.parametrize("name", D.SCENES)
def test_the_loop_is_never_farther_than_the_walk_and_every_family_hits(name):
    o, d, fam, t, k, x, tt, _ = reference(name)
    assert (t <= tt).all(), f"the loop over every shape answers farther than the tree on rays {np.flatnonzero(t > tt)[:5]}"
    print(f"\n{name}: rays where the k-d tree walk differs from the loop over every shape, and hits, per family")
    for f in families(fam):
        m = fam == f
        differ, hits = int((t[m] != tt[m]).sum()), int((t[m] < MISS).sum())
        gap = np.abs(tt[m] - t[m])[(t[m] != tt[m]) & (tt[m] < MISS)]
        print(f"  {f:28s} {m.sum():4d} rays, {hits:4d} hit, {differ:3d} differ"
              + (f" (the walk farther by {gap.min():.1e} .. {gap.max():.1e})" if gap.size else "")
              + (f", {int(((tt[m] >= MISS) & (t[m] < MISS)).sum())} hits missed by the walk" if differ else ""))
        assert hits >= FLOORS[name][f], f"{name} {f}: {hits} rays hit, the floor is {FLOORS[name][f]}"
    if name == "tiny":
        assert not (k == _abi.SHAPE_TRIANGLE).any()      # every triangle test rejects on |det| < EPS
    if name == "flat":
        assert (t[fam == "flat_in_plane"] >= MISS).all()   # det = 0 in the mesh's own plane, and the floor is never met


# ------------------------------------------------------------------ 4. a hit triangle's own padded box
@pytest.mark.parametrize("name", D.MESH_POSES + ["instanced"])
def test_every_triangle_hit_enters_its_own_padded_box(name):
    o, d, fam, t, k, x, _, os_ = reference(name)
    m = np.flatnonzero(k == _abi.SHAPE_TRIANGLE)
    assert name == "tiny" or m.size > 500
    flat = os_.flat
    lo, hi = D.pad_box(flat.tri_v1[x[m]], flat.tri_v2[x[m]], flat.tri_v3[x[m]])
    inside = D.slab1(lo, hi, o[m], d[m], D.tmax_bound(np.full(m.size, MISS)))
    assert inside.all(), f"{(~inside).sum()} of {m.size} triangle hits lie outside their own padded box, first ray {m[~inside][:5]}"


@pytest.mark.parametrize("name", D.SCENES)
def test_few_hits_lie_nearer_than_their_own_box(name):
    st, ref_scene, (o, d, fam) = D.raw_case(name)
    out = D.nearer_than_own_box(O.OracleScene(ref_scene), o, d)
    print(f"\n{name}: {out.sum()} of {len(o)} rays hit a triangle nearer than its own padded box is entered at that t: "
          f"{dict((f, int((out & (fam == f)).sum())) for f in families(fam) if (out & (fam == f)).any())}")
    assert out.sum() <= len(o) // 100, "more than 1 % of the rays are taken out: change the family"
    kept = D.case(name)[2]
    assert len(kept[0]) == len(o) - out.sum() and np.array_equal(kept[0], o[~out]) and np.array_equal(kept[1], d[~out])


# ------------------------------------------------------------------ 5. no near ties on the lattice
def test_the_lattice_has_no_near_tie():
    o, d, fam, t, k, x, _, _ = reference("lattice")
    names = D.lattice_scene()[3]
    runner_up = np.full(len(o), np.nan)
    owners = np.zeros(len(o), np.int32)
    for name in names:
        without, _, _ = D.oracle_hits(O.OracleScene(D.lattice_scene(without=name)[0]), o, d, brute=True)
        changed = without != t
        assert (without[changed] > t[changed]).all()
        runner_up[changed] = without[changed]
        owners += changed
    hit = t < MISS
    assert (owners[hit] == 1).all(), f"rays whose hit is shared by two shapes bit for bit: {np.flatnonzero(hit & (owners != 1))[:5]}"
    assert (owners[~hit] == 0).all()
    near = hit & ~(runner_up > t * (1 + 1e-2))
    assert not near.any(), (f"{near.sum()} of {hit.sum()} hitting rays have a second shape within 1e-2 t: "
                            f"{[(int(i), fam[i], t[i], runner_up[i]) for i in np.flatnonzero(near)[:5]]}")
    print(f"\nlattice: {hit.sum()} hitting rays of {len(o)}, none with a second shape within 1e-2 t")


# ------------------------------------------------------------------ 6. triangles against analytic shapes
@pytest.mark.parametrize("name", D.MESH_POSES + ["instanced"])
def test_triangles_and_analytic_shapes_never_nearly_tie(name):
    st, ref_scene, (o, d, fam) = D.case(name)
    parts = [Scene(), Scene()]
    for s in ref_scene.Shapes:
        parts[isinstance(s, (Cube, Sphere))].Add(s)
    assert len(parts[1].Shapes) == 2 and len(parts[0].Shapes) >= 4
    (tt, _, _), (ta, _, _) = (D.oracle_hits(O.OracleScene(p), o, d, brute=True) for p in parts)
    both = (tt < MISS) & (ta < MISS)
    near = both & (np.abs(tt - ta) <= 1e-3 * np.minimum(tt, ta))
    assert not near.any(), f"{near.sum()} rays hit a triangle and an analytic shape within 1e-3 t: {np.flatnonzero(near)[:5]}"
    whole = reference(name)[3]
    assert np.array_equal(whole, np.minimum(tt, ta))


# ------------------------------------------------------------------ 7. the instanced scene's reference
def test_the_split_instances_are_the_loop_over_their_triangles():
    o, d, fam, t, k, x, _, _ = reference("instanced")
    st = D.case("instanced")[0]
    as_uploaded, ku, _ = D.oracle_hits(O.OracleScene(st[0]), o, d, brute=True)    # an instance through its own tree
    assert (t <= as_uploaded).all()
    differ = t != as_uploaded
    print(f"\ninstanced: {differ.sum()} of {len(o)} rays where an instance's own tree differs from the loop over its "
          f"triangles: {dict((f, int((differ & (fam == f)).sum())) for f in families(fam) if (differ & (fam == f)).any())}")
    assert not differ[~np.char.startswith(fam.astype(str), "instance")].any()
    assert (k[t < MISS] == ku[t < MISS])[~differ[t < MISS]].all()
