"""Helpers of tests/test_gpu_look.py (pt_update_materials, pt_update_textures): the scenes, built from a table of named
materials so that an edited scene comes from its builder and the edit alone, the edits, and the comparisons.

look_scene: one of every shape the light test treats differently, each with a material of its own, in this Scene.Shapes
order: a floor cube, a ball (sphere), a box (cube), the lamp (a sphere, the scene's only light), a wall (plane), a
loose triangle, two instances of one mesh, a Volume of five windows (MaterialAt(origin) is its first window's), an SDF
shape.  The ball, the box, the floor lie before the lamp in Scene.Shapes.  textures: "all" (the floor and the ball
textured, an environment map), "env" (only the environment map: no material is textured, so the routed shade is on)
or None.  ball, tri: where the ball and the loose triangle are (test 3 moves
them).  instances=False: the mesh once at top level instead.
many_lights: a floor and 17 spheres, 16 of them lit."""
from __future__ import annotations

import numpy as np

from ptsharp_amd import Renderer, TransformedShape, Vector, _abi, scenes
from ptsharp_amd.geometry import Box, Colour, Matrix, Util
from ptsharp_amd.renderer import Buffer
from ptsharp_amd.scene import (Camera, ColorTexture, Cube, DefaultSampler, LightMode, Material, Plane, Scene, SDFShape,
                               Sphere, SphereSDF, TransformSDF, Triangle, Volume, VolumeWindow)

F = np.float32
W, H, SPP, SEED = 64, 48, 2, 31
TEX_SIZES = {"env": (67, 33), "floor": (3, 5), "ball": (2, 2)}   # width, height
BALL, BALL_MOVED = (-1.6, 0.7, 0.4), (-1.1, 1.0, 0.9)
TRI = ((-3, 0.01, -2), (3, 0.01, -2), (0, 2.5, -2.5))
TRI_MOVED = ((-2.5, 0.3, -1.5), (2.5, 0.2, -1.8), (0.2, 2.8, -2.0))


def bytes_image(name, seed, channels=3):
    w, h = TEX_SIZES[name]
    return np.random.default_rng(seed).integers(0, 256, (h, w, channels), dtype=np.uint8)


def texture(name, seed, channels=3):
    """NewTexture().Pow(1.3).MulScalar(0.5) over seeded bytes: the table the issue names."""
    return ColorTexture.NewTexture(bytes_image(name, seed, channels)).Pow(1.3).MulScalar(0.5)


def materials():
    g = Material.GlossyMaterial
    m = {"floor": Material.DiffuseMaterial(Colour(0.8, 0.8, 0.8)), "lamp": Material.LightMaterial(Colour.White, 10),
         "ball": g(Colour.HexColor(0x334D5C), 1.5, Util.Radians(10)), "box": Material.DiffuseMaterial(Colour(0.9, 0.3, 0.2)),
         "wall": Material.DiffuseMaterial(Colour(0.5, 0.6, 0.5)), "tri": Material.DiffuseMaterial(Colour(0.2, 0.4, 0.9)),
         "mesh": g(Colour.HexColor(0xBEDB39), 1.4, Util.Radians(10)), "sdf": g(Colour.HexColor(0x468966), F(1.2), Util.Radians(20))}
    for k, c in enumerate((0x004358, 0x1F8A70, 0xBEDB39, 0xFFE11A, 0xFD7400)):
        m[f"w{k}"] = g(Colour.HexColor(c), F(1.3), Util.Radians(0))
    return m


def look_scene(mats=None, env=None, textures="all", ball=BALL, tri=TRI, instances=True, light_mode=LightMode.LightModeRandom,
               tex_seed=0):
    """-> (scene, camera, sampler, names): names maps a material's name to the Material the scene uses, and "tex:<name>"
    to its textures.  mats / env: overrides by name, the edit a fresh upload is to contain."""
    m = materials()
    tex = {n: texture(n, 100 + 7 * k + tex_seed) for k, n in enumerate(TEX_SIZES)} if textures else {}
    if textures == "all":
        m["floor"] = m["floor"].with_(Texture=tex["floor"])
        m["ball"] = m["ball"].with_(Texture=tex["ball"])
    for k, v in (mats or {}).items():
        m[k] = v(m[k], tex) if callable(v) else v
    s = Scene()
    s.Color = Colour(0.25, 0.3, 0.4)
    if textures:
        s.Texture, s.TextureAngle = tex["env"], Util.Radians(30)
    for k, v in (env or {}).items():
        setattr(s, k, tex[v[4:]] if isinstance(v, str) and v.startswith("tex:") else v)
    s.Add(Cube.NewCube(Vector(-12, -1, -12), Vector(12, 0, 12), m["floor"]))
    s.Add(Sphere.NewSphere(Vector(*ball), 0.7, m["ball"]))
    s.Add(Cube.NewCube(Vector(1.0, 0, 0.2), Vector(1.8, 0.8, 1.0), m["box"]))
    s.Add(Sphere.NewSphere(Vector(0, 4.5, 1), 0.8, m["lamp"]))
    s.Add(Plane.NewPlane(Vector(0, 0, -4), Vector(0, 0, 1), m["wall"]))
    s.Add(Triangle.NewTriangle(Vector(*tri[0]), Vector(*tri[1]), Vector(*tri[2]), Vector(0, 0, 0), Vector(1, 0, 0),
                               Vector(0.5, 1, 0), m["tri"]))
    mesh = scenes.blob_mesh(300, seed=21, amplitude=0.15)
    mesh.SetMaterial(m["mesh"])
    mesh.SmoothNormals()
    if not instances:   # the same mesh at top level, in the world BVH: pt_update_triangles serves such a scene
        mesh.FitInside(Box(Vector(-0.5, 0.2, 1.3), Vector(0.1, 0.8, 1.9)), Vector(F(0.5), 0, F(0.5)))
        s.Add(mesh)
    else:
        for at, sc in (((-0.2, 0.5, 1.6), 0.4), ((0.7, 1.7, -0.4), 0.5)):
            s.Add(TransformedShape.NewTransformedShape(mesh, Matrix.TranslateM(Vector(*at)).Mul(Matrix.ScaleM(Vector(sc, sc, sc)))))
    proto = scenes.volume(4, 4, 2)[0].Shapes[0]
    wins = [VolumeWindow(w.Lo, w.Hi, m[f"w{k}"]) for k, w in enumerate(proto.Windows)]
    s.Add(Volume.NewVolume(Box(Vector(1.9, 0.05, -1.7), Vector(3.1, 1.25, -0.5)), scenes.volume_slices(16, 16, 8, 3),
                           F(3.4) / F(0.9765625), wins))
    s.Add(SDFShape.NewSDFShape(TransformSDF.NewTransformSDF(SphereSDF.NewSphereSDF(F(0.35)), Matrix.TranslateM(Vector(-0.9, 0.35, 1.9))),
                               m["sdf"]))
    cam = Camera.LookAt(Vector(0, 2.2, 5), Vector(0, 0.8, 0), Vector(0, 1, 0), 45)
    smp = DefaultSampler.NewSampler(2, 3)
    smp.SetLightMode(light_mode)
    names = dict(m)
    names.update({f"tex:{k}": v for k, v in tex.items()})
    return s, cam, smp, names


def many_lights(lit=16):
    """A floor and 17 small spheres in a ring, each with a material of its own; the first `lit` emit."""
    s = Scene()
    s.Color = Colour(0.05, 0.05, 0.08)
    s.Add(Cube.NewCube(Vector(-12, -1, -12), Vector(12, 0, 12), Material.DiffuseMaterial(Colour(0.8, 0.8, 0.8))))
    names = {}
    for k in range(17):
        a = 2 * np.pi * k / 17
        col = Colour(0.3 + 0.04 * k, 1.0 - 0.03 * k, 0.5)
        names[f"s{k}"] = Material.LightMaterial(col, 4) if k < lit else Material.DiffuseMaterial(col)
        s.Add(Sphere.NewSphere(Vector(2.2 * np.cos(a), 0.3 + 0.05 * k, 2.2 * np.sin(a) - 0.5), 0.25, names[f"s{k}"]))
    cam = Camera.LookAt(Vector(0, 3.5, 5), Vector(0, 0.3, -0.5), Vector(0, 1, 0), 45)
    smp = DefaultSampler.NewSampler(2, 3)
    smp.SetLightMode(LightMode.LightModeAll)
    return s, cam, smp, names


def lit(m, e=6.0):
    return m.with_(Emittance=e)


# name -> (materials override, environment override, textures mode): each value of the first is the new Material, or a
# function (old Material, textures) -> new Material
EDITS = {
    "recolour": ({"ball": lambda m, t: m.with_(Color=Colour(0.9, 0.2, 0.1), Gloss=Util.Radians(35), Index=1.2)}, None, "all"),
    "dim": ({"lamp": lambda m, t: m.with_(Emittance=3.0)}, None, "all"),
    "off": ({"lamp": lambda m, t: m.with_(Emittance=0.0)}, None, "all"),
    "sphere-on": ({"ball": lambda m, t: lit(m)}, None, "all"),
    "cube-on": ({"box": lambda m, t: lit(m)}, None, "all"),
    "plane-on": ({"wall": lambda m, t: lit(m, 2.0)}, None, "all"),
    "triangle-on": ({"tri": lambda m, t: lit(m)}, None, "all"),
    "instance-on": ({"mesh": lambda m, t: lit(m)}, None, "all"),
    "volume-on": ({"w0": lambda m, t: lit(m)}, None, "all"),
    "sdf-on": ({"sdf": lambda m, t: lit(m)}, None, "all"),
    "texture-given": ({"box": lambda m, t: m.with_(Texture=t["env"])}, None, "env"),
    "env-colour": (None, {"Color": Colour(0.9, 0.5, 0.2), "Texture": None}, "all"),
    "env-angle": (None, {"TextureAngle": Util.Radians(140)}, "all"),
    "env-swap": (None, {"Texture": "tex:floor"}, "all"),
    "env-none": (None, {"Texture": None}, "all"),
}


def renderer(st, engine=_abi.ENGINE_WAVEFRONT, w=W, h=H):
    r = Renderer.NewRenderer(st[0], st[1], st[2], w, h, True, device=0)
    r.SamplesPerPixel, r.Seed, r.Engine = SPP, SEED, engine
    return r


def frame(r, reset=True):
    if reset:
        r.ResetBuffer()
    r.RenderParallel()
    b = r.ReadBuffer()
    out = Buffer(r.W, r.H)
    out.M, out.V, out.N = b.M.copy(), b.V.copy(), b.N.copy()
    return out, r.Stats().rays


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def apply(r, st, edit):
    """Renderer.UpdateMaterials with a named edit of st's scene (keys: the scene's own Material objects)."""
    mats, env, _ = EDITS[edit] if isinstance(edit, str) else edit
    names = st[3]
    upd = [(names[k], f(names[k], {n[4:]: v for n, v in names.items() if n.startswith("tex:")})) for k, f in (mats or {}).items()]
    e = None
    if env is not None:
        e = {k: (names[v] if isinstance(v, str) and v.startswith("tex:") else v) for k, v in env.items()}
    return r.UpdateMaterials(upd, env=e)


def fresh_scene(edit, **kw):
    mats, env, textures = EDITS[edit] if isinstance(edit, str) else edit
    return look_scene(mats=mats, env=env, textures=textures, **kw)


def look_words(r):
    """Everything pt_read_materials returns, as comparable values."""
    d = r.ReadMaterials()
    i = d["info"]
    info = (i.num_materials, i.num_textures, i.num_lights, i.lights_lean, i.route, i.shade_route, i.env_texture,
            tuple(i.env_color), i.env_texture_angle)
    return info, bytes(d["materials"])[:i.num_materials * 96], d["light_rows"], d["light_spheres"]


def same_look(a, b, what="", index=True):
    # (the Python FlatScene lists only the textures a material or the environment names: num_textures, info[1], is left
    # out, an edit that lets go of a texture keeps it on the device)
    assert a[0][:1] + a[0][2:] == b[0][:1] + b[0][2:], f"{what}: info {a[0]} vs {b[0]}"
    assert a[1] == b[1], f"{what}: the material rows differ"
    rows_a, rows_b = (a[2], b[2]) if index else (np.delete(a[2], 1, axis=1), np.delete(b[2], 1, axis=1))
    assert np.array_equal(rows_a, rows_b), f"{what}: light rows {a[2].tolist()} vs {b[2].tolist()}"
    assert np.array_equal(bits(a[3]), bits(b[3])), f"{what}: light spheres {a[3].tolist()} vs {b[3].tolist()}"


def geometry_words(r):
    """pt_read_tri_bvh, pt_read_blas, pt_read_volume and the analytic BVH's nodes, records and heavy records."""
    out = list(r.ReadTriBvh()) + list(r.ReadShapeBvh()[:3])
    if r._uploaded.counts_ext[3]:
        out += [a for a in r.ReadBlas() if isinstance(a, np.ndarray)]
    for i in range(r._uploaded.counts_ext[2]):
        v = r.ReadVolume(i)
        out += [v[k] for k in ("info", "data", "windows", "materials", "runs", "cells") if v[k] is not None]
    return out


def same_words(a, b, what=""):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), f"{what}: array {k} differs"
