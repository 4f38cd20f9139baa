"""pt_update_materials and pt_update_textures on the GPU: the look of the uploaded scene edited in place.

  1. word for word: after an edit pt_read_materials (the material rows, the lights in order, the flags, the
     environment) and pt_read_shape_bvh's lights equal those of a second context that uploaded the edited scene, built
     from its builder and the edit alone; pt_read_tri_bvh, pt_read_blas, pt_read_volume and the analytic BVH are as
     before the call;
  2. renders on both engines against that fresh upload bit for bit and against the oracle on the mirrored scene within
     tests/parity.py's bar, the frame before the edit differing from the one after it (on the CPU the oracle alone
     shows between 129 and 3,010 of 3,072 pixels changed for every edit here); a shape before the lamp in Scene.Shapes
     switched on under both light modes; 16 lights becoming 17 and 16 again; a texture slot given and taken away; on
     the routed test scene an SDF shape and a transformed Volume lit and unlit (route 1 -> 0 -> 1); TransformedShapes
     over spheres and over a cube lit;
  3. after motion: a sphere moved by pt_update_shapes and a loose triangle moved by pt_update_triangles, then both lit;
     a further move and a pose move the new lights; pt_update_volumes after a Volume was lit;
  4. textures: RGB8 and RGBA8 images of 2x2, 3x5 and 67x33 decoded on the device equal the host's Data bit for bit, a
     NULL entry is untouched, an F64 update, renders as in 2;
  5. an edit between two passes of one accumulation;
  6. pt_intersect_hits' albedo, material and gloss after an edit;
  7. every refusal, each followed by the same read-backs and one render.
Scenes and helpers: tests/look_ref.py.  Frames are 64x48 at 2 spp."""
import ctypes as C

import numpy as np
import pytest

import look_ref as L
import oracle_lib as O
from parity import check, same_buffer
from ptsharp_amd import Renderer, TransformedShape, _abi, scenes
from ptsharp_amd.geometry import Colour, Matrix, Util  # noqa: F401
from ptsharp_amd.renderer import Buffer
from ptsharp_amd.scene import ColorTexture, LightMode, SDFShape

pytestmark = pytest.mark.gpu

ENGINES = pytest.mark.parametrize("engine", [_abi.ENGINE_MEGAKERNEL, _abi.ENGINE_WAVEFRONT], ids=["mega", "wavefront"])
# what each edit does to the list and the flags: (num_lights, lights_lean, shade_route) after it
EXPECT = {"recolour": (1, 1, 0), "dim": (1, 1, 0), "off": (0, 1, 0), "sphere-on": (2, 1, 0), "cube-on": (2, 1, 0),
          "plane-on": (2, 1, 0), "triangle-on": (2, 1, 0), "instance-on": (1, 1, 0), "volume-on": (2, 0, 0),
          "sdf-on": (2, 0, 0), "texture-given": (1, 1, 0), "env-colour": (1, 1, 0), "env-angle": (1, 1, 0),
          "env-swap": (1, 1, 0), "env-none": (1, 1, 0)}


def oracle(st):
    return O.render(O.OracleScene(st[0]), st[1], st[2], L.W, L.H, L.SPP, seed=L.SEED)


# ------------------------------------------------------------------ 1. word for word
@pytest.mark.parametrize("edit", list(L.EDITS))
def test_word_for_word(gpu, edit):
    tex = L.EDITS[edit][2]
    st = L.look_scene(textures=tex)
    r = L.renderer(st)
    try:
        geo0, look0 = L.geometry_words(r), L.look_words(r)
        assert look0[0][2:4] == (1, 1) and look0[0][5] == (1 if tex == "env" else 0)   # one light, lean; the routed shade
        assert L.apply(r, st, edit) == 0.0
        got = L.look_words(r)
        assert got[0][2:4] == EXPECT[edit][:2] and got[0][5] == EXPECT[edit][2], got[0]
        fresh = L.renderer(L.fresh_scene(edit))
        try:
            L.same_look(got, L.look_words(fresh), edit)
            assert np.array_equal(L.bits(r.ReadShapeBvh()[3]), L.bits(fresh.ReadShapeBvh()[3])), "pt_read_shape_bvh's lights"
            for i in range(L.look_words(fresh)[0][1]):   # (the fresh scene lists the textures it still names, in the same order)
                assert np.array_equal(L.bits(r.ReadTexture(i)), L.bits(fresh.ReadTexture(i)))
        finally:
            fresh.close()
        L.same_words(L.geometry_words(r), geo0, f"{edit}: the geometry")
        assert got[0] != look0[0] or got[1] != look0[1], f"{edit} changed nothing"
    finally:
        r.close()


# ------------------------------------------------------------------ 2. renders
def edited_render(st, fresh_st, engine, edits):
    """A frame of st's scene, then each edit applied and a frame compared with the fresh upload of fresh_st(edit) and
    with the oracle on the mirrored scene."""
    r = L.renderer(st, engine)
    try:
        old, _ = L.frame(r)
        for edit in edits:
            L.apply(r, st, edit)
            g, grays = L.frame(r)
            assert not np.array_equal(g.M, old.M), f"{edit}: the edit changed no pixel"
            fresh = L.renderer(fresh_st(edit), engine)
            try:
                f, frays = L.frame(fresh)
                assert grays == frays, edit
                same_buffer(g, f)
                L.same_look(L.look_words(r), L.look_words(fresh), str(edit))
            finally:
                fresh.close()
            o, orays = oracle(st)   # the scene the update mirrored into
            check(g, grays, o, orays)
            old = g
    finally:
        r.close()


@ENGINES
@pytest.mark.parametrize("edit", list(L.EDITS))
def test_renders_after_an_edit(gpu, engine, edit):
    edited_render(L.look_scene(textures=L.EDITS[edit][2]), lambda e: L.fresh_scene(e), engine, [edit])


@ENGINES
@pytest.mark.parametrize("mode", [LightMode.LightModeRandom, LightMode.LightModeAll], ids=["random", "all"])
def test_a_shape_before_the_lamp_switched_on(gpu, engine, mode):
    """The ball precedes the lamp in Scene.Shapes: the new light takes the list's first place."""
    st = L.look_scene(light_mode=mode)
    edited_render(st, lambda e: L.fresh_scene(e, light_mode=mode), engine, ["sphere-on"])


@ENGINES
def test_seventeen_lights_and_back(gpu, engine):
    """16 lights fit the shadow kernels' LDS form, 17 do not: the forms are left and entered again."""
    st = L.many_lights(16)
    r = L.renderer(st, engine)
    try:
        f16, _ = L.frame(r)
        assert L.look_words(r)[0][2] == 16
        on = st[3]["s16"].with_(Emittance=4.0)
        r.UpdateMaterials([(st[3]["s16"], on)])
        assert L.look_words(r)[0][2] == 17
        f17, rays17 = L.frame(r)
        ref = L.renderer(L.many_lights(17), engine)
        try:
            b, rays = L.frame(ref)
            assert rays == rays17
            same_buffer(f17, b)
            L.same_look(L.look_words(r), L.look_words(ref), "17 lights")
        finally:
            ref.close()
        o, orays = oracle(st)
        check(f17, rays17, o, orays)
        r.UpdateMaterials([(on, st[3]["s16"])])
        assert L.look_words(r)[0][2] == 16
        again, _ = L.frame(r)
        same_buffer(again, f16)
        assert not np.array_equal(f16.M, f17.M)
    finally:
        r.close()


@ENGINES
def test_a_texture_slot_given_and_taken_away(gpu, engine):
    st = L.look_scene(textures="env")
    r = L.renderer(st, engine)
    try:
        f0, _ = L.frame(r)
        assert L.look_words(r)[0][5] == 1
        L.apply(r, st, "texture-given")
        assert L.look_words(r)[0][5] == 0   # a textured material: the routed shade is off
        f1, rays1 = L.frame(r)
        fresh = L.renderer(L.fresh_scene("texture-given"), engine)
        try:
            b, rays = L.frame(fresh)
            assert rays == rays1
            same_buffer(f1, b)
        finally:
            fresh.close()
        o, orays = oracle(st)
        check(f1, rays1, o, orays)
        box = [m for m in st[0].Compile().material_list if m.Texture is st[3]["tex:env"]]
        r.UpdateMaterials([(box[0], box[0].with_(Texture=None))])
        assert L.look_words(r)[0][5] == 1
        f2, _ = L.frame(r)
        same_buffer(f2, f0)
        assert not np.array_equal(f0.M, f1.M)
    finally:
        r.close()


# ------------------------------------------------------------------ 2b. the routed split left and entered again; instances lit
def substituted(builder, rows):
    """builder()'s scene with fields of its compiled material rows set: {index: {field: value}}.  The descriptor a fresh
    context uploads (and the oracle reads) holds the edit; nothing of it comes from an update."""
    st = builder()
    flat = st[0].Compile()
    for i, kw in rows.items():
        for k, v in kw.items():
            setattr(flat.materials[i], k, v)
    return st


def index_of(st, material):
    return [i for i, m in enumerate(st[0].Compile().material_list) if m.key() == material.key()][0]


def by_index(st, engine, rows, builder, expect):
    """The rows' emittances set by pt_update_materials against a fresh upload of the substituted descriptor and the
    oracle; expect: (num_lights, lights_lean, route) after the edit.  Then the edit taken back: the first frame again."""
    r = L.renderer(st, engine)
    try:
        flat = st[0].Compile()
        old = {i: flat.material_list[i] for i in rows}
        look0 = L.look_words(r)
        f0, _ = L.frame(r)
        r.UpdateMaterials({i: old[i].with_(Emittance=kw["emittance"]) for i, kw in rows.items()})
        got = L.look_words(r)
        assert got[0][2:5] == expect, got[0]
        f1, rays1 = L.frame(r)
        assert not np.array_equal(f0.M, f1.M)
        ref_st = substituted(builder, rows)
        ref = L.renderer(ref_st, engine)
        try:
            L.same_look(got, L.look_words(ref), "against the substituted upload")
            b, rays = L.frame(ref)
            assert rays == rays1
            same_buffer(f1, b)
        finally:
            ref.close()
        o, orays = oracle(st)
        check(f1, rays1, o, orays)
        r.UpdateMaterials({i: old[i] for i in rows})
        L.same_look(L.look_words(r), look0, "taken back")
        f2, _ = L.frame(r)
        same_buffer(f2, f0)
        return look0
    finally:
        r.close()


def routed():
    s, cam, smp = scenes.mixed(3000, seed=5)   # the C5 kind at test size: its routed split is on
    smp.MaxBounces = 3
    return s, cam, smp


@ENGINES
@pytest.mark.parametrize("what", ["sdf", "volume"])
def test_the_routed_split_left_and_entered_again(gpu, engine, what):
    """A lit SDF shape is a light the lean kernels do not serve: route and lights_lean go 1 -> 0 with the edit and
    0 -> 1 when it is taken back, the routed queues allocated again.  A lit Volume under its transform is a phantom
    light: the list grows and the route stays."""
    st = routed()
    if what == "sdf":
        mat = [x for x in st[0].Shapes if isinstance(x, SDFShape)][0].Material
        expect = (3, 0, 0)
    else:   # the window nearest the origin's sample, 0: the Volume's MaterialAt(origin); under a transform: a phantom
        mat = [x for x in st[0].Shapes if isinstance(x, TransformedShape)][0].Shape.Windows[0].VolumeWindowMaterial
        expect = (3, 1, 1)
    look0 = by_index(st, engine, {index_of(st, mat): {"emittance": 5.0}}, routed, expect)
    assert look0[0][2:5] == (2, 1, 1)   # two light spheres, lean, routed


@ENGINES
def test_transformed_spheres_and_a_transformed_cube_lit(gpu, engine):
    """TransformedShapes over a sphere and over a cube become lights: phantom, their spheres from the instances' boxes."""
    st = scenes.transformed()
    stones = [x for x in st[0].Shapes if isinstance(x, TransformedShape)]
    white, cube = stones[0].Shape.Material, stones[5].Shape.Material
    rows = {index_of(st, white): {"emittance": 3.0}, index_of(st, cube): {"emittance": 8.0}}
    r = L.renderer(st, engine)
    try:
        n0 = L.look_words(r)[0][2]
    finally:
        r.close()
    st = scenes.transformed()
    by_index(st, engine, rows, scenes.transformed, (n0 + 3, 1, 0))
    r = L.renderer(substituted(scenes.transformed, rows), engine)
    try:
        rows_ = L.look_words(r)[2]
        assert (rows_[:, 0] == 7).sum() >= 4 and (rows_[rows_[:, 0] == 7, 3] == 1).all()   # KIND_XFORM lights are phantoms
    finally:
        r.close()


# ------------------------------------------------------------------ 3. after motion
def moved_arrays(tri):
    """The six triangle arrays of the scene with its loose triangle at `tri` (NewTriangle derives the normals)."""
    flat = L.look_scene(instances=False, tri=tri)[0].Compile()
    return [a.copy() for a in (flat.tri_v1, flat.tri_v2, flat.tri_v3, flat.tri_n1, flat.tri_n2, flat.tri_n3)]


@ENGINES
def test_lit_after_motion(gpu, engine):
    both = ({"ball": lambda m, t: L.lit(m), "tri": lambda m, t: L.lit(m, 4.0)}, None, "all")
    st = L.look_scene(instances=False)
    r = L.renderer(st, engine)
    try:
        flat = st[0].Compile()
        rest = [a.copy() for a in (flat.tri_v1, flat.tri_v2, flat.tri_v3, flat.tri_n1, flat.tri_n2, flat.tri_n3)]
        centres = flat.sphere_center.copy()
        centres[0] = L.BALL_MOVED   # the ball is the scene's first sphere
        r.UpdateShapes(sphere_center=centres)
        r.UpdateTriangles(*moved_arrays(L.TRI_MOVED))
        L.apply(r, st, both)

        def against(ball, tri, what, posed=False):
            ref_st = L.fresh_scene(both, instances=False, ball=ball, tri=tri)
            ref = L.renderer(ref_st, engine)
            try:
                if posed:   # Mesh.Transform normalises the mesh's normals again, by the identity too: the reference is posed alike
                    ref.PoseMeshes([Matrix.Identity()])
                # (the fresh upload sorts the analytic BVH of the moved scene: a light's record index is left out)
                L.same_look(L.look_words(r), L.look_words(ref), what, index=False)
                g, grays = L.frame(r)
                f, frays = L.frame(ref)
                assert grays == frays, what
                same_buffer(g, f)
                o, orays = oracle(ref_st)
                check(g, grays, o, orays)
            finally:
                ref.close()

        assert L.look_words(r)[0][2] == 3
        against(L.BALL_MOVED, L.TRI_MOVED, "lit after motion")
        again = (-0.6, 1.4, 0.2)
        centres[0] = again
        r.UpdateShapes(sphere_center=centres)
        against(again, L.TRI_MOVED, "the lit ball moved again")
        r.SetRestPose(*rest)
        r.PoseMeshes([Matrix.Identity()])   # the mesh stays; the loose triangle returns to its rest vertices
        against(again, L.TRI, "the lit triangle back at rest", posed=True)
    finally:
        r.close()


def test_update_volumes_after_a_volume_was_lit(gpu):
    st, ref_st = L.look_scene(), L.fresh_scene("volume-on")
    r, ref = L.renderer(st), L.renderer(ref_st)
    try:
        L.apply(r, st, "volume-on")
        for x, y in ((r, st), (ref, ref_st)):
            vol = y[0].Compile().volume_objects[0]
            x.UpdateVolumes({0: (None, [(w.Lo + 0.01, w.Hi + 0.015) for w in vol.Windows])})
        L.same_look(L.look_words(r), L.look_words(ref), "windows dragged")
        L.same_words(L.geometry_words(r), L.geometry_words(ref), "windows dragged")
        same_buffer(L.frame(r)[0], L.frame(ref)[0])
        for x, y in ((r, st), (ref, ref_st)):   # the lit window dragged away until a dull one is nearer the origin's sample
            vol = y[0].Compile().volume_objects[0]
            away = [(w.Lo, w.Hi) for w in vol.Windows]
            away[0], away[1] = (0.6, 0.61), (0.1, 0.11)
            with pytest.raises(_abi.PTError) as e:
                x.UpdateVolumes({0: (None, away)})
            assert e.value.code == _abi.PT_ERR_UNSUPPORTED
        L.same_look(L.look_words(r), L.look_words(ref), "after the refusal")
    finally:
        r.close()
        ref.close()


# ------------------------------------------------------------------ 4. textures
@ENGINES
def test_textures_decoded_on_the_device(gpu, engine):
    st = L.look_scene()
    r = L.renderer(st, engine)
    try:
        flat = st[0].Compile()
        order = {name: [i for i, t in enumerate(flat.texture_list) if t is st[3][f"tex:{name}"]][0] for name in L.TEX_SIZES}
        old, _ = L.frame(r)
        ball0 = r.ReadTexture(order["ball"])

        def decoded(new, what):
            ms = r.UpdateTextures({st[3][f"tex:{k}"]: t for k, t in new.items()})
            assert ms > 0
            for k, t in new.items():
                w, h = L.TEX_SIZES[k]
                assert t.Source8 is not None
                assert np.array_equal(L.bits(r.ReadTexture(order[k])), L.bits(t.Data.reshape(h, w, 3))), f"{what} {k}: not the host's Data"
                mine = st[3][f"tex:{k}"]   # the mirror: the texels, and the 8-bit source with its table
                assert np.array_equal(L.bits(mine.Data), L.bits(t.Data)) and mine.Source8 is t.Source8
                assert np.array_equal(L.bits(mine.Table()), L.bits(t.Table()))

        # RGB8 for the 67x33 texture, RGBA8 for the 3x5 one; the 2x2 texture's entry is NULL
        decoded({"env": L.texture("env", 901), "floor": L.texture("floor", 902, channels=4)}, "first")
        assert np.array_equal(L.bits(r.ReadTexture(order["ball"])), L.bits(ball0)), "a NULL entry was written"
        g, grays = L.frame(r)
        assert not np.array_equal(g.M, old.M)
        o, orays = oracle(st)
        check(g, grays, o, orays)
        # the other pairing: in the staging the images follow one another in texture order (3x5 RGB8 = 45 bytes, then
        # 2x2, then 67x33), so the later ones start off the dword grid
        decoded({"env": L.texture("env", 911, channels=4), "floor": L.texture("floor", 912), "ball": L.texture("ball", 913, channels=4)}, "second")
        decoded({"ball": L.texture("ball", 921), "floor": L.texture("floor", 922)}, "third")
        final = {"env": L.texture("env", 911, channels=4).Data, "floor": L.texture("floor", 922).Data}
        final["ball"] = np.random.default_rng(914).random((4, 3))   # an F64 update
        assert r.UpdateTextures({order["ball"]: final["ball"].reshape(2, 2, 3)}) == 0.0
        assert np.array_equal(L.bits(r.ReadTexture(order["ball"])), L.bits(final["ball"].reshape(2, 2, 3)))
        # a fresh upload of the scene with those texels (host-decoded) holds and renders the same
        ref_st = L.look_scene()
        for k, data in final.items():
            ref_st[3][f"tex:{k}"].Data[...] = data
        ref = L.renderer(ref_st, engine)
        try:
            for i in range(len(order)):
                assert np.array_equal(L.bits(r.ReadTexture(i)), L.bits(ref.ReadTexture(i)))
            g2, rays2 = L.frame(r)
            f, frays = L.frame(ref)
            assert rays2 == frays
            same_buffer(g2, f)
            assert not np.array_equal(g2.M, g.M)
            o, orays = oracle(st)
            check(g2, rays2, o, orays)
        finally:
            ref.close()
    finally:
        r.close()


# ------------------------------------------------------------------ 5. between two passes
def test_update_between_two_passes_of_one_accumulation(gpu):
    """Pass 1 sees the uploaded scene, pass 2 the edited one, both in one Buffer: what a fresh context given the first
    Buffer by pt_write_buffer and the new look leaves."""
    st = L.look_scene()
    r = L.renderer(st)
    ref = L.renderer(L.fresh_scene("sphere-on"))
    try:
        r.RenderParallel()
        first = r.ReadBuffer()
        m, v, n = first.M.copy(), first.V.copy(), first.N.copy()
        L.apply(r, st, "sphere-on")
        r.UpdateTextures({st[3]["tex:floor"]: L.texture("floor", 77)})
        a, _ = L.frame(r, reset=False)
        [t for t in ref.Scene.Compile().texture_list if t.Width == 3][0].Data[...] = L.texture("floor", 77).Data
        saved = Buffer(L.W, L.H)   # (not Renderer.PBuffer: the next ReadBuffer writes into that one's arrays)
        saved.M, saved.V, saved.N = m, v, n
        ref.LoadBuffer(saved, 1)
        b, _ = L.frame(ref, reset=False)
        assert (n > 0).all() and (a.N == 2 * n).all()
        same_buffer(a, b)
    finally:
        r.close()
        ref.close()


# ------------------------------------------------------------------ 6. pt_intersect_hits
def test_intersect_hits_after_an_edit(gpu):
    boxed = ({"box": lambda m, t: m.with_(Color=Colour(0.1, 0.7, 0.3), Gloss=Util.Radians(20), Index=1.4)}, None, "all")
    st = L.look_scene()
    r = L.renderer(st)
    ref = L.renderer(L.fresh_scene(boxed))
    try:
        gx, gy = np.meshgrid(np.linspace(-3, 3, 48), np.linspace(0.0, 2.6, 32))
        target = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], 1)
        o = np.tile(np.array([[0, 2.2, 5]], np.float32), (len(target), 1))
        d = (target - o).astype(np.float32)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        h0 = r.IntersectHits(o, d)
        L.apply(r, st, boxed)
        ha, hb = r.IntersectHits(o, d), ref.IntersectHits(o, d)
        for key in ha:
            assert np.array_equal(L.bits(ha[key]), L.bits(hb[key])), f"pt_intersect_hits {key}"
        for key in ("t", "kind", "index", "prim", "shape", "position", "normal", "inside", "material"):
            assert np.array_equal(L.bits(ha[key]), L.bits(h0[key])), f"{key} changed with the look"
        box = ha["shape"] == 2   # the box is Scene.Shapes' third slot
        assert box.sum() >= 20 and not np.array_equal(ha["albedo"][box], h0["albedo"][box])
        assert not np.array_equal(ha["gloss"][box], h0["gloss"][box])
        assert np.array_equal(L.bits(ha["albedo"][~box]), L.bits(h0["albedo"][~box]))
    finally:
        r.close()
        ref.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_scene_untouched(gpu):
    st = L.look_scene()
    r = L.renderer(st)
    lib = None
    try:
        lib = r._lib
        assert lib.pt_get_version() == 10
        look0, geo0 = L.look_words(r), L.geometry_words(r)
        tex0 = [r.ReadTexture(i) for i in range(len(st[0].Compile().texture_list))]
        img0, _ = L.frame(r)
        flat = st[0].Compile()
        nm, nt = len(flat.material_list), len(flat.texture_list)
        rows = (_abi.pt_material * nm)(*flat.materials)
        rows[0].emittance = 9.0   # what a call that went through would change
        MU, TU, TI = _abi.pt_material_update, _abi.pt_texture_update, _abi.pt_texture_image

        def mu(n=nm, flags=0, reserved=(0, 0), mats=rows, env_tex=0):
            u = MU()
            u.num_materials, u.flags, u.reserved = n, flags, (C.c_int32 * 2)(*reserved)
            u.materials = C.cast(mats, C.POINTER(_abi.pt_material)) if mats is not None else None
            u.env_texture, u.env_color = env_tex, (C.c_double * 3)(1, 0, 0)
            return u

        def bad_slot(field):
            b = (_abi.pt_material * nm)(*flat.materials)
            setattr(b[1], field, nt + 1)
            return b

        neg = (_abi.pt_material * nm)(*flat.materials)
        neg[2].texture = -1
        cases = {"NULL ctx": (None, mu()), "NULL u": (r._ctx, None), "reserved[0]": (r._ctx, mu(reserved=(1, 0))),
                 "reserved[1]": (r._ctx, mu(reserved=(0, 5))), "flags 2": (r._ctx, mu(flags=2)), "flags 3": (r._ctx, mu(flags=3)),
                 "one material fewer": (r._ctx, mu(n=nm - 1)), "one material more": (r._ctx, mu(n=nm + 1)),
                 "a negative slot": (r._ctx, mu(mats=neg)), "env slot past the textures": (r._ctx, mu(flags=1, env_tex=nt + 1)),
                 "env slot negative": (r._ctx, mu(flags=1, env_tex=-1))}
        for f in ("texture", "normal_texture", "bump_texture", "gloss_texture"):
            cases[f"{f} past the textures"] = (r._ctx, mu(mats=bad_slot(f)))

        def untouched(what):
            L.same_look(L.look_words(r), look0, what)
            L.same_words(L.geometry_words(r), geo0, what)
            for i in range(nt):
                assert np.array_equal(L.bits(r.ReadTexture(i)), L.bits(tex0[i])), what
            same_buffer(L.frame(r)[0], img0)

        for what, (ctx, u) in cases.items():
            ms = C.c_double(-3.0)
            rc = lib.pt_update_materials(ctx, None if u is None else C.byref(u), C.byref(ms))
            assert rc == _abi.PT_ERR_INVALID_ARG and ms.value == -3.0, what
            untouched(what)
        ms = C.c_double(-3.0)
        assert lib.pt_update_materials(r._ctx, C.byref(mu(mats=None)), C.byref(ms)) == _abi.PT_OK and ms.value == 0.0
        assert lib.pt_update_materials(r._ctx, C.byref(mu(n=nm + 3, mats=None)), None) == _abi.PT_OK   # the count is the array's
        untouched("nothing to do")

        # textures
        sizes = [(t.Width, t.Height) for t in flat.texture_list]
        px = [np.full((h, w, 4), 200, np.uint8) for w, h in sizes]
        lut = np.linspace(0, 1, 256)
        dp = C.POINTER(C.c_double)

        def image(i, w=None, h=None, fmt=_abi.TEXELS_RGBA8, reserved=0, data=True, table=True):
            im = TI()
            im.width, im.height = sizes[i][0] if w is None else w, sizes[i][1] if h is None else h
            im.format, im.reserved = fmt, reserved
            im.data = px[i].ctypes.data_as(C.c_void_p) if data else None
            im.lut = lut.ctypes.data_as(dp) if table else None
            return im

        def tu(images, n=nt, reserved=(0, 0, 0)):
            u = TU()
            u.num_textures, u.reserved = n, (C.c_int32 * 3)(*reserved)
            arr = (C.POINTER(TI) * max(1, len(images)))(*[C.pointer(im) if im is not None else C.POINTER(TI)() for im in images])
            u.images = C.cast(arr, C.POINTER(C.POINTER(TI)))
            u._keep = (arr, images)
            return u

        good = [image(i) for i in range(nt)]
        tcases = {"NULL ctx": (None, tu(good)), "NULL u": (r._ctx, None), "reserved[1]": (r._ctx, tu(good, reserved=(0, 1, 0))),
                  "one texture fewer": (r._ctx, tu(good[:-1], n=nt - 1)), "one texture more": (r._ctx, tu(good + [None], n=nt + 1)),
                  "a wrong width": (r._ctx, tu([image(0, w=sizes[0][0] + 1)] + good[1:])),
                  "a wrong height": (r._ctx, tu(good[:1] + [image(1, h=sizes[1][1] - 1)] + good[2:])),
                  "format 3": (r._ctx, tu(good[:2] + [image(2, fmt=3)])), "format -1": (r._ctx, tu([image(0, fmt=-1)] + good[1:])),
                  "an image's reserved": (r._ctx, tu([image(0, reserved=1)] + good[1:])),
                  "NULL data": (r._ctx, tu(good[:2] + [image(2, data=False)])),
                  "NULL lut, RGB8": (r._ctx, tu([None, image(1, fmt=_abi.TEXELS_RGB8, table=False), None])),
                  "NULL lut, RGBA8": (r._ctx, tu([None, None, image(2, table=False)]))}
        for what, (ctx, u) in tcases.items():
            ms = C.c_double(-3.0)
            rc = lib.pt_update_textures(ctx, None if u is None else C.byref(u), C.byref(ms))
            assert rc == _abi.PT_ERR_INVALID_ARG and ms.value == -3.0, what
            untouched("textures: " + what)
        ms = C.c_double(-3.0)
        assert lib.pt_update_textures(r._ctx, C.byref(tu([None] * nt)), C.byref(ms)) == _abi.PT_OK and ms.value == 0.0
        none = TU()
        none.num_textures = nt
        assert lib.pt_update_textures(r._ctx, C.byref(none), C.byref(ms)) == _abi.PT_OK and ms.value == 0.0
        untouched("textures: nothing to do")
        assert lib.pt_read_texture(r._ctx, nt, None, None) == _abi.PT_ERR_INVALID_ARG
        assert lib.pt_read_texture(r._ctx, -1, None, None) == _abi.PT_ERR_INVALID_ARG
        with pytest.raises(ValueError):
            r.UpdateMaterials([(st[3]["box"], st[3]["box"].with_(Texture=ColorTexture(2, 2, np.zeros((4, 3)))))])   # not uploaded
        with pytest.raises(ValueError):
            r.UpdateMaterials({nm: st[3]["box"]})
        with pytest.raises(ValueError):
            r.UpdateTextures({0: np.zeros((7, 7, 3))})
        untouched("the wrapper's refusals")
    finally:
        r.close()
    # no scene
    r = Renderer.NewRenderer(None, None, None, L.W, L.H, True, device=0)
    try:
        assert lib.pt_update_materials(r._ctx, C.byref(_abi.pt_material_update()), None) == _abi.PT_ERR_NO_SCENE
        assert lib.pt_update_textures(r._ctx, C.byref(_abi.pt_texture_update()), None) == _abi.PT_ERR_NO_SCENE
        assert lib.pt_read_materials(r._ctx, None, None, None, None) == _abi.PT_ERR_NO_SCENE
        assert lib.pt_read_texture(r._ctx, 0, None, None) == _abi.PT_ERR_NO_SCENE
    finally:
        r.close()
