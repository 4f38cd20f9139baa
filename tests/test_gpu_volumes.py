"""pt_update_volumes on the GPU: new voxels and new iso-windows for the uploaded Volumes, their derived tables (the
uniform-cell signs of the march skip, the cell-major corners) rebuilt on the device.

  1. word for word: after each edit pt_read_volume of every volume (voxels, window rows, signs, corners, header words)
     equals that of a second context that uploaded the edited scene fresh, in every layout the upload can choose
     (cell-major corners or none, the Volume staged in LDS or not); the analytic BVH and pt_stats' bvh_bytes stay;
  2. rays: pt_intersect in the three march forms and pt_occluded after an edit against the oracle of the edited
     scene (t bit for bit) and against the fresh context, with floors on how many rays hit a Volume and on how many
     changed their t, so that an edit that changed nothing cannot pass;
  3. renders on both engines, the feature pass and pt_intersect_hits' material and albedo after an edit against the
     fresh context bit for bit, the renders against the oracle within tests/parity.py's bar;
  4. the identity edit, an edit between two passes of one accumulation, and both orders with pt_update_shapes;
  5. every refusal leaves the volumes and a render as they were, the light refusal included; the trivial calls launch
     nothing.
Scenes and helpers: tests/volume_update_ref.py.  Frames are 96x64 at 2 spp, ray sets 4,096 rays.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import volume_update_ref as V
from parity import check, same_buffer
from ptsharp_amd import Renderer, TransformedShape, Vector, _abi, scenes
from ptsharp_amd.geometry import Box, Colour, Matrix
from ptsharp_amd.scene import Material, Scene, Volume, VolumeWindow

pytestmark = pytest.mark.gpu

ENGINES = pytest.mark.parametrize("engine", [_abi.ENGINE_MEGAKERNEL, _abi.ENGINE_WAVEFRONT], ids=["mega", "wavefront"])
LAYOUTS = {"default": {}, "no-cells": {"PT_VOL_CELLS": "0"}, "no-lds": {"PT_VOL_LDS": "0"}}
MODES = {"auto": 0, "lane": _abi.MARCH_LANE, "wave": _abi.MARCH_WAVE}
F = np.float32


def apply_to_scene(scene, updates, keys_from=None):
    """An edit written into the Python Volumes of a scene that was not compiled yet: the edited scene, for a fresh
    upload that owes nothing to UpdateVolumes' mirror.  keys_from: the scene whose Volume objects key `updates`."""
    scene = scene[0] if isinstance(scene, tuple) else scene
    vols = V.volumes_of(scene)
    scene._flat = None   # compiled only to list the volumes; the upload compiles the edited objects
    src = V.volumes_of(keys_from) if keys_from is not None else vols
    for key, (data, wins) in updates.items():
        i = key if isinstance(key, (int, np.integer)) else [k for k, o in enumerate(src) if o is key][0]
        if data is not None:
            vols[i].Data[...] = data
        if wins is not None:
            for w, (lo, hi) in zip(vols[i].Windows, wins):
                w.Lo, w.Hi = lo, hi


def lit_scene():
    """Example.volume's five windows on two Volumes: a top-level one that is no light (the sample at the origin, 0, is
    nearest its first window, which is dull; its second emits) and, through a TransformedShape, one that is (its
    first window emits).  No window holds 0: such a window makes the whole box one surface of
    samples that are exactly 0, whose NormalAt is 0 / 0."""
    dull = Material.DiffuseMaterial(Colour(0.3, 0.5, 0.8))
    glow = Material.LightMaterial(Colour(1.0, 0.9, 0.7), 6)
    proto = scenes.volume(4, 4, 2)[0].Shapes[0]
    box = Box(Vector(-1, -1, F(-0.2)), Vector(1, 1, 1))
    wins = lambda lit: [VolumeWindow(w.Lo, w.Hi, glow if k == lit else dull) for k, w in enumerate(proto.Windows)]
    a = Volume.NewVolume(box, scenes.volume_slices(24, 24, 12, 3), F(3.4) / F(0.9765625), wins(1))
    b = Volume.NewVolume(box, scenes.volume_slices(16, 16, 8, 3), F(3.4) / F(0.9765625), wins(0))
    s = Scene()
    s.Color = Colour(0.2, 0.2, 0.25)
    s.Add(a)
    s.Add(TransformedShape.NewTransformedShape(b, Matrix.TranslateM(Vector(0.4, 0.3, -0.6)).Mul(Matrix.ScaleM(Vector(0.8, 0.8, 0.8)))))
    assert len(s.Lights) == 1
    _, cam, smp = scenes.volume(4, 4, 2)
    return s, cam, smp


def build(name):
    return lit_scene() if name == "lit" else V.SCENES[name]()


# ------------------------------------------------------------------ 1. word for word
WORDS = [(n, l) for n in ("top", "odd", "two", "mixed") for l in LAYOUTS] + [("lit", "default")]


@pytest.mark.parametrize("name,layout", WORDS, ids=[f"{a}-{b}" for a, b in WORDS])
def test_word_for_word(gpu, monkeypatch, name, layout):
    for k, v in LAYOUTS[layout].items():
        monkeypatch.setenv(k, v)
    st = build(name)
    r = V.renderer(st)
    try:
        before = V.read_all(r)
        assert all((v["cells"] is not None) == (layout != "no-cells") for v in before)
        if name == "two":
            assert before[0]["runs"].size % 2 == 1   # 25 * 25 * 13 cells: the second table starts at an odd byte
        bvh0, bytes0 = r.ReadShapeBvh(), r.Stats().bvh_bytes
        kinds = ["windows"] if name == "lit" else ["data", "windows", "both"] + (["second"] if name == "two" else [])
        history = []
        for step, kind in enumerate(kinds):   # cumulative: every step after the first is also a sequence of updates
            upd = V.edit(st[0], kind, step)
            history.append(upd)
            ms = r.UpdateVolumes(upd)
            assert ms > 0
            got = V.read_all(r)
            st2 = build(name)   # the edited scene, from its builder and the edits alone
            for h in history:
                apply_to_scene(st2, h, keys_from=st[0])
            for a, b in zip(V.volumes_of(st[0]), V.volumes_of(st2)):   # and the mirror wrote the same scene
                assert np.array_equal(V.bits(a.Data), V.bits(b.Data))
                assert [(w.Lo, w.Hi) for w in a.Windows] == [(w.Lo, w.Hi) for w in b.Windows]
            st2[0]._flat = None
            fresh = V.renderer(st2)
            try:
                V.same_volume_words(got, V.read_all(fresh), f"{name} {layout} after {kinds[:step + 1]}")
            finally:
                fresh.close()
            for x, y in zip(r.ReadShapeBvh(), bvh0):
                assert np.array_equal(V.bits(x), V.bits(y)), f"{kind}: the analytic BVH moved"
            assert r.Stats().bvh_bytes == bytes0
            changed = [i for i in range(len(got)) if not np.array_equal(got[i]["runs"], before[i]["runs"])]
            assert changed, f"{kind}: no sign byte changed"
            before = got
    finally:
        r.close()


# ------------------------------------------------------------------ 2. rays
# The oracle's own counts on the CPU, 4,096 rays of volume_rays(seed 11) aimed at the scene's Volumes, edit "both":
#   top    160 rays hit the Volume after the edit, 225 rays change their t
#   two    123 and 182
#   mixed  517 and 642
# The floors are half of each.
RAYS = [("top", 80, 112), ("two", 61, 91), ("mixed", 258, 321)]


@pytest.mark.parametrize("name,min_hits,min_changed", RAYS, ids=[a for a, _, _ in RAYS])
def test_rays_after_an_update(gpu, name, min_hits, min_changed):
    st = build(name)
    r = V.renderer(st, w=8, h=8)
    try:
        o, d = V.volume_rays(*V.volume_target(st[0]), 4096, seed=11)
        t0, k0 = r.Intersect(o, d)
        upd = V.edit(st[0], "both")
        r.UpdateVolumes(upd)
        res = {m: r.Intersect(o, d, f) for m, f in MODES.items()}
        os_ = O.OracleScene(st[0])   # the scene the update mirrored into
        ot, ok = V.oracle_hits(os_, o, d)
        st2 = build(name)
        apply_to_scene(st2, upd)
        fresh = V.renderer(st2, w=8, h=8)
        try:
            ft, fk = fresh.Intersect(o, d)
        finally:
            fresh.close()
        for m, (t, k) in res.items():
            bad = np.flatnonzero((V.bits(t) != V.bits(ot)) | (k != ok))
            assert bad.size == 0, (f"{m}: {bad.size} of {len(o)} rays differ from the oracle, first {bad[:5]}: gpu t {t[bad[:3]]} "
                                   f"kind {k[bad[:3]]}, oracle t {ot[bad[:3]]} kind {ok[bad[:3]]}")
            assert np.array_equal(V.bits(t), V.bits(ft)) and np.array_equal(k, fk), f"{m}: differs from the fresh context"
        hits = int(V.is_volume_kind(ok).sum())
        changed = int((V.bits(res["auto"][0]) != V.bits(t0)).sum())
        print(f"{name}: {hits} rays hit a Volume after the edit, {changed} rays changed their t")
        assert hits >= min_hits, f"only {hits} Volume hits"
        assert changed >= min_changed, f"only {changed} rays changed their t"
        rng = np.random.default_rng(7)
        tl = np.where(ot < 1e9, ot, 5.0)
        for what, tm in {"at_hit": tl, "past_hit": np.nextafter(tl, np.inf), "random": tl * rng.uniform(0.0, 1.6, len(tl))}.items():
            want = np.array([os_.any_nearer(o[i], d[i], tm[i]) for i in range(len(o))], np.int32)
            for m, f in MODES.items():
                got = r.Occluded(o, d, tm, f)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, f"occluded {what} {m}: {bad.size} rays differ, first {bad[:5]}"
    finally:
        r.close()


# ------------------------------------------------------------------ 3. renders and features
RENDERS = [("top", "both"), ("mixed", "both"), ("two", "both"), ("lit", "windows")]
# pt_intersect_hits' rays (2,048 of volume_rays(seed 17)): the oracle's own counts of Volume hits after the edit are
# top 66, mixed 260, two 59, lit 5 (its two boxes lie apart, so the rays' target box is mostly empty); floors at half
HIT_FLOORS = {"top": 33, "mixed": 130, "two": 29, "lit": 2}


@ENGINES
@pytest.mark.parametrize("name,kind", RENDERS, ids=[f"{a}-{b}" for a, b in RENDERS])
def test_renders_after_an_update(gpu, engine, name, kind):
    st = build(name)
    r = V.renderer(st, engine)
    try:
        old, _ = V.frame(r)   # a pass of the uploaded scene first: the update comes between passes
        upd = V.edit(st[0], kind)
        r.UpdateVolumes(upd)
        g, grays = V.frame(r)
        assert not np.array_equal(g.M, old.M), "the edit changed no pixel"
        st2 = build(name)
        apply_to_scene(st2, upd, keys_from=st[0])
        fresh = V.renderer(st2, engine)
        try:
            f, frays = V.frame(fresh)
            assert grays == frays
            same_buffer(g, f)
            o, orays = O.render(O.OracleScene(st[0]), st[1], st[2], V.W, V.H, V.SPP, seed=23)
            check(g, grays, o, orays)
            if engine == _abi.ENGINE_WAVEFRONT:
                r.RenderFeatures()
                fresh.RenderFeatures()
                for a, b, what in zip(r.Features(), fresh.Features(), ("albedo", "normal", "depth", "kind", "material")):
                    assert np.array_equal(V.bits(a), V.bits(b)), f"features after the update: {what} differs"
                ro, rd = V.volume_rays(*V.volume_target(st[0]), 2048, seed=17)
                ha, hb = r.IntersectHits(ro, rd), fresh.IntersectHits(ro, rd)
                on = V.is_volume_kind(ha["kind"])
                assert on.sum() >= HIT_FLOORS[name], f"only {int(on.sum())} Volume hits"
                for key in ("t", "kind", "material", "albedo", "normal", "position"):
                    assert np.array_equal(V.bits(ha[key][on]), V.bits(hb[key][on])), f"pt_intersect_hits {key} on Volume hits"
        finally:
            fresh.close()
    finally:
        r.close()


# ------------------------------------------------------------------ 4. identity and composition
@pytest.mark.parametrize("name", ["two", "mixed"])
def test_identity(gpu, name):
    st = build(name)
    r = V.renderer(st)
    try:
        before, bvh0 = V.read_all(r), r.ReadShapeBvh()
        img0, rays0 = V.frame(r)
        assert r.UpdateVolumes(V.edit(st[0], "identity")) > 0
        V.same_volume_words(V.read_all(r), before, "identity")
        for x, y in zip(r.ReadShapeBvh(), bvh0):
            assert np.array_equal(V.bits(x), V.bits(y))
        img1, rays1 = V.frame(r)
        assert rays0 == rays1
        same_buffer(img1, img0)
    finally:
        r.close()


def test_update_between_two_passes_of_one_accumulation(gpu):
    """Pass 1 sees the uploaded scene, pass 2 the edited one, both accumulated in one Buffer: what a context that
    renders pass 1, takes an upload of the edited scene, and renders pass 2 leaves."""
    st, st2 = build("mixed"), build("mixed")
    r, ref = V.renderer(st), V.renderer(st2)
    try:
        r.RenderParallel()
        upd = V.edit(st[0], "both")
        r.UpdateVolumes(upd)
        a, _ = V.frame(r, reset=False)
        ref.RenderParallel()
        n1 = ref.ReadBuffer().N.copy()
        st3 = build("mixed")
        apply_to_scene(st3, upd)
        ref.Scene = st3[0]   # the next pass uploads it; the Buffer and the pass count stay
        b, _ = V.frame(ref, reset=False)
        assert (n1 > 0).all() and (a.N == 2 * n1).all()   # two passes in one Buffer
        same_buffer(a, b)
    finally:
        r.close()
        ref.close()


def test_composes_with_update_shapes_in_either_order(gpu):
    """The instance that holds the Volume moved by pt_update_shapes, before or after the Volume is edited."""
    sa, sb, sc = build("mixed"), build("mixed"), build("mixed")
    r1, r2 = V.renderer(sa), V.renderer(sb)
    try:
        upd = V.edit(sa[0], "both")
        inst = sa[0].Shapes[-1]
        m = Matrix.TranslateM(Vector(-0.3, 0.2, 0.25)).Mul(Matrix.RotateM(Vector(0, 1, 0), 0.4)).Mul(inst.Matrix)
        r1.UpdateVolumes(upd)
        r1.UpdateShapes(matrices=[m.m])
        r2.UpdateShapes(matrices=[m.m])
        r2.UpdateVolumes(V.edit(sb[0], "both"))
        V.same_volume_words(V.read_all(r1), V.read_all(r2), "either order")
        for x, y in zip(r1.ReadShapeBvh(), r2.ReadShapeBvh()):
            assert np.array_equal(V.bits(x), V.bits(y))
        f1, n1 = V.frame(r1)
        f2, n2 = V.frame(r2)
        assert n1 == n2
        same_buffer(f1, f2)
        # and both are the edited, moved scene: its Volume words are a fresh upload's, its frame the oracle's
        apply_to_scene(sc, upd)
        sc[0].Shapes[-1] = TransformedShape.NewTransformedShape(sc[0].Shapes[-1].Shape, m)
        sc[0]._flat = None
        fresh = V.renderer(sc)
        try:
            V.same_volume_words(V.read_all(r1), V.read_all(fresh), "against the fresh upload")
        finally:
            fresh.close()
        o, orays = O.render(O.OracleScene(sc[0]), sc[1], sc[2], V.W, V.H, V.SPP, seed=23)
        check(f1, n1, o, orays)
    finally:
        r1.close()
        r2.close()


# ------------------------------------------------------------------ 5. errors
def test_errors_leave_the_scene_untouched(gpu):
    st = build("lit")
    r = V.renderer(st)
    dp, wp = C.POINTER(C.c_double), C.POINTER(_abi.pt_volume_window)
    try:
        assert r._lib.pt_get_version() == 10
        before = V.read_all(r)
        img0, _ = V.frame(r)
        vols = V.volumes_of(st[0])
        flat = st[0].Compile()
        data = [V.new_data(v, 50 + i) for i, v in enumerate(vols)]
        dptr = (dp * 2)(*[a.ctypes.data_as(dp) for a in data])
        rows = []
        for i, v in enumerate(vols):
            wa = (_abi.pt_volume_window * len(v.Windows))()
            for k, (lo, hi) in enumerate(V.new_windows(v, 0.01)):
                wa[k] = _abi.pt_volume_window(lo, hi, flat.volumes[i].windows[k].material, 0)
            rows.append(wa)
        wptr = (wp * 2)(*[C.cast(w, wp) for w in rows])
        other = (_abi.pt_volume_window * 5)(*rows[1])
        other[1].material = rows[1][1].material + 1 if rows[1][1].material + 1 < len(flat.materials) else rows[1][1].material - 1
        bad_wptr = (wp * 2)(C.cast(rows[0], wp), C.cast(other, wp))
        U = _abi.pt_volume_update
        dd, ww = C.cast(dptr, C.POINTER(dp)), C.cast(wptr, C.POINTER(wp))

        def call(ctx, u):
            ms = C.c_double(-3.0)
            return r._lib.pt_update_volumes(ctx, None if u is None else C.byref(u), C.byref(ms)), ms.value

        cases = {
            "NULL ctx": lambda: call(None, U(2, (C.c_int32 * 3)(), dd, ww)),
            "NULL u": lambda: call(r._ctx, None),
            "reserved[0]": lambda: call(r._ctx, U(2, (C.c_int32 * 3)(1, 0, 0), dd, ww)),
            "reserved[2]": lambda: call(r._ctx, U(2, (C.c_int32 * 3)(0, 0, 7), dd, ww)),
            "one volume fewer": lambda: call(r._ctx, U(1, (C.c_int32 * 3)(), dd, ww)),
            "one volume more": lambda: call(r._ctx, U(3, (C.c_int32 * 3)(), dd, ww)),
            "a window's material": lambda: call(r._ctx, U(2, (C.c_int32 * 3)(), dd, C.cast(bad_wptr, C.POINTER(wp)))),
        }
        for what, fn in cases.items():
            rc, ms = fn()
            assert rc == _abi.PT_ERR_INVALID_ARG and ms == -3.0, what
            V.same_volume_words(V.read_all(r), before, what)
            same_buffer(V.frame(r)[0], img0)
        # the light refusals: the dull Volume's emissive window dragged onto the origin's sample; the lit one's
        # emissive window dragged away until a dull one is nearer
        onto, away = V.new_windows(vols[0], 0.0), V.new_windows(vols[1], 0.0)
        onto[1] = (-0.05, 0.05)
        away[0], away[1] = (0.6, 0.61), (0.1, 0.11)
        for what, upd in {"no light becomes one": {0: (data[0], onto)},
                          "a light stops being one": {vols[1]: (None, away)}}.items():
            with pytest.raises(_abi.PTError) as e:
                r.UpdateVolumes(upd)
            assert e.value.code == _abi.PT_ERR_UNSUPPORTED, what
            V.same_volume_words(V.read_all(r), before, what)
            same_buffer(V.frame(r)[0], img0)
        # nothing to do: both arrays NULL, every entry NULL
        for what, u in {"both NULL": U(2, (C.c_int32 * 3)()),
                        "every entry NULL": U(2, (C.c_int32 * 3)(), C.cast((dp * 2)(), C.POINTER(dp)), C.cast((wp * 2)(), C.POINTER(wp)))}.items():
            rc, ms = call(r._ctx, u)
            assert rc == _abi.PT_OK and ms == 0.0, what
            V.same_volume_words(V.read_all(r), before, what)
        assert r.UpdateVolumes({}) == 0.0
        same_buffer(V.frame(r)[0], img0)
        with pytest.raises(ValueError):
            r.UpdateVolumes({0: (data[1], None)})   # the other volume's voxel count
        with pytest.raises(ValueError):
            r.UpdateVolumes({5: (None, None)})
        assert r._lib.pt_read_volume(r._ctx, 2, None, None, None, None, None) == _abi.PT_ERR_INVALID_ARG
        assert r._lib.pt_read_volume(r._ctx, -1, None, None, None, None, None) == _abi.PT_ERR_INVALID_ARG
    finally:
        r.close()
    # no scene
    r = Renderer.NewRenderer(None, None, None, V.W, V.H, True, device=0)
    try:
        assert r._lib.pt_update_volumes(r._ctx, C.byref(_abi.pt_volume_update()), None) == _abi.PT_ERR_NO_SCENE
        assert r._lib.pt_read_volume(r._ctx, 0, None, None, None, None, None) == _abi.PT_ERR_NO_SCENE
    finally:
        r.close()
    # a scene without volumes and num_volumes 0: nothing to do
    s, cam, smp = scenes.gopher3()
    r = V.renderer((s, cam, smp))
    try:
        img0, _ = V.frame(r)
        ms = C.c_double(-1.0)
        assert r._lib.pt_update_volumes(r._ctx, C.byref(_abi.pt_volume_update()), C.byref(ms)) == _abi.PT_OK and ms.value == 0.0
        assert r._lib.pt_update_volumes(r._ctx, C.byref(_abi.pt_volume_update(1)), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
        same_buffer(V.frame(r)[0], img0)
    finally:
        r.close()
