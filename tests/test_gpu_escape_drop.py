"""The dropping shade (k_wf_shade<.., DROP>, PT_ESCAPE_DROP=1, the default where it applies): a child ray that
k_wf_trace_head would turn into a miss with nothing to shade is counted as its Scene.Intersect call and not queued.
Against PT_ESCAPE_DROP=0 (every child queued): the same Stats().rays, the same counters and the same Buffer bits
{M, V, N}.  Shared shape: 64x48, spp 2, 2 passes, bunny_frame(4000, seed=9), wavefront engine.  The depth-0 rule is
the default; PT_ESCAPE_DROP=all (the dropping shade at every depth) is held to the same equality."""
from __future__ import annotations

import re

import numpy as np
import pytest

import oracle_lib as O
from parity import check, render_gpu, same_buffer
from ptsharp_amd import Renderer, _abi, scenes
from ptsharp_amd.scene import Camera, Colour, Material, Vector

pytestmark = pytest.mark.gpu

W, H, SPP, PASSES, SEED = 64, 48, 2, 2, 43
BOX_LO, BOX_HI = np.array([-1.0, 0.0, -1.0]), np.array([1.0, 2.0, 1.0])   # bunny_frame's FitInside box
KNOBS = ("PT_ESCAPE_DROP", "PT_HEAD_STATS", "PT_SHADE_FORM", "PT_HEAD", "PT_LANES", "PT_WF_MAX_CAP")
COUNTED = ("rays", "nodes_visited", "prims_tested", "shadow_rays", "shadow_nodes", "shadow_prims", "lit_shadow_rays")


def _scene():
    return scenes.bunny_frame(4000, seed=9)


def _env(monkeypatch, **kv):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in kv.items():
        monkeypatch.setenv(k, v)


def _render(monkeypatch, env, scene=None, w=W, h=H, spp=SPP, passes=PASSES, **kw):
    _env(monkeypatch, **env)
    s, c, smp = scene if scene is not None else _scene()
    return render_gpu(s, c, smp, w, h, spp=spp, passes=passes, seed=SEED, engine=_abi.ENGINE_WAVEFRONT, **kw)


def _dropped(err):
    """PT_HEAD_STATS=1's lines: {vertex depth: child rays the shade of that depth did not queue}, summed over launches."""
    out = {}
    for d, n in re.findall(r"head depth (\d+): shade dropped (\d+) child rays", err):
        out[int(d)] = out.get(int(d), 0) + int(n)
    return out


def _on_off(monkeypatch, scene_fn=None, on="1", **kw):
    """The pass with the drop on and off: equal rays and bits.  Returns the `on` Buffer and rays."""
    a, ra = _render(monkeypatch, {"PT_ESCAPE_DROP": on}, scene_fn() if scene_fn else None, **kw)
    b, rb = _render(monkeypatch, {"PT_ESCAPE_DROP": "0"}, scene_fn() if scene_fn else None, **kw)
    assert ra == rb and ra > 0
    same_buffer(a, b)
    return a, ra


def _box_hits(camera, w, h):
    """Slab test of the rays through every pixel-cell corner of the frame (the frustum's corner rays
    among them; cast_ray's px / py over x + u - 0.5 in [-0.5, w - 0.5]) against the mesh's box: [h + 1, w + 1] bools."""
    p, u, v, cw = (np.array([q.X, q.Y, q.Z], dtype=np.float64) for q in (camera.p, camera.u, camera.v, camera.w))
    px = (np.arange(w + 1) - 0.5) / (w - 1.0) * 2 - 1
    py = (np.arange(h + 1) - 0.5) / (h - 1.0) * 2 - 1
    d = (-px[None, :, None] * (w / h)) * u + (-py[:, None, None]) * v + camera.m * cw
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (BOX_LO - p) / d, (BOX_HI - p) / d
    near, far = np.minimum(t0, t1).max(axis=2), np.maximum(t0, t1).min(axis=2)
    return (near <= far) & (far > 0)


def _bare_floor():
    s, _, smp = _scene()
    return s, Camera.LookAt(Vector(20, 2, 20), Vector(30, 0, 30), Vector(0, 1, 0), 50), smp


def _close_to_mesh():
    s, _, smp = _scene()
    return s, Camera.LookAt(Vector(0, 1, 2), Vector(0, 1, 0), Vector(0, 1, 0), 20), smp


def test_equal_bits_rays_and_oracle(gpu, monkeypatch):
    a, ra = _on_off(monkeypatch)
    e, re_ = _render(monkeypatch, {"PT_ESCAPE_DROP": "all"})
    assert re_ == ra
    same_buffer(a, e)
    s, c, smp = _scene()
    o, orr = O.render(O.OracleScene(s), c, smp, W, H, SPP, passes=PASSES, seed=SEED)
    check(a, ra, o, orr)


def test_counted_pass_equal(gpu, monkeypatch):
    out = {}
    for drop in ("0", "1", "all"):
        _env(monkeypatch, PT_ESCAPE_DROP=drop)
        s, c, smp = _scene()
        r = Renderer.NewRenderer(s, c, smp, W, H, True, device=0)
        try:
            r.SamplesPerPixel, r.Seed, r.Engine = SPP, SEED, _abi.ENGINE_WAVEFRONT
            ctr = r.RenderCounted()
            out[drop] = tuple(int(getattr(ctr, k)) for k in COUNTED)
        finally:
            r.close()
    print("counted pass", COUNTED, out)
    assert out["0"] == out["1"] == out["all"]
    assert out["1"][0] > 0 and out["1"][1] > 0 and out["1"][2] > 0 and out["1"][3] > 0


def test_engaged_on_shared_scene(gpu, monkeypatch, capfd):
    """PT_HEAD_STATS=1: the shade of the camera hits drops child rays; under the default rule no deeper shade does,
    under PT_ESCAPE_DROP=all deeper ones do too; with the drop off none does, and the head then decides at least as
    many depth-1 rays as a miss with nothing to shade as the shade dropped."""
    capfd.readouterr()
    _render(monkeypatch, {"PT_ESCAPE_DROP": "1", "PT_HEAD_STATS": "1"}, passes=1)
    d1 = _dropped(capfd.readouterr().err)
    _render(monkeypatch, {"PT_ESCAPE_DROP": "all", "PT_HEAD_STATS": "1"}, passes=1)
    dall = _dropped(capfd.readouterr().err)
    _render(monkeypatch, {"PT_ESCAPE_DROP": "0", "PT_HEAD_STATS": "1"}, passes=1)
    err0 = capfd.readouterr().err
    d0 = _dropped(err0)
    print("dropped by vertex depth: default", d1, "all", dall, "off", d0)
    assert d1[0] > 0 and all(n == 0 for d, n in d1.items() if d > 0)
    assert dall[0] == d1[0] and sum(n for d, n in dall.items() if d > 0) > 0
    assert d0 and all(n == 0 for n in d0.values())
    escaped = {}
    for d, n in re.findall(r"head depth (\d+): closest hit (\d+) of \d+ missed with nothing to shade", err0):
        escaped[int(d)] = escaped.get(int(d), 0) + int(n)
    assert escaped[1] == d1[0]   # the predicate is the head's decision, ray for ray


@pytest.mark.parametrize("which", ["env_colour", "gopher3"])
def test_off_where_it_must_be(gpu, monkeypatch, capfd, which):
    """A non-black environment (a miss adds light: nothing may be dropped) and a scene outside the head rule
    (gopher3: analytic shapes only, no triangle BVH): the dropped count is 0 and the Buffers are equal."""
    def scene():
        if which == "gopher3":
            s, c, smp = scenes.gopher3()
            smp.MaxBounces = 4
            return s, c, smp
        s, c, smp = _scene()
        s.Color = Colour(0.05, 0.05, 0.08)
        return s, c, smp
    _on_off(monkeypatch, scene)
    capfd.readouterr()
    _render(monkeypatch, {"PT_ESCAPE_DROP": "1", "PT_HEAD_STATS": "1"}, scene(), passes=1)
    err = capfd.readouterr().err
    d = _dropped(err)
    assert all(n == 0 for n in d.values())
    assert (which == "gopher3") == (not d)   # (outside the head rule the stats lines are not printed at all)


def test_extremes(gpu, monkeypatch, capfd):
    """The bare-floor camera: no camera ray meets the mesh's box, nearly every child leaves the scene.  The
    close-to-mesh camera: every camera ray meets it, nearly no child is dropped."""
    assert not _box_hits(_bare_floor()[1], W, H).any()
    assert _box_hits(_close_to_mesh()[1], W, H).all()
    _on_off(monkeypatch, _bare_floor)
    _on_off(monkeypatch, _close_to_mesh)
    share = {}
    for name, fn in (("floor", _bare_floor), ("mesh", _close_to_mesh)):
        capfd.readouterr()
        _render(monkeypatch, {"PT_ESCAPE_DROP": "1", "PT_HEAD_STATS": "1"}, fn(), passes=1)
        err = capfd.readouterr().err
        queued = sum(int(n) for n in re.findall(r"head depth 1: closest hit \d+ listed of (\d+)", err))
        dropped = _dropped(err)[0]
        share[name] = dropped / (dropped + queued)
    print("dropped share of the camera hits' children:", share)
    # (floor: every child starts on the floor's top face and points up, where only the two light spheres and the
    # far-off mesh are: more than half leave; mesh: a child that starts inside the mesh's box reaches it)
    assert share["floor"] > 0.5 and share["mesh"] < share["floor"]


@pytest.mark.parametrize("fh,w,h,spp", [(16, W, H, SPP), (64, 32, 32, 1)])
def test_child_count_paths(gpu, monkeypatch, fh, w, h, spp):
    """FirstHitSamples 16: 32 children, the last block-major size.  64: 128 children, each wave fills its own
    share and children >= 64 decide again in the second sweep."""
    def scene():
        s, c, smp = _scene()
        smp.FirstHitSamples = fh
        return s, c, smp
    _on_off(monkeypatch, scene, w=w, h=h, spp=spp)
    _on_off(monkeypatch, scene, on="all", w=w, h=h, spp=spp, passes=1)


def test_ragged_sizes(gpu, monkeypatch):
    """70x50: dead camera slots and counts that are no multiples of 64 or 256."""
    a, _ = _on_off(monkeypatch, w=70, h=50)
    assert (a.N == PASSES).all()


def test_offset_origin(gpu, monkeypatch, capfd):
    """A transparent mesh: refracted children start at pos + rd * 1e-4 (bounce_dir), and that origin is what the
    predicate sees."""
    def scene():
        s, c, smp = _scene()
        s.Shapes[0].SetMaterial(Material.TransparentMaterial(Colour.HexColor(0xF2EBC7), 1.5, 0, 0.5))
        return s, c, smp
    a, ra = _on_off(monkeypatch, scene)
    _on_off(monkeypatch, scene, on="all", passes=1)
    for form in ("direct", "scan"):   # (the direct form takes the origin from bounce_origin, the SCAN form from bounce_dir)
        f, rf = _render(monkeypatch, {"PT_ESCAPE_DROP": "1", "PT_SHADE_FORM": form}, scene())
        assert rf == ra
        same_buffer(f, a)
    capfd.readouterr()
    _render(monkeypatch, {"PT_ESCAPE_DROP": "all", "PT_HEAD_STATS": "1"}, scene(), passes=1)
    d = _dropped(capfd.readouterr().err)
    assert d[0] > 0 and sum(n for k, n in d.items() if k > 0) > 0


def test_shade_forms(gpu, monkeypatch):
    off, roff = _render(monkeypatch, {"PT_ESCAPE_DROP": "0"})
    for drop in ("1", "all"):
        a, ra = _render(monkeypatch, {"PT_ESCAPE_DROP": drop, "PT_SHADE_FORM": "direct"})
        b, rb = _render(monkeypatch, {"PT_ESCAPE_DROP": drop, "PT_SHADE_FORM": "scan"})
        assert ra == rb == roff
        same_buffer(a, b)
        same_buffer(a, off)


def test_adaptive_phase(gpu, monkeypatch):
    """AdaptiveSamples 4 (FirstHitSamples unchanged): the extra phases run the same depth loop."""
    _on_off(monkeypatch, adaptive=4)
