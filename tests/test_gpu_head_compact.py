"""The head pass and the list-fed refill kernels (k_wf_trace_head / k_wf_shadow_head, then
k_wf_trace_lanes<.., LIST> / k_wf_shadow_lanes<.., LIST>; PT_HEAD=1, the default where they apply) against
the refill kernels that do their own head work (PT_HEAD=0): the same rays, the same counters and the same
Buffer bits {M, V, N}.  Shared shape: 64x48, spp 2, 2 passes, bunny_frame(4000, seed=9), wavefront engine."""
from __future__ import annotations

import numpy as np
import pytest

import oracle_lib as O
from parity import check, render_gpu, same_buffer
from ptsharp_amd import Renderer, _abi, scenes
from ptsharp_amd.renderer import Buffer
from ptsharp_amd.scene import Camera, Vector

pytestmark = pytest.mark.gpu

W, H, SPP, PASSES, SEED = 64, 48, 2, 2, 43
BOX_LO, BOX_HI = np.array([-1.0, 0.0, -1.0]), np.array([1.0, 2.0, 1.0])   # bunny_frame's FitInside box


def _scene():
    return scenes.bunny_frame(4000, seed=9)


def _env(monkeypatch, **kv):
    for k in ("PT_HEAD", "PT_LANES", "PT_SHADOW_TAIL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in kv.items():
        monkeypatch.setenv(k, v)


def _render(monkeypatch, env, scene=None, w=W, h=H, spp=SPP, passes=PASSES):
    _env(monkeypatch, **env)
    s, c, smp = scene if scene is not None else _scene()
    return render_gpu(s, c, smp, w, h, spp=spp, passes=passes, seed=SEED, engine=_abi.ENGINE_WAVEFRONT)


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


def test_refill_kernels_are_default_on_shared_scene(gpu, monkeypatch):
    """The shared scene's triangle BVH is large enough for the refill kernels (more than 64 nodes below the
    root: pt_wavefront.hip kLanesMinNodes), so PT_HEAD switches kernels here without PT_LANES=1."""
    _env(monkeypatch)
    s, c, smp = _scene()
    r = Renderer.NewRenderer(s, c, smp, W, H, True, device=0)
    try:
        r._ensure_scene()
        assert r.Stats().bvh_nodes - 1 > 64
    finally:
        r.close()


def test_three_way_equality_and_oracle(gpu, monkeypatch):
    a, ra = _render(monkeypatch, {"PT_HEAD": "1"})
    b, rb = _render(monkeypatch, {"PT_HEAD": "0"})
    l, rl = _render(monkeypatch, {"PT_LANES": "0"})
    assert ra == rb == rl
    same_buffer(a, b)
    same_buffer(a, l)
    s, c, smp = _scene()
    o, orr = O.render(O.OracleScene(s), c, smp, W, H, SPP, passes=PASSES, seed=SEED)
    check(a, ra, o, orr)


def test_counted_pass_equal(gpu, monkeypatch):
    out = {}
    for head in ("0", "1"):
        _env(monkeypatch, PT_HEAD=head)
        s, c, smp = _scene()
        r = Renderer.NewRenderer(s, c, smp, W, H, True, device=0)
        try:
            r.SamplesPerPixel, r.Seed, r.Engine = SPP, SEED, _abi.ENGINE_WAVEFRONT
            ctr = r.RenderCounted()
            out[head] = tuple(int(getattr(ctr, k)) for k in ("rays", "nodes_visited", "prims_tested", "shadow_rays",
                                                              "shadow_nodes", "shadow_prims", "lit_shadow_rays"))
        finally:
            r.close()
    print("counted pass (rays, nodes, prims, shadow rays, shadow nodes, shadow prims, lit):", out)
    assert out["0"] == out["1"]
    assert out["1"][0] > 0 and out["1"][1] > 0 and out["1"][3] > 0 and out["1"][4] > 0


def test_empty_list(gpu, monkeypatch):
    """The camera aimed at bare floor: no camera ray meets the mesh's box, so every partition's list of
    camera rays is empty and the list-fed closest hit has nothing to do at depth 0; the kernels finish."""
    def scene():
        s, _, smp = _scene()
        return s, Camera.LookAt(Vector(20, 2, 20), Vector(30, 0, 30), Vector(0, 1, 0), 50), smp
    assert not _box_hits(scene()[1], W, H).any()
    a, ra = _render(monkeypatch, {"PT_HEAD": "1"}, scene())
    b, rb = _render(monkeypatch, {"PT_HEAD": "0"}, scene())
    assert ra == rb and ra > 0
    same_buffer(a, b)


def test_full_list(gpu, monkeypatch):
    """The camera close to the mesh: every camera ray meets the mesh's box."""
    def scene():
        s, _, smp = _scene()
        return s, Camera.LookAt(Vector(0, 1, 2), Vector(0, 1, 0), Vector(0, 1, 0), 20), smp
    assert _box_hits(scene()[1], W, H).all()
    a, ra = _render(monkeypatch, {"PT_HEAD": "1"}, scene())
    b, rb = _render(monkeypatch, {"PT_HEAD": "0"}, scene())
    assert ra == rb and ra > 0
    same_buffer(a, b)


def test_ragged_sizes_and_many_chunks(gpu, monkeypatch):
    """70x50: dead camera slots (the frame's 6 tiles hold 6144 pixel slots for 3500 pixels) and counts that
    are no multiples of 64 or 256.  Queues of 2^20 entries and FirstHitSamples 16 (32 children per camera hit);
    spp 8 here, because the frame's 49,152 camera slots then exceed the 32,768 a chunk of these queues
    takes and two chunks run (at spp 2 one chunk would hold them all): the camera kernel's launch count says so."""
    monkeypatch.setenv("PT_WF_MAX_CAP", "1048576")
    out = {}
    for head in ("1", "0"):
        _env(monkeypatch, PT_HEAD=head)
        s, c, smp = _scene()
        smp.FirstHitSamples = 16
        r = Renderer.NewRenderer(s, c, smp, 70, 50, True, device=0)
        try:
            r.SamplesPerPixel, r.Seed, r.Engine = 8, SEED, _abi.ENGINE_WAVEFRONT
            r.Flags = _abi.PASS_KERNEL_TIMING
            rays = 0
            for _ in range(PASSES):
                r.RenderParallel()
                rays += r.Stats().rays
                assert r.Stats().kernel_launches[_abi.K_CAMERA] >= 2, "one chunk only"
            g = r.ReadBuffer()
            buf = Buffer(70, 50)
            buf.M, buf.V, buf.N = g.M.copy(), g.V.copy(), g.N.copy()
            out[head] = (buf, rays)
        finally:
            r.close()
    assert out["1"][1] == out["0"][1]
    same_buffer(out["1"][0], out["0"][0])
    assert (out["1"][0].N == PASSES).all()   # (one Welford sample per pixel per pass)


def test_uneven_partitions_and_batches(gpu, monkeypatch):
    """A 3-tile subset of a 160x120 frame (3 of 20 tiles: the 8 partitions get unequal shares, some
    none) as RenderPasses(3): the separate passes' bits, with and without the head pass."""
    w, h = 160, 120
    tiles = np.array([1, 7, 13], dtype=np.int32)   # (whole 32x32 tiles of the 5 x 4 grid)

    def run(head, batched):
        _env(monkeypatch, PT_HEAD=head)
        s, c, smp = _scene()
        r = Renderer.NewRenderer(s, c, smp, w, h, True, device=0)
        try:
            r.SamplesPerPixel, r.Seed, r.Tiles, r.Engine = SPP, SEED, tiles, _abi.ENGINE_WAVEFRONT
            rays = 0
            if batched:
                r.RenderPasses(3)
                rays = r.Stats().rays
            else:
                for _ in range(3):
                    r.RenderParallel()
                    rays += r.Stats().rays
            g = r.ReadBuffer()
            buf = Buffer(w, h)
            buf.M, buf.V, buf.N = g.M.copy(), g.V.copy(), g.N.copy()
            return buf, rays
        finally:
            r.close()
    a, ra = run("1", True)
    b, rb = run("1", False)
    c0, rc = run("0", True)
    assert ra == rb == rc and ra > 0
    same_buffer(a, b)
    same_buffer(a, c0)
    assert int((a.N > 0).sum()) == 3 * 1024


def test_forced_tail_with_head(gpu, monkeypatch):
    """PT_SHADOW_TAIL=early (the hand-off protocol all pass long) on the list-fed shadow kernel equals its
    default tail bit for bit, and PT_HEAD=0."""
    e, re_ = _render(monkeypatch, {"PT_HEAD": "1", "PT_SHADOW_TAIL": "early"})
    d, rd = _render(monkeypatch, {"PT_HEAD": "1"})
    z, rz = _render(monkeypatch, {"PT_HEAD": "0"})
    assert re_ == rd == rz
    same_buffer(e, d)
    same_buffer(e, z)
