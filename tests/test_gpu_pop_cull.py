"""Keyed stack entries in the closest-hit refill kernels (pt_stack_key.h; k_wf_trace_lanes culls a popped entry whose
entry distance is beyond the ray's bound of that moment): the default against PT_POP_CULL=0 (bare refs, nothing
culled) and against the lockstep kernels (PT_LANES=0, unkeyed).  The cull drops only entries that cannot hold a
nearer hit, so rays, shadow work and the Buffer bits {M, V, N} are the same and only the closest-hit node and
triangle counts shrink.  Shared shape as in test_gpu_head_compact.py: bunny_frame(4000, seed=9), 64x48, spp 2,
2 passes, wavefront engine."""
from __future__ import annotations

import pytest

import oracle_lib as O
from parity import check, render_gpu, same_buffer
from ptsharp_amd import Renderer, _abi, scenes, tiles_for_rank
from ptsharp_amd.renderer import Buffer
from ptsharp_amd.scene import Camera, Vector

pytestmark = pytest.mark.gpu

W, H, SPP, PASSES, SEED = 64, 48, 2, 2, 43
KNOBS = ("PT_HEAD", "PT_LANES", "PT_SHADOW_TAIL", "PT_POP_CULL", "PT_POP_CULL_BITS", "PT_WF_MAX_CAP")
COUNTERS = ("rays", "nodes_visited", "prims_tested", "shadow_rays", "shadow_nodes", "shadow_prims", "lit_shadow_rays")


def _scene():
    return scenes.bunny_frame(4000, seed=9)


def _env(monkeypatch, **kv):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in kv.items():
        monkeypatch.setenv(k, v)


def _render(monkeypatch, env, scene=None, w=W, h=H, spp=SPP, passes=PASSES):
    _env(monkeypatch, **env)
    s, c, smp = scene if scene is not None else _scene()
    return render_gpu(s, c, smp, w, h, spp=spp, passes=passes, seed=SEED, engine=_abi.ENGINE_WAVEFRONT)


@pytest.fixture(scope="module")
def oracle():
    s, c, smp = _scene()
    return O.render(O.OracleScene(s), c, smp, W, H, SPP, passes=PASSES, seed=SEED)


@pytest.mark.parametrize("head", ["1", "0"])
def test_equality_and_oracle(gpu, monkeypatch, oracle, head):
    a, ra = _render(monkeypatch, {"PT_HEAD": head})
    z, rz = _render(monkeypatch, {"PT_HEAD": head, "PT_POP_CULL": "0"})
    l, rl = _render(monkeypatch, {"PT_HEAD": head, "PT_LANES": "0"})
    assert ra == rz == rl and ra > 0
    same_buffer(a, z)
    same_buffer(a, l)
    check(a, ra, *oracle)


def _counted(monkeypatch, **env):
    _env(monkeypatch, **env)
    s, c, smp = _scene()
    r = Renderer.NewRenderer(s, c, smp, W, H, True, device=0)
    try:
        r.SamplesPerPixel, r.Seed, r.Engine = SPP, SEED, _abi.ENGINE_WAVEFRONT
        ctr = r.RenderCounted()
        return {k: int(getattr(ctr, k)) for k in COUNTERS}
    finally:
        r.close()


def test_counted_pass(gpu, monkeypatch):
    on = _counted(monkeypatch)
    off = _counted(monkeypatch, PT_POP_CULL="0")
    on0 = _counted(monkeypatch, PT_HEAD="0")
    on1 = _counted(monkeypatch, PT_HEAD="1")
    print("counted pass, cull on:", on, "\ncounted pass, cull off:", off)
    for k in ("rays", "shadow_rays", "shadow_nodes", "shadow_prims", "lit_shadow_rays"):
        assert on[k] == off[k] and on[k] > 0, k
    assert on["nodes_visited"] < off["nodes_visited"]   # (fails with the cull inactive)
    assert on["prims_tested"] <= off["prims_tested"]
    assert on0 == on1 == on


@pytest.mark.parametrize("bits", ["1", "15"])
def test_packing_ends(gpu, monkeypatch, bits):
    a, ra = _render(monkeypatch, {})
    b, rb = _render(monkeypatch, {"PT_POP_CULL_BITS": bits})
    assert ra == rb
    same_buffer(a, b)


def test_ragged_two_chunks(gpu, monkeypatch):
    """The 70x50 two-chunk case of the head-pass tests (dead camera slots, counts that are no multiples of 64 or
    256, queues of 2^20 entries, FirstHitSamples 16, spp 8), cull on against off."""
    out = {}
    for cull in ("1", "0"):
        _env(monkeypatch, PT_POP_CULL=cull, PT_WF_MAX_CAP="1048576")
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
            out[cull] = (buf, rays)
        finally:
            r.close()
    assert out["1"][1] == out["0"][1] and out["1"][1] > 0
    same_buffer(out["1"][0], out["0"][0])
    assert (out["1"][0].N == PASSES).all()


def test_empty_lists(gpu, monkeypatch):
    """The camera aimed at bare floor: no camera ray meets the mesh's box, the lists of camera rays are empty."""
    def scene():
        s, _, smp = _scene()
        return s, Camera.LookAt(Vector(20, 2, 20), Vector(30, 0, 30), Vector(0, 1, 0), 50), smp
    a, ra = _render(monkeypatch, {}, scene())
    b, rb = _render(monkeypatch, {"PT_POP_CULL": "0"}, scene())
    assert ra == rb and ra > 0
    same_buffer(a, b)


def test_spill_column_c4_tiles(gpu, monkeypatch):
    """Four 32x32 tiles of the 1M-triangle frame at 1920x1080 (every 512th), 2 passes: the deepest stacks there pass
    the 16 entries a lane keeps in LDS, so keyed entries go through the global spill column too.  Cull on
    against off bit for bit, and the default within the oracle's bar.  (Its seconds are the 1M-triangle scene and
    the oracle's own tree over it, as in test_c4_mesh1m_tiles; the two GPU renders take a fraction of one.)"""
    s, c, smp = scenes.bunny_frame(1_000_000)
    tiles = tiles_for_rank(1920, 1080, 0, 512)
    assert len(tiles) == 4
    out, open_renderers = [], []
    try:
        for env in ({}, {"PT_POP_CULL": "0"}):   # (the first renderer stays open: the second upload finds its BVH build)
            _env(monkeypatch, **env)
            r = Renderer.NewRenderer(s, c, smp, 1920, 1080, True, device=0)
            open_renderers.append(r)
            r.SamplesPerPixel, r.Seed, r.Tiles, r.Engine = 1, 1234, tiles, _abi.ENGINE_WAVEFRONT
            rays = 0
            for _ in range(2):
                r.RenderParallel()
                rays += r.Stats().rays
            g = r.ReadBuffer()
            buf = Buffer(1920, 1080)
            buf.M, buf.V, buf.N = g.M.copy(), g.V.copy(), g.N.copy()
            out.append((buf, rays))
    finally:
        for r in open_renderers:
            r.close()
    (a, ra), (b, rb) = out
    assert ra == rb and int((a.N > 0).sum()) == 4 * 1024
    same_buffer(a, b)
    o, orr = O.render(O.OracleScene(s), c, smp, 1920, 1080, 1, passes=2, seed=1234, tiles=tiles)
    check(a, ra, o, orr)
