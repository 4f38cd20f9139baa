"""The plan that tests/test_pass_plan_host.py checks on the CPU is the plan a pass launches with: the camera kernel
runs once per chunk, so its launch count is rounds x ceil(camera samples / chunk), with `chunk` read from the row of
tests/golden/pass_plan_v1.json for exactly this pass (64x64, scenes.simplesphere() with its own sampler, 4 spp,
wavefront engine, PT_PASS_KERNEL_TIMING).  Queues of 2^20 entries hold the pass in one chunk, queues of 2^16 entries
take four; a stratified pass runs one round per sample index."""
from __future__ import annotations

import json
import os

import pytest

from ptsharp_amd import Renderer, _abi, scenes

pytestmark = pytest.mark.gpu

W = H = 64
SPP = 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pass_plan_v1.json")


@pytest.fixture(scope="module")
def rows():
    with open(GOLDEN) as f:
        g = json.load(f)
    return {r[0]: dict(zip(g["columns"], r)) for r in g["rows"]}


@pytest.mark.parametrize("cap, stratified, chunks", [(1 << 20, False, 1), (1 << 16, False, 4), (1 << 16, True, 1)])
def test_camera_launches_follow_the_plan(gpu, monkeypatch, rows, cap, stratified, chunks):
    row = rows[f"gpu_simplesphere_64x64_spp4_cap{cap}" + ("_stratified" if stratified else "")]
    scene, camera, sampler = scenes.simplesphere()
    lights = 1   # simplesphere's one emissive sphere
    # the row is the plan of this very pass
    assert (row["width"], row["height"], row["num_tiles"], row["spp"], row["stratified"]) == (W, H, 4, SPP, int(stratified))
    assert (row["first_hit_samples"], row["max_bounces"], row["light_mode"], row["specular_mode"], row["num_lights"]) == (
        sampler.FirstHitSamples, sampler.MaxBounces, int(sampler.LightMode), int(sampler.SpecularMode), lights)
    assert (row["engine"], row["flags"], row["passes"], row["adaptive_samples"], row["firefly_samples"], row["counted"]) == (
        _abi.ENGINE_WAVEFRONT, _abi.PASS_KERNEL_TIMING, 1, 0, 0, 0)
    assert (row["wf_max_cap"], row["side_stream"], row["rc"], row["out_engine"]) == (cap, -1, 0, _abi.ENGINE_WAVEFRONT)
    rounds = SPP if stratified else 1
    total = 4 * 1024 * (1 if stratified else SPP)
    assert -(-total // row["chunk"]) == chunks   # one chunk, and several

    monkeypatch.setenv("PT_WF_MAX_CAP", str(cap))
    monkeypatch.delenv("PT_SIDE_STREAM", raising=False)
    r = Renderer.NewRenderer(scene, camera, sampler, W, H, True, device=0)
    try:
        r.SamplesPerPixel, r.Seed, r.Engine, r.Flags = SPP, 5, _abi.ENGINE_WAVEFRONT, _abi.PASS_KERNEL_TIMING
        r.StratifiedSampling = stratified
        r.RenderParallel()
        st = r.Stats()
        launches = st.kernel_launches[_abi.K_CAMERA]
        print(f"cap {cap} stratified {stratified}: chunk {row['chunk']}, camera launches {launches}, rays {st.rays}")
        assert launches == rounds * -(-total // row["chunk"])
        assert st.rays > 0
    finally:
        r.close()
