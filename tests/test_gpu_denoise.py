"""pt_denoise on the GPU: the variance-guided à-trous denoiser (ptsharp_amd/csrc/pt_denoise.hip)
against its numpy restatement in denoise_ref.py.  Buffers are injected with LoadBuffer, so only the
render tests need a scene.

Both sides do the same fp64 operations in the same order; only the last bit of exp and of a division
may differ, so the bar is the host check's: rtol 1e-11, atol 1e-13 (test_denoise_host.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_ref as D
import image_ref as R
from parity import same_buffer
from ptsharp_amd import Renderer, _abi, scenes
from ptsharp_amd.renderer import Buffer

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-11, 1e-13
# the kernels' block is 64x4 pixels: 131x97 spans 3 blocks across and 25 down, off every block and
# 4-pixel boundary
SHAPES = [(2, 1), (3, 1), (7, 1), (1, 5), (5, 4), (37, 19), (101, 70), (131, 97)]
ITERATIONS = [1, 5, 8]


def _buffer(M, V, N) -> Buffer:
    b = Buffer(N.shape[1], N.shape[0])
    b.M, b.V, b.N = M, V, N
    return b


def _copy(b) -> Buffer:
    return _buffer(b.M.copy(), b.V.copy(), b.N.copy())


def _context(M, V, N, iterations=5, sigma=4.0) -> Renderer:
    r = Renderer.NewRenderer(None, None, None, N.shape[1], N.shape[0], True, device=0)
    r.LoadBuffer(_buffer(M, V, N), passes_done=0)
    r.DenoiseParams = _abi.pt_denoise_params(iterations, 0, sigma)
    return r


def assert_close(got, want, what):
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), what
    diff = np.abs(got[fin] - want[fin])
    rel = diff / np.maximum(np.abs(want[fin]), 1e-300)
    print(f"{what}: max abs diff {diff.max() if diff.size else 0:.3g}, max rel diff {rel.max() if rel.size else 0:.3g}")
    np.testing.assert_allclose(got[fin], want[fin], rtol=RTOL, atol=ATOL, err_msg=what)


@pytest.mark.parametrize("iterations", ITERATIONS)
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_denoise_matches_restatement(gpu, w, h, iterations):
    M, V, N = D.seeded(w, h)
    want_c, want_s = D.reference(w, h, iterations)
    r = _context(M, V, N, iterations)
    try:
        ms = r.DenoiseBuffer()
        assert ms > 0
        assert_close(r.DenoisedColour(), want_c, f"{w}x{h} it {iterations} colour")
        assert_close(r.DenoisedVariance(), want_s, f"{w}x{h} it {iterations} variance")
    finally:
        r.close()


@pytest.mark.parametrize("iterations", ITERATIONS)
def test_denoise_special_pixels(gpu, iterations):
    M, V, N = D.seeded_with_specials()
    ok = D.valid(M, V, N)
    want_c, want_s = D.reference(101, 70, iterations, special=True)
    r = _context(M, V, N, iterations)
    try:
        r.DenoiseBuffer()
        got_c, got_s = r.DenoisedColour(), r.DenoisedVariance()
    finally:
        r.close()
    assert_close(got_c, want_c, f"specials it {iterations} colour")
    assert_close(got_s, want_s, f"specials it {iterations} variance")
    assert np.array_equal(got_c[~ok], M[~ok], equal_nan=True)   # invalid pixels pass through
    assert not got_s[~ok].any()


def test_denoise_firefly_with_its_variance_one_level(gpu):
    M, V, N = D.firefly_with_its_variance()
    want_c, want_s = D.denoise(M, V, N, 1)
    r = _context(M, V, N, 1)
    try:
        r.DenoiseBuffer()
        assert_close(r.DenoisedColour(), want_c, "firefly colour")
        assert_close(r.DenoisedVariance(), want_s, "firefly variance")
    finally:
        r.close()


def test_denoised_bytes_are_the_color_encoding(gpu):
    """Denoised() is image_ref's Color encoding of the reference floats, byte for byte, after asserting
    that none of them lies on a byte boundary; the special pixels' NaN is 0 and +inf 255."""
    M, V, N = D.seeded_with_specials()
    want_c, _ = D.reference(101, 70, 5, special=True)
    col = R.colour(want_c, np.zeros_like(want_c), np.ones(N.shape, np.int32), R.COLOR)
    assert not R.near_boundary(col).any()
    want = R.to_bytes(col)
    r = _context(M, V, N, 5)
    try:
        r.DenoiseBuffer()
        rgb, rgba = r.Denoised(), r.Denoised(rgba=True)
    finally:
        r.close()
    assert rgb.dtype == np.uint8 and rgb.shape == (70, 101, 3) and rgba.shape == (70, 101, 4)
    for got, what in ((rgb, "rgb8"), (rgba[..., :3], "rgba8")):
        bad = (got != want).any(axis=2)
        assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first (y, x) = {np.argwhere(bad)[0]}"
    assert (rgba[..., 3] == 255).all()


def _furnace():
    s, c, smp = scenes.furnace()
    r = Renderer.NewRenderer(s, c, smp, 64, 48, True, device=0)
    r.SamplesPerPixel, r.Seed = 2, 7
    return r


def test_denoise_leaves_the_buffer_and_the_passes_alone(gpu):
    """ReadBuffer before and after DenoiseBuffer() is the same, and a context that renders a pass,
    denoises, then renders another ends bit-identical to one that never denoised."""
    r, q = _furnace(), _furnace()
    try:
        r.RenderParallel()
        q.RenderParallel()
        before = _copy(r.ReadBuffer())
        assert (before.N == 1).all()
        r.DenoiseBuffer()
        same_buffer(_copy(r.ReadBuffer()), before)
        want_c, _ = D.denoise(before.M, before.V, before.N)
        assert_close(r.DenoisedColour(), want_c, "furnace colour")
        r.RenderParallel()
        q.RenderParallel()
        two = _copy(q.ReadBuffer())
        assert (two.N == 2).all()
        same_buffer(_copy(r.ReadBuffer()), two)
    finally:
        r.close()
        q.close()


def test_denoised_is_a_snapshot(gpu):
    """A pass issued after DenoiseBuffer() does not change Denoised(); the next DenoiseBuffer() does."""
    r = _gopher()
    try:
        r.RenderParallel()
        r.DenoiseBuffer()
        snap, snap_c, snap_s = r.Denoised(), r.DenoisedColour(), r.DenoisedVariance()
        first = _copy(r.ReadBuffer())
        r.RenderParallel()
        assert not np.array_equal(r.ReadBuffer().M, first.M)
        assert np.array_equal(r.Denoised(), snap)
        assert np.array_equal(r.DenoisedColour(), snap_c)
        assert np.array_equal(r.DenoisedVariance(), snap_s)
        r.DenoiseBuffer()
        assert not np.array_equal(r.DenoisedColour(), snap_c)
    finally:
        r.close()


def test_denoise_errors_on_a_live_context(gpu):
    M, V, N = D.seeded(37, 19)
    r = _context(M, V, N)
    lib = _abi.load_library()
    out = np.zeros((19, 37, 4), np.float64)
    p = out.ctypes.data_as(C.c_void_p)
    ms = C.c_double(-1.0)
    try:
        # pt_read_denoised before any pt_denoise
        for fmt in (0, 1, 2, 3):
            assert lib.pt_read_denoised(r._ctx, fmt, p) == _abi.PT_ERR_INVALID_ARG
            assert b"before" in lib.pt_last_error()
        with pytest.raises(_abi.PTError):
            r.Denoised()
        bad = [_abi.pt_denoise_params(0, 0, 4.0), _abi.pt_denoise_params(9, 0, 4.0), _abi.pt_denoise_params(-1, 0, 4.0),
               _abi.pt_denoise_params(5, 1, 4.0), _abi.pt_denoise_params(5, 0, 0.0), _abi.pt_denoise_params(5, 0, -2.0),
               _abi.pt_denoise_params(5, 0, float("nan")), _abi.pt_denoise_params(5, 0, float("inf"))]
        for prm in bad:
            assert lib.pt_denoise(r._ctx, C.byref(prm), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG, (
                prm.iterations, prm.reserved, prm.sigma_colour)
            assert lib.pt_last_error()
        assert ms.value == -1.0
        # nothing was launched: there is still no result
        assert lib.pt_read_denoised(r._ctx, 2, p) == _abi.PT_ERR_INVALID_ARG
        # NULL params are the defaults, a NULL out_kernel_ms is allowed
        assert lib.pt_denoise(r._ctx, None, None) == _abi.PT_OK
        assert lib.pt_denoise(r._ctx, None, C.byref(ms)) == _abi.PT_OK and ms.value > 0
        for fmt, ptr in [(-1, p), (4, p), (0, None), (2, None)]:
            assert lib.pt_read_denoised(r._ctx, fmt, ptr) == _abi.PT_ERR_INVALID_ARG, fmt
            assert lib.pt_last_error()
        assert lib.pt_read_denoised(None, 0, p) == _abi.PT_ERR_INVALID_ARG
        assert not out.any()   # nothing was written
        want_c, _ = D.reference(37, 19, 5)
        assert_close(r.DenoisedColour(), want_c, "defaults after errors")
    finally:
        r.close()


def _render(scene, camera, sampler, spp, passes, seed):
    r = Renderer.NewRenderer(scene, camera, sampler, 96, 64, True, device=0)
    r.SamplesPerPixel, r.Seed = spp, seed
    try:
        r.RenderPasses(passes)
        r.DenoiseBuffer()
        return r.ReadBuffer().M.copy(), r.DenoisedColour()
    finally:
        r.close()


@pytest.mark.parametrize("name", ["simplesphere", "example1", "example3"])
def test_denoise_quality_gate(gpu, name):
    """96x64, four passes of 1 spp, seed 0, default parameters, against one 256-spp pass with seed 7:
    the RMSE of clip(c, 0, 1)^(1/2.2) must fall below 0.9 of the noisy picture's (the restatement
    gives 0.59, 0.77 and 0.755 on the oracle's renders of these inputs).  The single-pass ratios at 4
    and 16 spp (N = 1: the spatial variance estimate, scene-dependent) are printed, not gated."""
    scene, camera, sampler = getattr(scenes, name)()
    truth, _ = _render(scene, camera, sampler, 256, 1, 7)
    noisy, denoised = _render(scene, camera, sampler, 1, 4, 0)
    ratio = D.rmse_ratio(denoised, noisy, truth)
    print(f"{name}: 4 passes of 1 spp: denoised/noisy RMSE ratio {ratio:.3f}")
    for spp in (4, 16):
        one, den = _render(scene, camera, sampler, spp, 1, 0)
        print(f"{name}: 1 pass of {spp} spp (N = 1): ratio {D.rmse_ratio(den, one, truth):.3f}")
    assert ratio < 0.9


def _gopher():
    s, c, smp = scenes.gopher3()
    smp.MaxBounces = 4
    r = Renderer.NewRenderer(s, c, smp, 64, 48, True, device=0)
    r.SamplesPerPixel, r.Seed = 2, 7
    return r


def test_iterative_render_with_denoise(gpu, tmp_path):
    """Denoise = True: the four PNG kinds in pathTemplate's directory, and the returned image is
    Denoised(); Denoise = False: only the pass images, and the returned image is the Color channel."""
    (tmp_path / "on").mkdir()
    (tmp_path / "off").mkdir()
    r = _gopher()
    try:
        r.Denoise = True
        img = r.IterativeRender(str(tmp_path / "on" / "out{0}.png"), 2)
        assert img.dtype == np.uint8 and img.shape == (48, 64, 3)
        assert np.array_equal(img, r.Denoised())
        b = _copy(r.ReadBuffer())
        want_c, _ = D.denoise(b.M, b.V, b.N)
        assert_close(r.DenoisedColour(), want_c, "after IterativeRender")
    finally:
        r.close()
    assert sorted(os.listdir(tmp_path / "on")) == ["albedo_channel.png", "denoised_output.png", "normal_channel.png",
                                                   "out1.png", "out2.png"]
    r = _gopher()
    try:
        off = r.IterativeRender(str(tmp_path / "off" / "out{0}.png"), 2)
        assert np.array_equal(off, r.ReadBuffer().Image())
        same_buffer(_copy(r.ReadBuffer()), b)
        assert not np.array_equal(off, img)
    finally:
        r.close()
    assert sorted(os.listdir(tmp_path / "off")) == ["out1.png", "out2.png"]
    for i in (1, 2):   # the pass images do not depend on Denoise
        assert (tmp_path / "on" / f"out{i}.png").read_bytes() == (tmp_path / "off" / f"out{i}.png").read_bytes()
