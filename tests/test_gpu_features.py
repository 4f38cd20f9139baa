"""pt_render_features, pt_read_features, pt_write_features and pt_denoise_guided on the GPU: the
first-hit features against the CPU oracle pixel by pixel (features_ref.py), the guided filter against
its numpy restatement on injected data (denoise_guided_ref.py), against the unguided filter on the
same context, and the state and error rules of the four entry points.

The guided filter and its restatement do the same fp64 operations in the same order; only the last
bit of exp and of a division may differ, so the bar is the unguided filter's: rtol 1e-11, atol 1e-13."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_guided_ref as G
import denoise_ref as D
import features_ref as F
from parity import same_buffer
from ptsharp_amd import Renderer, _abi, scenes, tiles_for_rank
from ptsharp_amd.renderer import Buffer

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-11, 1e-13
# the level kernels' block is 64x4 pixels: 131x97 spans 3 blocks across and 25 down, off every boundary
SHAPES = [(2, 1), (3, 1), (7, 1), (1, 5), (5, 4), (37, 19), (101, 70), (131, 97)]
ITERATIONS = [1, 5, 8]
SIZES, SCENES, scene_of, expected = F.SIZES, F.SCENES, F.scene_of, F.expected


def _buffer(M, V, N) -> Buffer:
    b = Buffer(N.shape[1], N.shape[0])
    b.M, b.V, b.N = M, V, N
    return b


def _copy(b) -> Buffer:
    return _buffer(b.M.copy(), b.V.copy(), b.N.copy())


def _context(M, V, N, feats=None, iterations=5, sigmas=(4.0, 0.3, 0.3, 0.1)) -> Renderer:
    r = Renderer.NewRenderer(None, None, None, N.shape[1], N.shape[0], True, device=0)
    r.LoadBuffer(_buffer(M, V, N), passes_done=0)
    if feats is not None:
        r.LoadFeatures(*feats)
    r.DenoiseParams = _abi.pt_denoise_params(iterations, 0, sigmas[0])
    r.DenoiseGuidedParams = _abi.pt_denoise_guided_params(iterations, 0, *sigmas)
    return r


def assert_close(got, want, what):
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), what
    diff = np.abs(got[fin] - want[fin])
    rel = diff / np.maximum(np.abs(want[fin]), 1e-300)
    print(f"{what}: max abs diff {diff.max() if diff.size else 0:.3g}, max rel diff {rel.max() if rel.size else 0:.3g}")
    np.testing.assert_allclose(got[fin], want[fin], rtol=RTOL, atol=ATOL, err_msg=what)


def assert_features(got, want, what):
    """Every pixel: kind, material and the depth's and the fp32 normal's bits equal, the albedo within
    1e-9·max(1, |albedo|) (the project's colour bar)."""
    ga, gn, gz, gk, gm = got
    wa, wn, wz, wk, wm = want
    bad = np.argwhere(gk != wk)
    assert not bad.size, f"{what}: kind differs on {len(bad)} pixels, first (y, x) {bad[0]}: {gk[tuple(bad[0])]} vs {wk[tuple(bad[0])]}"
    bad = np.argwhere(gz.view(np.int64) != wz.view(np.int64))
    assert not bad.size, (f"{what}: depth bits differ on {len(bad)} pixels, first (y, x) {bad[0]}: "
                          f"{gz[tuple(bad[0])]!r} vs {wz[tuple(bad[0])]!r}")
    bad = np.argwhere(gm != wm)
    assert not bad.size, f"{what}: material differs on {len(bad)} pixels, first (y, x) {bad[0]}"
    bad = np.argwhere((gn.view(np.int32) != wn.view(np.int32)).any(axis=2))
    assert not bad.size, (f"{what}: normal bits differ on {len(bad)} pixels, first (y, x) {bad[0]}: "
                          f"{gn[tuple(bad[0])]} vs {wn[tuple(bad[0])]}")
    err = np.abs(ga - wa)
    print(f"{what}: {int((wk >= 0).sum())} hits of {wk.size}, kinds {sorted(set(wk.ravel().tolist()))}, max |d albedo| {err.max():.3g}")
    assert (err <= 1e-9 * np.maximum(1.0, np.abs(wa))).all(), f"{what}: albedo max err {err.max()}"


# ------------------------------------------------------------------ features against the oracle
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("name", list(SCENES))
def test_features_match_the_oracle(gpu, name, w, h):
    s, c, smp = scene_of(name)
    want = expected(name, w, h)
    r = Renderer.NewRenderer(s, c, smp, w, h, True, device=0)
    try:
        assert r.RenderFeatures() > 0
        got = r.Features()
    finally:
        r.close()
    assert_features(got, want, f"{name} {w}x{h}")


def test_the_lens_is_ignored(gpu):
    s, c, smp = scenes.example1()
    assert c.apertureRadius == 0.1
    w, h = 67, 45
    r = Renderer.NewRenderer(s, c, smp, w, h, True, device=0)
    try:
        r.RenderFeatures()
        with_lens = r.Features()
        c.apertureRadius = 0.0
        r.RenderFeatures()
        without = r.Features()
    finally:
        c.apertureRadius = 0.1
        r.close()
    for a, b in zip(with_lens, without):
        assert np.array_equal(a, b)
    assert_features(with_lens, F.features(s, c, w, h), "example1 with a lens")


def test_a_tile_sharded_context_gets_whole_frame_features(gpu):
    s, c, smp = scene_of("gopher3")
    w, h = 67, 45
    r = Renderer.NewRenderer(s, c, smp, w, h, True, device=0)
    try:
        r.Tiles = tiles_for_rank(w, h, 1, 2)
        r.SamplesPerPixel, r.Seed = 1, 3
        r.RenderParallel()
        assert (r.ReadBuffer().N > 0).sum() < w * h
        r.RenderFeatures()
        got = r.Features()
    finally:
        r.close()
    assert_features(got, expected("gopher3", w, h), "gopher3 sharded")


# ------------------------------------------------------------------ the guided filter on injected data
@pytest.mark.parametrize("iterations", ITERATIONS)
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_guided_matches_restatement(gpu, w, h, iterations):
    M, V, N = D.seeded(w, h)
    want_c, want_s = G.reference(w, h, iterations)
    r = _context(M, V, N, G.seeded_features(w, h), iterations)
    try:
        assert r.DenoiseBuffer(guided=True) > 0
        assert_close(r.DenoisedColour(), want_c, f"{w}x{h} it {iterations} colour")
        assert_close(r.DenoisedVariance(), want_s, f"{w}x{h} it {iterations} variance")
    finally:
        r.close()


@pytest.mark.parametrize("iterations", ITERATIONS)
def test_guided_special_pixels(gpu, iterations):
    M, V, N = D.seeded_with_specials()
    ok = D.valid(M, V, N)
    want_c, want_s = G.reference(101, 70, iterations, special=True)
    r = _context(M, V, N, G.seeded_features(101, 70), iterations)
    try:
        r.DenoiseBuffer(guided=True)
        got_c, got_s = r.DenoisedColour(), r.DenoisedVariance()
    finally:
        r.close()
    assert_close(got_c, want_c, f"specials it {iterations} colour")
    assert_close(got_s, want_s, f"specials it {iterations} variance")
    assert np.array_equal(got_c[~ok], M[~ok], equal_nan=True)   # invalid pixels pass through
    assert not got_s[~ok].any()


def test_features_read_back_what_went_in(gpu):
    w, h = 37, 19
    feats = G.seeded_features(w, h)
    r = _context(*D.seeded(w, h), feats)
    try:
        a, n, z, k, m = r.Features()
    finally:
        r.close()
    for got, want in zip((a, n, z, k), feats):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert m.dtype == np.int32 and (m == -1).all()


def _all_hits(w, h):
    a, n, z, k = G.seeded_features(w, h)
    hit = k >= 0
    return (np.where(hit[..., None], a, 0.5), np.where(hit[..., None], n, np.float32(0.57735026)).astype(np.float32),
            np.where(hit, z, 5.0), np.where(hit, k, 0).astype(np.int32))


def test_sigmas_off_is_the_unguided_filter_and_the_unguided_filter_is_unchanged(gpu):
    """On one context: with the guide sigmas 0 and every pixel a hit the guided result is pt_denoise's bit
    for bit, and pt_denoise after features exist still matches denoise_ref."""
    for (M, V, N), special in ((D.seeded(131, 97), False), (D.seeded_with_specials(), True)):
        h, w = N.shape
        r = _context(M, V, N, _all_hits(w, h), 5, (4.0, 0.0, 0.0, 0.0))
        try:
            r.DenoiseBuffer()
            plain_c, plain_s = r.DenoisedColour(), r.DenoisedVariance()
            r.DenoiseBuffer(guided=True)
            assert np.array_equal(r.DenoisedColour(), plain_c, equal_nan=True)
            assert np.array_equal(r.DenoisedVariance(), plain_s, equal_nan=True)
            r.DenoiseGuidedParams = _abi.pt_denoise_guided_params(5, 0, 4.0, 0.3, 0.3, 0.1)
            r.DenoiseBuffer(guided=True)
            assert not np.array_equal(r.DenoisedColour(), plain_c, equal_nan=True)
            r.DenoiseBuffer()
            assert np.array_equal(r.DenoisedColour(), plain_c, equal_nan=True)
        finally:
            r.close()
        want_c, want_s = D.reference(w, h, 5, special=special)
        assert_close(plain_c, want_c, f"{w}x{h} unguided colour with features on the context")
        assert_close(plain_s, want_s, f"{w}x{h} unguided variance with features on the context")


# ------------------------------------------------------------------ state
def _furnace():
    s, c, smp = scenes.furnace()
    r = Renderer.NewRenderer(s, c, smp, 64, 48, True, device=0)
    r.SamplesPerPixel, r.Seed = 2, 7
    return r


def test_features_and_guided_denoise_leave_the_buffer_and_the_passes_alone(gpu):
    """ReadBuffer before and after RenderFeatures() and the guided filter is the same, and a context that
    renders a pass, renders features, filters, then renders another pass ends bit-identical to a twin
    that did neither; the ray counter of the pass is untouched too."""
    r, q = _furnace(), _furnace()
    try:
        r.RenderParallel()
        q.RenderParallel()
        before = _copy(r.ReadBuffer())
        rays = r.Stats().rays_total
        r.RenderFeatures()
        same_buffer(_copy(r.ReadBuffer()), before)
        r.DenoiseBuffer(guided=True)
        same_buffer(_copy(r.ReadBuffer()), before)
        assert r.Stats().rays_total == rays == q.Stats().rays_total
        feats = r.Features()
        want_c, _ = G.denoise_guided(before.M, before.V, before.N, *feats[:4])
        assert_close(r.DenoisedColour(), want_c, "furnace guided colour")
        r.RenderParallel()
        q.RenderParallel()
        two = _copy(q.ReadBuffer())
        assert (two.N == 2).all()
        same_buffer(_copy(r.ReadBuffer()), two)
        assert r.Stats().rays_total == q.Stats().rays_total
    finally:
        r.close()
        q.close()


def _gopher():
    s, c, smp = scenes.gopher3()
    smp.MaxBounces = 4
    r = Renderer.NewRenderer(s, c, smp, 64, 48, True, device=0)
    r.SamplesPerPixel, r.Seed = 2, 7
    return r


def test_guided_result_is_a_snapshot(gpu):
    r = _gopher()
    try:
        r.RenderParallel()
        r.RenderFeatures()
        r.DenoiseBuffer(guided=True)
        snap, snap_c, snap_s = r.Denoised(), r.DenoisedColour(), r.DenoisedVariance()
        first = _copy(r.ReadBuffer())
        r.RenderParallel()
        assert not np.array_equal(r.ReadBuffer().M, first.M)
        r.RenderFeatures()
        assert np.array_equal(r.Denoised(), snap)
        assert np.array_equal(r.DenoisedColour(), snap_c)
        assert np.array_equal(r.DenoisedVariance(), snap_s)
        r.DenoiseBuffer(guided=True)
        assert not np.array_equal(r.DenoisedColour(), snap_c)
    finally:
        r.close()


# ------------------------------------------------------------------ errors
def test_errors_on_a_live_context(gpu):
    w, h = 37, 19
    M, V, N = D.seeded(w, h)
    r = _context(M, V, N)   # no features, no scene
    lib = _abi.load_library()
    out = np.zeros((h, w, 4), np.float64)
    p = out.ctypes.data_as(C.c_void_p)
    ms = C.c_double(-1.0)
    cam = _abi.pt_camera()
    good = _abi.pt_denoise_guided_params(5, 0, 4.0, 0.3, 0.3, 0.1)
    feats = G.seeded_features(w, h)
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    fa, fn, fz, fk = (feats[0].ctypes.data_as(dp), feats[1].ctypes.data_as(fp), feats[2].ctypes.data_as(dp),
                      feats[3].ctypes.data_as(ip))
    try:
        # before any features: the guided filter and the read refuse, with "before" in the message
        for prm in (None, good):
            assert lib.pt_denoise_guided(r._ctx, C.byref(prm) if prm is not None else None, C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
            assert b"before" in lib.pt_last_error()
        for feature in range(5):
            assert lib.pt_read_features(r._ctx, feature, p) == _abi.PT_ERR_INVALID_ARG
            assert b"before" in lib.pt_last_error()
        with pytest.raises(_abi.PTError):
            r.Features()
        # no scene
        assert lib.pt_render_features(r._ctx, C.byref(cam), C.byref(ms)) == _abi.PT_ERR_NO_SCENE
        assert lib.pt_render_features(r._ctx, None, C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
        assert lib.pt_render_features(None, C.byref(cam), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
        # pt_write_features needs all four arrays
        for args in ((None, fn, fz, fk), (fa, None, fz, fk), (fa, fn, None, fk), (fa, fn, fz, None)):
            assert lib.pt_write_features(r._ctx, *args) == _abi.PT_ERR_INVALID_ARG
            assert lib.pt_last_error()
        assert lib.pt_write_features(None, fa, fn, fz, fk) == _abi.PT_ERR_INVALID_ARG
        assert lib.pt_read_features(r._ctx, 0, p) == _abi.PT_ERR_INVALID_ARG   # still none
        assert ms.value == -1.0 and not out.any()
        # with features: out-of-range fields
        r.LoadFeatures(*feats)
        nan, inf = float("nan"), float("inf")
        bad = [(0, 0, 4.0, 0.3, 0.3, 0.1), (9, 0, 4.0, 0.3, 0.3, 0.1), (-1, 0, 4.0, 0.3, 0.3, 0.1), (5, 1, 4.0, 0.3, 0.3, 0.1),
               (5, 0, 0.0, 0.3, 0.3, 0.1), (5, 0, -2.0, 0.3, 0.3, 0.1), (5, 0, nan, 0.3, 0.3, 0.1), (5, 0, inf, 0.3, 0.3, 0.1)]
        for i in (3, 4, 5):
            for v in (nan, inf, -0.1):
                f = [5, 0, 4.0, 0.3, 0.3, 0.1]
                f[i] = v
                bad.append(tuple(f))
        for f in bad:
            prm = _abi.pt_denoise_guided_params(*f)
            assert lib.pt_denoise_guided(r._ctx, C.byref(prm), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG, f
            assert lib.pt_last_error()
        assert lib.pt_denoise_guided(None, C.byref(good), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
        assert ms.value == -1.0
        # nothing was launched: there is still no denoised result
        assert lib.pt_read_denoised(r._ctx, 2, p) == _abi.PT_ERR_INVALID_ARG
        for feature, ptr in [(-1, p), (5, p), (0, None)]:
            assert lib.pt_read_features(r._ctx, feature, ptr) == _abi.PT_ERR_INVALID_ARG, feature
        assert lib.pt_read_features(None, 0, p) == _abi.PT_ERR_INVALID_ARG
        assert not out.any()   # nothing was written
        # NULL params are the defaults, a NULL out_kernel_ms is allowed
        assert lib.pt_denoise_guided(r._ctx, None, None) == _abi.PT_OK
        assert lib.pt_denoise_guided(r._ctx, None, C.byref(ms)) == _abi.PT_OK and ms.value > 0
        want_c, _ = G.reference(w, h, 5)
        assert_close(r.DenoisedColour(), want_c, "defaults after errors")
    finally:
        r.close()


# ------------------------------------------------------------------ quality
def _render(scene, camera, sampler, spp, passes, seed, both=False):
    r = Renderer.NewRenderer(scene, camera, sampler, 96, 64, True, device=0)
    r.SamplesPerPixel, r.Seed = spp, seed
    try:
        r.RenderPasses(passes)
        noisy = r.ReadBuffer().M.copy()
        if not both:
            return noisy
        r.DenoiseBuffer()
        plain = r.DenoisedColour()
        r.RenderFeatures()
        r.DenoiseBuffer(guided=True)
        return noisy, plain, r.DenoisedColour()
    finally:
        r.close()


@pytest.mark.parametrize("name", ["simplesphere", "example1", "example3", "textured"])
def test_guided_quality_gate(gpu, name):
    """The scenes test_features_host.py gates at 0.97 on the CPU, at its settings (96x64, four passes of
    1 spp, seed 0, defaults, against one 256-spp pass with seed 7): the guided RMSE must not exceed the
    unguided one, both from the device's own filters on the same Buffer."""
    scene, camera, sampler = getattr(scenes, name)()
    truth = _render(scene, camera, sampler, 256, 1, 7)
    noisy, plain, guided = _render(scene, camera, sampler, 1, 4, 0, both=True)
    pr, gr = D.tonemapped_rmse(plain, truth), D.tonemapped_rmse(guided, truth)
    print(f"{name}: noisy RMSE {D.tonemapped_rmse(noisy, truth):.5f}, unguided {pr:.5f}, guided {gr:.5f}, "
          f"guided / unguided {gr / pr:.3f}")
    assert gr <= pr


# ------------------------------------------------------------------ IterativeRender
def test_iterative_render_with_guided_denoise(gpu, tmp_path):
    """Denoise = DenoiseGuided = True: the returned image is Denoised() and its colour the guided
    restatement of the final Buffer with the context's features; DenoiseGuided = False (with Denoise on
    or off) is what it was: the same files, byte for byte, and the unguided result."""
    for d in ("guided", "plain", "off"):
        (tmp_path / d).mkdir()
    r = _gopher()
    try:
        r.Denoise = r.DenoiseGuided = True
        img = r.IterativeRender(str(tmp_path / "guided" / "out{0}.png"), 2)
        assert img.dtype == np.uint8 and img.shape == (48, 64, 3)
        assert np.array_equal(img, r.Denoised())
        b = _copy(r.ReadBuffer())
        feats = r.Features()
        want_c, _ = G.denoise_guided(b.M, b.V, b.N, *feats[:4])
        assert_close(r.DenoisedColour(), want_c, "after IterativeRender, guided")
    finally:
        r.close()
    r = _gopher()
    try:
        r.Denoise = True
        plain = r.IterativeRender(str(tmp_path / "plain" / "out{0}.png"), 2)
        same_buffer(_copy(r.ReadBuffer()), b)
        want_c, _ = D.denoise(b.M, b.V, b.N)
        assert_close(r.DenoisedColour(), want_c, "after IterativeRender, unguided")
        assert not np.array_equal(plain, img)
        with pytest.raises(_abi.PTError):
            r.Features()   # the unguided path never renders features
    finally:
        r.close()
    r = _gopher()
    try:
        r.DenoiseGuided = True   # without Denoise it does nothing
        off = r.IterativeRender(str(tmp_path / "off" / "out{0}.png"), 2)
        assert np.array_equal(off, r.ReadBuffer().Image())
        same_buffer(_copy(r.ReadBuffer()), b)
    finally:
        r.close()
    names = ["albedo_channel.png", "denoised_output.png", "normal_channel.png", "out1.png", "out2.png"]
    assert sorted(os.listdir(tmp_path / "guided")) == sorted(os.listdir(tmp_path / "plain")) == names
    assert sorted(os.listdir(tmp_path / "off")) == ["out1.png", "out2.png"]
    for n in names:
        same = (tmp_path / "guided" / n).read_bytes() == (tmp_path / "plain" / n).read_bytes()
        assert same == (n != "denoised_output.png"), n
    for i in (1, 2):
        assert (tmp_path / "off" / f"out{i}.png").read_bytes() == (tmp_path / "plain" / f"out{i}.png").read_bytes()
