"""pt_read_image on the GPU: a Buffer channel resolved to 8-bit RGB / RGBA on the device
(ptsharp_amd/csrc/pt_image.hip) against Buffer.cs restated in image_ref.py.  Buffers are injected
with LoadBuffer, so no test but the two render tests needs a scene.

Color, StdDev and Normal go through pow, sqrt and divisions that are accurate to about an ulp on
both sides, so two correct implementations can differ only where c·255 lies within 1e-9 of an
integer: every comparison of those channels first asserts that its input holds no such value
(image_ref.near_boundary), then demands byte equality."""
import ctypes as C

import numpy as np
import pytest

import image_ref as R
from parity import same_buffer
from ptsharp_amd import Renderer, _abi, scenes, tiles_for_rank
from ptsharp_amd.renderer import Buffer, Channel, write_png

pytestmark = pytest.mark.gpu

NAMES = {R.COLOR: "Color", R.VARIANCE: "Variance", R.STDDEV: "StdDev", R.SAMPLES: "Samples", R.ALBEDO: "Albedo",
         R.NORMAL: "Normal"}
INEXACT = (R.COLOR, R.STDDEV, R.NORMAL)


def _buffer(M, V, N) -> Buffer:
    b = Buffer(N.shape[1], N.shape[0])
    b.M, b.V, b.N = M, V, N
    return b


def _context(w, h, M=None, V=None, N=None) -> Renderer:
    r = Renderer.NewRenderer(None, None, None, w, h, True, device=0)
    if N is not None:
        r.LoadBuffer(_buffer(M, V, N), passes_done=0)
    return r


def _reference(M, V, N, ch):
    """image_ref's bytes for channel ch, after asserting the input is clear of byte boundaries."""
    col = R.colour(M, V, N, ch)
    if ch in INEXACT:
        assert not R.near_boundary(col).any(), f"{NAMES[ch]}: the input has values on a byte boundary"
    return R.to_bytes(col)


def _assert_image(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, what
    bad = (got != want).any(axis=2)
    assert not bad.any(), (f"{what}: {int(bad.sum())} pixels differ, first (y, x) = {np.argwhere(bad)[0]}: "
                           f"{got[bad][0]} vs {want[bad][0]}")


def _check_all_channels(r, M, V, N, what):
    for ch in R.CHANNELS:
        _assert_image(r.Image(Channel(ch)), _reference(M, V, N, ch), f"{what} {NAMES[ch]}")


@pytest.fixture(scope="module")
def seeded_context(gpu):
    M, V, N, cols, imgs = R.seeded_101x70()
    r = _context(101, 70, M, V, N)
    yield r
    r.close()


@pytest.mark.parametrize("rgba", [False, True], ids=["rgb8", "rgba8"])
@pytest.mark.parametrize("ch", R.CHANNELS, ids=[NAMES[c] for c in R.CHANNELS])
def test_read_image_written_buffer(seeded_context, ch, rgba):
    """101x70: an odd width, RGB8 rows that are not dword-aligned, P % 4 = 2, both dimensions off the
    32-pixel tile grid."""
    M, V, N, cols, imgs = R.seeded_101x70()
    if ch in INEXACT:
        assert not R.near_boundary(cols[ch]).any()
    got = seeded_context.Image(Channel(ch), rgba=rgba)
    assert got.shape == (70, 101, 4 if rgba else 3)
    _assert_image(got[..., :3], imgs[ch], NAMES[ch])
    if rgba:
        assert (got[..., 3] == 255).all()


def test_read_image_special_values(gpu):
    """33x2 of 0, -0.0, 1, 2, 1e300, +inf, -1 and NaN in M (one pixel with a single NaN component, one
    all-equal pixel), a negative V, N in {0, 1, 2, -1, 3}; then an empty Buffer's Samples image."""
    M, V, N = R.special_rows(33)
    assert np.isnan(M).any() and np.isinf(M).any() and (M == 1e300).any() and (M < 0).any() and np.signbit(M[M == 0]).any()
    assert (np.isnan(M).sum(axis=2) == 1).any() and ((M[..., 0] == M[..., 1]) & (M[..., 1] == M[..., 2]) & (M[..., 0] > 0)).any()
    assert (V < 0).any() and set(np.unique(N)) >= {0, 1, 2, -1}
    r = _context(33, 2, M, V, N)
    try:
        _check_all_channels(r, M, V, N, "special")
        rgba = r.Image(Channel.AlbedoChannel, rgba=True)
        _assert_image(rgba[..., :3], _reference(M, V, N, R.ALBEDO), "special Albedo rgba")
        assert (rgba[..., 3] == 255).all()
        zero = np.zeros_like(N)
        r.LoadBuffer(_buffer(M, V, zero), passes_done=0)
        got = r.Image(Channel.SamplesChannel)
        assert not got.any()
        _assert_image(got, R.image(M, V, zero, R.SAMPLES), "empty Samples")
    finally:
        r.close()


# P < 4 (2x1, 3x1), every P % 4 (4x1: 0, 1x5: 1, 2x3 and 2x1: 2, 7x1 and 257x3: 3), Normal stencils with
# a single in-image neighbour (2x1) or none above and below (7x1) or beside (1x5), and a row longer than
# one block (257).  A 1x1 context cannot be made: pt_create refuses it (test_abi.py::
# test_bad_dimensions_rejected pins that), so its empty stencil is covered on the host alone
# (pt_image.h is the kernel's text: test_image_host.py).
@pytest.mark.parametrize("w,h", [(2, 1), (3, 1), (4, 1), (2, 3), (7, 1), (1, 5), (257, 3)])
def test_read_image_small_shapes(gpu, w, h):
    M, V, N = R.seeded(w, h, seed=1000 * w + h)
    r = _context(w, h, M, V, N)
    try:
        _check_all_channels(r, M, V, N, f"{w}x{h}")
        got = r.Image(Channel.ColorChannel, rgba=True)
        _assert_image(got[..., :3], _reference(M, V, N, R.COLOR), f"{w}x{h} Color rgba")
        assert (got[..., 3] == 255).all()
    finally:
        r.close()


def _gopher(tiles=None):
    s, c, smp = scenes.gopher3()
    smp.MaxBounces = 4
    r = Renderer.NewRenderer(s, c, smp, 64, 48, True, device=0)
    r.SamplesPerPixel, r.Seed, r.Tiles = 2, 7, tiles
    return r


def _copy(b) -> Buffer:
    return _buffer(b.M.copy(), b.V.copy(), b.N.copy())


@pytest.mark.parametrize("sharded", [False, True], ids=["whole", "rank1of2"])
def test_read_image_after_render_and_tiles(gpu, sharded):
    """After two passes (whole frame; then rank 1 of 2's tiles, zero elsewhere) every channel equals
    image_ref of ReadBuffer(); the call leaves the Buffer and the pass state as they were."""
    tiles = tiles_for_rank(64, 48, 1, 2) if sharded else None
    r, q = _gopher(tiles), _gopher(tiles)
    try:
        for _ in range(2):
            r.RenderParallel()
            q.RenderParallel()
        before = _copy(r.ReadBuffer())
        if sharded:
            assert (before.N > 0).any() and (before.N == 0).any()
        for ch in R.CHANNELS:
            want = _reference(before.M, before.V, before.N, ch)
            _assert_image(r.Image(Channel(ch)), want, NAMES[ch])
            _assert_image(r.Image(Channel(ch), rgba=True)[..., :3], want, NAMES[ch] + " rgba")
        same_buffer(_copy(r.ReadBuffer()), before)
        r.RenderParallel()
        q.RenderParallel()
        three = _copy(q.ReadBuffer())
        same_buffer(_copy(r.ReadBuffer()), three)
    finally:
        r.close()
        q.close()


def test_read_image_errors(gpu):
    r = _gopher()
    lib = _abi.load_library()
    out = np.zeros((48, 64, 4), np.uint8)
    p = out.ctypes.data_as(C.POINTER(C.c_uint8))
    try:
        for channel, fmt, ptr in [(-1, 0, p), (6, 0, p), (0, 2, p), (0, -1, p), (0, 0, None)]:
            assert lib.pt_read_image(r._ctx, channel, fmt, ptr) == _abi.PT_ERR_INVALID_ARG, (channel, fmt)
            assert lib.pt_last_error()
        assert lib.pt_read_image(None, 0, 0, p) == _abi.PT_ERR_INVALID_ARG
        assert lib.pt_last_error()
        assert not out.any()   # nothing was written
        r.RenderParallel()
        b = _copy(r.ReadBuffer())
        assert (b.N > 0).all()
        _assert_image(r.Image(Channel.ColorChannel), _reference(b.M, b.V, b.N, R.COLOR), "Color after errors")
    finally:
        r.close()


def test_iterative_render_device_images(gpu, tmp_path):
    """IterativeRender with DeviceImages writes the default path's PNG files, returns its array and
    leaves Renderer.PBuffer equal to the device's Buffer."""
    (tmp_path / "host").mkdir()
    (tmp_path / "dev").mkdir()
    r = _gopher()
    try:
        host = r.IterativeRender(str(tmp_path / "host" / "out{0}.png"), 2)
        final = _copy(r.ReadBuffer())
    finally:
        r.close()
    assert not R.near_boundary(R.colour(final.M, final.V, final.N, R.COLOR)).any()
    r = _gopher()
    try:
        r.DeviceImages = True
        dev = r.IterativeRender(str(tmp_path / "dev" / "out{0}.png"), 2)
        pbuf = _copy(Renderer.PBuffer)
        same_buffer(pbuf, _copy(r.ReadBuffer()))
        same_buffer(pbuf, final)
    finally:
        r.close()
    assert dev.dtype == np.uint8 and dev.shape == (48, 64, 3)
    assert np.array_equal(dev, host)
    for i in (1, 2):
        a, b = [(tmp_path / d / f"out{i}.png").read_bytes() for d in ("host", "dev")]
        assert a == b and len(a) > 100, i
    # the second file is the returned image
    ref = tmp_path / "ref.png"
    write_png(str(ref), host)
    assert ref.read_bytes() == (tmp_path / "dev" / "out2.png").read_bytes()
