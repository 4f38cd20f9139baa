"""The denoiser on the host side of pt_denoise (no GPU): the per-pixel text the kernels run
(ptsharp_amd/csrc/pt_denoise.h, built here with g++ into tests/native/denoise_check.cpp) against the
numpy restatement in denoise_ref.py, properties of the filter that need no restatement, the ABI
declarations, and IterativeRender's use of the entry points.

Both sides do the same fp64 operations in the same order; only the last bit of exp and of a division
may differ, so a final difference of about 1e-15 is expected and the bar is rtol 1e-11, atol 1e-13."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import denoise_ref as D
from ptsharp_amd import _abi
from ptsharp_amd.renderer import Renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-11, 1e-13
SHAPES = [(1, 1), (2, 1), (7, 1), (1, 5), (5, 4), (37, 19), (101, 70)]
ITERATIONS = [1, 5, 8]


@pytest.fixture(scope="module")
def denoise_check(tmp_path_factory):
    """tests/native/denoise_check.cpp (pt_denoise.h under plain g++), built once."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/native/denoise_check.cpp"
    exe = tmp_path_factory.mktemp("denoise_check") / "denoise_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "denoise_check.cpp")], check=True)
    return str(exe)


def run_check(exe, tmp_path, M, V, N, iterations=5, sigma=4.0):
    H, W = np.asarray(N).shape
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([W, H, iterations, 0], np.int32).tobytes() + np.array([sigma], np.float64).tobytes() +
                np.ascontiguousarray(M, np.float64).tobytes() + np.ascontiguousarray(V, np.float64).tobytes() +
                np.ascontiguousarray(N, np.int32).tobytes())
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    out = np.fromfile(tmp_path / "out.bin", np.float64).reshape(2, H, W, 3)
    return out[0], out[1]


def assert_close(got, want, what):
    """Within the bar, NaN and inf (invalid pixels passed through) in the same places; prints the
    largest difference."""
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), what
    diff = np.abs(got[fin] - want[fin])
    rel = diff / np.maximum(np.abs(want[fin]), 1e-300)
    print(f"{what}: max abs diff {diff.max() if diff.size else 0:.3g}, max rel diff {rel.max() if rel.size else 0:.3g}")
    np.testing.assert_allclose(got[fin], want[fin], rtol=RTOL, atol=ATOL, err_msg=what)


@pytest.mark.parametrize("iterations", ITERATIONS)
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_host_matches_restatement(denoise_check, tmp_path, w, h, iterations):
    M, V, N = D.seeded(w, h)
    want_c, want_s = D.reference(w, h, iterations)
    got_c, got_s = run_check(denoise_check, tmp_path, M, V, N, iterations)
    assert_close(got_c, want_c, f"{w}x{h} it {iterations} colour")
    assert_close(got_s, want_s, f"{w}x{h} it {iterations} variance")


@pytest.mark.parametrize("iterations", ITERATIONS)
def test_host_special_pixels(denoise_check, tmp_path, iterations):
    M, V, N = D.seeded_with_specials()
    ok = D.valid(M, V, N)
    assert np.isnan(M).any() and np.isposinf(M).any() and np.isposinf(V).any() and (N == 0).any() and (N == 1).any()
    assert not ok[32:64, 64:96].any() and (M == 1e6).any()
    assert ((V == 0).all(axis=2) & (N >= 2)).any()
    want_c, want_s = D.reference(101, 70, iterations, special=True)
    got_c, got_s = run_check(denoise_check, tmp_path, M, V, N, iterations)
    assert_close(got_c, want_c, f"specials it {iterations} colour")
    assert_close(got_s, want_s, f"specials it {iterations} variance")
    # invalid pixels come back as they went in, with variance 0
    assert np.array_equal(got_c[~ok], M[~ok], equal_nan=True)
    assert not got_s[~ok].any()
    assert np.isfinite(got_c[ok]).all() and np.isfinite(got_s[ok]).all()


def test_host_firefly_with_its_variance_one_level(denoise_check, tmp_path):
    M, V, N = D.firefly_with_its_variance()
    want_c, want_s = D.denoise(M, V, N, 1)
    got_c, got_s = run_check(denoise_check, tmp_path, M, V, N, 1)
    assert want_s.max() > 1e9 and (want_c[9, 19:22] > 10).all()   # the firefly spreads to its neighbours
    assert_close(got_c, want_c, "firefly colour")
    assert_close(got_s, want_s, "firefly variance")


def test_sigma_changes_the_result(denoise_check, tmp_path):
    """A guard for the comparisons above: the colour weight is live (a filter that ignored it would
    still match a restatement that ignored it)."""
    M, V, N = D.seeded(37, 19)
    a, _ = run_check(denoise_check, tmp_path, M, V, N, 5, 4.0)
    b, _ = run_check(denoise_check, tmp_path, M, V, N, 5, 0.5)
    assert np.abs(a - b).max() > 1e-3


def test_constant_image_is_a_fixed_point(denoise_check, tmp_path):
    """Every weight is h: the colour comes back within 1e-15 relative, and one level turns a constant
    variance s into s·Σh²/(Σh)² over the taps inside the image."""
    w, h, n = 23, 17, 4
    col = np.array([0.3, 0.7, 1.9])
    M = np.broadcast_to(col, (h, w, 3)).copy()
    s = np.array([2e-3, 5e-4, 1e-2])
    V = np.broadcast_to(s * (n - 1) * n, (h, w, 3)).copy()
    N = np.full((h, w), n, np.int32)
    for iterations in (1, 5):
        got_c, got_s = run_check(denoise_check, tmp_path, M, V, N, iterations)
        assert np.abs(got_c / col - 1.0).max() <= 1e-15
    got_c, got_s = run_check(denoise_check, tmp_path, M, V, N, 1)
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    for y, x in [(0, 0), (8, 11), (1, 21), (16, 22)]:
        ky = np.array([k[d + 2] if 0 <= y + d < h else 0.0 for d in range(-2, 3)])
        kx = np.array([k[d + 2] if 0 <= x + d < w else 0.0 for d in range(-2, 3)])
        hh = np.outer(ky, kx)
        np.testing.assert_allclose(got_s[y, x], s * (hh ** 2).sum() / hh.sum() ** 2, rtol=1e-13)


def test_huge_sigma_is_the_plain_atrous_blur(denoise_check, tmp_path):
    """sigma_colour = 1e30: every exp(−d) is 1, and the filter is the renormalised B3-spline à-trous
    blur of the valid pixels (convolved separately, pixel by pixel)."""
    M, V, N = D.seeded(19, 13)
    M, V, N = M.copy(), V.copy(), N.copy()
    N[4, 7] = 0
    M[9, 2, 1] = np.nan
    ok = D.valid(M, V, N)
    for iterations in (1, 3):
        got_c, _ = run_check(denoise_check, tmp_path, M, V, N, iterations, 1e30)
        want = D.atrous_blur(M, ok, iterations)
        np.testing.assert_allclose(got_c[ok], want[ok], rtol=1e-13, atol=0)
        assert np.array_equal(got_c[~ok], M[~ok], equal_nan=True)


def test_step_edge_with_zero_variance_is_unchanged(denoise_check, tmp_path):
    w, h = 40, 12
    M = np.zeros((h, w, 3))
    M[:, :17] = [0.1, 0.2, 0.3]
    M[:, 17:] = [0.8, 0.6, 0.9]
    V = np.zeros((h, w, 3))
    N = np.full((h, w), 3, np.int32)
    got_c, got_s = run_check(denoise_check, tmp_path, M, V, N, 5)
    # across the edge d is about 1e12 and exp(−d) is exactly 0; on its own side a pixel is the
    # normalised sum of equal values, so it comes back to the rounding of that sum (1e-15 relative,
    # as for the constant image), four orders below the smallest step of the edge
    np.testing.assert_allclose(got_c, M, rtol=1e-15, atol=0)
    assert not got_s.any()


# ------------------------------------------------------------------ ABI
def test_abi_denoise():
    assert _abi.SIGNATURES["pt_denoise"] == (C.c_int, [C.c_void_p, C.POINTER(_abi.pt_denoise_params), C.POINTER(C.c_double)])
    assert _abi.SIGNATURES["pt_read_denoised"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p])
    src = open(os.path.join(ROOT, "include", "ptsharp_hip.h")).read()
    assert re.search(r"int pt_denoise\(void\* ctx, const pt_denoise_params\* params, double\* out_kernel_ms\);", src)
    assert re.search(r"int pt_read_denoised\(void\* ctx, int32_t format, void\* out\);", src)
    body = re.search(r"typedef struct pt_denoise_params \{(.*?)\} pt_denoise_params;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [tuple(d.split()) for d in body.split(";") if d.strip()]
    assert fields == [("int32_t", "iterations"), ("int32_t", "reserved"), ("double", "sigma_colour")]
    ctypes_of = {"int32_t": C.c_int32, "double": C.c_double}
    assert _abi.pt_denoise_params._fields_ == [(name, ctypes_of[t]) for t, name in fields]
    assert C.sizeof(_abi.pt_denoise_params) == 16 and _abi.pt_denoise_params.sigma_colour.offset == 8
    fmt = dict((k, int(v)) for k, v in re.findall(r"PT_DENOISED_(\w+) = (\d+)", src))
    assert fmt == {"RGB8": _abi.DENOISED_RGB8, "RGBA8": _abi.DENOISED_RGBA8, "COLOUR_F64": _abi.DENOISED_COLOUR_F64,
                   "VARIANCE_F64": _abi.DENOISED_VARIANCE_F64}
    cs = open(os.path.join(ROOT, "csharp", "HipRenderer.cs")).read()
    cs_body = re.search(r"struct pt_denoise_params\s*\{(.*?)\}", cs, re.S).group(1)
    assert re.findall(r"public (\w+) (\w+);", cs_body) == [("int", "iterations"), ("int", "reserved"), ("double", "sigma_colour")]


def test_abi_version_and_invalid_arguments_without_a_context():
    lib = _abi.load_library()
    assert lib.pt_get_version() == 10 == _abi.ABI_VERSION
    ms = C.c_double(-1.0)
    out = (C.c_uint8 * 64)()
    good = _abi.pt_denoise_params(5, 0, 4.0)
    cases = [None, good, _abi.pt_denoise_params(0, 0, 4.0), _abi.pt_denoise_params(9, 0, 4.0),
             _abi.pt_denoise_params(5, 1, 4.0), _abi.pt_denoise_params(5, 0, 0.0), _abi.pt_denoise_params(5, 0, -1.0),
             _abi.pt_denoise_params(5, 0, float("nan")), _abi.pt_denoise_params(5, 0, float("inf"))]
    for p in cases:
        assert lib.pt_denoise(None, C.byref(p) if p is not None else None, C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
        assert lib.pt_last_error()
    assert ms.value == -1.0
    for fmt in (-1, 0, 1, 2, 3, 4):
        assert lib.pt_read_denoised(None, fmt, out) == _abi.PT_ERR_INVALID_ARG
        assert lib.pt_last_error()
    assert not any(out)


# ------------------------------------------------------------------ IterativeRender
class _StubLibrary:
    """Stands in for libptsharp_hip.so: every entry point records its name and reports success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("pt_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append(name)
            return _abi.PT_OK
        return entry


class _Compiled:
    desc = _abi.pt_scene_desc()


class _StubScene:
    _flat = _Compiled()

    def Compile(self):
        return self._flat


class _StubToC:
    def __init__(self, c):
        self._c = c

    def to_c(self):
        return self._c


def _stub_renderer(lib, w=8, h=6):
    r = Renderer()
    r.Scene, r.Camera, r.Sampler = _StubScene(), _StubToC(_abi.pt_camera()), _StubToC(_abi.pt_sampler())
    r.W, r.H = w, h
    r._lib, r._ctx = lib, C.c_void_p(1)
    return r


@pytest.mark.parametrize("device_images", [False, True])
def test_iterative_render_without_denoise_never_calls_the_denoiser(tmp_path, device_images):
    lib = _StubLibrary()
    r = _stub_renderer(lib)
    r.DeviceImages = device_images
    assert r.Denoise is False
    try:
        r.IterativeRender(str(tmp_path / "out{0}.png"), 2)
        r.IterativeRender(None, 1)
    finally:
        r._ctx = None
    assert "pt_render_pass" in lib.calls
    assert not [c for c in lib.calls if "denois" in c]
    assert sorted(os.listdir(tmp_path)) == ["out1.png", "out2.png"]


def test_iterative_render_with_denoise_calls_the_denoiser(tmp_path):
    lib = _StubLibrary()
    r = _stub_renderer(lib)
    r.Denoise = True
    try:
        img = r.IterativeRender(str(tmp_path / "out{0}.png"), 2)
        assert lib.calls.count("pt_denoise") == 2 and lib.calls.count("pt_read_denoised") == 2
        r.IterativeRender(None, 3)
        assert lib.calls.count("pt_denoise") == 3 and lib.calls.count("pt_read_denoised") == 3
    finally:
        r._ctx = None
    assert img.shape == (6, 8, 3) and img.dtype == np.uint8
    assert sorted(os.listdir(tmp_path)) == ["albedo_channel.png", "denoised_output.png", "normal_channel.png", "out1.png",
                                            "out2.png"]
    assert (r.DenoiseParams.iterations, r.DenoiseParams.reserved, r.DenoiseParams.sigma_colour) == (5, 0, 4.0)
