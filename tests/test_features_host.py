"""The feature-guided denoiser on the host side of pt_denoise_guided (no GPU): the ABI declarations, the
per-pixel text the guided kernels run (ptsharp_amd/csrc/pt_denoise.h, built here with g++ into
tests/native/denoise_guided_check.cpp) against the numpy restatement in denoise_guided_ref.py,
properties of the guided filter that need no restatement, and the chosen default sigmas' quality table.

Both sides do the same fp64 operations in the same order; only the last bit of exp and of a division
may differ, so the bar is the unguided filter's: rtol 1e-11, atol 1e-13 (test_denoise_host.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import denoise_guided_ref as G
import denoise_ref as D
import features_ref as F
from ptsharp_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-11, 1e-13
SHAPES = [(1, 1), (2, 1), (7, 1), (1, 5), (5, 4), (37, 19), (101, 70)]
ITERATIONS = [1, 5, 8]
SIGMAS = (4.0, 0.3, 0.3, 0.1)   # colour, normal, albedo, depth: the defaults


def _build(tmp_path_factory, name):
    cxx = shutil.which("g++")
    assert cxx, f"g++ is needed to build tests/native/{name}.cpp"
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", f"{name}.cpp")], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def guided_check(tmp_path_factory):
    """tests/native/denoise_guided_check.cpp (pt_denoise.h's guided level under plain g++), built once."""
    return _build(tmp_path_factory, "denoise_guided_check")


@pytest.fixture(scope="module")
def denoise_check(tmp_path_factory):
    """tests/native/denoise_check.cpp: the unguided filter, for the bit-for-bit comparison."""
    return _build(tmp_path_factory, "denoise_check")


def run_guided(exe, tmp_path, M, V, N, feats, iterations=5, sigmas=SIGMAS):
    albedo, normal, depth, kind = feats
    H, W = np.asarray(N).shape
    with open(tmp_path / "gin.bin", "wb") as f:
        f.write(np.array([W, H, iterations, 0], np.int32).tobytes() + np.array(sigmas, np.float64).tobytes() +
                np.ascontiguousarray(M, np.float64).tobytes() + np.ascontiguousarray(V, np.float64).tobytes() +
                np.ascontiguousarray(N, np.int32).tobytes() + np.ascontiguousarray(albedo, np.float64).tobytes() +
                np.ascontiguousarray(normal, np.float32).tobytes() + np.ascontiguousarray(depth, np.float64).tobytes() +
                np.ascontiguousarray(kind, np.int32).tobytes())
    subprocess.run([exe, str(tmp_path / "gin.bin"), str(tmp_path / "gout.bin")], check=True)
    out = np.fromfile(tmp_path / "gout.bin", np.float64).reshape(2, H, W, 3)
    return out[0], out[1]


def run_plain(exe, tmp_path, M, V, N, iterations=5, sigma=4.0):
    H, W = np.asarray(N).shape
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([W, H, iterations, 0], np.int32).tobytes() + np.array([sigma], np.float64).tobytes() +
                np.ascontiguousarray(M, np.float64).tobytes() + np.ascontiguousarray(V, np.float64).tobytes() +
                np.ascontiguousarray(N, np.int32).tobytes())
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    out = np.fromfile(tmp_path / "out.bin", np.float64).reshape(2, H, W, 3)
    return out[0], out[1]


def assert_close(got, want, what):
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), what
    diff = np.abs(got[fin] - want[fin])
    rel = diff / np.maximum(np.abs(want[fin]), 1e-300)
    print(f"{what}: max abs diff {diff.max() if diff.size else 0:.3g}, max rel diff {rel.max() if rel.size else 0:.3g}")
    np.testing.assert_allclose(got[fin], want[fin], rtol=RTOL, atol=ATOL, err_msg=what)


# ------------------------------------------------------------------ ABI
def test_abi_features_and_guided_denoise():
    S = _abi.SIGNATURES
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    assert S["pt_render_features"] == (C.c_int, [C.c_void_p, C.POINTER(_abi.pt_camera), dp])
    assert S["pt_read_features"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p])
    assert S["pt_write_features"] == (C.c_int, [C.c_void_p, dp, fp, dp, ip])
    assert S["pt_denoise_guided"] == (C.c_int, [C.c_void_p, C.POINTER(_abi.pt_denoise_guided_params), dp])
    src = open(os.path.join(ROOT, "include", "ptsharp_hip.h")).read()
    assert re.search(r"int pt_render_features\(void\* ctx, const pt_camera\* camera, double\* out_kernel_ms\);", src)
    assert re.search(r"int pt_read_features\(void\* ctx, int32_t feature, void\* out\);", src)
    assert re.search(r"int pt_write_features\(void\* ctx, const double\* albedo, const float\* normal, const double\* depth, "
                     r"const int32_t\* kind\);", src)
    assert re.search(r"int pt_denoise_guided\(void\* ctx, const pt_denoise_guided_params\* params, double\* out_kernel_ms\);", src)
    body = re.search(r"typedef struct pt_denoise_guided_params \{(.*?)\} pt_denoise_guided_params;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [tuple(d.split()) for d in body.split(";") if d.strip()]
    assert fields == [("int32_t", "iterations"), ("int32_t", "reserved"), ("double", "sigma_colour"), ("double", "sigma_normal"),
                      ("double", "sigma_albedo"), ("double", "sigma_depth")]
    ctypes_of = {"int32_t": C.c_int32, "double": C.c_double}
    assert _abi.pt_denoise_guided_params._fields_ == [(name, ctypes_of[t]) for t, name in fields]
    assert C.sizeof(_abi.pt_denoise_guided_params) == 40 and _abi.pt_denoise_guided_params.sigma_depth.offset == 32
    feat = dict((k, int(v)) for k, v in re.findall(r"PT_FEATURE_(\w+) = (\d+)", src))
    assert feat == {"ALBEDO_F64": _abi.FEATURE_ALBEDO_F64, "NORMAL_F32": _abi.FEATURE_NORMAL_F32,
                    "DEPTH_F64": _abi.FEATURE_DEPTH_F64, "KIND_I32": _abi.FEATURE_KIND_I32,
                    "MATERIAL_I32": _abi.FEATURE_MATERIAL_I32} == {"ALBEDO_F64": 0, "NORMAL_F32": 1, "DEPTH_F64": 2,
                                                                   "KIND_I32": 3, "MATERIAL_I32": 4}
    cs = open(os.path.join(ROOT, "csharp", "HipRenderer.cs")).read()
    cs_body = re.search(r"struct pt_denoise_guided_params\s*\{(.*?)\}", cs, re.S).group(1)
    assert re.findall(r"public (\w+) (\w+);", cs_body) == [("int", "iterations"), ("int", "reserved"), ("double", "sigma_colour"),
                                                           ("double", "sigma_normal"), ("double", "sigma_albedo"),
                                                           ("double", "sigma_depth")]
    for name in ("RenderFeatures", "ReadFeatures", "DenoiseGuided"):
        assert re.search(r"public [^;{]*\b%s\b" % name, cs), name


def test_abi_version_and_invalid_arguments_without_a_context():
    lib = _abi.load_library()
    assert lib.pt_get_version() == 10 == _abi.ABI_VERSION
    ms = C.c_double(-1.0)
    out = (C.c_uint8 * 64)()
    cam = _abi.pt_camera()
    good = _abi.pt_denoise_guided_params(5, 0, 4.0, 0.3, 0.1, 0.1)
    for p in (None, good, _abi.pt_denoise_guided_params(0, 0, 4.0, 0.3, 0.1, 0.1)):
        assert lib.pt_denoise_guided(None, C.byref(p) if p is not None else None, C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
        assert lib.pt_last_error()
    assert lib.pt_render_features(None, C.byref(cam), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
    assert lib.pt_render_features(None, None, None) == _abi.PT_ERR_INVALID_ARG
    assert lib.pt_write_features(None, None, None, None, None) == _abi.PT_ERR_INVALID_ARG
    assert ms.value == -1.0
    for feature in (-1, 0, 1, 2, 3, 4, 5):
        assert lib.pt_read_features(None, feature, out) == _abi.PT_ERR_INVALID_ARG
        assert lib.pt_last_error()
    assert not any(out)


# ------------------------------------------------------------------ host program against the restatement
@pytest.mark.parametrize("iterations", ITERATIONS)
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_host_matches_restatement(guided_check, tmp_path, w, h, iterations):
    M, V, N = D.seeded(w, h)
    want_c, want_s = G.reference(w, h, iterations)
    got_c, got_s = run_guided(guided_check, tmp_path, M, V, N, G.seeded_features(w, h), iterations)
    assert_close(got_c, want_c, f"{w}x{h} it {iterations} colour")
    assert_close(got_s, want_s, f"{w}x{h} it {iterations} variance")


@pytest.mark.parametrize("iterations", ITERATIONS)
def test_host_special_pixels(guided_check, tmp_path, iterations):
    M, V, N = D.seeded_with_specials()
    ok = D.valid(M, V, N)
    want_c, want_s = G.reference(101, 70, iterations, special=True)
    got_c, got_s = run_guided(guided_check, tmp_path, M, V, N, G.seeded_features(101, 70), iterations)
    assert_close(got_c, want_c, f"specials it {iterations} colour")
    assert_close(got_s, want_s, f"specials it {iterations} variance")
    assert np.array_equal(got_c[~ok], M[~ok], equal_nan=True)   # invalid pixels pass through
    assert not got_s[~ok].any()
    assert np.isfinite(got_c[ok]).all() and np.isfinite(got_s[ok]).all()


def test_seeded_features_have_every_region():
    a, n, z, k = G.seeded_features(37, 19)
    assert set(np.unique(k)) == {-1, 0, 1, 2}
    miss = k < 0
    assert (z[miss] == 1e9).all() and not n[miss].any() and (z[~miss] < 10).all()
    np.testing.assert_allclose(np.linalg.norm(n[~miss].astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert n.dtype == np.float32 and a.dtype == z.dtype == np.float64 and k.dtype == np.int32


# ------------------------------------------------------------------ properties that need no restatement
def _all_hits(w, h):
    a, n, z, k = G.seeded_features(w, h)
    hit = k >= 0
    fill = lambda x, v: np.where(hit[..., None] if x.ndim == 3 else hit, x, v).astype(x.dtype)   # noqa: E731
    return fill(a, 0.5), fill(n, np.float32(0.57735026)), fill(z, 5.0), np.where(hit, k, 0).astype(np.int32)


@pytest.mark.parametrize("iterations", [1, 5])
def test_sigmas_off_and_all_hits_is_the_unguided_filter_bit_for_bit(guided_check, denoise_check, tmp_path, iterations):
    for M, V, N in (D.seeded(37, 19), D.seeded_with_specials()):
        h, w = N.shape
        got_c, got_s = run_guided(guided_check, tmp_path, M, V, N, _all_hits(w, h), iterations, (4.0, 0.0, 0.0, 0.0))
        want_c, want_s = run_plain(denoise_check, tmp_path, M, V, N, iterations)
        assert np.array_equal(got_c, want_c, equal_nan=True)
        assert np.array_equal(got_s, want_s, equal_nan=True)


def _alone(M, V, N, keep):
    """The Buffer with every pixel outside `keep` made invalid (N = 0)."""
    return M, V, np.where(keep, N, 0).astype(np.int32)


def _noisy_with_flat_variance(w, h):
    """seeded(w, h)'s noisy colour with N >= 2 and a variance of the mean of exactly 2^-8 on every pixel
    and channel: V = 2^-8·(N−1)·N is exact, so is its quotient, and the 3x3 blur of a power of two over
    any set of taps returns it exactly.  Prepare (which is pt_denoise's and does look across a feature
    border) then gives the same s2 whether or not the other side is valid, and the comparison below is
    of the guided levels alone."""
    M, V, N = D.seeded(w, h)
    N = np.maximum(N, 2)
    V = np.zeros_like(M) + (2.0 ** -8 * (N - 1.0) * N)[..., None]
    return M, V, N


def test_hit_flag_partitions_the_filter(guided_check, tmp_path):
    """Each side of the hit / miss border equals the filter run on that side alone, the other side
    invalid: a tap across the border is skipped exactly like an invalid one."""
    M, V, N = _noisy_with_flat_variance(37, 19)
    feats = G.seeded_features(37, 19)
    hit = feats[3] >= 0
    assert hit.any() and (~hit).any()
    for sig in (SIGMAS, (4.0, 0.0, 0.0, 0.0)):
        both_c, both_s = run_guided(guided_check, tmp_path, M, V, N, feats, 5, sig)
        for side in (hit, ~hit):
            c, s = run_guided(guided_check, tmp_path, *_alone(M, V, N, side), feats, 5, sig)
            assert np.array_equal(c[side], both_c[side])
            assert np.array_equal(s[side], both_s[side])
    # and the border does matter: with every pixel a hit the two sides mix
    mixed_c, _ = run_guided(guided_check, tmp_path, M, V, N, _all_hits(37, 19), 5, (4.0, 0.0, 0.0, 0.0))
    assert np.abs(mixed_c - both_c).max() > 1e-3


def test_albedo_step_separates_the_sides(guided_check, tmp_path):
    """An albedo step of 30 at sigma_albedo 0.1 gives a distance of 3·30²/0.01 = 270000, and exp(−d)
    is exactly 0: under noisy colour with N >= 2 each side equals the filter run on that side alone."""
    w, h = 37, 19
    M, V, N = _noisy_with_flat_variance(w, h)
    left = np.mgrid[0:h, 0:w][1] < 17
    albedo = np.where(left[..., None], 0.25, 30.25) + np.zeros((h, w, 3))
    normal = np.zeros((h, w, 3), np.float32)
    normal[..., 2] = 1.0
    feats = (albedo, normal, np.full((h, w), 4.0), np.zeros((h, w), np.int32))
    both_c, both_s = run_guided(guided_check, tmp_path, M, V, N, feats, 5, (4.0, 0.0, 0.1, 0.0))
    plain_c, _ = run_guided(guided_check, tmp_path, M, V, N, feats, 5, (4.0, 0.0, 0.0, 0.0))
    assert np.abs(both_c - plain_c).max() > 1e-3   # without the term the sides do mix
    for side in (left, ~left):
        c, s = run_guided(guided_check, tmp_path, *_alone(M, V, N, side), feats, 5, (4.0, 0.0, 0.1, 0.0))
        assert np.array_equal(c[side], both_c[side])
        assert np.array_equal(s[side], both_s[side])


def test_each_sigma_changes_the_result(guided_check, tmp_path):
    """A guard for the comparisons above: each guide term is live."""
    M, V, N = D.seeded(37, 19)
    feats = G.seeded_features(37, 19)
    base, _ = run_guided(guided_check, tmp_path, M, V, N, feats, 5, SIGMAS)
    for i in range(4):
        sig = list(SIGMAS)
        sig[i] *= 0.5
        other, _ = run_guided(guided_check, tmp_path, M, V, N, feats, 5, tuple(sig))
        assert np.abs(other - base).max() > 1e-4, f"sigma {i} has no effect"
        if i:
            sig[i] = 0.0
            off, _ = run_guided(guided_check, tmp_path, M, V, N, feats, 5, tuple(sig))
            assert np.abs(off - base).max() > 1e-4, f"sigma {i} = 0 has no effect"


# ------------------------------------------------------------------ the features' reference
@pytest.mark.parametrize("name", list(F.SCENES))
def test_features_ref_is_self_consistent(name):
    """Before the device is compared with it: the reference's tree walk and its brute-force loop over
    every shape give the same features on the scenes of the GPU comparison, bit for bit."""
    s, c, _ = F.scene_of(name)
    for w, h in F.SIZES:
        tree = F.expected(name, w, h)
        brute = F.features(s, c, w, h, brute=True, oscene=F.oracle_of(name))
        for a, b in zip(tree, brute):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        a, n, z, k, m = tree
        hit = k >= 0
        assert (z[~hit] == 1e9).all() and not n[~hit].any() and (m[~hit] == -1).all() and (m[hit] >= 0).all()
        assert (z[hit] > 0).all() and (z[hit] < 1e9).all()
        np.testing.assert_allclose(np.linalg.norm(n[hit].astype(np.float64), axis=1), 1.0, atol=1e-5)


def test_the_feature_scenes_reach_every_path():
    """The cases do cover hits and misses, every shape kind, and an environment texture."""
    kinds = set()
    for name in F.SCENES:
        kinds |= set(F.expected(name, 67, 45)[3].ravel().tolist())
    assert kinds >= {-1, _abi.SHAPE_SPHERE, _abi.SHAPE_CUBE, _abi.SHAPE_PLANE, _abi.SHAPE_TRIANGLE, _abi.SHAPE_SDF,
                     _abi.SHAPE_VOLUME, _abi.SHAPE_TRANSFORMED}, kinds
    a, _, _, k, _ = F.expected("mixed", 67, 45)
    miss = k < 0
    assert miss.sum() > 50 and np.ptp(a[miss], axis=0).max() > 0.01   # the environment texture varies over the misses


# ------------------------------------------------------------------ the chosen defaults: quality table
QUALITY_SCENES = ["simplesphere", "example1", "example3", "textured"]
# the scenes where the defaults reach guided <= 0.97 x unguided on the CPU (DESIGN.md §4b's table: 0.920, 0.926, 0.960, 0.862)
GATED = ["simplesphere", "example1", "example3", "textured"]


def quality_inputs(name):
    """tests/golden/features_<name>.npz (tools/make_features_golden.py): the oracle's 96x64 renders (four
    passes of 1 spp, seed 0; one 256-spp pass, seed 7) and features_ref's features of the scene."""
    z = np.load(os.path.join(ROOT, "tests", "golden", f"features_{name}.npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", QUALITY_SCENES)
def test_guided_quality_table(name):
    q = quality_inputs(name)
    M, V, N, truth = q["noisy_M"], q["noisy_V"], q["noisy_N"], q["truth"]
    assert M.shape == (64, 96, 3) and (N == 4).all()
    plain, _ = D.denoise(M, V, N)
    guided, _ = G.denoise_guided(M, V, N, q["albedo"], q["normal"], q["depth"], q["kind"], **G.DEFAULTS)
    noisy_rmse = D.tonemapped_rmse(M, truth)
    plain_rmse, guided_rmse = D.tonemapped_rmse(plain, truth), D.tonemapped_rmse(guided, truth)
    print(f"{name}: noisy RMSE {noisy_rmse:.5f}, unguided {plain_rmse:.5f} (ratio {D.rmse_ratio(plain, M, truth):.3f}), "
          f"guided {guided_rmse:.5f} (ratio {D.rmse_ratio(guided, M, truth):.3f}), guided / unguided "
          f"{guided_rmse / plain_rmse:.3f}" + (" [gated]" if name in GATED else ""))
    if name in GATED:
        assert guided_rmse <= 0.97 * plain_rmse


# ------------------------------------------------------------------ IterativeRender
def test_iterative_render_guided_renders_features_once_and_filters_with_them(tmp_path):
    from test_denoise_host import _StubLibrary, _stub_renderer
    lib = _StubLibrary()
    r = _stub_renderer(lib)
    assert r.DenoiseGuided is False
    g = r.DenoiseGuidedParams
    assert (g.iterations, g.reserved, g.sigma_colour, g.sigma_normal, g.sigma_albedo, g.sigma_depth) == (5, 0, 4.0, 0.3, 0.3, 0.1)
    r.Denoise = r.DenoiseGuided = True
    try:
        r.IterativeRender(str(tmp_path / "out{0}.png"), 3)
        assert lib.calls.count("pt_render_features") == 1 and lib.calls.index("pt_render_features") < lib.calls.index("pt_render_pass")
        assert lib.calls.count("pt_denoise_guided") == 3 and lib.calls.count("pt_read_denoised") == 3
        assert "pt_denoise" not in lib.calls
        r.IterativeRender(None, 2)
        assert lib.calls.count("pt_render_features") == 2 and lib.calls.count("pt_denoise_guided") == 4
        # DenoiseGuided without Denoise does nothing
        lib.calls.clear()
        r.Denoise = False
        r.IterativeRender(None, 1)
        assert not [c for c in lib.calls if "denois" in c or "features" in c]
    finally:
        r._ctx = None
    assert sorted(os.listdir(tmp_path)) == ["albedo_channel.png", "denoised_output.png", "normal_channel.png", "out1.png",
                                            "out2.png", "out3.png"]
