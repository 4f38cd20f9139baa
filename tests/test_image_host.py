"""Buffer.Image on the host side of pt_read_image (no GPU): the per-pixel text the kernel runs
(ptsharp_amd/csrc/pt_image.h, built here with g++ into tests/native/image_check.cpp), the Python
Buffer.Image's Albedo and Normal channels, and the ABI declarations, each against Buffer.cs restated
in image_ref.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import image_ref as R
from ptsharp_amd import _abi
from ptsharp_amd.renderer import Buffer, Channel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {R.COLOR: "Color", R.VARIANCE: "Variance", R.STDDEV: "StdDev", R.SAMPLES: "Samples", R.ALBEDO: "Albedo",
         R.NORMAL: "Normal"}


def assert_no_boundary_values(cols):
    """The inputs hold no value whose byte a 1-ulp difference in pow, sqrt or a division could flip."""
    for ch in (R.COLOR, R.STDDEV, R.NORMAL):
        assert not R.near_boundary(cols[ch]).any(), NAMES[ch]


@pytest.fixture(scope="module")
def image_check(tmp_path_factory):
    """tests/native/image_check.cpp (pt_image.h under plain g++), built once."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/native/image_check.cpp"
    exe = tmp_path_factory.mktemp("image_check") / "image_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "image_check.cpp")], check=True)
    return str(exe)


def run_image_check(exe, tmp_path, M, V, N):
    H, W = N.shape
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([W, H], np.int32).tobytes() + np.ascontiguousarray(M).tobytes() +
                np.ascontiguousarray(V).tobytes() + np.ascontiguousarray(N).tobytes())
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    return np.fromfile(tmp_path / "out.bin", np.uint8).reshape(6, H, W, 3)


def test_resolve_arithmetic_matches_buffer_cs(image_check, tmp_path):
    M, V, N, cols, imgs = R.seeded_with_specials()
    assert_no_boundary_values(cols)
    got = run_image_check(image_check, tmp_path, M, V, N)
    for ch in R.CHANNELS:
        bad = (got[ch] != imgs[ch]).any(axis=2)
        assert not bad.any(), f"{NAMES[ch]}: {int(bad.sum())} pixels differ, first at (y, x) = {np.argwhere(bad)[0]}"


@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (2, 3), (7, 1), (1, 5)])
def test_resolve_small_shapes_host(image_check, tmp_path, w, h):
    """The stencil at the image's edges, down to the 1x1 image no context can hold (pt_create refuses it)."""
    M, V, N = R.seeded(w, h, seed=1000 * w + h)
    cols = {ch: R.colour(M, V, N, ch) for ch in R.CHANNELS}
    assert_no_boundary_values(cols)
    got = run_image_check(image_check, tmp_path, M, V, N)
    for ch in R.CHANNELS:
        assert np.array_equal(got[ch], R.to_bytes(cols[ch])), NAMES[ch]


def test_buffer_image_albedo_normal_host():
    M, V, N, cols, imgs = R.seeded_with_specials()
    assert_no_boundary_values(cols)
    b = Buffer(N.shape[1], N.shape[0])
    b.M, b.V, b.N = M, V, N
    for ch in (Channel.AlbedoChannel, Channel.NormalChannel):
        got = b.Image(ch)
        assert got.dtype == np.uint8 and got.shape == imgs[int(ch)].shape
        assert np.array_equal(got, imgs[int(ch)]), ch.name
    # the channels Buffer.Image already had resolve the same inputs to the same bytes
    for ch in (Channel.ColorChannel, Channel.VarianceChannel, Channel.StandardDeviationChannel, Channel.SamplesChannel):
        with np.errstate(invalid="ignore"):   # the root of a negative variance: NaN, byte 0
            assert np.array_equal(b.Image(ch), imgs[int(ch)]), ch.name


def test_abi_read_image():
    assert _abi.SIGNATURES["pt_read_image"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)])
    src = open(os.path.join(ROOT, "include", "ptsharp_hip.h")).read()
    assert re.search(r"int pt_read_image\(void\* ctx, int32_t channel, int32_t format, uint8_t\* out\);", src)
    enum = dict((k, int(v)) for k, v in re.findall(r"PT_CHANNEL_(\w+) = (\d+)", src))
    assert enum == {"COLOR": Channel.ColorChannel, "VARIANCE": Channel.VarianceChannel,
                    "STDDEV": Channel.StandardDeviationChannel, "SAMPLES": Channel.SamplesChannel,
                    "ALBEDO": Channel.AlbedoChannel, "NORMAL": Channel.NormalChannel}
    fmt = dict((k, int(v)) for k, v in re.findall(r"PT_IMAGE_(RGBA?8) = (\d+)", src))
    assert fmt == {"RGB8": _abi.IMAGE_RGB8, "RGBA8": _abi.IMAGE_RGBA8}
    lib = _abi.load_library()
    assert lib.pt_get_version() == 10 == _abi.ABI_VERSION
    # argument checks come before any device call
    out = (C.c_uint8 * 16)()
    assert lib.pt_read_image(None, 0, 0, out) == _abi.PT_ERR_INVALID_ARG
    assert lib.pt_last_error()
