"""The arithmetic of pt_pose_meshes on the host (no GPU): tests/native/pose_check.cpp drives
ptsharp_amd/csrc/pt_pose.h's pose_triangle, the function the device kernel calls, against a plain restatement of
Matrix.MulPosition / MulDirection written in the check: a seeded set, -0 and denormals, a 1e30 translation, a singular
matrix (its zero directions give NaN normals) and the identity (masked: verbatim; unmasked: -0 becomes +0).  The same
stand-alone program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer.  Its dumped outputs are
compared here with geometry.Matrix.MulPosition_arrays / MulDirection_arrays, what Mesh.Transform computes and what
the GPU tests pose their reference with, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from ptsharp_amd.geometry import Matrix

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
EXE = os.path.join(NATIVE, "_build", "pose_check")
EXE_ASAN = os.path.join(NATIVE, "_build", "pose_check_asan")
CASES = ("seeded0", "seeded1", "seeded2", "seeded3", "zeros-denormals", "far", "singular", "identity")
COUNTS = {"seeded0": 1, "seeded1": 257, "seeded2": 1000, "seeded3": 3208, "zeros-denormals": 36, "far": 300, "singular": 200,
          "identity": 200}


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "pose.mk", "pose_check"], check=True)
    return EXE


@pytest.fixture(scope="module")
def dumped(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_dump")
    r = subprocess.run([built, "--dump", str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return str(d)


def test_pose_check(built):
    r = subprocess.run([built], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "pose_check: 0 failures"
    for case in CASES:
        assert f"case {case} ok" in lines, r.stdout


def test_pose_check_sanitized():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "pose.mk", "asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE_ASAN], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("pose_check: 0 failures")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, what
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), f"{what}: {int(bad.sum())} floats differ, first at {np.argwhere(bad)[0]}"


@pytest.mark.parametrize("case", CASES)
def test_matrix_arrays_match_native(dumped, case):
    m = Matrix(np.fromfile(os.path.join(dumped, f"{case}_matrix.f64"), np.float64).reshape(4, 4))
    tri_in = np.fromfile(os.path.join(dumped, f"{case}_in.f32"), np.float32).reshape(-1, 6, 3)
    tri_out = np.fromfile(os.path.join(dumped, f"{case}_out.f32"), np.float32).reshape(-1, 6, 3)
    assert len(tri_in) == len(tri_out) == COUNTS[case]
    with np.errstate(all="ignore"):
        for k in range(3):
            same_bits(tri_out[:, k], m.MulPosition_arrays(np.ascontiguousarray(tri_in[:, k])), f"{case} v{k + 1}")
        for k in range(3, 6):
            same_bits(tri_out[:, k], m.MulDirection_arrays(np.ascontiguousarray(tri_in[:, k])), f"{case} n{k - 2}")
    nans = int(np.isnan(tri_out[:, 3:]).sum())
    if case == "singular":
        assert nans == 360
    elif case != "zeros-denormals":
        assert nans == 0
    if case == "identity":
        was_neg0 = tri_in[:, :3].view(np.uint32) == 0x80000000
        assert was_neg0.sum() > 0 and (tri_out[:, :3].view(np.uint32)[was_neg0] == 0).all()
