"""The host side of pt_update_volumes (no GPU): tests/native/volumes_check.cpp drives
ptsharp_amd/csrc/pt_volume_update.h, the per-cell functions that the upload's table loops and the device kernels both
run, cell by cell through the kernel's index functions, against a plain restatement of the loops the upload had
before, for every byte of the uniform-cell table and every double of the cell-major corners: seeded grids 1x1x1,
2x3x5, 17x9x5 and 24x24x12 under no windows, Example.volume's five, overlapping and unsorted windows, 130 windows (a
Sign past int8), voxels exactly on a lo and a hi, and NaN and infinite voxels and bounds.  Then zero_sign, every
refusal of the argument check, the light test (top-level and through a transform; an emissive window dragged onto the
value at the test point is refused) and the 64-bit index arithmetic at dimensions whose table passes 2^32 bytes.  The
same stand-alone program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
EXE = os.path.join(NATIVE, "_build", "volumes_check")
EXE_ASAN = os.path.join(NATIVE, "_build", "volumes_check_asan")
GRIDS = ("1x1x1", "2x3x5", "17x9x5", "24x24x12")
SETS = ("none", "example", "overlapping-unsorted", "130-windows", "on-the-bounds", "non-finite-bounds",
        "non-finite-voxels example", "non-finite-voxels non-finite-bounds", "non-finite-voxels none")
OTHER = ("sign-past-int8", "index-64-bit", "arguments", "lights")


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "volumes.mk", "volumes_check"], check=True)
    return EXE


def test_volumes_check(built):
    r = subprocess.run([built], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "volumes_check: 0 failures"
    for g in GRIDS:
        for s in SETS:
            assert f"case {g} {s} ok" in lines, r.stdout
    for case in OTHER:
        assert f"case {case} ok" in lines, r.stdout


def test_volumes_check_sanitized():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "volumes.mk", "asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE_ASAN], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("volumes_check: 0 failures")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
