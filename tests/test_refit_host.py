"""The arithmetic of pt_update_triangles on the host (no GPU): tests/native/refit_check.cpp drives
ptsharp_amd/csrc/pt_refit.h leaves-then-levels, as the kernels do, against the scene compile: the identity
(a refit with the upload's vertices reproduces every byte), the deformed poses, a sequence of poses and the level
table.  The same stand-alone program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer.
tests/refit_ref.py, the numpy restatement the GPU tests compare the device against, is checked here against
the program's `--dump` of the sine pose."""
import os
import subprocess

import numpy as np
import pytest

import refit_ref

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
EXE = os.path.join(NATIVE, "_build", "refit_check")
EXE_ASAN = os.path.join(NATIVE, "_build", "refit_check_asan")


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "refit.mk", "refit_check"], check=True)
    return EXE


def test_refit_check(built):
    r = subprocess.run([built], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.strip().endswith("refit_check: 0 failures")
    for name in ("grid", "one", "two", "nine"):
        assert any(line.startswith(f"identity {name} ") and line.endswith(": ok") for line in out.splitlines()), out
    for pose in ("translate", "scale", "sine", "flat", "point", "huge", "tiny"):
        assert any(line.split() == ["pose", pose, "ok"] for line in out.splitlines()), out


def test_refit_check_sanitized():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "refit.mk", "asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE_ASAN], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("refit_check: 0 failures")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_refit_ref_matches_native(built, tmp_path):
    r = subprocess.run([built, "--dump", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr

    def load(name, dtype, cols):
        return np.fromfile(os.path.join(tmp_path, name), dtype).reshape(-1, cols)

    nodes0, chunks0, recs0 = (load(f"{n}0.u32", np.uint32, 32) for n in ("nodes", "chunks", "recs"))
    src = np.fromfile(os.path.join(tmp_path, "src_of_pos.i32"), np.int32)
    arrays = [load(f"{n}.f32", np.float32, 3) for n in ("v1", "v2", "v3", "n1", "n2", "n3")]
    assert len(nodes0) > 100 and len(src) == 3203
    nodes, chunks, recs, box = refit_ref.refit(nodes0, chunks0, recs0, src, *arrays)
    assert np.array_equal(nodes, load("nodes1.u32", np.uint32, 32))
    assert np.array_equal(chunks, load("chunks1.u32", np.uint32, 32))
    assert np.array_equal(recs, load("recs1.u32", np.uint32, 32))
    assert np.array_equal(box.view(np.uint32), np.fromfile(os.path.join(tmp_path, "box1.f32"), np.uint32))
    assert not np.array_equal(nodes, nodes0) and not np.array_equal(recs[:, 12:21], recs0[:, 12:21])
    # without normals the rows 3-5 stay
    _, _, kept, _ = refit_ref.refit(nodes0, chunks0, recs0, src, *arrays[:3])
    assert np.array_equal(kept[:, 12:24], recs0[:, 12:24]) and np.array_equal(kept[:, :12], recs[:, :12])
