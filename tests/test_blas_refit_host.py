"""The arithmetic of pt_update_meshes for instanced meshes on the host (no GPU): tests/native/blas_check.cpp drives
ptsharp_amd/csrc/pt_blas_refit.h tris, bounds, levels and then the shape refit, as the kernels do, against the scene
compile: the identity (a refit with the upload's vertices reproduces every word), the moved poses against a fresh
compile, the sequences, the level table and non-finite vertices.  The same stand-alone program runs once more under
AddressSanitizer and UndefinedBehaviorSanitizer.  tests/blas_refit_ref.py, the numpy restatement the GPU tests compare
the device against, is checked here against the program's `--dump` of a moved scene."""
import os
import subprocess

import numpy as np
import pytest

import blas_refit_ref

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
EXE = os.path.join(NATIVE, "_build", "blas_check")
EXE_ASAN = os.path.join(NATIVE, "_build", "blas_check_asan")
SCENES = ("routed", "instances", "two", "only")
POSES = ("translate", "sine", "flat", "point", "huge", "tiny")


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "blas.mk", "blas_check"], check=True)
    return EXE


def test_blas_check(built):
    r = subprocess.run([built], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "blas_check: 0 failures"
    for name in SCENES:
        assert any(ln.startswith(f"identity {name} ") and ln.endswith(": ok") for ln in lines), r.stdout
        for pose in POSES:
            assert f"pose {name} {pose} ok" in lines, r.stdout
    assert "nonfinite ok" in lines
    # the scenes reach the paths they are there for: `identity NAME blases B nodes N tris T levels L chunks C ...`
    ident = {ln.split()[1]: ln.split() for ln in lines if ln.startswith("identity ")}
    num = lambda name, key: int(ident[name][ident[name].index(key) + 1])
    assert num("routed", "blases") == 1 and num("routed", "tris") == 8
    assert num("instances", "blases") == 0
    assert num("two", "blases") == 2 and num("two", "tris") == 289 and num("two", "levels") >= 3 and num("two", "chunks") > 0
    assert num("only", "blases") == 1 and num("only", "chunks") == 0


def test_blas_check_sanitized():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "blas.mk", "asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE_ASAN], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("blas_check: 0 failures")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_blas_refit_ref_matches_native(built, tmp_path):
    r = subprocess.run([built, "--dump", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr

    def load(name, dtype, cols=None):
        a = np.fromfile(os.path.join(tmp_path, name), dtype)
        return a if cols is None else a.reshape(-1, cols)

    desc = load("desc.i32", np.int32, 4)
    nodes0, recs0, shade0 = load("nodes0.u32", np.uint32, 32), load("recs0.u32", np.uint32, 12), load("shade0.u32", np.uint32, 12)
    assert len(desc) == 2 and desc[1, 0] > 0 and desc[1, 2] > 0   # the second BLAS's offsets are not zero
    assert blas_refit_ref.tri_counts(desc, len(recs0)) == list(desc[:, 3])
    v = [load(f"v{k}.f32", np.float32, 3) for k in (1, 2, 3)]
    n = [load(f"n{k}.f32", np.float32, 3) for k in (1, 2, 3)]
    nodes, recs, shade, boxes = blas_refit_ref.refit(desc, nodes0, recs0, shade0, load("src_of_pos.i32", np.int32), *v, normals=n)
    assert np.array_equal(nodes, load("nodes1.u32", np.uint32, 32))
    assert np.array_equal(recs, load("recs1.u32", np.uint32, 12))
    assert np.array_equal(shade, load("shade1.u32", np.uint32, 12))
    assert np.array_equal(boxes, load("boxes1.f32", np.float32, 6))
    inner = blas_refit_ref.inner_boxes(load("xf_inner_box0.f32", np.float32, 6), load("xf_blas.i32", np.int32), boxes)
    assert np.array_equal(inner, load("xf_inner_box1.f32", np.float32, 6))
    assert not np.array_equal(nodes, nodes0) and not np.array_equal(recs, recs0) and not np.array_equal(shade, shade0)
    assert np.array_equal(nodes[:, 24:], nodes0[:, 24:]) and np.array_equal(shade[:, 9], shade0[:, 9])
