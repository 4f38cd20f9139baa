"""The arithmetic of pt_update_shapes on the host (no GPU): tests/native/shapes_check.cpp drives
ptsharp_amd/csrc/pt_shape_refit.h xforms, records, heavy, levels, as the kernels do, against the scene compile: the
identity (a refit with the upload's parameters reproduces every word), the moved poses against a fresh compile, the
sequences, the level table and non-finite parameters.  The same stand-alone program runs once more under
AddressSanitizer and UndefinedBehaviorSanitizer.  tests/shape_refit_ref.py, the numpy restatement the GPU tests compare
the device against, is checked here against the program's `--dump` of two moved scenes."""
import os
import subprocess

import numpy as np
import pytest

import shape_refit_ref

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
EXE = os.path.join(NATIVE, "_build", "shapes_check")
EXE_ASAN = os.path.join(NATIVE, "_build", "shapes_check_asan")

POSES = {"beads": ("translate", "swap", "point", "huge", "tiny", "lit"),
         "few": ("translate", "lit", "huge", "tiny"),
         "routed": ("translate", "spin", "lit", "huge", "tiny"),
         "instances": ("translate", "swap", "point", "spin", "shared", "huge", "tiny"),
         "one": ("translate", "lit", "huge", "tiny")}


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "shapes.mk", "shapes_check"], check=True)
    return EXE


def test_shapes_check(built):
    r = subprocess.run([built], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "shapes_check: 0 failures"
    for name in ("beads", "few", "routed", "instances", "one", "none"):
        assert any(ln.startswith(f"identity {name} ") and ln.endswith(": ok") for ln in lines), r.stdout
    for scene, poses in POSES.items():
        for pose in poses:
            assert f"pose {scene} {pose} ok" in lines, r.stdout
    assert "partial ok" in lines and "nonfinite ok" in lines
    # the scenes reach the paths they are there for: at least 3 BVH4 levels, heavy records, the lone-leaf root
    ident = {ln.split()[1]: ln.split() for ln in lines if ln.startswith("identity ")}
    assert int(ident["beads"][5]) == 302 and int(ident["beads"][9]) >= 3
    assert int(ident["routed"][7]) >= 3 and int(ident["routed"][5]) <= 8
    assert int(ident["one"][3]) == 1 and int(ident["none"][3]) == 0


def test_shapes_check_sanitized():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "shapes.mk", "asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE_ASAN], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("shapes_check: 0 failures")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


@pytest.mark.parametrize("scene", ["routed", "instances"])
def test_shape_refit_ref_matches_native(built, tmp_path, scene):
    for s in ("routed", "instances"):
        os.makedirs(tmp_path / s)
    r = subprocess.run([built, "--dump", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    d = tmp_path / scene

    def load(name, dtype, cols=None):
        a = np.fromfile(os.path.join(d, name), dtype)
        return a if cols is None else a.reshape(-1, cols)

    nodes0, recs0, heavy0 = load("nodes0.u32", np.uint32, 32), load("recs0.u32", np.uint32, 12), load("heavy0.u32", np.uint32, 8)
    lights0 = load("lights0.f64", np.float64, 4)
    assert len(recs0) >= 6 and len(lights0) == 1
    nodes, recs, heavy, lights = shape_refit_ref.refit(
        nodes0, recs0, heavy0, lights0, load("rec_box0.f32", np.float32, 6), load("xf_kind.i32", np.int32),
        load("xf_index.i32", np.int32), load("xf_inner_box.f32", np.float32, 6), load("light_kind.i32", np.int32),
        load("light_index.i32", np.int32), load("sphere_center.f32", np.float32, 3), load("sphere_radius.f64", np.float64),
        load("cube_min.f32", np.float32, 3), load("cube_max.f32", np.float32, 3), load("xf_matrix.f64", np.float64, 16),
        load("xf_inverse.f64", np.float64, 16))
    assert np.array_equal(nodes, load("nodes1.u32", np.uint32, 32))
    assert np.array_equal(recs, load("recs1.u32", np.uint32, 12))
    assert np.array_equal(heavy, load("heavy1.u32", np.uint32, 8))
    assert np.array_equal(lights.view(np.uint64), load("lights1.f64", np.float64, 4).view(np.uint64))
    assert not np.array_equal(nodes, nodes0) and not np.array_equal(recs, recs0) and not np.array_equal(lights, lights0)
    assert np.array_equal(nodes[:, 24:], nodes0[:, 24:])   # the topology stays
