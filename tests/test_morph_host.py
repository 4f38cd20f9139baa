"""The arithmetic and the packed layout of pt_set_morph / pt_morph_meshes on the host (no GPU):
tests/native/morph_check.cpp drives ptsharp_amd/csrc/pt_morph.h (the arithmetic the device kernel calls, the packer, the
unpacker and the argument check pt_set_morph runs) against a plain restatement written in the check: seeded sets of 1,
63, 64, 65, 257 and 3,208 triangles, a corner with 40 deltas beside 63 with none, an empty target, a target touching
every corner, target 65534, all-zero weights (verbatim, -0 kept), a weight of -0, a NaN weight (live), non-finite
deltas on dead targets (no effect), denormal deltas and a 1e30 delta, loose triangles with deltas, with and without
normal deltas, a zero-length resulting normal (NaN); pack -> unpack identity, the padded count, 128-byte aligned
planes, and every malformed input refused.  The same stand-alone program runs once more under AddressSanitizer and
UndefinedBehaviorSanitizer.  Its dumped cases are compared here with tests/morph_ref.py, the numpy restatement the GPU
tests morph their reference with, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import morph_ref
from normals_ref import same_bits

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
EXE = os.path.join(NATIVE, "_build", "morph_check")
EXE_ASAN = os.path.join(NATIVE, "_build", "morph_check_asan")
# case -> (triangles, targets)
COUNTS = {"seeded0": (1, 3), "seeded1": (63, 5), "seeded2": (64, 8), "seeded3": (65, 8), "seeded4": (257, 40),
          "seeded5": (3208, 300), "no-dnrm": (200, 12), "lengths": (128, 40), "targets": (70, 65535), "zero-weights": (200, 9),
          "neg-zero-weight": (100, 3), "nan-weight": (100, 2), "dead-nonfinite": (150, 6), "denormal-far": (60, 3),
          "zero-normal": (10, 1)}
CASES = tuple(COUNTS)


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "morph.mk", "morph_check"], check=True)
    return EXE


@pytest.fixture(scope="module")
def dumped(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("morph_dump")
    r = subprocess.run([built, "--dump", str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return str(d)


def load(dumped, case):
    path = lambda part: os.path.join(dumped, f"{case}_{part}")
    f = lambda part, dtype: np.fromfile(path(part), dtype)
    n, t = COUNTS[case]
    k = dict(group=f("group.i32", np.int32), first=f("first.i64", np.int64), corner=f("corner.i32", np.int32),
             dpos=f("dpos.f32", np.float32).reshape(-1, 3), weights=f("weights.f32", np.float32),
             dnrm=f("dnrm.f32", np.float32).reshape(-1, 3) if os.path.exists(path("dnrm.f32")) else None,
             tri_in=f("in.f32", np.float32).reshape(-1, 6, 3), out=f("out.f32", np.float32).reshape(-1, 6, 3),
             outp=f("outp.f32", np.float32).reshape(-1, 6, 3))
    assert len(k["group"]) == len(k["tri_in"]) == len(k["out"]) == len(k["outp"]) == n
    assert len(k["first"]) == t + 1 == len(k["weights"]) + 1 and k["first"][-1] == len(k["corner"]) == len(k["dpos"])
    a = k["first"]
    k["targets"] = [(k["corner"][a[i]:a[i + 1]], k["dpos"][a[i]:a[i + 1]]) + (() if k["dnrm"] is None else (k["dnrm"][a[i]:a[i + 1]],))
                    for i in range(t)]
    return k


def test_morph_check(built):
    r = subprocess.run([built], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "morph_check: 0 failures"
    for case in CASES + ("refusals",):
        assert f"case {case} ok" in lines, r.stdout


def test_morph_check_sanitized():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "morph.mk", "asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE_ASAN], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("morph_check: 0 failures")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


@pytest.mark.parametrize("case", CASES)
def test_morph_ref_matches_native(dumped, case):
    k = load(dumped, case)
    rest = [np.ascontiguousarray(k["tri_in"][:, j]) for j in range(6)]
    for normals, got in ((True, k["out"]), (False, k["outp"])):
        want = morph_ref.morph(rest, k["group"], k["targets"], k["weights"], normals=normals)
        for j in range(6):
            same_bits(got[:, j], want[j], f"{case} normals={normals} array {j}")
    p = morph_ref.packed(k["targets"])
    assert np.array_equal(p["target_first"], k["first"]) and np.array_equal(p["corner"], k["corner"])
    assert np.array_equal(p["dpos"].view(np.uint32), k["dpos"].view(np.uint32)) and (p["dnrm"] is None) == (k["dnrm"] is None)
    # what each case is there for, seen from here
    moved = k["out"].view(np.uint32) != k["tri_in"].view(np.uint32)
    loose = k["group"] < 0
    assert not moved[loose].any()
    assert not (k["outp"][:, 3:].view(np.uint32) != k["tri_in"][:, 3:].view(np.uint32)).any()
    named = np.zeros(3 * len(loose), bool)
    named[k["corner"]] = True
    if case.startswith("seeded") and case != "seeded0":
        assert loose.any() and named.reshape(-1, 3)[loose].any(), "no loose triangle is named by a delta"
        assert moved[~loose, :3].mean() > 0.5 and moved[~loose, 3:].mean() > 0.5
        assert any(len(t[0]) == 0 for t in k["targets"])
    if case == "no-dnrm":
        assert k["dnrm"] is None and moved[:, :3].any() and not moved[:, 3:].any()
    if case == "lengths":
        per_corner = np.bincount(k["corner"], minlength=3 * 128)
        assert per_corner[27] == 40 and (per_corner[np.arange(0, 192, 3)] > 0).sum() == 1 and per_corner[61] == 5 and per_corner[64] == 1
    if case == "targets":
        a = k["first"]
        assert a[1] - a[0] == 210 and a[2] == a[1] and a[65535] - a[65534] == 3
    if case == "zero-weights":
        assert not moved.any() and (k["out"].view(np.uint32) == 0x80000000).any() and not k["weights"].any()
        assert (np.signbit(k["weights"])).any() and (~np.signbit(k["weights"])).any()
    if case == "neg-zero-weight":
        assert k["weights"][1] == 0 and np.signbit(k["weights"][1]) and np.abs(k["dpos"]).max() > 1e19 and np.abs(k["out"][:, :3]).max() < 100
    if case == "nan-weight":
        assert np.isnan(k["out"]).sum() == 150 and np.isnan(k["weights"]).sum() == 1
    if case == "dead-nonfinite":
        assert np.isfinite(k["out"]).all() and not np.isfinite(k["dpos"]).all() and moved.any()
    if case == "denormal-far":
        tiny = np.abs(k["out"][:, :3])
        assert ((tiny > 0) & (tiny < 1.17e-38)).any() and (tiny > 1e29).any()
    if case == "zero-normal":
        assert np.isnan(k["out"][:, 3:]).all() and np.isfinite(k["out"][:, :3]).all()
