"""The arithmetic of pt_update_triangles_normals on the host (no GPU): tests/native/normals_check.cpp drives
ptsharp_amd/csrc/pt_normals.h in the kernels' order (face normals, keys, a stable sort, the segment walk) against
pt_obj.cpp's face normal and pt_mesh_smooth_normals, bit for bit, on the scene and the poses of the GPU test.  The
same stand-alone program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer.  The scene
compile's group table and tests/normals_ref.py, the restatement the GPU tests compare the device against, are
checked here against the program's `--dump`.  The two entry points are exported and reject bad arguments without
a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import normals_ref
from ptsharp_amd import _abi

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
EXE = os.path.join(NATIVE, "_build", "normals_check")
EXE_ASAN = os.path.join(NATIVE, "_build", "normals_check_asan")
POSES = ("translate", "scale", "sine", "huge", "tiny", "zero-sign", "degenerate")


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "normals.mk", "normals_check"], check=True)
    return EXE


@pytest.fixture(scope="module")
def dumped(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("normals_dump")
    r = subprocess.run([built, "--dump", str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return str(d)


def test_normals_check(built):
    r = subprocess.run([built], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "normals_check: 0 failures"
    for pose in POSES:
        assert f"scene pose {pose} ok" in lines, r.stdout
    assert "single pose sine ok" in lines and "empty pose sine ok" in lines


def test_normals_check_sanitized():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "normals.mk", "asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE_ASAN], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("normals_check: 0 failures")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_group_table(dumped):
    """compile_scene's RefitTables::tri_group on two grid meshes with a loose triangle before, between and after
    them and the fan mesh: the mesh index per source triangle, -1 for the loose ones."""
    group = np.fromfile(os.path.join(dumped, "group.i32"), np.int32)
    first = np.fromfile(os.path.join(dumped, "mesh_first.i32"), np.int32)
    count = np.fromfile(os.path.join(dumped, "mesh_count.i32"), np.int32)
    assert list(first) == [1, 1602, 3202] and list(count) == [1600, 1600, 300]
    want = np.concatenate([[-1], np.full(1600, 0), [-1], np.full(1600, 1), np.full(300, 2), [-1]]).astype(np.int32)
    assert np.array_equal(group, want)


@pytest.mark.parametrize("pose", POSES)
def test_normals_ref_matches_native(dumped, pose):
    load = lambda name: np.fromfile(os.path.join(dumped, f"{pose}_{name}.f32"), np.float32).reshape(-1, 3)
    v = [load(k) for k in ("v1", "v2", "v3")]
    first = np.fromfile(os.path.join(dumped, "mesh_first.i32"), np.int32)
    count = np.fromfile(os.path.join(dumped, "mesh_count.i32"), np.int32)
    assert len(v[0]) == 3503
    face = normals_ref.normals(*v, first, count, "face")
    for k in range(3):
        normals_ref.same_bits(face[k], load("face"), f"{pose} face n{k + 1}")
    smooth = normals_ref.normals(*v, first, count, "smooth")
    for k in range(3):
        normals_ref.same_bits(smooth[k], load(f"n{k + 1}"), f"{pose} smooth n{k + 1}")
    nans = sum(int(np.isnan(a).any(axis=1).sum()) for a in smooth)
    if pose == "degenerate":
        assert 12 <= nans <= 0.02 * 3 * 3503
    else:
        assert nans == 0
    assert sum(int((a.view(np.uint32) != b.view(np.uint32)).any(axis=1).sum()) for a, b in zip(smooth, face)) > 3503


def test_library_exports_the_entry_points():
    lib = _abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("pt_update_triangles_normals", "pt_read_tri_normals"):
        assert hasattr(lib, name) and f" T {name}\n" in out, name
        assert name in _abi.SIGNATURES
    assert (_abi.NORMALS_FACE, _abi.NORMALS_SMOOTH) == (1, 2)
    assert lib.pt_get_version() == 10


def test_bad_arguments_rejected_without_a_context():
    lib = _abi.load_library()
    fp = C.POINTER(C.c_float)
    a = np.zeros((1, 3), np.float32)
    p, null = a.ctypes.data_as(fp), fp()
    ms = C.c_double(-1.0)
    for mode in (_abi.NORMALS_FACE, _abi.NORMALS_SMOOTH, 0, 3):
        assert lib.pt_update_triangles_normals(None, 1, p, p, p, mode, C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
        assert b"ctx is NULL" in lib.pt_last_error()
    assert ms.value == -1.0
    assert lib.pt_read_tri_normals(None, p, p, p) == _abi.PT_ERR_INVALID_ARG
    assert b"ctx is NULL" in lib.pt_last_error()
    # the argument checks come before the context is read: a block of zeros stands in for one
    fake = C.create_string_buffer(1 << 16)
    ctx = C.cast(fake, C.c_void_p)
    for ptrs in ((null, p, p), (p, null, p), (p, p, null)):
        assert lib.pt_update_triangles_normals(ctx, 1, *ptrs, _abi.NORMALS_SMOOTH, None) == _abi.PT_ERR_INVALID_ARG
        assert b"required" in lib.pt_last_error()
        assert lib.pt_read_tri_normals(ctx, *ptrs) == _abi.PT_ERR_INVALID_ARG
        assert b"required" in lib.pt_last_error()
    for mode in (0, 3, -1, 1 << 20):
        assert lib.pt_update_triangles_normals(ctx, 1, p, p, p, mode, None) == _abi.PT_ERR_INVALID_ARG, mode
        assert b"pt_normals_mode" in lib.pt_last_error()
