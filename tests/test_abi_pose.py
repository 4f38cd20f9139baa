"""pt_set_rest_pose, pt_pose_meshes and pt_read_pose: exported with C linkage, declared in the Python and C# bindings
field for field, and their NULL and argument errors returned without a device (no context can exist without one, so
the checks that need a scene are in tests/test_gpu_pose.py)."""
import ctypes as C
import re
import subprocess

import numpy as np

import test_abi as A
from ptsharp_amd import _abi

NAMES = ("pt_set_rest_pose", "pt_pose_meshes", "pt_read_pose")


def test_symbols_exported():
    lib = _abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True).stdout
    cs = open(A.os.path.join(A.ROOT, "csharp", "HipRenderer.cs")).read()
    for name in NAMES:
        assert name in A.declared_functions() and name in _abi.SIGNATURES and hasattr(lib, name)
        assert re.search(rf"\bT {name}\b", out), f"{name} not exported with C linkage"
        assert re.search(rf"static extern int {name}\(", cs), f"{name} has no DllImport"
    assert "public double PoseMeshes(" in cs
    assert lib.pt_get_version() == 10 and _abi.ABI_VERSION == 10


def test_struct_matches_header_in_both_bindings():
    A.test_python_binding_matches_header("pt_mesh_pose")
    A.test_csharp_binding_matches_header("pt_mesh_pose")
    assert C.sizeof(_abi.pt_mesh_pose) == 4 * 4 + 2 * 8
    assert _abi.pt_mesh_pose.matrices.offset == 16
    assert _abi.pt_mesh_pose.mesh_mask.offset == 24


def test_renderer_has_the_methods():
    from ptsharp_amd import Renderer
    for name in ("SetRestPose", "PoseMeshes", "ReadPose"):
        assert callable(getattr(Renderer, name))


def test_argument_errors_without_a_device():
    lib = _abi.load_library()
    v = np.zeros((2, 3), np.float32)
    p = v.ctypes.data_as(C.POINTER(C.c_float))
    m = np.tile(np.eye(4).reshape(-1), 2)
    mp = m.ctypes.data_as(C.POINTER(C.c_double))
    on = np.ones(2, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    U = _abi.pt_mesh_pose
    two = (C.c_int32 * 2)
    fake = C.c_void_p(1)   # never dereferenced: every case fails on an argument checked before the context is read
    ms = C.c_double(-1.0)
    assert lib.pt_pose_meshes(None, C.byref(U(2, 0, two(0, 0), mp, on)), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
    assert b"ctx" in lib.pt_last_error()
    cases = {
        "NULL u": None,
        "reserved[0]": U(2, 0, two(1, 0), mp),
        "reserved[1]": U(2, 0, two(0, 1), mp, on),
        "mode 3": U(2, 3, two(0, 0), mp),
        "mode -1": U(2, -1, two(0, 0), mp),
        "NULL matrices": U(2, 0, two(0, 0), None, on),
        "NULL matrices, FACE": U(2, _abi.NORMALS_FACE, two(0, 0), None),
        "NULL matrices, SMOOTH": U(2, _abi.NORMALS_SMOOTH, two(0, 0), None),
    }
    for what, u in cases.items():
        rc = lib.pt_pose_meshes(fake, None if u is None else C.byref(u), C.byref(ms))
        assert rc == _abi.PT_ERR_INVALID_ARG, what
        assert lib.pt_last_error(), what
    assert ms.value == -1.0   # nothing ran
    # pt_set_rest_pose: all six arrays are required
    assert lib.pt_set_rest_pose(None, 2, p, p, p, p, p, p) == _abi.PT_ERR_INVALID_ARG
    assert b"ctx" in lib.pt_last_error()
    for k in range(6):
        args = [p] * 6
        args[k] = None
        assert lib.pt_set_rest_pose(fake, 2, *args) == _abi.PT_ERR_INVALID_ARG, k
        assert b"required" in lib.pt_last_error()
    assert lib.pt_read_pose(None, p, p, p, p, p, p) == _abi.PT_ERR_INVALID_ARG
    assert lib.pt_read_pose(None, None, None, None, None, None, None) == _abi.PT_ERR_INVALID_ARG
