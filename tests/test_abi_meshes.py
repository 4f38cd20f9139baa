"""pt_update_meshes and pt_read_blas: exported with C linkage, declared in the Python and C# bindings field for field,
and their NULL and argument errors returned without a device (no context can exist without one, so the checks that
need a scene are in tests/test_gpu_blas_refit.py)."""
import ctypes as C
import re
import subprocess

import numpy as np

import test_abi as A
from ptsharp_amd import _abi


def test_symbols_exported():
    lib = _abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("pt_update_meshes", "pt_read_blas"):
        assert name in A.declared_functions() and name in _abi.SIGNATURES and hasattr(lib, name)
        assert re.search(rf"\bT {name}\b", out), f"{name} not exported with C linkage"
    assert lib.pt_get_version() == 10


def test_struct_matches_header_in_both_bindings():
    A.test_python_binding_matches_header("pt_mesh_update")
    A.test_csharp_binding_matches_header("pt_mesh_update")
    assert C.sizeof(_abi.pt_mesh_update) == 4 * 4 + 6 * 8
    assert _abi.pt_mesh_update.v1.offset == 16


def test_argument_errors_without_a_device():
    lib = _abi.load_library()
    v = np.zeros((2, 3), np.float32)
    p = v.ctypes.data_as(C.POINTER(C.c_float))
    U = _abi.pt_mesh_update
    two = (C.c_int32 * 2)
    fake = C.c_void_p(1)   # never dereferenced: every case fails on an argument checked before the context is read
    ms = C.c_double(-1.0)
    assert lib.pt_update_meshes(None, C.byref(U(2, 0, two(0, 0), p, p, p)), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
    assert b"ctx" in lib.pt_last_error()
    # per case the message after the entry point's prefix: with several arguments wrong, which one wins is part of the ABI
    # (reserved, the mode, normals beside a mode, the vertices, the normals all or none)
    reserved, mode = b"reserved must be 0", b" is not 0 or a pt_normals_mode"
    both, verts, normals = b"n1/n2/n3 are given and normals_mode derives them", b"v1, v2 and v3 are required", b"n1/n2/n3 must be all set or all NULL"
    cases = {
        "NULL u": (None, b"u is NULL"),
        "reserved[0]": (U(2, 0, two(1, 0), p, p, p), reserved),
        "reserved[1]": (U(2, 0, two(0, 1), p, p, p), reserved),
        "mode 3": (U(2, 3, two(0, 0), p, p, p), b"normals_mode 3" + mode),
        "mode -1": (U(2, -1, two(0, 0), p, p, p), b"normals_mode -1" + mode),
        "normals with FACE": (U(2, _abi.NORMALS_FACE, two(0, 0), p, p, p, p, p, p), both),
        "one normal with SMOOTH": (U(2, _abi.NORMALS_SMOOTH, two(0, 0), p, p, p, None, p, None), both),
        "NULL v1": (U(2, 0, two(0, 0), None, p, p), verts),
        "NULL v2": (U(2, 0, two(0, 0), p, None, p), verts),
        "NULL v3": (U(2, 0, two(0, 0), p, p, None), verts),
        "n1 only": (U(2, 0, two(0, 0), p, p, p, p, None, None), normals),
        "n3 missing": (U(2, 0, two(0, 0), p, p, p, p, p, None), normals),
        "reserved and mode 3": (U(2, 3, two(1, 0), p, p, p), reserved),
        "mode 3 and NULL v1": (U(2, 3, two(0, 0), None, p, p), b"normals_mode 3" + mode),
        "normals with FACE and NULL v1": (U(2, _abi.NORMALS_FACE, two(0, 0), None, p, p, p, p, p), both),
        "NULL v1 and n1 only": (U(2, 0, two(0, 0), None, p, p, p, None, None), verts),
    }
    for name, prefix in (("pt_update_meshes", b"update meshes: "), ("pt_rebuild_meshes", b"rebuild meshes: ")):
        for what, (u, message) in cases.items():
            if u is None and name == "pt_rebuild_meshes":
                continue   # pt_rebuild_meshes(ctx, NULL) is a call of its own: the staged pose, which reads the context
            rc = getattr(lib, name)(fake, None if u is None else C.byref(u), C.byref(ms))
            assert rc == _abi.PT_ERR_INVALID_ARG, (name, what)
            assert lib.pt_last_error() == prefix + message, (name, what, lib.pt_last_error())
    assert ms.value == -1.0   # nothing ran
    assert lib.pt_read_blas(None, None, None, None, None, None, None) == _abi.PT_ERR_INVALID_ARG
