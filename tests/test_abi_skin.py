"""pt_set_skin, pt_skin_meshes and pt_read_skin: exported with C linkage, declared in the Python and C# bindings field
for field, and their NULL and argument errors returned without a device (no context can exist without one, so the
checks that need a scene are in tests/test_gpu_skin.py)."""
import ctypes as C
import re
import subprocess

import numpy as np

import test_abi as A
from ptsharp_amd import _abi

NAMES = ("pt_set_skin", "pt_skin_meshes", "pt_read_skin")


def test_symbols_exported():
    lib = _abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True).stdout
    cs = open(A.os.path.join(A.ROOT, "csharp", "HipRenderer.cs")).read()
    for name in NAMES:
        assert name in A.declared_functions() and name in _abi.SIGNATURES and hasattr(lib, name)
        assert re.search(rf"\bT {name}\b", out), f"{name} not exported with C linkage"
        assert re.search(rf"static extern int {name}\(", cs), f"{name} has no DllImport"
    assert "public void SetSkin(" in cs and "public double SkinMeshes(" in cs
    assert lib.pt_get_version() == 10 and _abi.ABI_VERSION == 10


def test_structs_match_header_in_both_bindings():
    for name in ("pt_skin_desc", "pt_mesh_skin"):
        A.test_python_binding_matches_header(name)
        A.test_csharp_binding_matches_header(name)
    assert C.sizeof(_abi.pt_skin_desc) == 4 * 4 + 6 * 8
    assert [getattr(_abi.pt_skin_desc, f).offset for f in ("num_triangles", "num_bones", "reserved", "bone1", "bone2", "bone3",
                                                            "weight1", "weight2", "weight3")] == [0, 4, 8, 16, 24, 32, 40, 48, 56]
    assert C.sizeof(_abi.pt_mesh_skin) == 4 * 4 + 8
    assert [getattr(_abi.pt_mesh_skin, f).offset for f in ("num_bones", "normals_mode", "reserved", "matrices")] == [0, 4, 8, 16]
    macros = A._macros(open(A.HEADER).read())
    assert macros["PT_SKIN_INFLUENCES"] == _abi.SKIN_INFLUENCES == 4
    assert macros["PT_SKIN_MAX_BONES"] == _abi.SKIN_MAX_BONES == 65536
    cs = open(A.os.path.join(A.ROOT, "csharp", "HipRenderer.cs")).read()
    assert "PT_SKIN_INFLUENCES = 4, PT_SKIN_MAX_BONES = 65536" in cs


def test_renderer_has_the_methods():
    from ptsharp_amd import Renderer
    for name in ("SetSkin", "SkinMeshes", "ReadSkin"):
        assert callable(getattr(Renderer, name))


def test_argument_errors_without_a_device():
    lib = _abi.load_library()
    b = np.zeros((2, 4), np.int32)
    w = np.ones((2, 4), np.float32)
    bp, wp = b.ctypes.data_as(C.POINTER(C.c_int32)), w.ctypes.data_as(C.POINTER(C.c_float))
    m = np.tile(np.eye(4).reshape(-1), 3)
    mp = m.ctypes.data_as(C.POINTER(C.c_double))
    D, U = _abi.pt_skin_desc, _abi.pt_mesh_skin
    two = (C.c_int32 * 2)
    fake = C.c_void_p(1)   # never dereferenced: every case fails on an argument checked before the context is read
    ms = C.c_double(-1.0)
    # pt_set_skin
    assert lib.pt_set_skin(None, C.byref(D(2, 3, two(0, 0), bp, bp, bp, wp, wp, wp))) == _abi.PT_ERR_INVALID_ARG
    assert b"ctx" in lib.pt_last_error()
    cases = {
        "NULL desc": None,
        "reserved[0]": D(2, 3, two(1, 0), bp, bp, bp, wp, wp, wp),
        "reserved[1]": D(2, 3, two(0, 1), bp, bp, bp, wp, wp, wp),
        "no bones": D(2, 0, two(0, 0), bp, bp, bp, wp, wp, wp),
        "negative bones": D(2, -1, two(0, 0), bp, bp, bp, wp, wp, wp),
        "too many bones": D(2, 65537, two(0, 0), bp, bp, bp, wp, wp, wp),
    }
    for k in range(6):
        args = [bp, bp, bp, wp, wp, wp]
        args[k] = None
        cases[f"NULL array {k}"] = D(2, 3, two(0, 0), *args)
    for what, d in cases.items():
        assert lib.pt_set_skin(fake, None if d is None else C.byref(d)) == _abi.PT_ERR_INVALID_ARG, what
        assert lib.pt_last_error(), what
    # pt_skin_meshes
    assert lib.pt_skin_meshes(None, C.byref(U(3, 0, two(0, 0), mp)), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
    assert b"ctx" in lib.pt_last_error()
    cases = {
        "NULL u": None,
        "reserved[0]": U(3, 0, two(1, 0), mp),
        "reserved[1]": U(3, 0, two(0, 1), mp),
        "mode 3": U(3, 3, two(0, 0), mp),
        "mode -1": U(3, -1, two(0, 0), mp),
        "NULL matrices": U(3, 0, two(0, 0), None),
        "NULL matrices, FACE": U(3, _abi.NORMALS_FACE, two(0, 0), None),
        "NULL matrices, SMOOTH": U(3, _abi.NORMALS_SMOOTH, two(0, 0), None),
    }
    for what, u in cases.items():
        assert lib.pt_skin_meshes(fake, None if u is None else C.byref(u), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG, what
        assert lib.pt_last_error(), what
    assert ms.value == -1.0   # nothing ran
    # pt_read_skin
    assert lib.pt_read_skin(None, bp, bp, bp, wp, wp, wp) == _abi.PT_ERR_INVALID_ARG
    assert lib.pt_read_skin(None, None, None, None, None, None, None) == _abi.PT_ERR_INVALID_ARG
