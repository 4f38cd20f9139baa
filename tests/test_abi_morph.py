"""pt_set_morph, pt_morph_meshes and pt_read_morph: exported with C linkage, declared in the Python and C# bindings field
for field, and their NULL and argument errors returned without a device (no context can exist without one, so the
checks that need a scene are in tests/test_gpu_morph.py)."""
import ctypes as C
import re
import subprocess

import numpy as np

import test_abi as A
from ptsharp_amd import _abi

NAMES = ("pt_set_morph", "pt_morph_meshes", "pt_read_morph")


def test_symbols_exported():
    lib = _abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True).stdout
    cs = open(A.os.path.join(A.ROOT, "csharp", "HipRenderer.cs")).read()
    for name in NAMES:
        assert name in A.declared_functions() and name in _abi.SIGNATURES and hasattr(lib, name)
        assert re.search(rf"\bT {name}\b", out), f"{name} not exported with C linkage"
        assert re.search(rf"static extern int {name}\(", cs), f"{name} has no DllImport"
    assert "public void SetMorph(" in cs and "public double MorphMeshes(" in cs
    assert lib.pt_get_version() == 10 and _abi.ABI_VERSION == 10
    header = open(A.HEADER).read()
    assert re.search(r"#define PT_ABI_VERSION 10\b", header)


def test_structs_match_header_in_both_bindings():
    for name in ("pt_morph_desc", "pt_mesh_morph"):
        A.test_python_binding_matches_header(name)
        A.test_csharp_binding_matches_header(name)
    assert C.sizeof(_abi.pt_morph_desc) == 4 * 4 + 4 * 8
    assert [getattr(_abi.pt_morph_desc, f).offset for f in ("num_triangles", "num_targets", "reserved", "target_first", "corner",
                                                             "dpos", "dnrm")] == [0, 4, 8, 16, 24, 32, 40]
    assert C.sizeof(_abi.pt_mesh_morph) == 4 * 4 + 2 * 8
    assert [getattr(_abi.pt_mesh_morph, f).offset for f in ("num_targets", "normals_mode", "num_bones", "reserved", "weights",
                                                             "skin_matrices")] == [0, 4, 8, 12, 16, 24]
    macros = A._macros(open(A.HEADER).read())
    assert macros["PT_MORPH_MAX_TARGETS"] == _abi.MORPH_MAX_TARGETS == 65535
    cs = open(A.os.path.join(A.ROOT, "csharp", "HipRenderer.cs")).read()
    assert "PT_MORPH_MAX_TARGETS = 65535" in cs


def test_renderer_has_the_methods():
    from ptsharp_amd import Renderer
    for name in ("SetMorph", "MorphMeshes", "ReadMorph"):
        assert callable(getattr(Renderer, name))


def test_argument_errors_without_a_device():
    lib = _abi.load_library()
    first = np.array([0, 1, 2], np.int64)
    corner = np.array([0, 3], np.int32)
    d3 = np.ones((2, 3), np.float32)
    lp, ip, fp = first.ctypes.data_as(C.POINTER(C.c_int64)), corner.ctypes.data_as(C.POINTER(C.c_int32)), d3.ctypes.data_as(C.POINTER(C.c_float))
    w = np.ones(2, np.float32)
    wp = w.ctypes.data_as(C.POINTER(C.c_float))
    m = np.tile(np.eye(4).reshape(-1), 3)
    mp = m.ctypes.data_as(C.POINTER(C.c_double))
    D, U = _abi.pt_morph_desc, _abi.pt_mesh_morph
    two = (C.c_int32 * 2)
    fake = C.c_void_p(1)   # never dereferenced: every case fails on an argument checked before the context is read
    ms = C.c_double(-1.0)
    # pt_set_morph
    assert lib.pt_set_morph(None, C.byref(D(2, 2, two(0, 0), lp, ip, fp, fp))) == _abi.PT_ERR_INVALID_ARG
    assert b"ctx" in lib.pt_last_error()
    cases = {
        "NULL desc": None,
        "reserved[0]": D(2, 2, two(1, 0), lp, ip, fp, fp),
        "reserved[1]": D(2, 2, two(0, 1), lp, ip, fp, None),
        "no targets": D(2, 0, two(0, 0), lp, ip, fp, fp),
        "negative targets": D(2, -1, two(0, 0), lp, ip, fp, fp),
        "too many targets": D(2, 65536, two(0, 0), lp, ip, fp, fp),
        "NULL target_first": D(2, 2, two(0, 0), None, ip, fp, fp),
        "NULL corner": D(2, 2, two(0, 0), lp, None, fp, fp),
        "NULL dpos": D(2, 2, two(0, 0), lp, ip, None, fp),
        "NULL dpos and dnrm": D(2, 2, two(0, 0), lp, ip, None, None),
    }
    for what, d in cases.items():
        assert lib.pt_set_morph(fake, None if d is None else C.byref(d)) == _abi.PT_ERR_INVALID_ARG, what
        assert lib.pt_last_error(), what
    # pt_morph_meshes
    assert lib.pt_morph_meshes(None, C.byref(U(2, 0, 0, 0, wp, None)), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
    assert b"ctx" in lib.pt_last_error()
    cases = {
        "NULL u": None,
        "reserved": U(2, 0, 0, 1, wp, None),
        "mode 3": U(2, 3, 0, 0, wp, None),
        "mode -1": U(2, -1, 0, 0, wp, None),
        "NULL weights": U(2, 0, 0, 0, None, None),
        "NULL weights, FACE": U(2, _abi.NORMALS_FACE, 0, 0, None, None),
        "NULL weights with a skin": U(2, _abi.NORMALS_SMOOTH, 3, 0, None, mp),
        "bones without matrices": U(2, 0, 3, 0, wp, None),
        "negative bones without matrices": U(2, 0, -1, 0, wp, None),
    }
    for what, u in cases.items():
        assert lib.pt_morph_meshes(fake, None if u is None else C.byref(u), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG, what
        assert lib.pt_last_error(), what
    assert ms.value == -1.0   # nothing ran
    # pt_read_morph
    counts = (C.c_int64 * 3)(-1, -1, -1)
    assert lib.pt_read_morph(None, counts, lp, ip, fp, fp) == _abi.PT_ERR_INVALID_ARG
    assert lib.pt_read_morph(None, None, None, None, None, None) == _abi.PT_ERR_INVALID_ARG
    assert list(counts) == [-1, -1, -1]
