"""pt_intersect_hits (and pt_query_kernel_ms): exported with C linkage, declared in the header and in the Python and C#
bindings field for field, and its NULL errors returned without a device (the checks that need a context are in
tests/test_gpu_query.py)."""
import ctypes as C
import re
import subprocess

import numpy as np

import test_abi as A
from ptsharp_amd import _abi

NAMES = ("pt_intersect_hits", "pt_query_kernel_ms")
FIELDS = ["reserved", "t", "kind", "index", "prim", "shape", "position", "normal", "inside", "material", "albedo", "gloss"]


def test_symbols_exported():
    lib = _abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True).stdout
    cs = open(A.os.path.join(A.ROOT, "csharp", "HipRenderer.cs")).read()
    for name in NAMES:
        assert name in A.declared_functions() and name in _abi.SIGNATURES and hasattr(lib, name)
        assert re.search(rf"\bT {name}\b", out), f"{name} not exported with C linkage"
        assert re.search(rf"static extern int {name}\(", cs), f"{name} has no DllImport"
    assert "public Hits IntersectHits(" in cs
    assert lib.pt_get_version() == 10 and _abi.ABI_VERSION == 10   # functions and a struct were added: no new version


def test_struct_matches_header_in_both_bindings():
    A.test_python_binding_matches_header("pt_hit_arrays")
    A.test_csharp_binding_matches_header("pt_hit_arrays")
    assert C.sizeof(_abi.pt_hit_arrays) == 8 + 11 * C.sizeof(C.c_void_p)
    assert [f[0] for f in _abi.pt_hit_arrays._fields_] == FIELDS
    assert list(_abi.HIT_ARRAYS) == FIELDS[1:]
    header = open(A.os.path.join(A.ROOT, "include", "ptsharp_hip.h")).read()
    body = re.search(r"typedef struct pt_hit_arrays \{(.*?)\} pt_hit_arrays;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[\d+\])?;", body) == FIELDS
    cs = open(A.os.path.join(A.ROOT, "csharp", "HipRenderer.cs")).read()
    cbody = re.search(r"struct pt_hit_arrays[^{]*\{(.*?)\n        \}", cs, re.S).group(1)
    assert re.findall(r"public (?:fixed int|IntPtr) (\w+)(?:\[\d+\])?;", cbody) == FIELDS
    for k, name in enumerate(FIELDS[1:]):
        assert getattr(_abi.pt_hit_arrays, name).offset == 8 + 8 * k


def test_renderer_has_the_method():
    from ptsharp_amd import Renderer
    assert callable(Renderer.IntersectHits) and callable(Renderer.QueryKernelMs)


def test_null_errors_without_a_device():
    lib = _abi.load_library()
    o = np.zeros((2, 3), np.float32)
    p = o.ctypes.data_as(C.POINTER(C.c_float))
    t = np.full(2, -7.0)
    arrays = _abi.pt_hit_arrays()
    arrays.t = t.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.pt_intersect_hits(None, 2, p, p, 0, C.byref(arrays)) == _abi.PT_ERR_INVALID_ARG
    assert b"NULL" in lib.pt_last_error()
    fake = C.c_void_p(1)   # never dereferenced: a NULL `out` fails before the context is read
    assert lib.pt_intersect_hits(fake, 2, p, p, 0, None) == _abi.PT_ERR_INVALID_ARG
    assert b"NULL" in lib.pt_last_error()
    assert lib.pt_query_kernel_ms(None, None) == _abi.PT_ERR_INVALID_ARG
    assert (t == -7.0).all()
