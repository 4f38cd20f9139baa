"""pt_rebuild_blas and pt_blas_cost at the ABI, without a GPU: the symbols exist in the header, the library, the ctypes
table and the C# drop-in with the same `what` values, the ABI version is still 10, and the error paths that need no
device answer PT_ERR_INVALID_ARG with a message (the others are tests/test_gpu_blas_rebuild.py's)."""
import ctypes as C
import os
import re

from ptsharp_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pt_rebuild_blas", "pt_blas_cost")


def test_symbols_and_version():
    lib = _abi.load_library()
    header = open(os.path.join(ROOT, "include", "ptsharp_hip.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "HipRenderer.cs")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert re.search(rf"static extern int {name}\(", cs), name
    assert re.search(r"^#define PT_REBUILD_WORLD 1\b", header, re.M) and re.search(r"^#define PT_REBUILD_BLAS 2\b", header, re.M)
    assert (_abi.REBUILD_WORLD, _abi.REBUILD_BLAS) == (1, 2)
    assert "PT_REBUILD_WORLD = 1, PT_REBUILD_BLAS = 2" in cs
    assert lib.pt_get_version() == _abi.ABI_VERSION == 10
    assert "#define PT_ABI_VERSION 10" in header
    from ptsharp_amd import Renderer
    assert callable(Renderer.RebuildBlas) and callable(Renderer.BlasCost)


def test_null_arguments():
    lib = _abi.load_library()
    ms = C.c_double(-1.0)
    u = _abi.pt_mesh_update()
    for what in (0, 1, 2, 3, 4):
        assert lib.pt_rebuild_blas(None, C.byref(u), what, C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
        assert b"NULL" in lib.pt_last_error()
    assert lib.pt_rebuild_blas(None, None, 0, None) == _abi.PT_ERR_INVALID_ARG
    assert ms.value == -1.0
    out = (C.c_double * 3)(7.0, 7.0, 7.0)
    assert lib.pt_blas_cost(None, 1, out) == _abi.PT_ERR_INVALID_ARG
    assert b"NULL" in lib.pt_last_error()
    assert lib.pt_blas_cost(None, 0, None) == _abi.PT_ERR_INVALID_ARG
    assert list(out) == [7.0, 7.0, 7.0]
