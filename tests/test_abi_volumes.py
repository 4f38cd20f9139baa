"""pt_update_volumes and pt_read_volume: exported with C linkage, declared in the header and in the Python and C#
bindings field for field, and their NULL errors returned without a device (the checks that need a context are in
tests/test_gpu_volumes.py)."""
import ctypes as C
import re
import subprocess

import test_abi as A
from ptsharp_amd import _abi

NAMES = ("pt_update_volumes", "pt_read_volume")
FIELDS = ["num_volumes", "reserved", "data", "windows"]


def test_symbols_exported():
    lib = _abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True).stdout
    cs = open(A.os.path.join(A.ROOT, "csharp", "HipRenderer.cs")).read()
    for name in NAMES:
        assert name in A.declared_functions() and name in _abi.SIGNATURES and hasattr(lib, name)
        assert re.search(rf"\bT {name}\b", out), f"{name} not exported with C linkage"
        assert re.search(rf"static extern int {name}\(", cs), f"{name} has no DllImport"
    assert "public double UpdateVolumes(" in cs
    assert lib.pt_get_version() == 10 and _abi.ABI_VERSION == 10   # functions and a struct were added: no new version


def test_struct_matches_header_in_both_bindings():
    A.test_python_binding_matches_header("pt_volume_update")
    A.test_csharp_binding_matches_header("pt_volume_update")
    assert C.sizeof(_abi.pt_volume_update) == 16 + 2 * C.sizeof(C.c_void_p)
    assert [f[0] for f in _abi.pt_volume_update._fields_] == FIELDS
    assert _abi.pt_volume_update.reserved.offset == 4 and _abi.pt_volume_update.reserved.size == 12
    assert _abi.pt_volume_update.data.offset == 16 and _abi.pt_volume_update.windows.offset == 24
    header = open(A.os.path.join(A.ROOT, "include", "ptsharp_hip.h")).read()
    body = re.search(r"typedef struct pt_volume_update \{(.*?)\} pt_volume_update;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[\d+\])?;", body) == FIELDS
    cs = open(A.os.path.join(A.ROOT, "csharp", "HipRenderer.cs")).read()
    cbody = re.search(r"struct pt_volume_update[^{]*\{(.*?)\n        \}", cs, re.S).group(1)
    assert re.findall(r"public (?:fixed int|int|IntPtr) (\w+)(?:\[\d+\])?;", cbody) == FIELDS
    # the window rows pt_read_volume writes are the header's pt_volume_window: 24 bytes
    assert C.sizeof(_abi.pt_volume_window) == 24


def test_signatures_match_header():
    header = re.sub(r"/\*.*?\*/", "", open(A.HEADER).read(), flags=re.S)
    upd = " ".join(re.search(r"int pt_update_volumes\((.*?)\);", header, re.S).group(1).split())
    assert upd == "void* ctx, const pt_volume_update* u, double* out_kernel_ms"
    rd = " ".join(re.search(r"int pt_read_volume\((.*?)\);", header, re.S).group(1).split())
    assert rd == ("void* ctx, int32_t index, int64_t info[8], double* data, pt_volume_window* windows, int8_t* runs, "
                  "double* cells")
    d, win = C.POINTER(C.c_double), C.POINTER(_abi.pt_volume_window)
    assert _abi.SIGNATURES["pt_update_volumes"] == (C.c_int, [C.c_void_p, C.POINTER(_abi.pt_volume_update), d])
    assert _abi.SIGNATURES["pt_read_volume"] == (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), d, win,
                                                           C.POINTER(C.c_int8), d])
    cs = open(A.os.path.join(A.ROOT, "csharp", "HipRenderer.cs")).read()
    assert re.search(r"extern int pt_update_volumes\(IntPtr ctx, ref pt_volume_update u, out double kernelMs\);", cs)
    assert re.search(r"extern int pt_read_volume\(IntPtr ctx, int index, long\[\] info, double\[\] data, "
                     r"\[In, Out\] pt_volume_window\[\] windows, sbyte\[\] runs, double\[\] cells\);", cs)


def test_renderer_has_the_methods():
    from ptsharp_amd import Renderer
    assert callable(Renderer.UpdateVolumes) and callable(Renderer.ReadVolume)


def test_null_errors_without_a_device():
    lib = _abi.load_library()
    ms = C.c_double(-7.0)
    u = _abi.pt_volume_update()
    assert lib.pt_update_volumes(None, C.byref(u), C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
    assert b"NULL" in lib.pt_last_error()
    fake = C.c_void_p(1)   # never dereferenced: a NULL `u` fails before the context is read
    assert lib.pt_update_volumes(fake, None, C.byref(ms)) == _abi.PT_ERR_INVALID_ARG
    assert b"NULL" in lib.pt_last_error()
    assert lib.pt_read_volume(None, 0, None, None, None, None, None) == _abi.PT_ERR_INVALID_ARG
    assert ms.value == -7.0
