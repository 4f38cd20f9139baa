"""pt_motion_snapshot, pt_render_motion, pt_read_motion, pt_accumulate_temporal, pt_read_temporal, pt_denoise_temporal and
pt_reset_temporal: exported with C linkage, declared in the Python and C# bindings field for field, the ABI still version
10, and their NULL and argument errors returned without a device (no context can exist without one, so the checks that
need a scene are in tests/test_gpu_motion.py)."""
import ctypes as C
import re
import subprocess

import test_abi as A
from ptsharp_amd import _abi

NAMES = ("pt_motion_snapshot", "pt_render_motion", "pt_read_motion", "pt_accumulate_temporal", "pt_read_temporal",
         "pt_denoise_temporal", "pt_reset_temporal")
MOTION_ARRAYS = ("PT_MOTION_SHAPE_I32", "PT_MOTION_PRIM_I32", "PT_MOTION_DEPTH_F64", "PT_MOTION_PREV_XY_F64",
                 "PT_MOTION_PREV_DEPTH_F64", "PT_MOTION_PREV_PIXEL_I32", "PT_MOTION_STATUS_I32")


def test_symbols_exported():
    lib = _abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True).stdout
    cs = open(A.os.path.join(A.ROOT, "csharp", "HipRenderer.cs")).read()
    for name in NAMES:
        assert name in A.declared_functions() and name in _abi.SIGNATURES and hasattr(lib, name)
        assert re.search(rf"\bT {name}\b", out), f"{name} not exported with C linkage"
        assert re.search(rf"static extern int {name}\(", cs), f"{name} has no DllImport"
    for method in ("public void MotionSnapshot(", "public double RenderMotion(", "public Array Motion(", "public double AccumulateTemporal(",
                   "public void Temporal(", "public unsafe double DenoiseTemporal(", "public void ResetTemporal(", "public void TemporalFrame("):
        assert method in cs, method
    assert lib.pt_get_version() == 10 and _abi.ABI_VERSION == 10
    header = open(A.HEADER).read()
    assert re.search(r"#define PT_ABI_VERSION 10\b", header)


def test_struct_and_enum_match_header_in_both_bindings():
    A.test_python_binding_matches_header("pt_temporal_params")
    A.test_csharp_binding_matches_header("pt_temporal_params")
    T = _abi.pt_temporal_params
    assert C.sizeof(T) == 16
    assert [getattr(T, f).offset for f in ("max_history", "reserved", "sigma_depth")] == [0, 4, 8]
    header = open(A.HEADER).read()
    cs = open(A.os.path.join(A.ROOT, "csharp", "HipRenderer.cs")).read()
    for value, name in enumerate(MOTION_ARRAYS):
        assert re.search(rf"\b{name} = {value}\b", header), name
        assert re.search(rf"\b{name} = {value}\b", cs), name
        assert getattr(_abi, name[3:]) == value
    # pt_read_features' enum is not extended
    assert re.search(r"PT_FEATURE_MATERIAL_I32 = 4\s*/\*[^*]*\*/\s*\} pt_feature;", header)


def test_renderer_has_the_methods():
    from ptsharp_amd import Renderer
    for name in ("MotionSnapshot", "RenderMotion", "Motion", "AccumulateTemporal", "Temporal", "DenoiseTemporal", "ResetTemporal",
                 "TemporalFrame"):
        assert callable(getattr(Renderer, name))
    r = Renderer()
    assert (r.TemporalParams.max_history, r.TemporalParams.reserved, r.TemporalParams.sigma_depth) == (32, 0, 0.1)


def test_argument_errors_without_a_device():
    lib = _abi.load_library()
    fake = C.c_void_p(1)   # never dereferenced: every case fails on an argument checked before the context is read
    cam = _abi.pt_camera()
    ms = C.c_double(-1.0)
    buf = (C.c_double * 4)()
    T, P, G = _abi.pt_temporal_params, _abi.pt_denoise_params, _abi.pt_denoise_guided_params
    bad = _abi.PT_ERR_INVALID_ARG
    # a NULL context, everywhere
    assert lib.pt_motion_snapshot(None, C.byref(cam)) == bad and lib.pt_last_error()
    assert lib.pt_render_motion(None, C.byref(cam), C.byref(ms)) == bad
    assert lib.pt_read_motion(None, 0, buf) == bad
    assert lib.pt_accumulate_temporal(None, None, C.byref(ms)) == bad and b"ctx" in lib.pt_last_error()
    assert lib.pt_read_temporal(None, None, None, None, None) == bad
    assert lib.pt_denoise_temporal(None, None, None, C.byref(ms)) == bad
    assert lib.pt_reset_temporal(None) == bad and b"ctx" in lib.pt_last_error()
    # a NULL camera or out pointer, an enum out of range
    assert lib.pt_motion_snapshot(fake, None) == bad and b"camera" in lib.pt_last_error()
    assert lib.pt_render_motion(fake, None, C.byref(ms)) == bad and b"camera" in lib.pt_last_error()
    assert lib.pt_read_motion(fake, 0, None) == bad
    for what in (-1, 7, 1 << 30):
        assert lib.pt_read_motion(fake, what, buf) == bad and b"pt_motion_array" in lib.pt_last_error()
    # pt_temporal_params out of range
    cases = {"negative max_history": T(-1, 0, 0.1), "max_history above 2^20": T((1 << 20) + 1, 0, 0.1), "reserved": T(32, 1, 0.1),
             "negative sigma_depth": T(32, 0, -0.1), "NaN sigma_depth": T(32, 0, float("nan")),
             "infinite sigma_depth": T(32, 0, float("inf"))}
    for what, p in cases.items():
        assert lib.pt_accumulate_temporal(fake, C.byref(p), C.byref(ms)) == bad, what
        assert lib.pt_last_error(), what
    # plain and guided at once
    assert lib.pt_denoise_temporal(fake, C.byref(P(5, 0, 4.0)), C.byref(G(5, 0, 4.0, 0.3, 0.3, 0.1)), C.byref(ms)) == bad
    assert b"not both" in lib.pt_last_error()
    assert ms.value == -1.0 and list(buf) == [0.0] * 4   # nothing ran
