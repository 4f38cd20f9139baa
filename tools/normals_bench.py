#!/usr/bin/env python3
"""pt_update_triangles_normals against the host route it replaces, on one GPU in one process: what the normals
of a moving smooth-shaded mesh cost.

On the bench's default scene (scenes.bunny_frame, the 1M-triangle frame of bench.py's c4 workload) with the sine
pose applied to every triangle vertex (z += 0.3 sin(5x) cos(3y)), each figure the median of `--reps` calls after
`--warmup` untimed ones, with min and max:

  face / smooth  pt_update_triangles_normals of the posed vertices in either mode: the wall time of the call (the
                 copy of the three arrays in, the kernels, the root node back) and its out_kernel_ms (device time
                 between two hipEvents around the normals kernels, the sort and the refit);
  host           what a caller does without it, per frame: the face normals on the host (scene.fix_normals_arrays),
                 pt_mesh_smooth_normals on every mesh, pt_update_triangles with six arrays; each part's wall time
                 and their sum;
  check          one 16-spp 1920x1080 step after the smooth device route and one after the host route, from an
                 empty Buffer with the same seed: the two Buffers compared bit for bit, and the normals
                 pt_read_tri_normals returns after the device route against the host's.

One JSON document goes to --out.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ptsharp_amd import _abi, scenes  # noqa: E402
from ptsharp_amd.scene import fix_normals_arrays  # noqa: E402

W, H, SPP = 1920, 1080, 16
FP = C.POINTER(C.c_float)


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def sine_pose(v, amplitude=0.3):
    f = np.float32
    out = v.copy()
    out[:, 2] = v[:, 2] + (f(amplitude) * np.sin(f(5) * v[:, 0]) * np.cos(f(3) * v[:, 1])).astype(f)
    return np.ascontiguousarray(out, f)


def check(lib, code, where):
    if code != _abi.PT_OK:
        raise RuntimeError(f"{where}: {code} {lib.pt_last_error().decode()}")


def ptrs(arrs):
    return [a.ctypes.data_as(FP) for a in arrs]


def device_route(lib, ctx, n, moved, mode, reps, warmup):
    wall, kernel = [], []
    for i in range(warmup + reps):
        ms = C.c_double(0.0)
        t0 = time.perf_counter()
        check(lib, lib.pt_update_triangles_normals(ctx, n, *ptrs(moved), mode, C.byref(ms)), "pt_update_triangles_normals")
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            wall.append(dt)
            kernel.append(ms.value)
    return {"wall_ms": summary(wall), "kernel_ms": summary(kernel)}


def host_route(lib, ctx, n, moved, flat, reps, warmup):
    parts = {"face_ms": [], "smooth_ms": [], "update_ms": [], "wall_ms": []}
    normals = None
    with np.errstate(all="ignore"):
        for i in range(warmup + reps):
            t0 = time.perf_counter()
            z = np.zeros_like(moved[0])
            normals = [np.ascontiguousarray(a, np.float32) for a in fix_normals_arrays(*moved, z, z, z)]
            t1 = time.perf_counter()
            for f, c in zip(flat.mesh_first, flat.mesh_count):
                r = slice(int(f), int(f) + int(c))
                part = [np.ascontiguousarray(a[r]) for a in moved + normals]
                if lib.pt_mesh_smooth_normals(int(c), *ptrs(part)) != _abi.PT_OK:
                    raise RuntimeError(lib.pt_obj_last_error().decode())
                for dst, src in zip(normals, part[3:]):
                    dst[r] = src
            t2 = time.perf_counter()
            check(lib, lib.pt_update_triangles(ctx, n, *ptrs(moved + normals), None), "pt_update_triangles")
            t3 = time.perf_counter()
            if i >= warmup:
                for key, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
                    parts[key].append(dt * 1e3)
    return {k: summary(v) for k, v in parts.items()}, normals


def step(lib, ctx, camera, sampler):
    """One 16-spp step from an empty Buffer: M, V, N."""
    cam, smp = camera.to_c(), sampler.to_c()
    check(lib, lib.pt_reset_buffer(ctx), "pt_reset_buffer")
    pp = _abi.pt_pass_params(SPP, 0, 1234, 1, 0, C.POINTER(C.c_int32)(), _abi.ENGINE_AUTO, 0, 0, 0, 1)
    check(lib, lib.pt_render_pass(ctx, C.byref(cam), C.byref(smp), C.byref(pp)), "pt_render_pass")
    M, V, N = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W), np.int32)
    check(lib, lib.pt_read_buffer(ctx, M.ctypes.data_as(C.POINTER(C.c_double)), V.ctypes.data_as(C.POINTER(C.c_double)),
                                  N.ctypes.data_as(C.POINTER(C.c_int32))), "pt_read_buffer")
    return M, V, N


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_bench.json"))
    a = ap.parse_args()
    lib = _abi.load_library()
    scene, camera, sampler = scenes.bunny_frame(a.tris)
    flat = scene.Compile()
    n = len(flat.tri_material)
    moved = [sine_pose(v) for v in (flat.tri_v1, flat.tri_v2, flat.tri_v3)]
    doc = {"tool": "tools/normals_bench.py", "scene": f"bunny_frame({a.tris})", "triangles": n,
           "meshes": [int(c) for c in flat.mesh_count], "pose": "z += 0.3 sin(5x) cos(3y)", "reps": a.reps, "warmup": a.warmup,
           "step": f"{W}x{H} at {SPP} spp"}
    ctx = C.c_void_p()
    opts = _abi.pt_device_opts(0, W, H)
    check(lib, lib.pt_create(C.byref(opts), C.byref(ctx)), "pt_create")
    try:
        check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")   # the rest pose
        doc["face"] = device_route(lib, ctx, n, moved, _abi.NORMALS_FACE, a.reps, a.warmup)
        doc["smooth"] = device_route(lib, ctx, n, moved, _abi.NORMALS_SMOOTH, a.reps, a.warmup)
        got = [np.zeros((n, 3), np.float32) for _ in range(3)]
        check(lib, lib.pt_read_tri_normals(ctx, *ptrs(got)), "pt_read_tri_normals")
        device_buffer = step(lib, ctx, camera, sampler)
        doc["host"], want = host_route(lib, ctx, n, moved, flat, a.reps, a.warmup)
        host_buffer = step(lib, ctx, camera, sampler)
        nan = [np.isnan(w) for w in want]
        doc["check"] = {
            "buffers_equal": bool(all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(device_buffer, host_buffer))),
            "normals_equal": bool(all(np.array_equal(np.isnan(g), m) and np.array_equal(g.view(np.uint32)[~m], w.view(np.uint32)[~m])
                                      for g, w, m in zip(got, want, nan))),
            "nan_components": int(sum(int(m.sum()) for m in nan)),
            "lit_pixels": float((device_buffer[0].sum(axis=2) > 0).mean()),
        }
        doc["host_over_smooth_wall"] = round(doc["host"]["wall_ms"]["median"] / doc["smooth"]["wall_ms"]["median"], 1)
    finally:
        lib.pt_destroy(ctx)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
