#!/usr/bin/env python3
"""pt_update_triangles against pt_upload_scene on one GPU in one process: what moving a mesh costs.

On the bench's default scene (scenes.bunny_frame, the 1M-triangle frame of bench.py's c4 workload) with the
sine pose applied to every triangle vertex (z += 0.3 sin(5x) cos(3y)), each figure the median of `--reps`
calls after `--warmup` untimed ones, with min and max:

  update     pt_update_triangles of the posed vertices: the wall time of the call (the copy of the three
             arrays in, the kernels, the root node back) and its out_kernel_ms (device time between two
             hipEvents around k_refit_leaves and the k_refit_level launches);
  upload     the wall time of pt_upload_scene of the same deformed scene (the host compile, the host
             triangle-BVH build, every array copied in).  Every timed upload is a geometry the process
             has not seen (the amplitude differs in its last digits), as the frames of an animation are,
             so none is served by the triangle-BVH cache;
  rays       one 16-spp 1920x1080 step at the refitted pose against the same step after a fresh upload of
             that pose: rays (pt_stats) per second of device time.  The refit keeps the topology the SAH
             build chose for the rest pose; this is what that costs.

`--upload-only --lib PATH` measures only `upload`, through another build of the library (one without
pt_update_triangles, to record what the only path cost there).  One JSON document goes to --out.
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

W, H, SPP = 1920, 1080, 16


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def sine_pose(v, amplitude=0.3):
    f = np.float32
    out = v.copy()
    out[:, 2] = v[:, 2] + (f(amplitude) * np.sin(f(5) * v[:, 0]) * np.cos(f(3) * v[:, 1])).astype(f)
    return np.ascontiguousarray(out, f)


def load(path):
    """The library at `path` with the prototypes of the entry points it has."""
    lib = C.CDLL(path)
    for name, (res, args) in _abi.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def check(lib, code, where):
    if code != _abi.PT_OK:
        raise RuntimeError(f"{where}: {code} {lib.pt_last_error().decode()}")


def set_pose(flat, rest, amplitude):
    for dst, src in zip((flat.tri_v1, flat.tri_v2, flat.tri_v3), rest):
        dst[...] = sine_pose(src, amplitude)


def timed_uploads(lib, ctx, flat, rest, reps, warmup):
    wall = []
    for i in range(warmup + reps):
        set_pose(flat, rest, 0.3 + 1e-5 * (i + 1))   # a geometry of its own: no cached build
        t0 = time.perf_counter()
        check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            wall.append(dt)
    return {"wall_ms": summary(wall)}


def step(lib, ctx, camera, sampler, reps, warmup):
    cam, smp = camera.to_c(), sampler.to_c()
    ms, rays = [], []
    for i in range(warmup + reps):
        pp = _abi.pt_pass_params(SPP, 0, 1234, i + 1, 0, C.POINTER(C.c_int32)(), _abi.ENGINE_AUTO, 0, 0, 0, 1)
        check(lib, lib.pt_render_pass(ctx, C.byref(cam), C.byref(smp), C.byref(pp)), "pt_render_pass")
        s = _abi.pt_stats()
        check(lib, lib.pt_stats_get(ctx, C.byref(s)), "pt_stats_get")
        if i >= warmup:
            ms.append(s.last_pass_ms)
            rays.append(int(s.rays))
    check(lib, lib.pt_reset_buffer(ctx), "pt_reset_buffer")
    m = statistics.median(ms)
    return {"step_ms": summary(ms), "rays_per_step": int(statistics.median(rays)),
            "rays_per_s": round(statistics.median(rays) / (m * 1e-3), 0)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--upload-reps", type=int, default=5, help="timed pt_upload_scene calls (seconds each at 1M triangles)")
    ap.add_argument("--step-reps", type=int, default=3)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--lib", default=_abi.LIB_PATH)
    ap.add_argument("--upload-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit_bench.json"))
    a = ap.parse_args()
    lib = load(a.lib)
    scene, camera, sampler = scenes.bunny_frame(a.tris)
    flat = scene.Compile()
    rest = [flat.tri_v1.copy(), flat.tri_v2.copy(), flat.tri_v3.copy()]
    n = len(flat.tri_material)
    doc = {"tool": "tools/refit_bench.py", "scene": f"bunny_frame({a.tris})", "triangles": n, "pose": "z += 0.3 sin(5x) cos(3y)",
           "reps": a.reps, "warmup": a.warmup, "upload_reps": a.upload_reps, "step": f"{W}x{H} at {SPP} spp",
           "library": os.path.relpath(a.lib, ROOT) if a.lib.startswith(ROOT) else os.path.basename(a.lib)}
    ctx = C.c_void_p()
    opts = _abi.pt_device_opts(0, W, H)
    check(lib, lib.pt_create(C.byref(opts), C.byref(ctx)), "pt_create")
    try:
        if not a.upload_only:
            check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")   # the rest pose
            moved = [sine_pose(v) for v in rest]
            fp = C.POINTER(C.c_float)
            ptrs = [v.ctypes.data_as(fp) for v in moved] + [fp()] * 3
            wall, kernel = [], []
            for i in range(a.warmup + a.reps):
                ms = C.c_double(0.0)
                t0 = time.perf_counter()
                check(lib, lib.pt_update_triangles(ctx, n, *ptrs, C.byref(ms)), "pt_update_triangles")
                dt = (time.perf_counter() - t0) * 1e3
                if i >= a.warmup:
                    wall.append(dt)
                    kernel.append(ms.value)
            counts = (C.c_int64 * 3)()
            check(lib, lib.pt_read_tri_bvh(ctx, counts, None, None, None, None), "pt_read_tri_bvh")
            doc["update"] = {"wall_ms": summary(wall), "kernel_ms": summary(kernel), "nodes": int(counts[0]),
                             "chunks": int(counts[1]), "input_bytes": 36 * n,
                             "written_bytes_min": 48 * int(counts[2]) + 128 * int(counts[1]) + 112 * int(counts[0])}
            doc["rays_refitted"] = step(lib, ctx, camera, sampler, a.step_reps, 1)
        doc["upload"] = timed_uploads(lib, ctx, flat, rest, a.upload_reps, 1)
        if not a.upload_only:
            set_pose(flat, rest, 0.3)
            check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")
            doc["rays_fresh_upload"] = step(lib, ctx, camera, sampler, a.step_reps, 1)
            doc["upload_over_update_wall"] = round(doc["upload"]["wall_ms"]["median"] / doc["update"]["wall_ms"]["median"], 1)
            doc["refitted_over_fresh_rays_per_s"] = round(doc["rays_refitted"]["rays_per_s"] / doc["rays_fresh_upload"]["rays_per_s"], 4)
    finally:
        lib.pt_destroy(ctx)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
