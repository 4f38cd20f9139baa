#!/usr/bin/env python3
"""pt_rebuild_meshes against pt_upload_scene on one GPU in one process: what re-sorting the triangle BVH costs, and
what the re-sorted tree is worth.

On the bench's default scene (scenes.bunny_frame, the 1M-triangle frame of bench.py's c4 workload), each figure the
median of `--reps` calls after `--warmup` untimed ones, with min and max:

  rebuild    pt_rebuild_meshes of the posed vertices: the wall time of the call (the copy of the three arrays in, the
             kernels, the root node and src_of_pos back) and its out_kernel_ms (every kernel of the call);
  update     pt_update_triangles of the same vertices, for scale;
  upload     the wall time of pt_upload_scene of the same deformed scene, the only remedy a build without
             pt_rebuild_meshes has.  Every timed upload is a geometry the process has not seen (the amplitude differs
             in its last digits), so none is served by the triangle-BVH cache;
  tree       at the sine pose (z += 0.3 sin(5x) cos(3y)) and the twist pose (about y by 3 y rad), one 16-spp 1920x1080
             step three ways: after a fresh upload of the pose, after a refit (pt_update_triangles) and after a
             rebuild, with pt_tri_bvh_cost beside each, so the surface-area proxy is calibrated against trace time.

`--upload-only --lib PATH` measures only `upload`, through another build of the library (one without
pt_rebuild_meshes, to record what the only path cost there).  One JSON document goes to --out.
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
f32 = np.float32


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def sine_pose(v, amplitude=0.3):
    out = v.copy()
    out[:, 2] = v[:, 2] + (f32(amplitude) * np.sin(f32(5) * v[:, 0]) * np.cos(f32(3) * v[:, 1])).astype(f32)
    return np.ascontiguousarray(out, f32)


def twist_pose(v, rate=3.0):
    a = (f32(rate) * v[:, 1]).astype(f32)
    c, s = np.cos(a).astype(f32), np.sin(a).astype(f32)
    return np.ascontiguousarray(np.stack([c * v[:, 0] + s * v[:, 2], v[:, 1], c * v[:, 2] - s * v[:, 0]], 1), f32)


POSES = {"sine": sine_pose, "twist": twist_pose}


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


def set_pose(flat, rest, fn, param):
    for dst, src in zip((flat.tri_v1, flat.tri_v2, flat.tri_v3), rest):
        dst[...] = fn(src, param)


def timed_uploads(lib, ctx, flat, rest, reps, warmup):
    wall = []
    for i in range(warmup + reps):
        set_pose(flat, rest, sine_pose, 0.3 + 1e-5 * (i + 1))   # a geometry of its own: no cached build
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
    out = {"step_ms": summary(ms), "rays_per_step": int(statistics.median(rays)),
           "rays_per_s": round(statistics.median(rays) / (m * 1e-3), 0)}
    cost = (C.c_double * 3)()
    check(lib, lib.pt_tri_bvh_cost(ctx, cost), "pt_tri_bvh_cost")
    out["tri_bvh_cost"] = {"inner": round(cost[0], 4), "leaf": round(cost[1], 4), "total": round(cost[0] + cost[1], 4)}
    return out


def timed_calls(lib, ctx, n, ptrs, reps, warmup, rebuild):
    fp = C.POINTER(C.c_float)
    wall, kernel = [], []
    u = _abi.pt_mesh_update()
    u.num_triangles = n
    u.v1, u.v2, u.v3 = ptrs
    for i in range(warmup + reps):
        ms = C.c_double(0.0)
        t0 = time.perf_counter()
        if rebuild:
            check(lib, lib.pt_rebuild_meshes(ctx, C.byref(u), C.byref(ms)), "pt_rebuild_meshes")
        else:
            check(lib, lib.pt_update_triangles(ctx, n, *ptrs, fp(), fp(), fp(), C.byref(ms)), "pt_update_triangles")
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            wall.append(dt)
            kernel.append(ms.value)
    return {"wall_ms": summary(wall), "kernel_ms": summary(kernel)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--upload-reps", type=int, default=5, help="timed pt_upload_scene calls (seconds each at 1M triangles)")
    ap.add_argument("--step-reps", type=int, default=3)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--lib", default=_abi.LIB_PATH)
    ap.add_argument("--upload-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rebuild_bench.json"))
    a = ap.parse_args()
    lib = load(a.lib)
    scene, camera, sampler = scenes.bunny_frame(a.tris)
    flat = scene.Compile()
    rest = [flat.tri_v1.copy(), flat.tri_v2.copy(), flat.tri_v3.copy()]
    n = len(flat.tri_material)
    doc = {"tool": "tools/rebuild_bench.py", "scene": f"bunny_frame({a.tris})", "triangles": n,
           "poses": {"sine": "z += 0.3 sin(5x) cos(3y)", "twist": "about y by 3 y rad"},
           "reps": a.reps, "warmup": a.warmup, "upload_reps": a.upload_reps, "step": f"{W}x{H} at {SPP} spp",
           "library": os.path.relpath(a.lib, ROOT) if a.lib.startswith(ROOT) else os.path.basename(a.lib)}
    ctx = C.c_void_p()
    opts = _abi.pt_device_opts(0, W, H)
    check(lib, lib.pt_create(C.byref(opts), C.byref(ctx)), "pt_create")
    fp = C.POINTER(C.c_float)
    try:
        if not a.upload_only:
            check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")   # the rest pose
            rest_step = step(lib, ctx, camera, sampler, a.step_reps, 1)
            doc["rest"] = rest_step
            doc["tree"] = {}
            for name, fn in POSES.items():
                moved = [fn(v) for v in rest]
                ptrs = [v.ctypes.data_as(fp) for v in moved]
                entry = {}
                entry["update"] = timed_calls(lib, ctx, n, ptrs, a.reps, a.warmup, rebuild=False)
                entry["refit"] = step(lib, ctx, camera, sampler, a.step_reps, 1)
                entry["rebuild"] = timed_calls(lib, ctx, n, ptrs, a.reps, a.warmup, rebuild=True)
                entry["rebuilt"] = step(lib, ctx, camera, sampler, a.step_reps, 1)
                counts = (C.c_int64 * 3)()
                check(lib, lib.pt_read_tri_bvh(ctx, counts, None, None, None, None), "pt_read_tri_bvh")
                entry["rebuilt_counts"] = {"nodes": int(counts[0]), "chunks": int(counts[1]), "positions": int(counts[2])}
                # a fresh upload of the pose (this also restores the SAH topology for the next pose's refit)
                for dst, v in zip((flat.tri_v1, flat.tri_v2, flat.tri_v3), moved):
                    dst[...] = v
                t0 = time.perf_counter()
                check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")
                entry["fresh_upload_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
                entry["fresh"] = step(lib, ctx, camera, sampler, a.step_reps, 1)
                for key in ("refit", "rebuilt"):
                    entry[f"{key}_over_fresh_rays_per_s"] = round(entry[key]["rays_per_s"] / entry["fresh"]["rays_per_s"], 4)
                doc["tree"][name] = entry
                for dst, v in zip((flat.tri_v1, flat.tri_v2, flat.tri_v3), rest):
                    dst[...] = v
                check(lib, lib.pt_upload_scene(ctx, C.byref(flat.desc)), "pt_upload_scene")   # back to the rest pose's tree
        doc["upload"] = timed_uploads(lib, ctx, flat, rest, a.upload_reps, 1)
        if not a.upload_only:
            r = doc["tree"]["sine"]["rebuild"]
            doc["upload_over_rebuild_wall"] = round(doc["upload"]["wall_ms"]["median"] / r["wall_ms"]["median"], 1)
    finally:
        lib.pt_destroy(ctx)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
