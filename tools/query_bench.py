#!/usr/bin/env python3
"""pt_intersect_hits against pt_intersect on one GPU in one process: what identity and Hit.Info cost per call.

The bench's default scene (scenes.bunny_frame, the 1M-triangle frame of bench.py's c4 workload) and 2^20 rays: the
camera rays of a 1024x512 frame in pixel order (Camera.CastRay at the pixel centres, no lens), then the same rays
shuffled (seeded), so half the waves are coherent and half are not.  `--reps` calls after `--warmup` untimed ones of

  intersect      Renderer.Intersect: pt_intersect, t and kind (wall time only: that entry point takes no device time)
  identity       Renderer.IntersectHits wanting t, kind, index, prim and shape: the kernel without Hit.Info
  all            Renderer.IntersectHits with every output

Each figure is the median with min and max: the wall time of the call, and for the two pt_intersect_hits variants the
device time between two hipEvents around the kernel (pt_query_kernel_ms).  Beside them pt_render_features' kernel time
on the same scene at 1024x1024 (the same trace and Hit.Info for one primary ray per pixel, 2^20 of them).  One JSON
document goes to --out.  k_intersect's own device time comes from a kernel trace of this tool (rocprofv3 --kernel-trace
--stats -- python tools/query_bench.py), which times every kernel named here.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from denoise_bench import summary  # noqa: E402
from ptsharp_amd import Renderer, scenes  # noqa: E402

IDENTITY = {"t", "kind", "index", "prim", "shape"}


def camera_rays(camera, w, h):
    """Camera.CastRay(x, y, w, h, 0.5, 0.5) of every pixel, row-major, the lens ignored: fp64 as the device forms
    them, rounded to fp32 once (a benchmark's rays: the last bit is not the point)."""
    c = camera.to_c()
    u, v, cw, p = (np.array(list(a), np.float64) for a in (c.u, c.v, c.w, c.p))
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    px = (x / (w - 1.0)) * 2 - 1
    py = (y / (h - 1.0)) * 2 - 1
    d = (-px * (w / h))[..., None] * u + (-py)[..., None] * v + c.m * cw
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    o = np.broadcast_to(p, d.shape)
    return np.ascontiguousarray(o.reshape(-1, 3), np.float32), np.ascontiguousarray(d.reshape(-1, 3), np.float32)


def timed(call, reps, warmup, kernel=None):
    for _ in range(warmup):
        call()
    wall, dev = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        if kernel:
            dev.append(kernel())
    out = {"wall_ms": summary(wall)}
    if kernel:
        out["kernel_ms"] = summary(dev)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_bench.json"))
    a = ap.parse_args()
    scene, camera, sampler = scenes.bunny_frame(a.tris)
    w, h = 1024, 512
    o, d = camera_rays(camera, w, h)
    perm = np.random.default_rng(2026).permutation(len(o))
    o = np.ascontiguousarray(np.concatenate([o, o[perm]]))
    d = np.ascontiguousarray(np.concatenate([d, d[perm]]))
    assert len(o) == 1 << 20
    doc = {"tool": "tools/query_bench.py", "scene": f"bunny_frame({a.tris})", "rays": len(o), "reps": a.reps, "warmup": a.warmup}
    r = Renderer.NewRenderer(scene, camera, sampler, 1024, 1024, True, device=0)
    try:
        doc["intersect"] = timed(lambda: r.Intersect(o, d), a.reps, a.warmup)
        doc["identity"] = timed(lambda: r.IntersectHits(o, d, want=IDENTITY), a.reps, a.warmup, r.QueryKernelMs)
        doc["all"] = timed(lambda: r.IntersectHits(o, d), a.reps, a.warmup, r.QueryKernelMs)
        hits = r.IntersectHits(o, d, want={"kind"})["kind"]
        doc["hit_share"] = round(float((hits >= 0).mean()), 4)
        for _ in range(a.warmup):
            r.RenderFeatures()
        doc["features_1024x1024_kernel_ms"] = summary([r.RenderFeatures() for _ in range(a.reps)])
    finally:
        r.close()
    n = len(o)
    doc["ns_per_ray"] = {"identity_kernel": round(doc["identity"]["kernel_ms"]["median"] * 1e6 / n, 4),
                         "all_kernel": round(doc["all"]["kernel_ms"]["median"] * 1e6 / n, 4),
                         "features_kernel": round(doc["features_1024x1024_kernel_ms"]["median"] * 1e6 / (1024 * 1024), 4)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
