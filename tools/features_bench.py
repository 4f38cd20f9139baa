#!/usr/bin/env python3
"""pt_render_features and pt_denoise_guided on one GPU in one process: kernel times, and the guided
filter against the unguided one.

For 1920x1080 and 3840x2160, `--reps` times after `--warmup` untimed calls:

  features   RenderFeatures() on the bench's default scene (scenes.bunny_frame, the 1M-triangle frame of
             bench.py's c4 workload): pt_render_features' out_kernel_ms (device time between two
             hipEvents around k_features) and the primary rays per second it amounts to;
  guided /   DenoiseBuffer(guided=True) and DenoiseBuffer() alternating on the same seeded Buffer and
  unguided   seeded features (LoadBuffer, LoadFeatures; 5 iterations, default sigmas): out_kernel_ms of
             each, and the ratio of the medians.

Each figure is the median with min and max.  One JSON document goes to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from denoise_bench import seeded_buffer, summary  # noqa: E402
from ptsharp_amd import Renderer, _abi, scenes  # noqa: E402

ITERATIONS = 5
SIGMAS = (4.0, 0.3, 0.3, 0.1)   # colour, normal, albedo, depth: the defaults


def seeded_features(w, h):
    """Three hit regions with their own normal, albedo and depth ramp, and a miss corner."""
    rng = np.random.default_rng(2025)
    yy, xx = np.mgrid[0:h, 0:w]
    u, v = xx / (w - 1), yy / (h - 1)
    region = (u + 0.3 * v > 0.45).astype(np.int32) + (v - 0.2 * u > 0.6).astype(np.int32)
    miss = (u > 0.7) & (v < 0.3)
    nrm = np.array([[0.0, 0.0, 1.0], [0.25, 0.0, 0.97], [0.0, 0.3, 0.95]])[region] + 0.05 * np.stack([u, v, 0 * u], axis=2)
    nrm = nrm / np.linalg.norm(nrm, axis=2, keepdims=True)
    alb = np.array([[0.60, 0.55, 0.50], [0.50, 0.62, 0.45], [0.55, 0.48, 0.62]])[region] + 0.003 * rng.standard_normal((h, w, 3))
    z = np.array([4.0, 4.6, 5.1])[region] + 0.5 * u + 0.3 * v
    return (np.where(miss[..., None], 0.5, alb), np.where(miss[..., None], 0.0, nrm).astype(np.float32),
            np.where(miss, 1e9, z), np.where(miss, -1, region).astype(np.int32))


def bench_features(scene, camera, sampler, w, h, reps, warmup):
    r = Renderer.NewRenderer(scene, camera, sampler, w, h, True, device=0)
    try:
        for _ in range(max(warmup, 1)):
            r.RenderFeatures()
        ms = [r.RenderFeatures() for _ in range(reps)]
        kind = r.Features()[3]
    finally:
        r.close()
    k = statistics.median(ms)
    return {"kernel_ms": summary(ms), "primary_rays": w * h, "rays_per_s": round(w * h / (k * 1e-3), 0),
            "hit_share": round(float((kind >= 0).mean()), 4)}


def bench_filters(w, h, reps, warmup):
    r = Renderer.NewRenderer(None, None, None, w, h, True, device=0)
    try:
        r.LoadBuffer(seeded_buffer(w, h), passes_done=0)
        r.LoadFeatures(*seeded_features(w, h))
        r.DenoiseParams = _abi.pt_denoise_params(ITERATIONS, 0, SIGMAS[0])
        r.DenoiseGuidedParams = _abi.pt_denoise_guided_params(ITERATIONS, 0, *SIGMAS)
        for _ in range(max(warmup, 1)):
            r.DenoiseBuffer(guided=True)
            r.DenoiseBuffer()
        guided, plain = [], []
        for _ in range(reps):
            guided.append(r.DenoiseBuffer(guided=True))
            plain.append(r.DenoiseBuffer())
    finally:
        r.close()
    return {"guided_kernel_ms": summary(guided), "unguided_kernel_ms": summary(plain),
            "guided_over_unguided": round(statistics.median(guided) / statistics.median(plain), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1920x1080,3840x2160")
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_bench.json"))
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    scene, camera, sampler = scenes.bunny_frame(a.tris)
    doc = {"tool": "tools/features_bench.py", "scene": f"bunny_frame({a.tris})", "iterations": ITERATIONS,
           "sigmas": dict(zip(("colour", "normal", "albedo", "depth"), SIGMAS)), "reps": a.reps, "warmup": a.warmup, "shapes": []}
    for w, h in shapes:
        s = {"width": w, "height": h, "features": bench_features(scene, camera, sampler, w, h, a.reps, a.warmup)}
        s.update(bench_filters(w, h, a.reps, a.warmup))
        doc["shapes"].append(s)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(f"{w}x{h}: features {s['features']['kernel_ms']['median']} ms ({s['features']['rays_per_s']:.3g} primary rays/s), "
              f"guided {s['guided_kernel_ms']['median']} ms, unguided {s['unguided_kernel_ms']['median']} ms, "
              f"ratio {s['guided_over_unguided']}", flush=True)


if __name__ == "__main__":
    main()
