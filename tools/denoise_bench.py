#!/usr/bin/env python3
"""pt_denoise on one GPU in one process: kernel time, call time, and the rate against the bytes the
filter must move.

For 1920x1080 and 3840x2160 a seeded Buffer is loaded (LoadBuffer) and, `--reps` times after
`--warmup` untimed calls, DenoiseBuffer() (5 iterations, sigma_colour 4) and Denoised() are timed:

  kernel_ms  pt_denoise's out_kernel_ms: device time between two hipEvents around its launches
             (prepare, blur and the levels);
  call_ms    a host clock around DenoiseBuffer() + Denoised(): the call ends in a stream
             synchronise, and the 8-bit read-back (resolve kernel and a 3 B per pixel copy) is
             included, so this is what IterativeRender pays per pass;
  numpy_ms   the numpy restatement (tests/denoise_ref.py) on the same input, 1920x1080 only, once.

`compulsory_bytes` is what the levels must move if every tap after the first came from cache: 48 B
read and 48 B written per pixel per level; `hbm_share` is that over the kernel time as a share of
the 8 TB/s HBM peak the project's roofline uses.  `exp_per_s` is the 25 fp64 exp per pixel per
level over the same time.  One JSON document goes to --out.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ptsharp_amd import Renderer, _abi  # noqa: E402
from ptsharp_amd.renderer import Buffer  # noqa: E402

HBM_PEAK = 8e12
ITERATIONS = 5
SIGMA = 4.0


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def seeded_buffer(w, h):
    """A smooth picture with an edge and noise, N in 1..5, V consistent with the noise."""
    rng = np.random.default_rng(2024)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([0.2 + 0.5 * xx / (w - 1), 0.6 - 0.3 * yy / (h - 1), np.where(xx * 2 >= w, 0.9, 0.15) + 0.0 * yy], axis=2)
    sd = 0.02 + 0.1 * rng.random((h, w, 3))
    buf = Buffer(w, h)
    buf.N = rng.integers(1, 6, (h, w)).astype(np.int32)
    n = buf.N.astype(np.float64)[..., None]
    buf.M = base + sd * rng.standard_normal((h, w, 3)) / np.sqrt(n)
    buf.V = sd * sd * (n - 1.0) * (0.5 + rng.random((h, w, 3)))
    return buf


def bench_shape(w, h, reps, warmup, with_numpy):
    buf = seeded_buffer(w, h)
    r = Renderer.NewRenderer(None, None, None, w, h, True, device=0)
    try:
        r.LoadBuffer(buf, passes_done=0)
        r.DenoiseParams = _abi.pt_denoise_params(ITERATIONS, 0, SIGMA)
        for _ in range(max(warmup, 1)):
            r.DenoiseBuffer()
            r.Denoised()
        kernel, call = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            ms = r.DenoiseBuffer()
            r.Denoised()
            call.append((time.perf_counter() - t0) * 1e3)
            kernel.append(ms)
        colour = r.DenoisedColour()
    finally:
        r.close()
    P = w * h
    k = statistics.median(kernel)
    nbytes = 96 * P * ITERATIONS
    out = {"width": w, "height": h, "iterations": ITERATIONS, "sigma_colour": SIGMA, "reps": reps, "warmup": warmup,
           "kernel_ms": summary(kernel), "call_ms": summary(call), "compulsory_bytes": nbytes,
           "kernel_gbs": round(nbytes / (k * 1e-3) / 1e9, 1), "hbm_share": round(nbytes / (k * 1e-3) / HBM_PEAK, 4),
           "exp_per_s": round(25 * P * ITERATIONS / (k * 1e-3), 0)}
    if with_numpy:
        import denoise_ref
        t0 = time.perf_counter()
        want, _ = denoise_ref.denoise(buf.M, buf.V, buf.N, ITERATIONS, SIGMA)
        out["numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out["max_abs_diff_vs_numpy"] = float(np.abs(colour - want).max())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1920x1080,3840x2160")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_bench.json"))
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    doc = {"tool": "tools/denoise_bench.py", "hbm_peak_bytes_per_s": HBM_PEAK, "shapes": []}
    for w, h in shapes:
        s = bench_shape(w, h, a.reps, a.warmup, with_numpy=(w, h) == (1920, 1080))
        doc["shapes"].append(s)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(f"{w}x{h}: kernel {s['kernel_ms']['median']} ms, call with 8-bit read-back {s['call_ms']['median']} ms, "
              f"{s['kernel_gbs']} GB/s compulsory ({s['hbm_share']:.2%} of HBM peak), {s['exp_per_s']:.3g} exp/s"
              + (f", numpy {s['numpy_ms']} ms" if "numpy_ms" in s else ""), flush=True)


if __name__ == "__main__":
    main()
