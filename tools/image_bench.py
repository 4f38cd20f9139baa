#!/usr/bin/env python3
"""Per-pass image step, host path against device path, on one GPU in one process.

For 1920x1080 and 3840x2160 a seeded Buffer is loaded (LoadBuffer) and two ways to the pass' image
are timed, alternating, `--reps` times after a warm-up of each:

  (a) host:   pt_read_buffer (52 B per pixel) + Buffer.Image(ColorChannel) in numpy, the path
              IterativeRender takes by default;
  (b) device: pt_read_image for every channel and format.  `call_ms` is a host clock around the call
              (it ends in a stream synchronise), `kernel_ms` the device time between two hipEvents
              around its launches (pt_stats.kernel_ms[PT_K_IMAGE]), `copy_ms` their difference: the
              device-to-host copy plus the launch and synchronise overhead.

Each figure is the median over the repetitions with the minimum and maximum.  `bytes` is what the
resolve kernel must move, computed from the shape (Color, Albedo, Normal: 24 B per pixel read;
Variance, StdDev: 28 B; Samples: 4 B twice; plus the 3 or 4 output bytes), and `hbm_share` that
over kernel time as a share of the 8 TB/s HBM peak.  One JSON document goes to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ptsharp_amd import Renderer, _abi  # noqa: E402
from ptsharp_amd.renderer import Buffer, Channel  # noqa: E402

HBM_PEAK = 8e12
READ_BYTES = {Channel.ColorChannel: 24, Channel.VarianceChannel: 28, Channel.StandardDeviationChannel: 28,
              Channel.SamplesChannel: 8, Channel.AlbedoChannel: 24, Channel.NormalChannel: 24}


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def host_path(r):
    t0 = time.perf_counter()
    b = r.ReadBuffer()
    t1 = time.perf_counter()
    with np.errstate(invalid="ignore"):
        img = b.Image(Channel.ColorChannel)
    t2 = time.perf_counter()
    return img, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def device_path(r, ch, rgba):
    t0 = time.perf_counter()
    img = r.Image(ch, rgba=rgba)
    call = (time.perf_counter() - t0) * 1e3
    return img, call, float(r.Stats().kernel_ms[_abi.K_IMAGE])


def bench_shape(w, h, reps, warmup):
    rng = np.random.default_rng(2024)
    buf = Buffer(w, h)
    buf.M = rng.random((h, w, 3)) * 1.5
    buf.V = rng.random((h, w, 3)) * 3
    buf.N = rng.integers(0, 6, (h, w)).astype(np.int32)
    r = Renderer.NewRenderer(None, None, None, w, h, True, device=0)
    try:
        r.LoadBuffer(buf, passes_done=0)
        legs = [(ch, rgba) for ch in Channel for rgba in (False, True)]
        differing = None
        for _ in range(max(warmup, 1)):
            host_img, _, _ = host_path(r)
            for ch, rgba in legs:
                dev_img, _, _ = device_path(r, ch, rgba)
                if ch == Channel.ColorChannel and not rgba:
                    differing = int((dev_img != host_img).sum())
        read_ms, image_ms = [], []
        dev = {leg: ([], []) for leg in legs}
        for _ in range(reps):
            _, a, b = host_path(r)
            read_ms.append(a)
            image_ms.append(b)
            for leg in legs:
                _, call, kern = device_path(r, *leg)
                dev[leg][0].append(call)
                dev[leg][1].append(kern)
    finally:
        r.close()
    P = w * h
    host_total = [a + b for a, b in zip(read_ms, image_ms)]
    out = {"width": w, "height": h, "reps": reps, "warmup": warmup,
           "color_bytes_differing_device_vs_host": differing,
           "host": {"read_buffer_ms": summary(read_ms), "buffer_image_ms": summary(image_ms), "total_ms": summary(host_total),
                    "bytes_copied": 52 * P},
           "device": []}
    for (ch, rgba), (call, kern) in dev.items():
        bpp = 4 if rgba else 3
        nbytes = (READ_BYTES[ch] + bpp) * P
        k = statistics.median(kern)
        out["device"].append({"channel": ch.name, "format": "RGBA8" if rgba else "RGB8", "call_ms": summary(call),
                              "kernel_ms": summary(kern), "copy_ms": summary([c - g for c, g in zip(call, kern)]),
                              "bytes_copied": bpp * P, "kernel_bytes": nbytes,
                              "kernel_gbs": round(nbytes / (k * 1e-3) / 1e9, 1),
                              "hbm_share": round(nbytes / (k * 1e-3) / HBM_PEAK, 4),
                              "speedup_vs_host": round(statistics.median(host_total) / statistics.median(call), 1)})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1920x1080,3840x2160")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "image_bench.json"))
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    doc = {"tool": "tools/image_bench.py", "hbm_peak_bytes_per_s": HBM_PEAK, "shapes": []}
    for w, h in shapes:
        s = bench_shape(w, h, a.reps, a.warmup)
        doc["shapes"].append(s)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        d = next(x for x in s["device"] if x["channel"] == "ColorChannel" and x["format"] == "RGB8")
        print(f"{s['width']}x{s['height']}: host {s['host']['total_ms']['median']} ms "
              f"(read {s['host']['read_buffer_ms']['median']}, image {s['host']['buffer_image_ms']['median']}); "
              f"device Color RGB8 {d['call_ms']['median']} ms (kernel {d['kernel_ms']['median']}, "
              f"copy {d['copy_ms']['median']}), {d['speedup_vs_host']}x", flush=True)


if __name__ == "__main__":
    main()
