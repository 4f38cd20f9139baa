#!/usr/bin/env python3
"""Motion vectors and temporal accumulation on one GPU in one process, on the bench's 1M-triangle 1920x1080 frame
(scenes.bunny_frame, bench.py's c4 workload): medians of `--reps` calls after `--warmup` untimed ones, with min and max.

  snapshot      MotionSnapshot(): the host's wall time of the synchronous call (pt_motion_snapshot returns no device
                time of its own: it is a scatter kernel and three device-to-device copies, then a synchronisation)
  motion /      RenderMotion() and RenderFeatures() alternating in the same session: each call's out_kernel_ms (device
  features      time between two hipEvents around the kernel), and the ratio of the medians
  accumulate    AccumulateTemporal() after a fresh RenderMotion(): out_kernel_ms of k_temporal_merge
  denoise       DenoiseTemporal() and DenoiseBuffer() alternating: out_kernel_ms of each

Bytes moved, counted from the layout: the merge reads the Buffer pixel (52 B), six motion values (32 B: shape, prim,
status, prev_pixel, depth, prev_depth) and one history pixel (68 B: M, V, depth, N, shape, prim) and writes one history
pixel and the status (72 B); the snapshot reads a 48-B record and a 4-B source index per BVH position and writes 48 B.
Over the kernel time (--kernel-stats: the CSV of a `rocprofv3 --kernel-trace --stats` run of this tool, a run of its
own; without it the event time of the call stands in for the merge, and the snapshot's share is not given) they are
reported as a share of the 8.0 TB/s HBM3E peak.  One JSON document goes to --out.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from denoise_bench import summary  # noqa: E402
from ptsharp_amd import Renderer, scenes  # noqa: E402

HBM_PEAK = 8.0e12   # bytes per second
MERGE_BYTES_PER_PIXEL = 52 + 32 + 68 + 72
SNAPSHOT_BYTES_PER_POSITION = 48 + 4 + 48


def kernel_stats(path):
    """{kernel name prefix: average ns} from rocprofv3's kernel stats CSV."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for key in ("k_temporal_merge", "k_motion_snapshot_tris", "k_motion<", "k_features<"):
                if key in name:
                    out[key.rstrip("<")] = {"calls": int(row["Calls"]), "average_ns": float(row["AverageNs"]),
                                            "min_ns": float(row["MinNs"]), "max_ns": float(row["MaxNs"])}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_bench.json"))
    a = ap.parse_args()
    w, h = a.width, a.height
    scene, camera, sampler = scenes.bunny_frame(a.tris)
    r = Renderer.NewRenderer(scene, camera, sampler, w, h, True, device=0)
    r.SamplesPerPixel, r.Seed = 1, 1234
    doc = {"tool": "tools/temporal_bench.py", "scene": f"bunny_frame({a.tris})", "width": w, "height": h, "reps": a.reps,
           "warmup": a.warmup, "hbm_peak_bytes_per_s": HBM_PEAK}
    try:
        r.RenderPasses(2)
        positions = len(r._uploaded.tri_material)
        snap, motion, feats, merge, dt, dp = [], [], [], [], [], []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            r.MotionSnapshot()
            t_snap = (time.perf_counter() - t0) * 1e3
            t_motion = r.RenderMotion()
            t_feat = r.RenderFeatures()
            t_merge = r.AccumulateTemporal()
            t_dt = r.DenoiseTemporal()
            t_dp = r.DenoiseBuffer()
            if i >= a.warmup:
                for xs, x in ((snap, t_snap), (motion, t_motion), (feats, t_feat), (merge, t_merge), (dt, t_dt), (dp, t_dp)):
                    xs.append(x)
        _, status = r.Temporal()
    finally:
        r.close()
    pixels = w * h
    doc.update({
        "snapshot_wall_ms": summary(snap), "snapshot_positions": positions,
        "motion_kernel_ms": summary(motion), "features_kernel_ms": summary(feats),
        "motion_over_features": round(statistics.median(motion) / statistics.median(feats), 4),
        "accumulate_kernel_ms": summary(merge), "merged_share": round(float((status == 0).mean()), 4),
        "denoise_temporal_kernel_ms": summary(dt), "denoise_kernel_ms": summary(dp),
        "merge_bytes": pixels * MERGE_BYTES_PER_PIXEL, "snapshot_bytes": positions * SNAPSHOT_BYTES_PER_POSITION,
    })
    merge_s = statistics.median(merge) * 1e-3
    doc["merge_time_source"] = "hipEvents around the launch"
    if a.kernel_stats:
        ks = kernel_stats(a.kernel_stats)
        doc["kernel_trace"] = ks
        if "k_temporal_merge" in ks:
            merge_s = ks["k_temporal_merge"]["average_ns"] * 1e-9
            doc["merge_time_source"] = "rocprofv3 kernel trace, average"
        if "k_motion_snapshot_tris" in ks:
            s = ks["k_motion_snapshot_tris"]["average_ns"] * 1e-9
            doc["snapshot_bytes_per_s"] = round(doc["snapshot_bytes"] / s, 0)
            doc["snapshot_share_of_hbm_peak"] = round(doc["snapshot_bytes"] / s / HBM_PEAK, 4)
    doc["merge_bytes_per_s"] = round(doc["merge_bytes"] / merge_s, 0)
    doc["merge_share_of_hbm_peak"] = round(doc["merge_bytes"] / merge_s / HBM_PEAK, 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
