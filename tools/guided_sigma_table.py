#!/usr/bin/env python3
"""The table pt_denoise_guided's default guide sigmas were chosen from: on the CPU, with
the numpy restatement (tests/denoise_guided_ref.py) and the committed oracle renders and features
(tests/golden/features_<scene>.npz, tools/make_features_golden.py), the tone-mapped RMSE of the guided
result over the unguided one, per scene, for a grid of (sigma_normal, sigma_albedo, sigma_depth).
5 iterations and sigma_colour 4.0 throughout, as pt_denoise's defaults.

Usage: python tools/guided_sigma_table.py [--normal 0.3,0.5] [--albedo 0.05,0.1] [--depth 0.1,0.2]
"""
from __future__ import annotations

import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import denoise_guided_ref as G  # noqa: E402
import denoise_ref as D  # noqa: E402

SCENES = ["simplesphere", "example1", "example3", "textured"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--normal", default="0,0.1,0.3,1.0")
    ap.add_argument("--albedo", default="0,0.03,0.1,0.3")
    ap.add_argument("--depth", default="0,0.03,0.1,0.3")
    a = ap.parse_args()
    grid = [[float(v) for v in s.split(",")] for s in (a.normal, a.albedo, a.depth)]
    data, plain = {}, {}
    for name in SCENES:
        z = np.load(os.path.join(ROOT, "tests", "golden", f"features_{name}.npz"))
        data[name] = {k: z[k] for k in z.files}
        q = data[name]
        c, _ = D.denoise(q["noisy_M"], q["noisy_V"], q["noisy_N"])
        plain[name] = D.tonemapped_rmse(c, q["truth"])
    print("sigma_normal sigma_albedo sigma_depth | " + " ".join(f"{n:>12}" for n in SCENES) + " |  worst")
    for sn, sa, sd in itertools.product(*grid):
        ratios = []
        for name in SCENES:
            q = data[name]
            c, _ = G.denoise_guided(q["noisy_M"], q["noisy_V"], q["noisy_N"], q["albedo"], q["normal"], q["depth"], q["kind"],
                                    iterations=5, sigma_colour=4.0, sigma_normal=sn, sigma_albedo=sa, sigma_depth=sd)
            ratios.append(D.tonemapped_rmse(c, q["truth"]) / plain[name])
        print(f"{sn:12g} {sa:12g} {sd:11g} | " + " ".join(f"{r:12.3f}" for r in ratios) + f" | {max(ratios):6.3f}", flush=True)


if __name__ == "__main__":
    main()
