#!/usr/bin/env python3
"""Generate tests/golden/features_<scene>.npz from the CPU oracle: the inputs of the guided
denoiser's quality table (tests/test_features_host.py).

Per scene (simplesphere, example1, example3, textured), at 96x64:
  noisy_M, noisy_V, noisy_N   four passes of 1 spp, seed 0
  truth                       M of one 256-spp pass, seed 7
  albedo, normal, depth, kind, material   tests/features_ref.py's first-hit features
The 256-spp renders take minutes on a CPU, so they are committed once; the file of a scene is a few
hundred KiB.

Usage: python tools/make_features_golden.py [scene ...]
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import features_ref  # noqa: E402
import oracle_lib as O  # noqa: E402
from ptsharp_amd import scenes  # noqa: E402

SCENES = ["simplesphere", "example1", "example3", "textured"]
W, H = 96, 64


def main():
    for name in sys.argv[1:] or SCENES:
        t0 = time.perf_counter()
        scene, camera, sampler = getattr(scenes, name)()
        os_ = O.OracleScene(scene)
        noisy, _ = O.render(os_, camera, sampler, W, H, spp=1, passes=4, seed=0)
        truth, _ = O.render(os_, camera, sampler, W, H, spp=256, passes=1, seed=7)
        albedo, normal, depth, kind, material = features_ref.features(scene, camera, W, H, oscene=os_)
        out = os.path.join(ROOT, "tests", "golden", f"features_{name}.npz")
        np.savez_compressed(out, noisy_M=noisy.M, noisy_V=noisy.V, noisy_N=noisy.N, truth=truth.M, albedo=albedo,
                            normal=normal, depth=depth, kind=kind, material=material)
        print(f"wrote {out} ({os.path.getsize(out)} bytes, {time.perf_counter() - t0:.1f} s)", flush=True)


if __name__ == "__main__":
    main()
