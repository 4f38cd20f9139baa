"""Helpers of tests/test_gpu_volumes.py (pt_update_volumes): the scenes, the edits, the rays and the comparisons.

Scenes (the smallest that reach each layout):
  top     scenes.volume(24, 24, 12): Example.volume's Volume, top-level, staged in LDS;
  odd     a 17x9x5 grid, top-level: no dimension a multiple of anything, 18*10*6 = 1,080 cells, more than one block of 256
          and a last block that is not full;
  two     a 24x24x12 Volume and, through a TransformedShape, a 17x9x5 one: the second volume's tables start at
          25*25*13 = 8,125 cells, an odd offset, so its sign bytes are not 4-aligned; two volumes are not staged in LDS;
  mixed   scenes.mixed(3000): the C5-kind scene at test size, its 32x32x16 Volume inside a TransformedShape, staged in
          LDS, behind a triangle mesh and an SDF shape, with routing.
The edits are seeded and deterministic; rays are aimed at the Volume as tests/test_gpu_volume_march.py aims them.
"""
from __future__ import annotations

import numpy as np

import oracle_lib as O
from ptsharp_amd import Renderer, TransformedShape, Vector, _abi, scenes
from ptsharp_amd.geometry import Box, Matrix
from ptsharp_amd.renderer import Buffer
from ptsharp_amd.scene import Scene, Volume, VolumeWindow
from test_gpu_volume_march import oracle_hits, volume_rays, world_box  # noqa: F401  (the aiming the issue names)

F = np.float32
W, H, SPP = 96, 64, 2


def _example_windows(like: Volume):
    return [VolumeWindow(w.Lo, w.Hi, w.VolumeWindowMaterial) for w in like.Windows]


def odd_volume(seed=9) -> Volume:
    proto = scenes.volume(4, 4, 2)[0].Shapes[0]
    box = Box(Vector(-1, -1, F(-0.2)), Vector(1, 1, 1))
    return Volume.NewVolume(box, scenes.volume_slices(17, 9, 5, seed), F(3.4) / F(0.9765625), _example_windows(proto))


def scene_top():
    return scenes.volume(24, 24, 12, seed=3)


def scene_odd():
    _, cam, smp = scenes.volume(24, 24, 12, seed=3)
    s = Scene()
    s.Color = scenes.volume(4, 4, 2)[0].Color
    s.Add(odd_volume())
    return s, cam, smp


def scene_two():
    a, cam, smp = scenes.volume(24, 24, 12, seed=3)
    s = Scene()
    s.Color = a.Color
    s.Add(a.Shapes[0])
    s.Add(TransformedShape.NewTransformedShape(odd_volume(), Matrix.TranslateM(Vector(0.3, 0.2, 0.5)).Mul(
        Matrix.ScaleM(Vector(0.9, 0.9, 0.9)))))
    return s, cam, smp


def scene_mixed():
    s, cam, smp = scenes.mixed(3000, seed=5)
    smp.MaxBounces = 3
    return s, cam, smp


SCENES = {"top": scene_top, "odd": scene_odd, "two": scene_two, "mixed": scene_mixed}


def volumes_of(scene):
    """The Volume objects in the order of the compiled scene's volumes (scene: a Scene, or a builder's tuple)."""
    scene = scene[0] if isinstance(scene, tuple) else scene
    return list(scene.Compile().volume_objects)


def new_data(vol: Volume, seed: int) -> np.ndarray:
    """Another seeded grid of the volume's dimensions, in its own layout, values in [0, 1] as NewVolume's."""
    sl = np.stack([np.asarray(im)[..., 0] if np.asarray(im).ndim == 3 else np.asarray(im)
                   for im in scenes.volume_slices(vol.W, vol.H, vol.D, seed)])
    sl = np.roll(sl, 2 + seed % 3, axis=2)   # the blob moves along x as well: most hits change
    return np.ascontiguousarray(sl.astype(np.float64).reshape(-1) / 255)


def new_windows(vol: Volume, shift: float, widen: float = 0.0):
    """The volume's windows dragged by `shift`, each widened by `widen`: (lo, hi) pairs."""
    return [(w.Lo + shift, w.Hi + shift + widen) for w in vol.Windows]


def edit(scene, kind: str, step: int = 0) -> dict:
    """The `updates` of Renderer.UpdateVolumes for a named edit of the scene as it stands."""
    vols = volumes_of(scene)
    if kind == "data":
        return {i: (new_data(v, 100 + 10 * step + i), None) for i, v in enumerate(vols)}
    if kind == "windows":
        return {i: (None, new_windows(v, 0.03 + 0.01 * step, 0.005)) for i, v in enumerate(vols)}
    if kind == "both":
        return {i: (new_data(v, 200 + 10 * step + i), new_windows(v, -0.02, 0.01)) for i, v in enumerate(vols)}
    if kind == "second":   # one volume of two, addressed by its object
        return {vols[-1]: (new_data(vols[-1], 300 + step), new_windows(vols[-1], 0.05))}
    if kind == "identity":
        return {i: (v.Data.copy(), [(w.Lo, w.Hi) for w in v.Windows]) for i, v in enumerate(vols)}
    raise KeyError(kind)


def renderer(st, engine=_abi.ENGINE_WAVEFRONT, seed=23, w=W, h=H):
    s, c, smp = st
    r = Renderer.NewRenderer(s, c, smp, w, h, True, device=0)
    r.SamplesPerPixel, r.Seed, r.Engine = SPP, seed, engine
    return r


def frame(r, reset=True):
    if reset:
        r.ResetBuffer()
    r.RenderParallel()
    b = r.ReadBuffer()
    out = Buffer(r.W, r.H)
    out.M, out.V, out.N = b.M.copy(), b.V.copy(), b.N.copy()
    return out, r.Stats().rays


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def read_all(r):
    """pt_read_volume of every volume of the uploaded scene."""
    r._ensure_scene()
    return [r.ReadVolume(i) for i in range(r._uploaded.counts_ext[2])]


def same_volume_words(a, b, what=""):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        for key in ("info", "data", "windows", "materials", "runs", "cells"):
            p, q = x[key], y[key]
            assert (p is None) == (q is None), f"{what} volume {i} {key}: one has cells, the other none"
            if p is None:
                continue
            assert p.shape == q.shape, f"{what} volume {i} {key}: shape {p.shape} vs {q.shape}"
            bad = np.argwhere(bits(p) != bits(q))
            assert not bad.size, (f"{what} volume {i} {key}: {len(bad)} words differ, first at {bad[0]}: "
                                  f"{p[tuple(bad[0])]} vs {q[tuple(bad[0])]}")


def volume_target(scene):
    """The world box rays are aimed at: the union of the scene's Volumes' boxes."""
    boxes = [world_box(s) for s in scene.Shapes
             if isinstance(s, Volume) or (isinstance(s, TransformedShape) and isinstance(s.Shape, Volume))]
    return np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0)


def is_volume_kind(k):
    return (k == _abi.SHAPE_VOLUME) | (k == _abi.SHAPE_TRANSFORMED)


def oracle_rays(scene, o, d):
    return oracle_hits(O.OracleScene(scene), o, d)
