"""Host-side mirror of PTSharp's Renderer and Buffer (PTSharpCore/Renderer.cs,
Buffer.cs) driving the MI355X path through libptsharp_hip.so.

`Renderer.NewRenderer(scene, camera, sampler, w, h, multithreaded)` keeps the
reference's factory and knobs (SamplesPerPixel, StratifiedSampling, ...);
`RenderParallel()` is one GPU pass; `IterativeRender(pathTemplate, iter)` runs
`iter` passes and writes a PNG after each, as Renderer.cs:702-765 does; with
`Denoise` set it also writes the Albedo and Normal channels and the denoised
image after each pass (Renderer.cs:731-761), the denoiser being the library's
own variance-guided à-trous filter (pt_denoise), not OIDN; with `DenoiseGuided` too the filter
is guided by the first-hit albedo, normal and depth of one primary ray per pixel
(pt_render_features, pt_denoise_guided).  The Welford state stays in HBM between passes; `Renderer.PBuffer` is refreshed
from it on demand.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import struct
import time
import zlib
from enum import IntEnum

import numpy as np

from . import _abi
from .geometry import Colour
from .scene import Camera, DefaultSampler, Scene

TILE = 32


class Channel(IntEnum):  # Buffer.cs:8-16
    ColorChannel = 0
    VarianceChannel = 1
    StandardDeviationChannel = 2
    SamplesChannel = 3
    AlbedoChannel = 4
    NormalChannel = 5


def tiles_for_rank(width: int, height: int, rank: int, world: int) -> np.ndarray:
    """Static interleaved 32x32 tile ownership: tile t belongs to rank t % world."""
    n = ((width + TILE - 1) // TILE) * ((height + TILE - 1) // TILE)
    return np.arange(rank, n, world, dtype=np.int32)


class Buffer:
    """PTSharpCore.Buffer: per-pixel Welford {Samples, M, V} (Buffer.cs:18-97), held as
    arrays M,V [H,W,3] float64 and N [H,W] int32 (row-major, like pt_read_buffer)."""

    def __init__(self, w: int, h: int):
        self.W, self.H = w, h
        self.M = np.zeros((h, w, 3), np.float64)
        self.V = np.zeros((h, w, 3), np.float64)
        self.N = np.zeros((h, w), np.int32)

    def Samples(self, x, y) -> int:
        return int(self.N[y, x])

    def Color(self, x, y) -> Colour:
        return Colour(*self.M[y, x])

    def Variance(self, x, y) -> Colour:
        n = self.N[y, x]
        if n < 2:
            return Colour(0, 0, 0)
        return Colour(*(self.V[y, x] / (n - 1)))

    def StandardDeviation(self, x, y) -> Colour:
        return self.Variance(x, y).Pow(float(np.float32(0.5)))

    def Image(self, channel: Channel = Channel.ColorChannel) -> np.ndarray:
        """Buffer.Image (Buffer.cs:134-202) as an [H,W,3] uint8 array."""
        if channel == Channel.ColorChannel:
            with np.errstate(invalid="ignore"):
                c = np.power(self.M, 1.0 / 2.2)
        elif channel == Channel.VarianceChannel:
            n = self.N[..., None].astype(np.float64)
            c = np.where(n >= 2, self.V / np.maximum(n - 1, 1), 0.0)
        elif channel == Channel.StandardDeviationChannel:
            n = self.N[..., None].astype(np.float64)
            c = np.power(np.where(n >= 2, self.V / np.maximum(n - 1, 1), 0.0), float(np.float32(0.5)))
        elif channel == Channel.SamplesChannel:
            mx = max(int(self.N.max()), 1)
            c = np.repeat((self.N / mx)[..., None], 3, axis=2)
        elif channel == Channel.AlbedoChannel:  # CalculateAlbedo (Buffer.cs:240-282)
            mx = self.M.max(axis=2, keepdims=True)  # NaN where a component is NaN
            with np.errstate(invalid="ignore", divide="ignore"):
                c = self.M / mx
                c = np.where(c < 0, 0.0, np.where(c > 1, 1.0, c))  # Math.Clamp keeps a NaN (inf / inf)
            c = np.where(np.isnan(mx) | (mx == 0), 0.0, c)
        elif channel == Channel.NormalChannel:  # GetNormalAt + CalculateNormal (Buffer.cs:99-124,222-233)
            p = np.zeros((self.H + 2, self.W + 2, 2), np.float64)  # GetPixelOrDefault: 0 outside the image
            p[1:-1, 1:-1] = self.M[..., :2]
            top, mid, bot = p[:-2], p[1:-1], p[2:]
            L, X, R = slice(0, -2), slice(1, -1), slice(2, None)
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                nx = (top[:, L, 0] + 2 * mid[:, L, 0] + bot[:, L, 0] - top[:, R, 0] - 2 * mid[:, R, 0] - bot[:, R, 0]) / 8.0
                ny = (top[:, L, 1] + 2 * top[:, X, 1] + top[:, R, 1] - bot[:, L, 1] - 2 * bot[:, X, 1] - bot[:, R, 1]) / 8.0
                length = np.sqrt(nx * nx + ny * ny + 1.0)
                # new Vector(nx, ny, nz) holds floats (Vector.cs:222-225)
                v = np.stack([nx / length, ny / length, 1.0 / length], axis=2).astype(np.float32).astype(np.float64)
                c = np.stack([(v[..., 0] + 1.0) * 0.5, (v[..., 1] + 1.0) * 0.5, v[..., 2]], axis=2)
        else:
            raise ValueError(f"channel {channel} is not a Buffer channel")
        with np.errstate(invalid="ignore"):
            v = np.clip(c * 255, 0, 255)
        v = np.nan_to_num(v, nan=0.0)
        return v.astype(np.uint8)  # (byte) truncates toward zero


def write_png(path: str, rgb: np.ndarray) -> None:
    """Minimal PNG (8-bit RGB) writer — stands in for SkiaSharp's encoder (Renderer.cs:723-729)."""
    h, w, _ = rgb.shape
    raw = b"".join(b"\x00" + rgb[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


class Renderer:
    """PTSharpCore.Renderer on the MI355X path."""

    PBuffer: Buffer = None  # static, as Renderer.PBuffer (Renderer.cs:20)

    def __init__(self):
        self.Scene: Scene = None
        self.Camera: Camera = None
        self.Sampler: DefaultSampler = None
        self.SamplesPerPixel = 2
        self.StratifiedSampling = False
        self.AdaptiveSamples = 0
        self.FireflySamples = 0
        self.Denoise = False     # IterativeRender: the denoise step of Renderer.cs:731-761, by pt_denoise
        self.DenoiseParams = _abi.pt_denoise_params(5, 0, 4.0)   # iterations (1..8), reserved, sigma_colour
        self.DenoiseGuided = False   # with Denoise: RenderFeatures() once, then pt_denoise_guided instead of pt_denoise
        # iterations (1..8), reserved, sigma_colour, sigma_normal, sigma_albedo, sigma_depth (0 = term off)
        self.DenoiseGuidedParams = _abi.pt_denoise_guided_params(5, 0, 4.0, 0.3, 0.3, 0.1)
        # AccumulateTemporal: max_history (0..2^20), reserved, sigma_depth (0 = depth test off); design defaults, not tuned
        self.TemporalParams = _abi.pt_temporal_params(32, 0, 0.1)
        self.NumCPU = 1
        # MI355X extensions (no reference counterpart)
        self.Seed = 0            # Random.Shared is unseedable; this keys the counter-based stream
        self.Device = 0
        self.Tiles = None        # optional 32x32 tile ids this context renders (multi-GPU sharding)
        self.Engine = _abi.ENGINE_AUTO  # scheduling only: both engines compute identical per-ray arithmetic
        self.Flags = 0                  # _abi.PASS_KERNEL_TIMING: per-kernel hipEvent timing in Stats()
        self.DeviceImages = False       # IterativeRender: each pass' image from Image() (pt_read_image), PBuffer once at the end
        self.Verbose = False
        self._ctx = None
        self._lib = None
        self._uploaded = None
        self._rest_of = None         # the FlatScene whose rest pose the device holds (SetRestPose)
        self._morph_of = None        # (the FlatScene whose morph the device holds, whether it carries normal deltas) (SetMorph)
        self._mirror_stale = False   # PoseMeshes(mirror=False) left the uploaded FlatScene's triangle arrays behind
        self._pass = 0
        self.iterations = 0

    @staticmethod
    def NewRenderer(scene: Scene, camera: Camera, sampler: DefaultSampler, w: int, h: int, multithreaded: bool = True,
                    device: int = 0) -> "Renderer":
        r = Renderer()
        r.Scene, r.Camera, r.Sampler = scene, camera, sampler
        r.W, r.H = int(w), int(h)
        r.NumCPU = os.cpu_count() if multithreaded else 1
        r.Device = device
        Renderer.PBuffer = Buffer(r.W, r.H)
        r._lib = _abi.load_library()
        ctx = C.c_void_p()
        opts = _abi.pt_device_opts(device, r.W, r.H)
        _abi.check(r._lib.pt_create(C.byref(opts), C.byref(ctx)), "pt_create")
        r._ctx = ctx
        return r

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._lib is not None:
            self._lib.pt_destroy(self._ctx)
            self._ctx = None

    # ------------------------------------------------------------- passes
    def _ensure_scene(self):
        flat = self.Scene.Compile()  # Scene.Compile (Renderer.cs:208)
        if self._uploaded is not flat:
            _abi.check(self._lib.pt_upload_scene(self._ctx, C.byref(flat.desc)), "pt_upload_scene")
            self._uploaded = flat
            self._rest_of = None
            self._morph_of = None
            self._mirror_stale = False

    def _pass_params(self, spp=None, pass_index=None):
        tiles = self.Tiles
        if tiles is not None:
            tiles = np.ascontiguousarray(tiles, dtype=np.int32)
            self._tiles_keep = tiles
        pp = _abi.pt_pass_params(int(spp or self.SamplesPerPixel), int(bool(self.StratifiedSampling)),
                                 C.c_uint64(self.Seed & 0xFFFFFFFFFFFFFFFF).value,
                                 int(self._pass if pass_index is None else pass_index),
                                 0 if tiles is None else len(tiles),
                                 C.POINTER(C.c_int32)() if tiles is None else tiles.ctypes.data_as(C.POINTER(C.c_int32)),
                                 int(self.Engine), int(self.Flags), int(self.AdaptiveSamples),
                                 int(self.FireflySamples), 1)
        return pp

    def RenderParallel(self) -> None:
        """One pass of Renderer.RenderParallel (Renderer.cs:199-338) on the GPU."""
        self._ensure_scene()
        self._pass += 1
        cam, smp = self.Camera.to_c(), self.Sampler.to_c()
        pp = self._pass_params()
        t0 = time.perf_counter()
        _abi.check(self._lib.pt_render_pass(self._ctx, C.byref(cam), C.byref(smp), C.byref(pp)), "pt_render_pass")
        if self.Verbose:
            print(f"{self.W} x {self.H}, {self.SamplesPerPixel} spp, MI355X device {self.Device}")
            print("time elapsed:", time.perf_counter() - t0)

    def RenderPasses(self, k: int) -> None:
        """k consecutive RenderParallel passes in one call (pt_pass_params.passes): the Buffer is the
        one k RenderParallel() calls leave, bit for bit; plain passes run as one batch on the GPU."""
        k = int(k)
        if k < 1:
            raise ValueError("k must be >= 1")
        self._ensure_scene()
        cam, smp = self.Camera.to_c(), self.Sampler.to_c()
        pp = self._pass_params(pass_index=self._pass + 1)
        pp.passes = k
        _abi.check(self._lib.pt_render_pass(self._ctx, C.byref(cam), C.byref(smp), C.byref(pp)), "pt_render_pass")
        self._pass += k

    def Render(self) -> None:
        """One pass of Renderer.Render (Renderer.cs:80-198), the NumCPU == 1 twin: the same main
        samples, then per pixel AdaptiveSamples individual samples when its standard deviation
        reaches 1 and FireflySamples when it then exceeds 1 (PT_PASS_SERIAL)."""
        flags = self.Flags
        self.Flags = flags | _abi.PASS_SERIAL
        try:
            self.RenderParallel()
        finally:
            self.Flags = flags

    def RenderCounted(self) -> _abi.pt_trace_counters:
        """One pass with traversal counters (bench roofline accounting)."""
        self._ensure_scene()
        self._pass += 1
        cam, smp = self.Camera.to_c(), self.Sampler.to_c()
        pp = self._pass_params()
        out = _abi.pt_trace_counters()
        _abi.check(self._lib.pt_render_pass_counted(self._ctx, C.byref(cam), C.byref(smp), C.byref(pp), C.byref(out)),
                   "pt_render_pass_counted")
        return out

    def Synchronize(self) -> None:
        _abi.check(self._lib.pt_synchronize(self._ctx), "pt_synchronize")

    def ReadBuffer(self) -> Buffer:
        """Copy the HBM Welford state into Renderer.PBuffer."""
        b = Renderer.PBuffer
        if b is None or b.W != self.W or b.H != self.H:
            b = Renderer.PBuffer = Buffer(self.W, self.H)
        _abi.check(self._lib.pt_read_buffer(self._ctx, b.M.ctypes.data_as(C.POINTER(C.c_double)),
                                            b.V.ctypes.data_as(C.POINTER(C.c_double)),
                                            b.N.ctypes.data_as(C.POINTER(C.c_int32))), "pt_read_buffer")
        return b

    def Image(self, channel: Channel = Channel.ColorChannel, rgba: bool = False) -> np.ndarray:
        """Buffer.Image(channel) resolved on the device (pt_read_image): [H,W,3] uint8, or [H,W,4] with
        A = 255.  The same bytes as ReadBuffer().Image(channel) for a seventeenth of the copy."""
        out = np.empty((self.H, self.W, 4 if rgba else 3), np.uint8)
        _abi.check(self._lib.pt_read_image(self._ctx, int(channel), _abi.IMAGE_RGBA8 if rgba else _abi.IMAGE_RGB8,
                                           out.ctypes.data_as(C.POINTER(C.c_uint8))), "pt_read_image")
        return out

    def DenoiseBuffer(self, guided: bool = False) -> float:
        """Filter the Buffer as it stands into the context's denoised result (pt_denoise, DenoiseParams;
        guided: pt_denoise_guided, DenoiseGuidedParams, with the context's features); the Buffer and the
        pass state are unchanged.  Returns the device time of its kernels in ms."""
        ms = C.c_double(0.0)
        if guided:
            _abi.check(self._lib.pt_denoise_guided(self._ctx, C.byref(self.DenoiseGuidedParams), C.byref(ms)),
                       "pt_denoise_guided")
        else:
            _abi.check(self._lib.pt_denoise(self._ctx, C.byref(self.DenoiseParams), C.byref(ms)), "pt_denoise")
        return float(ms.value)

    def RenderFeatures(self) -> float:
        """The first-hit features of the whole frame (pt_render_features): one ray through each pixel's
        centre, the lens ignored.  The Buffer and the pass state are unchanged.  Returns the device time
        of the kernel in ms."""
        self._ensure_scene()
        cam = self.Camera.to_c()
        ms = C.c_double(0.0)
        _abi.check(self._lib.pt_render_features(self._ctx, C.byref(cam), C.byref(ms)), "pt_render_features")
        return float(ms.value)

    def Features(self):
        """The context's features (pt_read_features): albedo [H,W,3] float64, normal [H,W,3] float32,
        depth [H,W] float64 (1e9 on a miss), kind [H,W] int32 (the pt_shape_kind hit, or -1) and
        material [H,W] int32 (or -1)."""
        out = (np.empty((self.H, self.W, 3), np.float64), np.empty((self.H, self.W, 3), np.float32),
               np.empty((self.H, self.W), np.float64), np.empty((self.H, self.W), np.int32),
               np.empty((self.H, self.W), np.int32))
        for feature, a in enumerate(out):
            _abi.check(self._lib.pt_read_features(self._ctx, feature, a.ctypes.data_as(C.c_void_p)), "pt_read_features")
        return out

    def LoadFeatures(self, albedo, normal, depth, kind) -> None:
        """Install a host's own features (pt_write_features; layouts as Features()): a pixel is a hit
        where kind >= 0, and the material becomes -1."""
        a = np.ascontiguousarray(albedo, np.float64)
        n = np.ascontiguousarray(normal, np.float32)
        z = np.ascontiguousarray(depth, np.float64)
        k = np.ascontiguousarray(kind, np.int32)
        assert a.shape == n.shape == (self.H, self.W, 3) and z.shape == k.shape == (self.H, self.W)
        _abi.check(self._lib.pt_write_features(self._ctx, a.ctypes.data_as(C.POINTER(C.c_double)),
                                               n.ctypes.data_as(C.POINTER(C.c_float)),
                                               z.ctypes.data_as(C.POINTER(C.c_double)),
                                               k.ctypes.data_as(C.POINTER(C.c_int32))), "pt_write_features")

    def _read_denoised(self, fmt: int, out: np.ndarray) -> np.ndarray:
        _abi.check(self._lib.pt_read_denoised(self._ctx, int(fmt), out.ctypes.data_as(C.c_void_p)), "pt_read_denoised")
        return out

    def Denoised(self, rgba: bool = False) -> np.ndarray:
        """The last DenoiseBuffer()'s colour, encoded as Image(ColorChannel) encodes M: [H,W,3] uint8,
        or [H,W,4] with A = 255.  A snapshot: later passes do not change it."""
        return self._read_denoised(_abi.DENOISED_RGBA8 if rgba else _abi.DENOISED_RGB8,
                                   np.empty((self.H, self.W, 4 if rgba else 3), np.uint8))

    def DenoisedColour(self) -> np.ndarray:
        """The last DenoiseBuffer()'s linear colour, [H,W,3] float64."""
        return self._read_denoised(_abi.DENOISED_COLOUR_F64, np.empty((self.H, self.W, 3), np.float64))

    def DenoisedVariance(self) -> np.ndarray:
        """The variance of the mean the filter propagated to its output, [H,W,3] float64."""
        return self._read_denoised(_abi.DENOISED_VARIANCE_F64, np.empty((self.H, self.W, 3), np.float64))

    # ------------------------------------------------------------- motion vectors, temporal accumulation
    def MotionSnapshot(self) -> None:
        """Record the camera and the geometry as the device holds it as "the previous frame" (pt_motion_snapshot)."""
        self._ensure_scene()
        cam = self.Camera.to_c()
        _abi.check(self._lib.pt_motion_snapshot(self._ctx, C.byref(cam)), "pt_motion_snapshot")

    def RenderMotion(self) -> float:
        """One ray through each pixel's centre, the lens ignored, and where its hit point was in the snapshot's frame
        (pt_render_motion).  The Buffer and the pass state are unchanged.  Returns the device time of the kernel in ms."""
        self._ensure_scene()
        cam = self.Camera.to_c()
        ms = C.c_double(0.0)
        _abi.check(self._lib.pt_render_motion(self._ctx, C.byref(cam), C.byref(ms)), "pt_render_motion")
        return float(ms.value)

    def Motion(self) -> dict:
        """The last RenderMotion()'s arrays (pt_read_motion): shape, prim, prev_pixel, status [H,W] int32; depth,
        prev_depth [H,W] float64; prev_xy [H,W,2] float64."""
        hw = (self.H, self.W)
        out = {"shape": (_abi.MOTION_SHAPE_I32, np.empty(hw, np.int32)), "prim": (_abi.MOTION_PRIM_I32, np.empty(hw, np.int32)),
               "depth": (_abi.MOTION_DEPTH_F64, np.empty(hw, np.float64)),
               "prev_xy": (_abi.MOTION_PREV_XY_F64, np.empty(hw + (2,), np.float64)),
               "prev_depth": (_abi.MOTION_PREV_DEPTH_F64, np.empty(hw, np.float64)),
               "prev_pixel": (_abi.MOTION_PREV_PIXEL_I32, np.empty(hw, np.int32)),
               "status": (_abi.MOTION_STATUS_I32, np.empty(hw, np.int32))}
        for what, a in out.values():
            _abi.check(self._lib.pt_read_motion(self._ctx, what, a.ctypes.data_as(C.c_void_p)), "pt_read_motion")
        return {k: a for k, (_, a) in out.items()}

    def AccumulateTemporal(self) -> float:
        """Merge the history into the Buffer's statistics through the last RenderMotion() (pt_accumulate_temporal,
        TemporalParams); the Buffer is unchanged.  Returns the device time of the kernel in ms."""
        ms = C.c_double(0.0)
        _abi.check(self._lib.pt_accumulate_temporal(self._ctx, C.byref(self.TemporalParams), C.byref(ms)),
                   "pt_accumulate_temporal")
        return float(ms.value)

    def Temporal(self):
        """The last AccumulateTemporal()'s result (pt_read_temporal): a Buffer of its own and the status [H,W] int32."""
        b = Buffer(self.W, self.H)
        status = np.empty((self.H, self.W), np.int32)
        _abi.check(self._lib.pt_read_temporal(self._ctx, b.M.ctypes.data_as(C.POINTER(C.c_double)),
                                              b.V.ctypes.data_as(C.POINTER(C.c_double)),
                                              b.N.ctypes.data_as(C.POINTER(C.c_int32)),
                                              status.ctypes.data_as(C.POINTER(C.c_int32))), "pt_read_temporal")
        return b, status

    def DenoiseTemporal(self, guided: bool = False) -> float:
        """DenoiseBuffer() on the temporal result instead of the Buffer (pt_denoise_temporal); read it with Denoised()."""
        ms = C.c_double(0.0)
        plain = None if guided else C.byref(self.DenoiseParams)
        gd = C.byref(self.DenoiseGuidedParams) if guided else None
        _abi.check(self._lib.pt_denoise_temporal(self._ctx, plain, gd, C.byref(ms)), "pt_denoise_temporal")
        return float(ms.value)

    def ResetTemporal(self) -> None:
        """Drop the history and the temporal and motion results, keep the snapshot (pt_reset_temporal): after a cut, or
        after a change of materials or lights, which nothing detects."""
        _abi.check(self._lib.pt_reset_temporal(self._ctx), "pt_reset_temporal")

    def TemporalFrame(self) -> None:
        """The temporal half of one animated frame, after its passes: RenderMotion, AccumulateTemporal, MotionSnapshot."""
        self.RenderMotion()
        self.AccumulateTemporal()
        self.MotionSnapshot()

    def LoadBuffer(self, buf: Buffer, passes_done: int) -> None:
        """Resume an IterativeRender from a saved Buffer (pt_write_buffer): later passes keep adding
        Welford samples to it, numbered from passes_done + 1 (the random streams are keyed by pass)."""
        M = np.ascontiguousarray(buf.M, np.float64)
        V = np.ascontiguousarray(buf.V, np.float64)
        N = np.ascontiguousarray(buf.N, np.int32)
        _abi.check(self._lib.pt_write_buffer(self._ctx, M.ctypes.data_as(C.POINTER(C.c_double)),
                                             V.ctypes.data_as(C.POINTER(C.c_double)),
                                             N.ctypes.data_as(C.POINTER(C.c_int32))), "pt_write_buffer")
        self._pass = int(passes_done)

    def ReadTiles(self, tiles):
        """The Buffer pixels of 32x32 tiles, packed (pt_read_tiles): M, V [n, 32, 32, 3], N [n, 32, 32],
        row-major inside a tile; pixels outside the image are 0."""
        t = np.ascontiguousarray(tiles, np.int32)
        M = np.zeros((len(t), 32, 32, 3), np.float64)
        V = np.zeros((len(t), 32, 32, 3), np.float64)
        N = np.zeros((len(t), 32, 32), np.int32)
        _abi.check(self._lib.pt_read_tiles(self._ctx, t.ctypes.data_as(C.POINTER(C.c_int32)), len(t),
                                           M.ctypes.data_as(C.POINTER(C.c_double)), V.ctypes.data_as(C.POINTER(C.c_double)),
                                           N.ctypes.data_as(C.POINTER(C.c_int32))), "pt_read_tiles")
        return M, V, N

    def WriteTiles(self, tiles, M, V, N) -> None:
        """Write packed tiles (ReadTiles' layout) into the Buffer (pt_write_tiles)."""
        t = np.ascontiguousarray(tiles, np.int32)
        M = np.ascontiguousarray(M, np.float64)
        V = np.ascontiguousarray(V, np.float64)
        N = np.ascontiguousarray(N, np.int32)
        assert M.size == V.size == 3 * N.size == len(t) * 3 * 1024
        _abi.check(self._lib.pt_write_tiles(self._ctx, t.ctypes.data_as(C.POINTER(C.c_int32)), len(t),
                                            M.ctypes.data_as(C.POINTER(C.c_double)), V.ctypes.data_as(C.POINTER(C.c_double)),
                                            N.ctypes.data_as(C.POINTER(C.c_int32))), "pt_write_tiles")

    def Intersect(self, origins, dirs, flags: int = 0):
        """Scene.Intersect (Scene.cs:75-79) of n rays on the device (pt_intersect): (t [n] float64, 1e9 on
        a miss; kind [n] int32, the pt_shape_kind hit or -1).  flags: _abi.MARCH_LANE / MARCH_WAVE."""
        self._ensure_scene()
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        assert o.shape == d.shape
        t = np.zeros(len(o), np.float64)
        k = np.zeros(len(o), np.int32)
        _abi.check(self._lib.pt_intersect(self._ctx, len(o), o.ctypes.data_as(C.POINTER(C.c_float)),
                                          d.ctypes.data_as(C.POINTER(C.c_float)), int(flags),
                                          t.ctypes.data_as(C.POINTER(C.c_double)), k.ctypes.data_as(C.POINTER(C.c_int32))),
                   "pt_intersect")
        return t, k

    def IntersectHits(self, origins, dirs, flags: int = 0, want=None) -> dict:
        """Scene.Intersect of n rays with what was hit and where (pt_intersect_hits): a dict of numpy arrays by the
        names of pt_hit_arrays (_abi.HIT_ARRAYS: t, kind, index, prim, shape, position, normal, inside, material,
        albedo, gloss), [n] or [n, 3].  want: the names to compute (default: all); asking for none of position ..
        gloss runs the kernel without Hit.Info.  flags as for Intersect."""
        self._ensure_scene()
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        assert o.shape == d.shape
        names = list(_abi.HIT_ARRAYS) if want is None else [k for k in _abi.HIT_ARRAYS if k in set(want)]
        unknown = set(want or ()) - set(_abi.HIT_ARRAYS)
        if unknown:
            raise ValueError(f"IntersectHits: unknown outputs {sorted(unknown)}")
        out = {}
        arrays = _abi.pt_hit_arrays()
        for name in names:
            dtype, comps = _abi.HIT_ARRAYS[name]
            out[name] = np.zeros((len(o), comps) if comps > 1 else len(o), dtype)
            setattr(arrays, name, out[name].ctypes.data_as(dict(_abi.pt_hit_arrays._fields_)[name]))
        _abi.check(self._lib.pt_intersect_hits(self._ctx, len(o), o.ctypes.data_as(C.POINTER(C.c_float)),
                                               d.ctypes.data_as(C.POINTER(C.c_float)), int(flags), C.byref(arrays)),
                   "pt_intersect_hits")
        return out

    def QueryKernelMs(self) -> float:
        """The device time of the last IntersectHits' kernels in ms (pt_query_kernel_ms)."""
        ms = C.c_double(0.0)
        _abi.check(self._lib.pt_query_kernel_ms(self._ctx, C.byref(ms)), "pt_query_kernel_ms")
        return float(ms.value)

    def Occluded(self, origins, dirs, t_max, flags: int = 0) -> np.ndarray:
        """The shadow query after the light's own t (pt_occluded): [n] int32, 1 where a shape is hit
        strictly nearer than t_max."""
        self._ensure_scene()
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        tm = np.ascontiguousarray(t_max, np.float64).reshape(-1)
        assert o.shape == d.shape and len(tm) == len(o)
        b = np.zeros(len(o), np.int32)
        _abi.check(self._lib.pt_occluded(self._ctx, len(o), o.ctypes.data_as(C.POINTER(C.c_float)),
                                         d.ctypes.data_as(C.POINTER(C.c_float)), tm.ctypes.data_as(C.POINTER(C.c_double)),
                                         int(flags), b.ctypes.data_as(C.POINTER(C.c_int32))), "pt_occluded")
        return b

    def UpdateTriangles(self, v1, v2, v3, n1=None, n2=None, n3=None, normals=None) -> float:
        """New vertex positions (and optionally normals) for every triangle of the scene, [n, 3] float32 in
        the order of the compiled scene's tri_v1 (pt_update_triangles): the triangle BVH is refitted on the
        device, nothing is rebuilt or re-uploaded.  With normals="face" or "smooth" (exclusive with n1..n3)
        the normals are derived on the device from the positions (pt_update_triangles_normals): the face
        normal at every corner, or Mesh.SmoothNormals on each mesh.  The arrays (and the derived normals, read
        back) are then written into the uploaded FlatScene in place, so it describes what the device holds.
        Returns the device time of the kernels in ms."""
        self._ensure_scene()
        self._refresh_mirror()
        flat = self._uploaded
        n = len(flat.tri_material)
        if (n1 is None) != (n2 is None) or (n1 is None) != (n3 is None):
            raise ValueError("n1, n2 and n3 must be all given or all None")
        if normals is not None and n1 is not None:
            raise ValueError("normals= derives the normals: n1, n2 and n3 cannot be given with it")
        if normals not in (None, "face", "smooth"):
            raise ValueError('normals is None, "face" or "smooth"')
        arrs = [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (v1, v2, v3)]
        if n1 is not None:
            arrs += [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (n1, n2, n3)]
        if any(len(a) != n for a in arrs):
            raise ValueError(f"the scene has {n} triangles")
        fp = C.POINTER(C.c_float)
        ptrs = [a.ctypes.data_as(fp) for a in arrs] + [fp()] * (6 - len(arrs))
        ms = C.c_double(0.0)
        if normals is None:
            _abi.check(self._lib.pt_update_triangles(self._ctx, n, *ptrs, C.byref(ms)), "pt_update_triangles")
        else:
            mode = _abi.NORMALS_FACE if normals == "face" else _abi.NORMALS_SMOOTH
            _abi.check(self._lib.pt_update_triangles_normals(self._ctx, n, *ptrs[:3], mode, C.byref(ms)),
                       "pt_update_triangles_normals")
            arrs += list(self.ReadTriNormals())
        for dst, a in zip((flat.tri_v1, flat.tri_v2, flat.tri_v3, flat.tri_n1, flat.tri_n2, flat.tri_n3), arrs):
            dst[...] = a
        return float(ms.value)

    def ReadTriNormals(self):
        """The normals the uploaded scene holds on the device now (pt_read_tri_normals): n1, n2, n3, [n, 3]
        float32 each in the order of the compiled scene's tri_n1."""
        self._ensure_scene()
        self._refresh_mirror()   # pt_read_tri_normals reuses the staged arrays a pose is read from
        n = len(self._uploaded.tri_material)
        out = [np.zeros((n, 3), np.float32) for _ in range(3)]
        _abi.check(self._lib.pt_read_tri_normals(self._ctx, *[a.ctypes.data_as(C.POINTER(C.c_float)) for a in out]),
                   "pt_read_tri_normals")
        return out[0], out[1], out[2]

    def ReadTriBvh(self):
        """The context's triangle BVH as it stands on the device (pt_read_tri_bvh): (nodes [N, 32],
        chunks [C, 32], records [T, 32], all uint32, and the root box [6] float32)."""
        self._ensure_scene()
        counts = (C.c_int64 * 3)()
        _abi.check(self._lib.pt_read_tri_bvh(self._ctx, counts, None, None, None, None), "pt_read_tri_bvh")
        out = [np.zeros((int(c), 32), np.uint32) for c in counts]
        box = np.zeros(6, np.float32)
        up = C.POINTER(C.c_uint32)
        _abi.check(self._lib.pt_read_tri_bvh(self._ctx, counts, *[a.ctypes.data_as(up) for a in out],
                                             box.ctypes.data_as(C.POINTER(C.c_float))), "pt_read_tri_bvh")
        return out[0], out[1], out[2], box

    def UpdateShapes(self, sphere_center=None, sphere_radius=None, cube_min=None, cube_max=None, matrices=None,
                     inverses=None) -> float:
        """New parameters for the spheres, cubes and transformed shapes of the scene, in the order of the compiled
        scene's sphere_center, cube_min and transformed (pt_update_shapes): centres [n, 3] float32 (with radii [n]
        float64, or the radii stay), both cube corners [n, 3] float32, matrices [n, 4, 4] float64 with their inverses
        (derived with Matrix.Inverse when not given).  A group left None stays.  The analytic BVH is refitted on the
        device with its topology kept; nothing is rebuilt or re-uploaded.  The arrays are then written into the
        uploaded FlatScene in place, so it describes what the device holds.  Returns the device time of the kernels
        in ms."""
        self._ensure_scene()
        flat = self._uploaded
        if sphere_radius is not None and sphere_center is None:
            raise ValueError("sphere_radius needs sphere_center")
        if (cube_min is None) != (cube_max is None):
            raise ValueError("cube_min and cube_max must be both given or both None")
        if inverses is not None and matrices is None:
            raise ValueError("inverses needs matrices")
        u = _abi.pt_shape_update()
        fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
        keep = []

        def arr(a, dtype, shape, n, what):
            a = np.ascontiguousarray(a, dtype).reshape(shape)
            if len(a) != n:
                raise ValueError(f"the scene has {n} {what}")
            keep.append(a)
            return a

        sc = sr = ca = cb = m = inv = None
        if sphere_center is not None:
            sc = arr(sphere_center, np.float32, (-1, 3), len(flat.sphere_radius), "spheres")
            u.num_spheres, u.sphere_center = len(sc), sc.ctypes.data_as(fp)
            if sphere_radius is not None:
                sr = arr(sphere_radius, np.float64, (-1,), len(sc), "spheres")
                u.sphere_radius = sr.ctypes.data_as(dp)
        if cube_min is not None:
            ca = arr(cube_min, np.float32, (-1, 3), len(flat.cube_material), "cubes")
            cb = arr(cube_max, np.float32, (-1, 3), len(flat.cube_material), "cubes")
            u.num_cubes, u.cube_min, u.cube_max = len(ca), ca.ctypes.data_as(fp), cb.ctypes.data_as(fp)
        if matrices is not None:
            nx = flat.counts_ext[3]
            m = arr(matrices, np.float64, (-1, 4, 4), nx, "transformed shapes")
            if inverses is None:
                from .geometry import Matrix
                inverses = [Matrix(k).Inverse().m for k in m] if nx else np.zeros((0, 4, 4))
            inv = arr(inverses, np.float64, (-1, 4, 4), nx, "transformed shapes")
            u.num_transformed, u.xform_matrix, u.xform_inverse = len(m), m.ctypes.data_as(dp), inv.ctypes.data_as(dp)
        ms = C.c_double(0.0)
        _abi.check(self._lib.pt_update_shapes(self._ctx, C.byref(u), C.byref(ms)), "pt_update_shapes")
        for dst, a in ((flat.sphere_center, sc), (flat.sphere_radius, sr), (flat.cube_min, ca), (flat.cube_max, cb)):
            if a is not None:
                dst[...] = a
        if m is not None:
            for i in range(len(m)):
                flat.transformed[i].matrix[:] = m[i].reshape(-1).tolist()
                flat.transformed[i].inverse[:] = inv[i].reshape(-1).tolist()
        return float(ms.value)

    def ReadShapeBvh(self):
        """The context's analytic BVH as it stands on the device (pt_read_shape_bvh): (nodes [N, 32], records
        [R, 12], heavy records [H, 8], all uint32, and the lights [L, 4] float64: centre x, y, z and radius)."""
        self._ensure_scene()
        counts = (C.c_int64 * 4)()
        _abi.check(self._lib.pt_read_shape_bvh(self._ctx, counts, None, None, None, None), "pt_read_shape_bvh")
        out = [np.zeros((int(c), w), np.uint32) for c, w in zip(counts[:3], (32, 12, 8))]
        lights = np.zeros((int(counts[3]), 4), np.float64)
        up = C.POINTER(C.c_uint32)
        _abi.check(self._lib.pt_read_shape_bvh(self._ctx, counts, *[a.ctypes.data_as(up) for a in out],
                                               lights.ctypes.data_as(C.POINTER(C.c_double))), "pt_read_shape_bvh")
        return out[0], out[1], out[2], lights

    def UpdateVolumes(self, updates, mirror=True) -> float:
        """New voxels and new iso-windows for Volumes of the scene (pt_update_volumes).  `updates` maps a Volume
        object, or its index among the compiled scene's volumes, to (data or None, windows or None): data holds
        W*H*D float64 values in the Volume's own order (Data[x + y*W + z*W*H]); windows is one (lo, hi) pair, or a
        VolumeWindow whose Lo and Hi are taken, per uploaded window (the materials stay).  The volume's derived tables
        are rebuilt on the device; nothing else is re-sent or rebuilt, and a volume given windows only sends no
        voxels.  With `mirror` the new Data, Lo and Hi are written into the Python Volume and the uploaded FlatScene,
        so a later OracleScene(scene) or re-upload sees the same scene.  Returns the device time of the kernels in
        ms."""
        from .scene import VolumeWindow
        self._ensure_scene()
        flat = self._uploaded
        nv = flat.counts_ext[2]
        per = [None] * nv
        for key, val in dict(updates).items():
            if isinstance(key, (int, np.integer)):
                idx = [int(key)]
            else:
                idx = [i for i, o in enumerate(flat.volume_objects) if o is key]
            if not idx or min(idx) < 0 or max(idx) >= nv:
                raise ValueError(f"{key!r} is not a Volume of the uploaded scene")
            for i in idx:
                per[i] = tuple(val)
        u = _abi.pt_volume_update()
        u.num_volumes = nv
        dp = C.POINTER(C.c_double)
        dptr = (dp * max(1, nv))()
        wptr = (C.POINTER(_abi.pt_volume_window) * max(1, nv))()
        staged = [None] * nv
        for i, e in enumerate(per):
            if e is None:
                continue
            data, windows = e
            v, obj = flat.volumes[i], flat.volume_objects[i]
            a = rows = wa = None
            if data is not None:
                a = np.ascontiguousarray(data, np.float64).reshape(-1)
                if a.size != v.w * v.h * v.d:
                    raise ValueError(f"volume {i} holds {v.w}x{v.h}x{v.d} voxels")
                dptr[i] = a.ctypes.data_as(dp)
            if windows is not None:
                rows = []
                for k, w in enumerate(windows):
                    if isinstance(w, VolumeWindow):
                        if k < len(obj.Windows) and w.VolumeWindowMaterial is not obj.Windows[k].VolumeWindowMaterial:
                            raise ValueError(f"volume {i}, window {k}: the material of an uploaded window stays")
                        rows.append((w.Lo, w.Hi))
                    else:
                        rows.append((float(w[0]), float(w[1])))
                if len(rows) != v.num_windows:
                    raise ValueError(f"volume {i} has {v.num_windows} windows")
                wa = (_abi.pt_volume_window * max(1, len(rows)))()
                for k, (lo, hi) in enumerate(rows):
                    wa[k] = _abi.pt_volume_window(lo, hi, v.windows[k].material, 0)
                wptr[i] = C.cast(wa, C.POINTER(_abi.pt_volume_window))
            staged[i] = (a, rows, wa)
        if any(s is not None and s[0] is not None for s in staged):
            u.data = C.cast(dptr, C.POINTER(dp))
        if any(s is not None and s[1] is not None for s in staged):
            u.windows = C.cast(wptr, C.POINTER(C.POINTER(_abi.pt_volume_window)))
        ms = C.c_double(0.0)
        _abi.check(self._lib.pt_update_volumes(self._ctx, C.byref(u), C.byref(ms)), "pt_update_volumes")
        if mirror:
            for i, s in enumerate(staged):
                if s is None:
                    continue
                a, rows, _ = s
                obj = flat.volume_objects[i]
                if a is not None:
                    obj.Data[...] = a   # the array the FlatScene's pt_volume points at
                if rows is not None:
                    for k, (lo, hi) in enumerate(rows):
                        obj.Windows[k].Lo, obj.Windows[k].Hi = lo, hi
                        flat.volumes[i].windows[k].lo, flat.volumes[i].windows[k].hi = lo, hi
        return float(ms.value)

    def ReadVolume(self, i: int) -> dict:
        """What the device holds for volume i (pt_read_volume): a dict with `info` (int64 [8]: w, h, d, windows,
        zero_sign, has_cells, cells, 0), `data` [d, h, w] float64, `windows` [n, 2] float64 (lo, hi), `materials` [n]
        int32, `runs` [d+1, h+1, w+1] int8 and `cells` [cells, 8] float64, or None for a volume without them."""
        self._ensure_scene()
        info = (C.c_int64 * 8)()
        _abi.check(self._lib.pt_read_volume(self._ctx, int(i), info, None, None, None, None), "pt_read_volume")
        w, h, d, nwin, _, has_cells, ncells = (int(x) for x in info[:7])
        data = np.zeros((d, h, w), np.float64)
        wins = (_abi.pt_volume_window * max(1, nwin))()
        runs = np.zeros((d + 1, h + 1, w + 1), np.int8)
        cells = np.zeros((ncells, 8), np.float64) if has_cells else None
        dp = C.POINTER(C.c_double)
        _abi.check(self._lib.pt_read_volume(self._ctx, int(i), info, data.ctypes.data_as(dp),
                                            C.cast(wins, C.POINTER(_abi.pt_volume_window)),
                                            runs.ctypes.data_as(C.POINTER(C.c_int8)),
                                            cells.ctypes.data_as(dp) if has_cells else None), "pt_read_volume")
        return {"info": np.array(list(info), np.int64), "data": data,
                "windows": np.array([[wins[k].lo, wins[k].hi] for k in range(nwin)], np.float64).reshape(nwin, 2),
                "materials": np.array([wins[k].material for k in range(nwin)], np.int32), "runs": runs, "cells": cells}

    def UpdateMaterials(self, updates, env=None, mirror=True) -> float:
        """New materials and a new environment for the uploaded scene (pt_update_materials).  `updates` is a sequence of
        (old, new) pairs, or a dict keyed by index: old is a Material of the scene (matched by value, as the scene's
        materials are; a Material holds a Colour and does not hash, hence the pairs) or its index in the compiled
        scene's table, new the Material that takes its row.  A texture a new Material names must be one of the
        uploaded scene's.  `env` is None (the environment stays) or a dict with any of "Color" (a Colour), "Texture" (a
        ColorTexture of the uploaded scene, or None) and "TextureAngle"; the keys left out keep their values.  The
        lights and the routing flags follow on the device as at an upload; no geometry is re-sent.  With `mirror` the
        uploaded FlatScene, the Scene's Color, Texture and TextureAngle, every shape's Material and Scene.Lights are
        updated, so a later OracleScene(scene) sees the same scene.  Returns the device time of the call's kernels in
        ms: 0, it launches none."""
        from .scene import Material
        self._ensure_scene()
        flat = self._uploaded
        nm = len(flat.material_list)
        new = list(flat.material_list)
        updates = list(updates.items()) if isinstance(updates, dict) else list(updates or [])
        for key, val in updates:
            if isinstance(key, (int, np.integer)):
                idx = [int(key)]
            else:
                idx = [i for i, m in enumerate(flat.material_list) if m.key() == key.key()]
            if not idx or min(idx) < 0 or max(idx) >= nm:
                raise ValueError(f"{key!r} is not a material of the uploaded scene")
            if not isinstance(val, Material):
                raise ValueError("a material is replaced by a Material")
            for i in idx:
                new[i] = val

        def tid(t) -> int:
            if t is None:
                return 0
            for i, o in enumerate(flat.texture_list):
                if o is t:
                    return i + 1
            raise ValueError("a texture that is not in the uploaded scene needs an upload")

        rows = (_abi.pt_material * nm)()
        for i, m in enumerate(new):
            rows[i] = _abi.pt_material((C.c_double * 3)(m.Color.r, m.Color.g, m.Color.b), m.Emittance, m.Index, m.Gloss,
                                       m.Tint, m.Reflectivity, int(bool(m.Transparent)), tid(m.Texture),
                                       tid(m.NormalTexture), tid(m.BumpTexture), tid(m.GlossTexture), 0, m.BumpMultiplier)
        u = _abi.pt_material_update()
        u.num_materials = nm
        if updates:
            u.materials = C.cast(rows, C.POINTER(_abi.pt_material))
        color, tex, angle = self.Scene.Color, self.Scene.Texture, self.Scene.TextureAngle
        if env is not None:
            color, tex, angle = env.get("Color", color), env.get("Texture", tex), float(env.get("TextureAngle", angle))
            u.flags = _abi.LOOK_ENV
            u.env_color = (C.c_double * 3)(*color.tuple())
            u.env_texture, u.env_texture_angle = tid(tex), angle
        ms = C.c_double(0.0)
        _abi.check(self._lib.pt_update_materials(self._ctx, C.byref(u), C.byref(ms)), "pt_update_materials")
        if mirror:
            if updates:
                swap = {old.key(): m for old, m in zip(flat.material_list, new)}
                for i in range(nm):
                    flat.materials[i] = rows[i]
                flat.material_list[:] = new
                self._mirror_materials(swap)
            if env is not None:
                self.Scene.Color, self.Scene.Texture, self.Scene.TextureAngle = color, tex, angle
                flat.env, flat.env_texture, flat.env_texture_angle = color.tuple(), tid(tex), angle
                flat.desc.env_color = (C.c_double * 3)(*flat.env)
                flat.desc.env_texture, flat.desc.env_texture_angle = flat.env_texture, angle
        return float(ms.value)

    def _mirror_materials(self, swap) -> None:
        """Every shape of the Scene takes the Material `swap` maps its own to (by value); Scene.Lights follows."""
        from .scene import Mesh, SDFShape, TransformedShape, Volume
        sc = self.Scene
        seen = set()

        def visit(s):
            if id(s) in seen:
                return
            seen.add(id(s))
            if isinstance(s, TransformedShape):
                visit(s.Shape)
            elif isinstance(s, Mesh):
                s.materials = [swap.get(m.key(), m) for m in s.materials]
            elif isinstance(s, Volume):
                for w in s.Windows:
                    w.VolumeWindowMaterial = swap.get(w.VolumeWindowMaterial.key(), w.VolumeWindowMaterial)
            elif hasattr(s, "Material"):
                s.Material = swap.get(s.Material.key(), s.Material)

        for s in sc.Shapes:
            visit(s)
        sc.Lights = [s for s in sc.Shapes if s.MaterialAt().Emittance > 0]

    def ReadMaterials(self) -> dict:
        """What the device holds of the look (pt_read_materials): a dict with `info` (the pt_look_info), `materials`
        (the pt_material rows as a ctypes array), `light_rows` [L, 4] int32 (kind, index, material, phantom) and
        `light_spheres` [L, 4] float64 (centre, radius)."""
        self._ensure_scene()
        info = _abi.pt_look_info()
        _abi.check(self._lib.pt_read_materials(self._ctx, C.byref(info), None, None, None), "pt_read_materials")
        mats = (_abi.pt_material * max(1, info.num_materials))()
        rows = np.zeros((info.num_lights, 4), np.int32)
        spheres = np.zeros((info.num_lights, 4), np.float64)
        _abi.check(self._lib.pt_read_materials(self._ctx, C.byref(info), C.cast(mats, C.POINTER(_abi.pt_material)),
                                               rows.ctypes.data_as(C.POINTER(C.c_int32)),
                                               spheres.ctypes.data_as(C.POINTER(C.c_double))), "pt_read_materials")
        return {"info": info, "materials": mats, "light_rows": rows, "light_spheres": spheres}

    def UpdateTextures(self, updates, mirror=True) -> float:
        """New texels for textures of the uploaded scene (pt_update_textures).  `updates` maps a ColorTexture of the
        scene, or its index among the compiled scene's textures, to the new image of the same size: a ColorTexture
        (one that kept its 8-bit source, as NewTexture's do, sends its bytes and its 256-entry Table() and is decoded
        on the device; any other sends its Data), an [H, W, 3] float64 array, or a pair (uint8 [H, W, 3 or 4], table of
        256 float64).  With `mirror` the texture's Data is overwritten in place with the new texels, so a later
        OracleScene(scene) sees the same scene.  Returns the device time of the decode kernels in ms."""
        from .scene import ColorTexture
        self._ensure_scene()
        flat = self._uploaded
        nt = len(flat.texture_list)
        imgs = (C.POINTER(_abi.pt_texture_image) * max(1, nt))()
        keep, decoded, source = [], {}, {}
        for key, val in dict(updates or {}).items():
            if isinstance(key, (int, np.integer)):
                idx = [int(key)]
            else:
                idx = [i for i, o in enumerate(flat.texture_list) if o is key]
            if not idx or min(idx) < 0 or max(idx) >= nt:
                raise ValueError(f"{key!r} is not a texture of the uploaded scene")
            src8 = lut = data = None
            kept = (val.Source8, list(val._ops)) if isinstance(val, ColorTexture) else (None, [])
            if isinstance(val, ColorTexture):
                if val.Source8 is not None:
                    src8, lut = val.Source8, val.Table()
                else:
                    data = val.Data
            elif isinstance(val, tuple):
                src8, lut = np.ascontiguousarray(val[0], np.uint8), np.ascontiguousarray(val[1], np.float64).reshape(-1)
            else:
                data = val
            for i in idx:
                t = flat.texture_list[i]
                im = _abi.pt_texture_image()
                if src8 is not None:
                    if src8.ndim != 3 or src8.shape[2] not in (3, 4) or len(lut) != 256:
                        raise ValueError("an 8-bit image is [H, W, 3 or 4] uint8 with a table of 256 doubles")
                    im.height, im.width = src8.shape[:2]
                    im.format = _abi.TEXELS_RGB8 if src8.shape[2] == 3 else _abi.TEXELS_RGBA8
                    im.data, im.lut = src8.ctypes.data_as(C.c_void_p), lut.ctypes.data_as(C.POINTER(C.c_double))
                    keep += [src8, lut]
                    decoded[i] = lambda s=src8, l=lut: l[s[:, :, :3]].reshape(-1, 3)
                else:
                    a = np.ascontiguousarray(data, np.float64)
                    if a.size != 3 * t.Width * t.Height:
                        raise ValueError(f"texture {i} is {t.Width}x{t.Height}")
                    im.width, im.height, im.format = t.Width, t.Height, _abi.TEXELS_F64
                    im.data = a.ctypes.data_as(C.c_void_p)
                    keep.append(a)
                    decoded[i] = lambda a=a: a.reshape(-1, 3)
                keep.append(im)
                source[i] = kept
                imgs[i] = C.pointer(im)
        u = _abi.pt_texture_update()
        u.num_textures = nt
        u.images = C.cast(imgs, C.POINTER(C.POINTER(_abi.pt_texture_image)))
        ms = C.c_double(0.0)
        _abi.check(self._lib.pt_update_textures(self._ctx, C.byref(u), C.byref(ms)), "pt_update_textures")
        if mirror:
            for i, f in decoded.items():
                t = flat.texture_list[i]
                t.Data[...] = f()   # the array the FlatScene's pt_texture points at
                t.Source8, t._ops = source[i][0], list(source[i][1])   # a ColorTexture's 8-bit source and table come along
        return float(ms.value)

    def ReadTexture(self, i: int) -> np.ndarray:
        """The texels the device holds for texture i (pt_read_texture): [H, W, 3] float64."""
        self._ensure_scene()
        info = (C.c_int32 * 4)()
        _abi.check(self._lib.pt_read_texture(self._ctx, int(i), info, None), "pt_read_texture")
        out = np.zeros((int(info[1]), int(info[0]), 3), np.float64)
        _abi.check(self._lib.pt_read_texture(self._ctx, int(i), info, out.ctypes.data_as(C.POINTER(C.c_double))),
                   "pt_read_texture")
        return out

    def UpdateMeshes(self, v1, v2, v3, n1=None, n2=None, n3=None, normals=None) -> float:
        """UpdateTriangles for a scene that may hold instanced meshes (pt_update_meshes; UpdateTriangles refuses
        such a scene): new vertex positions for every triangle of the scene, instanced meshes' included, with the
        normals given (n1..n3), kept, or derived on the device (normals="face" or "smooth").  The world triangle BVH
        and every instanced mesh's BLAS are refitted on the device, the instances' boxes, the analytic BVH and the
        lights follow; nothing is rebuilt or re-uploaded.  The arrays (and the derived normals, read back) are then
        written into the uploaded FlatScene in place, so it describes what the device holds.  Returns the device time
        of the kernels in ms."""
        self._ensure_scene()
        self._refresh_mirror()
        flat = self._uploaded
        n = len(flat.tri_material)
        if (n1 is None) != (n2 is None) or (n1 is None) != (n3 is None):
            raise ValueError("n1, n2 and n3 must be all given or all None")
        if normals is not None and n1 is not None:
            raise ValueError("normals= derives the normals: n1, n2 and n3 cannot be given with it")
        if normals not in (None, "face", "smooth"):
            raise ValueError('normals is None, "face" or "smooth"')
        arrs = [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (v1, v2, v3)]
        if n1 is not None:
            arrs += [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (n1, n2, n3)]
        if any(len(a) != n for a in arrs):
            raise ValueError(f"the scene has {n} triangles")
        fp = C.POINTER(C.c_float)
        u = _abi.pt_mesh_update()
        u.num_triangles = n
        u.normals_mode = 0 if normals is None else _abi.NORMALS_FACE if normals == "face" else _abi.NORMALS_SMOOTH
        for name, a in zip(("v1", "v2", "v3", "n1", "n2", "n3"), arrs):
            setattr(u, name, a.ctypes.data_as(fp))
        ms = C.c_double(0.0)
        _abi.check(self._lib.pt_update_meshes(self._ctx, C.byref(u), C.byref(ms)), "pt_update_meshes")
        if normals is not None:
            arrs += self._derived_normals(arrs)
        for dst, a in zip((flat.tri_v1, flat.tri_v2, flat.tri_v3, flat.tri_n1, flat.tri_n2, flat.tri_n3), arrs):
            dst[...] = a
        return float(ms.value)

    def RebuildMeshes(self, v1=None, v2=None, v3=None, n1=None, n2=None, n3=None, normals=None) -> float:
        """UpdateMeshes that also re-sorts the world triangle BVH on the device (pt_rebuild_meshes): the topology is
        replaced by a balanced object-median tree for the new positions, for a mesh deformed far from the pose its tree
        was built for (TriBvhCost tells when).  RebuildMeshes() with no arrays takes the pose the last PoseMeshes or
        SkinMeshes left staged on the device; nothing is copied.  A scene with an instanced mesh is refused.  The uploaded FlatScene
        is kept as UpdateMeshes keeps it.  Returns the device time of the kernels in ms."""
        self._ensure_scene()
        ms = C.c_double(0.0)
        if v1 is None:
            if any(a is not None for a in (v2, v3, n1, n2, n3)) or normals is not None:
                raise ValueError("RebuildMeshes() takes the staged pose: no other argument goes with it")
            _abi.check(self._lib.pt_rebuild_meshes(self._ctx, None, C.byref(ms)), "pt_rebuild_meshes")
            self._refresh_mirror()
            return float(ms.value)
        self._refresh_mirror()
        flat = self._uploaded
        n = len(flat.tri_material)
        if (n1 is None) != (n2 is None) or (n1 is None) != (n3 is None):
            raise ValueError("n1, n2 and n3 must be all given or all None")
        if normals is not None and n1 is not None:
            raise ValueError("normals= derives the normals: n1, n2 and n3 cannot be given with it")
        if normals not in (None, "face", "smooth"):
            raise ValueError('normals is None, "face" or "smooth"')
        arrs = [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (v1, v2, v3)]
        if n1 is not None:
            arrs += [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (n1, n2, n3)]
        if any(len(a) != n for a in arrs):
            raise ValueError(f"the scene has {n} triangles")
        fp = C.POINTER(C.c_float)
        u = _abi.pt_mesh_update()
        u.num_triangles = n
        u.normals_mode = 0 if normals is None else _abi.NORMALS_FACE if normals == "face" else _abi.NORMALS_SMOOTH
        for name, a in zip(("v1", "v2", "v3", "n1", "n2", "n3"), arrs):
            setattr(u, name, a.ctypes.data_as(fp))
        _abi.check(self._lib.pt_rebuild_meshes(self._ctx, C.byref(u), C.byref(ms)), "pt_rebuild_meshes")
        if normals is not None:
            arrs += [a.copy() for a in self.ReadTriNormals()]
        for dst, a in zip((flat.tri_v1, flat.tri_v2, flat.tri_v3, flat.tri_n1, flat.tri_n2, flat.tri_n3), arrs):
            dst[...] = a
        return float(ms.value)

    def RebuildBlas(self, v1=None, v2=None, v3=None, n1=None, n2=None, n3=None, normals=None, what=0) -> float:
        """UpdateMeshes that also re-sorts every instanced mesh's BLAS on the device (pt_rebuild_blas): each BLAS gets a
        balanced object-median tree for the new positions (BlasCost tells when that pays); one whose balanced tree
        needs more nodes than the upload gave it is refitted instead.  `what` is _abi.REBUILD_WORLD (the world
        triangle BVH, as RebuildMeshes re-sorts it), _abi.REBUILD_BLAS, or both (0).  RebuildBlas() with no arrays
        takes the pose the last PoseMeshes or SkinMeshes left staged on the device.  The uploaded FlatScene is kept as UpdateMeshes
        keeps it.  Returns the device time of the kernels in ms."""
        self._ensure_scene()
        ms = C.c_double(0.0)
        if v1 is None:
            if any(a is not None for a in (v2, v3, n1, n2, n3)) or normals is not None:
                raise ValueError("RebuildBlas() takes the staged pose: no other argument goes with it")
            _abi.check(self._lib.pt_rebuild_blas(self._ctx, None, int(what), C.byref(ms)), "pt_rebuild_blas")
            self._refresh_mirror()
            return float(ms.value)
        self._refresh_mirror()
        flat = self._uploaded
        n = len(flat.tri_material)
        if (n1 is None) != (n2 is None) or (n1 is None) != (n3 is None):
            raise ValueError("n1, n2 and n3 must be all given or all None")
        if normals is not None and n1 is not None:
            raise ValueError("normals= derives the normals: n1, n2 and n3 cannot be given with it")
        if normals not in (None, "face", "smooth"):
            raise ValueError('normals is None, "face" or "smooth"')
        arrs = [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (v1, v2, v3)]
        if n1 is not None:
            arrs += [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (n1, n2, n3)]
        if any(len(a) != n for a in arrs):
            raise ValueError(f"the scene has {n} triangles")
        fp = C.POINTER(C.c_float)
        u = _abi.pt_mesh_update()
        u.num_triangles = n
        u.normals_mode = 0 if normals is None else _abi.NORMALS_FACE if normals == "face" else _abi.NORMALS_SMOOTH
        for name, a in zip(("v1", "v2", "v3", "n1", "n2", "n3"), arrs):
            setattr(u, name, a.ctypes.data_as(fp))
        _abi.check(self._lib.pt_rebuild_blas(self._ctx, C.byref(u), int(what), C.byref(ms)), "pt_rebuild_blas")
        if normals is not None:
            arrs += self._derived_normals(arrs)
        for dst, a in zip((flat.tri_v1, flat.tri_v2, flat.tri_v3, flat.tri_n1, flat.tri_n2, flat.tri_n3), arrs):
            dst[...] = a
        return float(ms.value)

    def BlasCost(self):
        """The surface-area cost of every BLAS as it stands on the device (pt_blas_cost): [B, 3] float64 of (inner,
        leaf, root_area), the first two relative to the BLAS's root box's area.  A refit keeps the topology, so the cost
        grows as a mesh deforms; its growth since the upload is the trigger for RebuildBlas."""
        self._ensure_scene()
        counts = (C.c_int64 * 3)()
        _abi.check(self._lib.pt_read_blas(self._ctx, counts, None, None, None, None, None), "pt_read_blas")
        nb = int(counts[0])
        out = np.zeros((nb, 3), np.float64)
        _abi.check(self._lib.pt_blas_cost(self._ctx, nb, out.ctypes.data_as(C.POINTER(C.c_double))), "pt_blas_cost")
        return out

    def TriBvhCost(self):
        """The surface-area cost of the world triangle BVH as it stands on the device (pt_tri_bvh_cost): (inner,
        leaf, root_area), the first two relative to the root box's area.  A refit keeps the topology, so the cost
        grows as a mesh deforms; its growth since the upload is the trigger for RebuildMeshes."""
        self._ensure_scene()
        out = (C.c_double * 3)()
        _abi.check(self._lib.pt_tri_bvh_cost(self._ctx, out), "pt_tri_bvh_cost")
        return float(out[0]), float(out[1]), float(out[2])

    def _derived_normals(self, verts):
        """The normals the device derived, in the scene's order: pt_read_tri_normals', and for the triangles of
        instanced meshes (zeros there unless the mesh is a top-level shape too) the BLAS shade rows, matched to their
        source triangles by the geometry rows, which hold {v1, v2 - v1, v3 - v1} exactly."""
        flat = self._uploaded
        out = [a.copy() for a in self.ReadTriNormals()]
        blas, _, recs, shade, _ = self.ReadBlas()
        meshes = []   # the BLASes' meshes, in the compile's order: first use by a transformed shape
        for x in flat.transformed[:flat.counts_ext[3]]:
            if x.shape_kind == 4 and x.shape_index not in meshes:
                meshes.append(x.shape_index)
        v1, v2, v3 = verts[:3]
        for b, j in enumerate(meshes[:len(blas)]):
            f, cnt, r0 = int(flat.mesh_first[j]), int(flat.mesh_count[j]), int(blas[b, 2])
            at = {recs[r0 + t, :9].tobytes(): r0 + t for t in range(cnt)}
            keys = np.concatenate([v1[f:f + cnt], v2[f:f + cnt] - v1[f:f + cnt], v3[f:f + cnt] - v1[f:f + cnt]],
                                  axis=1).astype(np.float32).view(np.uint32)
            for t in range(cnt):
                pos = at.get(keys[t].tobytes())
                if pos is not None:
                    nn = shade[pos, :9].view(np.float32)
                    out[0][f + t], out[1][f + t], out[2][f + t] = nn[0:3], nn[3:6], nn[6:9]
        return out

    def SetRestPose(self, v1=None, v2=None, v3=None, n1=None, n2=None, n3=None) -> None:
        """Installs the rest pose PoseMeshes poses from (pt_set_rest_pose): positions and normals of every triangle,
        [n, 3] float32 in the order of the compiled scene's tri_v1, kept on the device until the next upload.  An
        array left None is the uploaded FlatScene's current one."""
        self._ensure_scene()
        self._refresh_mirror()
        flat = self._uploaded
        n = len(flat.tri_material)
        given = (v1, v2, v3, n1, n2, n3)
        mine = (flat.tri_v1, flat.tri_v2, flat.tri_v3, flat.tri_n1, flat.tri_n2, flat.tri_n3)
        arrs = [np.ascontiguousarray(m if a is None else a, np.float32).reshape(-1, 3) for a, m in zip(given, mine)]
        if any(len(a) != n for a in arrs):
            raise ValueError(f"the scene has {n} triangles")
        fp = C.POINTER(C.c_float)
        _abi.check(self._lib.pt_set_rest_pose(self._ctx, n, *[a.ctypes.data_as(fp) for a in arrs]), "pt_set_rest_pose")
        self._rest_of = flat

    def PoseMeshes(self, matrices, normals=None, mask=None, mirror=True) -> float:
        """Mesh.Transform(matrices[j]) of every mesh j of the scene on the device, from the rest pose (pt_pose_meshes):
        `matrices` is a sequence of Matrix or an [M, 16] (or [M, 4, 4]) float64 array, indexed like the compiled
        scene's mesh_first; `mask` ([M], optional) is 0 for a mesh that takes its rest values; loose triangles take
        theirs.  normals=None transforms the rest normals as Mesh.Transform does, "face" or "smooth" derives them from
        the posed positions.  The BVHs, the instances' boxes and the lights are refitted as UpdateMeshes refits them.
        The rest pose is installed on first use (SetRestPose()).  With mirror=True the posed arrays are read back into
        the uploaded FlatScene in place, so it describes what the device holds; with mirror=False that readback (72 B
        per triangle) is skipped and the FlatScene's triangle arrays are stale until ReadPose(), or the next
        UpdateTriangles, UpdateMeshes, ReadTriNormals or SetRestPose, refreshes them.  Returns the device time of the
        kernels in ms."""
        self._ensure_scene()
        flat = self._uploaded
        if normals not in (None, "face", "smooth"):
            raise ValueError('normals is None, "face" or "smooth"')
        if self._rest_of is not flat:
            self.SetRestPose()
        nm = len(flat.mesh_first)
        m = np.ascontiguousarray([getattr(k, "m", k) for k in matrices] if nm else np.zeros((0, 16)), np.float64).reshape(-1, 16)
        if len(m) != nm:
            raise ValueError(f"the scene has {nm} meshes")
        u = _abi.pt_mesh_pose()
        u.num_meshes = nm
        u.normals_mode = 0 if normals is None else _abi.NORMALS_FACE if normals == "face" else _abi.NORMALS_SMOOTH
        u.matrices = m.ctypes.data_as(C.POINTER(C.c_double))
        if mask is not None:
            on = np.ascontiguousarray(mask, np.int32).reshape(-1)
            if len(on) != nm:
                raise ValueError(f"the scene has {nm} meshes")
            u.mesh_mask = on.ctypes.data_as(C.POINTER(C.c_int32))
        ms = C.c_double(0.0)
        _abi.check(self._lib.pt_pose_meshes(self._ctx, C.byref(u), C.byref(ms)), "pt_pose_meshes")
        # a device time of exactly 0: nothing was launched (no triangle of the scene is in a BVH), nothing to mirror
        self._mirror_stale = ms.value != 0.0
        if mirror:
            self._refresh_mirror()
        return float(ms.value)

    def SetSkin(self, bones, weights, num_bones) -> None:
        """Installs the skin SkinMeshes blends with (pt_set_skin): for every corner of every triangle of the compiled
        scene four bone indices and four weights.  `bones` is an [n, 3, 4] integer array or three [n, 4] arrays (corner
        1, 2, 3), `weights` the same in float32; a weight of 0 makes its influence dead.  Kept on the device until the
        next upload; an index outside [0, num_bones) is refused."""
        self._ensure_scene()
        n = len(self._uploaded.tri_material)

        def corners(a, dtype):
            if isinstance(a, np.ndarray) and a.ndim == 3:
                a = [a[:, k] for k in range(3)]
            a = [np.ascontiguousarray(x, dtype).reshape(-1, 4) for x in a]
            if len(a) != 3 or any(len(x) != n for x in a):
                raise ValueError(f"the scene has {n} triangles: three [n, 4] arrays, or one [n, 3, 4]")
            return a
        b, w = corners(bones, np.int32), corners(weights, np.float32)
        d = _abi.pt_skin_desc()
        d.num_triangles, d.num_bones = n, int(num_bones)
        d.bone1, d.bone2, d.bone3 = (x.ctypes.data_as(C.POINTER(C.c_int32)) for x in b)
        d.weight1, d.weight2, d.weight3 = (x.ctypes.data_as(C.POINTER(C.c_float)) for x in w)
        _abi.check(self._lib.pt_set_skin(self._ctx, C.byref(d)), "pt_set_skin")

    def SkinMeshes(self, matrices, normals=None, mirror=True) -> float:
        """Linear blend skinning of every mesh of the scene on the device, from the rest pose and the skin SetSkin
        installed (pt_skin_meshes): `matrices` is a sequence of Matrix or a [B, 16] (or [B, 4, 4]) float64 array, one
        per bone.  normals=None blends the transformed rest normals, "face" or "smooth" derives them from the skinned
        positions.  Loose triangles take their rest values.  The BVHs, the instances' boxes and the lights are refitted
        as UpdateMeshes refits them.  The rest pose is installed on first use (SetRestPose()); mirror is PoseMeshes'.
        Returns the device time of the kernels in ms."""
        self._ensure_scene()
        flat = self._uploaded
        if normals not in (None, "face", "smooth"):
            raise ValueError('normals is None, "face" or "smooth"')
        if self._rest_of is not flat:
            self.SetRestPose()
        m = np.ascontiguousarray([getattr(k, "m", k) for k in matrices], np.float64).reshape(-1, 16)
        u = _abi.pt_mesh_skin()
        u.num_bones = len(m)
        u.normals_mode = 0 if normals is None else _abi.NORMALS_FACE if normals == "face" else _abi.NORMALS_SMOOTH
        u.matrices = m.ctypes.data_as(C.POINTER(C.c_double))
        ms = C.c_double(0.0)
        _abi.check(self._lib.pt_skin_meshes(self._ctx, C.byref(u), C.byref(ms)), "pt_skin_meshes")
        # a device time of exactly 0: nothing was launched (no triangle of the scene is in a BVH), nothing to mirror
        self._mirror_stale = ms.value != 0.0
        if mirror:
            self._refresh_mirror()
        return float(ms.value)

    def ReadSkin(self):
        """The installed skin as SetSkin took it (pt_read_skin): (bones [n, 3, 4] int32, weights [n, 3, 4] float32)."""
        self._ensure_scene()
        n = len(self._uploaded.tri_material)
        b = [np.zeros((n, 4), np.int32) for _ in range(3)]
        w = [np.zeros((n, 4), np.float32) for _ in range(3)]
        _abi.check(self._lib.pt_read_skin(self._ctx, *[x.ctypes.data_as(C.POINTER(C.c_int32)) for x in b],
                                          *[x.ctypes.data_as(C.POINTER(C.c_float)) for x in w]), "pt_read_skin")
        return np.stack(b, axis=1), np.stack(w, axis=1)

    def SetMorph(self, targets, normal_deltas=None) -> None:
        """Installs the morph targets MorphMeshes adds to the rest pose (pt_set_morph).  `targets` is a list with one
        (corners, dpos[, dnrm]) per target: corners [k] integers 3 * triangle + c (c = 0, 1, 2 for v1, v2, v3), strictly
        ascending, dpos and dnrm [k, 3] float32; or the packed arrays as a dict with target_first [T + 1], corner [D],
        dpos [D, 3] and optionally dnrm [D, 3].  normal_deltas=True requires every target to carry dnrm, False drops
        them, None takes them when every target of the list has them.  Kept on the device until the next upload."""
        self._ensure_scene()
        n = len(self._uploaded.tri_material)
        if isinstance(targets, dict):
            first = np.ascontiguousarray(targets["target_first"], np.int64).reshape(-1)
            corner = np.ascontiguousarray(targets["corner"], np.int32).reshape(-1)
            dpos = np.ascontiguousarray(targets["dpos"], np.float32).reshape(-1, 3)
            dnrm = targets.get("dnrm")
            if normal_deltas and dnrm is None:
                raise ValueError("normal_deltas=True and the packed arrays have no dnrm")
            dnrm = None if dnrm is None or normal_deltas is False else np.ascontiguousarray(dnrm, np.float32).reshape(-1, 3)
        else:
            targets = list(targets)
            have = [len(t) > 2 and t[2] is not None for t in targets]
            if normal_deltas and not all(have):
                raise ValueError("normal_deltas=True and a target has no dnrm")
            with_n = bool(targets) and all(have) if normal_deltas is None else bool(normal_deltas)
            first = np.zeros(len(targets) + 1, np.int64)
            first[1:] = np.cumsum([len(np.asarray(t[0]).reshape(-1)) for t in targets])
            cat = lambda k, dtype, shape: (np.concatenate([np.asarray(t[k], dtype).reshape(shape) for t in targets])
                                           if targets else np.zeros(shape, dtype).reshape(shape)[:0])
            corner = np.ascontiguousarray(cat(0, np.int32, (-1,)))
            dpos = np.ascontiguousarray(cat(1, np.float32, (-1, 3)))
            dnrm = np.ascontiguousarray(cat(2, np.float32, (-1, 3))) if with_n else None
        if len(dpos) != len(corner) or (dnrm is not None and len(dnrm) != len(corner)) or (len(first) and first[-1] != len(corner)):
            raise ValueError("corner, dpos and dnrm hold one entry per delta, target_first[-1] of them")
        # (room for one entry past the end, so that a morph with no delta still passes non-NULL arrays)
        room = lambda x: None if x is None else np.ascontiguousarray(np.concatenate([x.reshape(-1), np.zeros(3, x.dtype)]))
        corner_a, dpos_a, dnrm_a = room(corner), room(dpos), room(dnrm)
        d = _abi.pt_morph_desc()
        d.num_triangles, d.num_targets = n, len(first) - 1
        d.target_first = first.ctypes.data_as(C.POINTER(C.c_int64))
        d.corner = corner_a.ctypes.data_as(C.POINTER(C.c_int32))
        d.dpos = dpos_a.ctypes.data_as(C.POINTER(C.c_float))
        d.dnrm = None if dnrm_a is None else dnrm_a.ctypes.data_as(C.POINTER(C.c_float))
        _abi.check(self._lib.pt_set_morph(self._ctx, C.byref(d)), "pt_set_morph")
        self._morph_of = (self._uploaded, dnrm is not None)

    def MorphMeshes(self, weights, normals=None, skin=None, mirror=True) -> float:
        """Morphs every mesh of the scene on the device, from the rest pose and the targets SetMorph installed
        (pt_morph_meshes): `weights` holds one float32 per target; a weight of 0 makes its target dead.  normals=None
        adds the targets' normal deltas to the rest normals and normalises (the rest normals stay when the morph has
        none), "face" or "smooth" derives them from the morphed positions.  `skin` (a sequence of Matrix or a [B, 16]
        float64 array, one per bone of the skin SetSkin installed) skins the morphed pose as SkinMeshes skins the rest
        pose.  Loose triangles take their rest values.  The BVHs, the instances' boxes and the lights are refitted as
        UpdateMeshes refits them.  The rest pose is installed on first use (SetRestPose()); mirror is PoseMeshes'.
        Returns the device time of the kernels in ms."""
        self._ensure_scene()
        flat = self._uploaded
        if normals not in (None, "face", "smooth"):
            raise ValueError('normals is None, "face" or "smooth"')
        if self._rest_of is not flat:
            self.SetRestPose()
        w = np.ascontiguousarray(weights, np.float32).reshape(-1)
        u = _abi.pt_mesh_morph()
        u.num_targets = len(w)
        u.normals_mode = 0 if normals is None else _abi.NORMALS_FACE if normals == "face" else _abi.NORMALS_SMOOTH
        u.weights = w.ctypes.data_as(C.POINTER(C.c_float))
        if skin is not None:
            m = np.ascontiguousarray([getattr(k, "m", k) for k in skin], np.float64).reshape(-1, 16)
            u.num_bones = len(m)
            u.skin_matrices = m.ctypes.data_as(C.POINTER(C.c_double))
        ms = C.c_double(0.0)
        _abi.check(self._lib.pt_morph_meshes(self._ctx, C.byref(u), C.byref(ms)), "pt_morph_meshes")
        # a device time of exactly 0: nothing was launched (no triangle of the scene is in a BVH), nothing to mirror
        self._mirror_stale = ms.value != 0.0
        if mirror:
            self._refresh_mirror()
        return float(ms.value)

    def ReadMorph(self):
        """The installed morph as the device holds it, unpacked (pt_read_morph): a dict with target_first [T + 1] int64,
        corner [D] int32, dpos [D, 3] float32, dnrm [D, 3] float32 or None when the morph carries no normal deltas, and
        padded: the entries the packed format holds on the device, padding included.  (Whether to ask for dnrm is what this
        Renderer's SetMorph installed.)"""
        self._ensure_scene()
        counts = (C.c_int64 * 3)()
        _abi.check(self._lib.pt_read_morph(self._ctx, counts, None, None, None, None), "pt_read_morph")
        t, k = int(counts[0]), int(counts[1])
        first = np.zeros(t + 1, np.int64)
        corner = np.zeros(k + 1, np.int32)
        dpos = np.zeros((k + 1, 3), np.float32)
        with_n = self._morph_of is not None and self._morph_of[0] is self._uploaded and self._morph_of[1]
        dnrm = np.zeros((k + 1, 3), np.float32) if with_n else None
        _abi.check(self._lib.pt_read_morph(self._ctx, counts, first.ctypes.data_as(C.POINTER(C.c_int64)),
                                           corner.ctypes.data_as(C.POINTER(C.c_int32)), dpos.ctypes.data_as(C.POINTER(C.c_float)),
                                           None if dnrm is None else dnrm.ctypes.data_as(C.POINTER(C.c_float))), "pt_read_morph")
        return dict(target_first=first, corner=corner[:k].copy(), dpos=dpos[:k].copy(), dnrm=None if dnrm is None else dnrm[:k].copy(),
                    padded=int(counts[2]))

    def ReadPose(self):
        """The six arrays the last PoseMeshes, SkinMeshes or MorphMeshes left on the device (pt_read_pose): v1, v2, v3, n1, n2, n3, [n, 3]
        float32 each, derived normals included.  Also brings a FlatScene left stale by mirror=False up to date."""
        self._ensure_scene()
        n = len(self._uploaded.tri_material)
        out = [np.zeros((n, 3), np.float32) for _ in range(6)]
        _abi.check(self._lib.pt_read_pose(self._ctx, *[a.ctypes.data_as(C.POINTER(C.c_float)) for a in out]), "pt_read_pose")
        if self._mirror_stale:
            flat = self._uploaded
            for dst, a in zip((flat.tri_v1, flat.tri_v2, flat.tri_v3, flat.tri_n1, flat.tri_n2, flat.tri_n3), out):
                dst[...] = a
            self._mirror_stale = False
        return tuple(out)

    def _refresh_mirror(self):
        """The uploaded FlatScene's triangle arrays brought up to date after a PoseMeshes(mirror=False), before a call
        that reads them or reuses the device's staged arrays."""
        if self._mirror_stale:
            self.ReadPose()

    def ReadBlas(self):
        """The context's BLASes, the object-space BVHs of instanced meshes, as they stand on the device
        (pt_read_blas): (blas [B, 4] int32: first node, nodes, first triangle, 0; nodes [N, 32], recs [T, 12] and
        shade [T, 12], all uint32; the meshes' unpadded boxes [B, 6] float32)."""
        self._ensure_scene()
        counts = (C.c_int64 * 3)()
        _abi.check(self._lib.pt_read_blas(self._ctx, counts, None, None, None, None, None), "pt_read_blas")
        nb, nn, nt = (int(c) for c in counts)
        blas = np.zeros((nb, 4), np.int32)
        nodes, recs, shade = np.zeros((nn, 32), np.uint32), np.zeros((nt, 12), np.uint32), np.zeros((nt, 12), np.uint32)
        boxes = np.zeros((nb, 6), np.float32)
        up = C.POINTER(C.c_uint32)
        _abi.check(self._lib.pt_read_blas(self._ctx, counts, blas.ctypes.data_as(C.POINTER(C.c_int32)),
                                          nodes.ctypes.data_as(up), recs.ctypes.data_as(up), shade.ctypes.data_as(up),
                                          boxes.ctypes.data_as(C.POINTER(C.c_float))), "pt_read_blas")
        return blas, nodes, recs, shade, boxes

    def ResetBuffer(self) -> None:
        _abi.check(self._lib.pt_reset_buffer(self._ctx), "pt_reset_buffer")
        self._pass = 0

    def Stats(self) -> _abi.pt_stats:
        s = _abi.pt_stats()
        _abi.check(self._lib.pt_stats_get(self._ctx, C.byref(s)), "pt_stats_get")
        return s

    def IterativeRender(self, pathTemplate: str | None, iterations: int) -> np.ndarray:
        """Renderer.IterativeRender (Renderer.cs:702-765).  Each iteration is one Render
        (NumCPU == 1) or RenderParallel pass, including its adaptive / firefly phases.  With Denoise
        (Renderer.cs:731-761) each pass also writes albedo_channel.png, normal_channel.png and
        denoised_output.png beside the pass image (in pathTemplate's directory), and the denoised
        image is returned; with no pathTemplate the Buffer is denoised once, after the last pass.  With
        DenoiseGuided as well, the features are rendered once before the loop and the filter is the
        guided one (pt_denoise_guided)."""
        self.iterations = iterations
        img = None
        denoised = None
        guided = bool(self.Denoise and self.DenoiseGuided)
        if guided:
            self.RenderFeatures()
        for i in range(1, iterations + 1):
            if self.Verbose:
                print(f"Iteration {i} of {iterations}")
            if self.NumCPU == 1:  # Renderer.cs:712-719
                self.Render()
            else:
                self.RenderParallel()
            if pathTemplate:
                img = self.Image(Channel.ColorChannel) if self.DeviceImages else self.ReadBuffer().Image(Channel.ColorChannel)
                write_png(pathTemplate.replace("{0}", str(i)), img)
                if self.Denoise:
                    where = os.path.dirname(pathTemplate)
                    write_png(os.path.join(where, "albedo_channel.png"), self.Image(Channel.AlbedoChannel))
                    write_png(os.path.join(where, "normal_channel.png"), self.Image(Channel.NormalChannel))
                    self.DenoiseBuffer(guided)
                    denoised = self.Denoised()
                    write_png(os.path.join(where, "denoised_output.png"), denoised)
        if self.Denoise and denoised is None:
            self.DenoiseBuffer(guided)
            denoised = self.Denoised()
        if self.DeviceImages:
            if img is None:
                img = self.Image(Channel.ColorChannel)
            self.ReadBuffer()  # Renderer.PBuffer once, after the last pass
        elif img is None:
            img = self.ReadBuffer().Image(Channel.ColorChannel)
        return denoised if self.Denoise else img

    # ------------------------------------------------------------- multi-GPU
    def CommInit(self, nranks: int, rank: int, unique_id: bytes) -> None:
        idb = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        _abi.check(self._lib.pt_comm_init(self._ctx, nranks, rank, idb), "pt_comm_init")

    def Gather(self, root: int = 0) -> None:
        _abi.check(self._lib.pt_comm_gather(self._ctx, root), "pt_comm_gather")

    @staticmethod
    def CommInitAll(renderers: list) -> None:
        """One communicator over renderers on distinct devices of this process (pt_comm_init_all)."""
        lib = _abi.load_library()
        arr = (C.c_void_p * len(renderers))(*[r._ctx.value for r in renderers])
        _abi.check(lib.pt_comm_init_all(arr, len(renderers)), "pt_comm_init_all")

    @staticmethod
    def GatherAll(renderers: list, root: int = 0) -> None:
        lib = _abi.load_library()
        arr = (C.c_void_p * len(renderers))(*[r._ctx.value for r in renderers])
        _abi.check(lib.pt_comm_gather_all(arr, len(renderers), root), "pt_comm_gather_all")

    @staticmethod
    def CommUniqueId() -> bytes:
        lib = _abi.load_library()
        buf = (C.c_uint8 * 128)()
        _abi.check(lib.pt_comm_unique_id(buf), "pt_comm_unique_id")
        return bytes(buf)
