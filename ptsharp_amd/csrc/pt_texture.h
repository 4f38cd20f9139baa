// pt_texture.h — the index arithmetic and the per-lane decode of pt_update_textures' 8-bit formats, stated once for
// the device kernel (pt_texture.hip k_tex_decode) and the host (tests/native/look_check.cpp runs the same function in
// the kernel's lane order).  Every function is host and device, makes no HIP call and compiles with g++.
//
// An 8-bit image is [h][w][bpp] bytes, rows packed (bpp 3: RGB8, 4: RGBA8, A ignored), so pixel p's bytes start at
// p * bpp whatever the row.  The image lies in the call's byte staging at src_off, which is any byte offset: the
// images of one call are packed one after another, and an RGB8 image of an odd pixel count leaves the next one
// off the dword grid.  A texel is 3 doubles; texture slices lie one after another in the scene's one texel
// allocation, so a slice of an odd number of doubles leaves the next one off the 16-byte grid.
//
// A lane decodes run r: the kTexRun consecutive pixels from r * kTexRun (the last run of an image may be shorter).
// Every channel is lut[byte]; no arithmetic touches a value, so the doubles are the table's bit patterns.
// Every pixel index, byte offset and texel index is 64-bit: an 8K x 8K texture is 1.6 GB of doubles.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define PT_TEX_HD __host__ __device__ __forceinline__
#define PT_TEX_UNROLL _Pragma("unroll")
#else
#define PT_TEX_HD inline
#define PT_TEX_UNROLL
#endif

namespace pt {

constexpr int kTexRun = 4;       // pixels per lane: 12 or 16 source bytes (3 or 4 dwords), 96 destination bytes (six 16-B stores)
constexpr int kTexBlock = 256;   // lanes per block, one table entry staged per lane
constexpr int kTexLut = 256;     // table entries

// bytes per pixel of a pt_texel_format's 8-bit formats (PT_TEXELS_RGB8 = 1, PT_TEXELS_RGBA8 = 2)
PT_TEX_HD int tex_bpp(int format) { return format == 2 ? 4 : 3; }
PT_TEX_HD uint64_t tex_pixels(int32_t w, int32_t h) { return (uint64_t)w * (uint64_t)h; }
PT_TEX_HD uint64_t tex_run_count(uint64_t pixels) { return (pixels + (uint64_t)kTexRun - 1) / (uint64_t)kTexRun; }
PT_TEX_HD uint64_t tex_run_first(uint64_t run) { return run * (uint64_t)kTexRun; }
// pixels of run `run`: kTexRun, or what is left of the image
PT_TEX_HD int tex_run_len(uint64_t run, uint64_t pixels) {
    const uint64_t first = tex_run_first(run);
    return first >= pixels ? 0 : (pixels - first < (uint64_t)kTexRun ? (int)(pixels - first) : kTexRun);
}
// first source byte of pixel p in the staging, first double of its texel in the slice
PT_TEX_HD uint64_t tex_src_byte(uint64_t src_off, uint64_t p, int bpp) { return src_off + p * (uint64_t)bpp; }
PT_TEX_HD uint64_t tex_dst_first(uint64_t p) { return 3 * p; }
// the blocks of a launch over `pixels` pixels
PT_TEX_HD uint64_t tex_block_count(uint64_t pixels) { return (tex_run_count(pixels) + (uint64_t)kTexBlock - 1) / (uint64_t)kTexBlock; }

// Run `run` of an image of `pixels` pixels: src is the staging's base, dst the texture's slice.  A full run whose
// source bytes start on a dword takes them as 3 or 4 whole dwords (one 16-B load for RGBA8 on a 16-B boundary), else
// byte by byte; a full run whose texels start on a 16-B boundary is written as six 16-B stores, else double by
// double.  Reads src[src_off + first * bpp .. + len * bpp), writes dst[3 * first .. 3 * (first + len)): nothing
// outside the image.
PT_TEX_HD void tex_decode_run(const uint8_t* src, uint64_t src_off, int bpp, uint64_t run, uint64_t pixels, const double* lut,
                              double* dst) {
    const int len = tex_run_len(run, pixels);
    if (len <= 0) return;
    const uint64_t first = tex_run_first(run);
    const uint8_t* s = src + tex_src_byte(src_off, first, bpp);
    double* d = dst + tex_dst_first(first);
    // (every loop below has constant bounds and unrolls, so b and v stay in registers on the device)
    uint8_t b[4 * kTexRun];
    const int nbytes = len * bpp;
    if (len == kTexRun && ((uintptr_t)s & 3u) == 0) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (bpp == 4 && ((uintptr_t)s & 15u) == 0) {
            __builtin_memcpy(w, __builtin_assume_aligned(s, 16), 16);
        } else {
            PT_TEX_UNROLL
            for (int k = 0; k < 4; k++)
                if (k < bpp) __builtin_memcpy(&w[k], __builtin_assume_aligned(s + 4 * k, 4), 4);
        }
        PT_TEX_UNROLL
        for (int k = 0; k < 4 * kTexRun; k++) b[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));   // little-endian, as the bytes lie
    } else {
        PT_TEX_UNROLL
        for (int k = 0; k < 4 * kTexRun; k++) b[k] = k < nbytes ? s[k] : (uint8_t)0;
    }
    double v[3 * kTexRun];
    PT_TEX_UNROLL
    for (int p = 0; p < kTexRun; p++) {
        PT_TEX_UNROLL
        for (int ch = 0; ch < 3; ch++) v[3 * p + ch] = lut[bpp == 4 ? b[4 * p + ch] : b[3 * p + ch]];
    }
    if (len == kTexRun && ((uintptr_t)d & 15u) == 0) {
        char* q = (char*)__builtin_assume_aligned(d, 16);
        PT_TEX_UNROLL
        for (int k = 0; k < 3 * kTexRun / 2; k++) __builtin_memcpy(q + 16 * k, &v[2 * k], 16);   // one 16-B store each
    } else {
        PT_TEX_UNROLL
        for (int k = 0; k < 3 * kTexRun; k++)
            if (k < 3 * len) d[k] = v[k];
    }
}

}  // namespace pt
