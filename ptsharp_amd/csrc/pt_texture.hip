// pt_texture.hip — the kernel of pt_update_textures (gfx950): an 8-bit image decoded into its texture's slice of the
// scene's texel allocation through the host's 256-entry table.  The per-lane decode and every index
// are pt_texture.h's, shared with the host check.
//   k_tex_decode<BPP>  blocks of kTexBlock (256) lanes; each lane first stages one entry of the table in LDS (2 KiB, one
//                      8-B LDS store per lane, conflict-free), then decodes run `blockIdx.x * 256 + lane`: kTexRun (4)
//                      consecutive pixels.  Their 12 or 16 source bytes are loaded as whole dwords when the run starts on
//                      one (RGBA8 on a 16-B boundary: one 16-B load), their 12 table reads are 8-B LDS loads at the
//                      bytes' indices, and their 96 B of texels leave as six 16-B vector stores when the slice starts
//                      on a 16-B boundary: a wave covers 6 KiB contiguous.  Off those grids (an image packed behind an
//                      RGB8 image of odd size; a slice behind one of an odd number of doubles) and in an image's last,
//                      shorter run the lane goes byte by byte and double by double.
// The table's values are never computed here: no pow on the device, the doubles are the host's bit patterns.
// Every index and byte offset is 64-bit.  Plain vector stores only, one writer per word; no atomics.
// A lane past the last run loads and stores nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_texture.h"

namespace pt {

template <int BPP>
__global__ __launch_bounds__(kTexBlock) void k_tex_decode(const uint8_t* __restrict__ src, uint64_t src_off, uint64_t pixels,
                                                         const double* __restrict__ lut, double* __restrict__ dst) {
    __shared__ double s_lut[kTexLut];
    static_assert(kTexLut == kTexBlock, "one table entry per lane");
    s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const uint64_t run = (uint64_t)blockIdx.x * kTexBlock + threadIdx.x;
    if (run < tex_run_count(pixels)) tex_decode_run(src, src_off, BPP, run, pixels, s_lut, dst);
}

// One image of `pixels` pixels decoded on `stream`: its bytes at src + src_off (device), its table of 256 doubles at
// lut (device), its texels to dst (device, the texture's slice).  format: PT_TEXELS_RGB8 or PT_TEXELS_RGBA8.
hipError_t launch_tex_decode(const uint8_t* src, uint64_t src_off, int format, uint64_t pixels, const double* lut, double* dst,
                             hipStream_t stream) {
    if (pixels == 0) return hipSuccess;
    const uint64_t blocks = tex_block_count(pixels);
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;   // 2^41 pixels: no texture the scene could hold
    const dim3 grid((unsigned)blocks), block(kTexBlock);
    if (tex_bpp(format) == 4) hipLaunchKernelGGL((k_tex_decode<4>), grid, block, 0, stream, src, src_off, pixels, lut, dst);
    else hipLaunchKernelGGL((k_tex_decode<3>), grid, block, 0, stream, src, src_off, pixels, lut, dst);
    return hipGetLastError();
}

}  // namespace pt
