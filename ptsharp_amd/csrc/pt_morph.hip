// pt_morph.hip — the kernel of pt_morph_meshes (gfx950): morph targets (blend shapes) added to the rest pose kept on
// the device, one weight per target per call, written where the refit kernels read their staged arrays, or where
// k_skin_meshes reads its rest pose when the call also skins.  The arithmetic is pt_morph.h's
// morph_begin / morph_live / morph_add / morph_end (shared with the host check), the input pt_morph.h's packed layout.
//   k_morph_meshes  one lane per corner, one wave per slice (64 consecutive triangles of one corner array), a block of
//                   256 lanes per tile of four slices, at most kMorphMaxBlocks blocks striding over the tiles.  A lane
//                   reads its triangle's mesh (group[t], -1: a loose triangle, copied), its 12 rest bytes (24 with the
//                   normal), walks its slice's len[s] steps and writes its corner (and normal).
// Lane mapping, by the access shape: the deltas arrive sparse and by target; a scatter from there would need float
// atomics and an order.  Packed by corner instead, every lane owns one output element and adds its deltas in ascending
// target order, so the result is fixed.  Corners are numbered corner-major (c * n + t), so the 64 lanes of a wave abut
// in one of v1/v2/v3 (and n1/n2/n3): a 12-byte access per lane, 768 contiguous bytes per wave-instruction, as in the
// skin kernel.  A step of a slice is 64 16-bit targets (one 128-byte line) and 64 x 3 floats of deltas (six lines, six
// more with normal deltas), all on 128-byte boundaries: whole lines, read once.  The loop bound len[s] belongs to the
// wave (the slice index is made scalar with readfirstlane), so a wave does not diverge on it; a lane whose step is
// padding or whose target is dead skips that step's delta loads by a branch.
// Where the weights live: a gather by target.  Up to kMorphLdsTargets targets, each block stages them in LDS once,
// before its first tile; above, they are read from global memory (they stay in L2).  Both are instantiations of one
// kernel text (kLds).  kMorphLdsTargets = 4096 makes the table 16 KiB: eight blocks of 256 lanes, the 32 waves a CU can
// hold at all, take 128 KiB of its 160 KiB, so the table never decides how many blocks are resident (the next power of
// two, 32 KiB, would stop at five).  A block fills only num_targets entries.  It is a bound from that budget, not a
// tuned optimum: no other value has been measured.
// Every index is 64-bit; every store is a plain vector store to the lane's own element, made whatever
// the data is; no atomics.  The table fill is bounded by num_targets; pt_set_morph's packer stores only targets below
// num_targets or kMorphPad, so no gather leaves the table or the weight array; the planes hold 64 entries for every
// step, so a step's reads stay inside them for every lane; a lane past the last triangle of a ragged slice leaves
// before any load of a triangle (no barrier follows the fill).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_morph.h"

namespace pt {

constexpr int kMorphBlock = 256;
constexpr int kMorphLdsTargets = 4096;   // targets whose weights fit the LDS table; above: read from global memory
constexpr int64_t kMorphMaxBlocks = 2048;

struct MorphArrays {
    const float* rest[6];       // v1 v2 v3 n1 n2 n3 of the rest pose, [n][3]
    float* out[6];              // the refit workspace's staged arrays, or the composed call's intermediate buffer
    const int32_t* len;         // [slices]
    const int64_t* first;       // [slices]
    const uint16_t* target;     // [steps][64]
    const float* dpos;          // [steps][64][3]
    const float* dnrm;          // [steps][64][3], or NULL
};

namespace {
struct __attribute__((packed, aligned(4))) MorphF3 { float x, y, z; };
}

// normals: kMorphNormalsNone: n1..n3 are not written (a mode derives them afterwards); kMorphNormalsCopy: the rest
// normals are copied; kMorphNormalsBlend: they take the normal deltas (A.dnrm is set)
enum { kMorphNormalsNone = 0, kMorphNormalsCopy = 1, kMorphNormalsBlend = 2 };

template <bool kLds>
__global__ __launch_bounds__(kMorphBlock) void k_morph_meshes(int64_t n, int64_t per_corner, int32_t num_targets,
                                                              const int32_t* __restrict__ group, const float* __restrict__ weights,
                                                              int normals, MorphArrays A) {
    __shared__ float s_w[kLds ? kMorphLdsTargets : 1];
    if (kLds) {
        for (int i = threadIdx.x; i < num_targets; i += kMorphBlock) s_w[i] = weights[i];
        __syncthreads();
    }
    const float* w = kLds ? s_w : weights;
    const int lane = threadIdx.x % kMorphSlice;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kMorphSlice));
    constexpr int64_t kPerTile = kMorphBlock / kMorphSlice;
    const int64_t slices = 3 * per_corner, tiles = (slices + kPerTile - 1) / kPerTile;
    const bool blend = normals == kMorphNormalsBlend;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t s = tile * kPerTile + wave;
        if (s >= slices) continue;   // the last tile's tail, a whole wave
        const int64_t c = s / per_corner, t = (s - c * per_corner) * kMorphSlice + lane;
        if (t >= n) continue;        // a ragged slice's tail: no load of a triangle, no store
        const bool moved = group[t] >= 0;
        const MorphF3 p = *(const MorphF3*)(A.rest[c] + 3 * t);
        MorphF3 q{0.f, 0.f, 0.f};
        if (normals != kMorphNormalsNone) q = *(const MorphF3*)(A.rest[3 + c] + 3 * t);
        const float pin[3] = {p.x, p.y, p.z}, nin[3] = {q.x, q.y, q.z};
        MorphAcc acc;
        morph_begin(acc, pin, nin);
        const int64_t step0 = A.first[s], steps = A.len[s];
        if (moved)
            for (int64_t k = 0; k < steps; k++) {
                const int64_t e = (step0 + k) * kMorphSlice + lane;
                const uint16_t g = A.target[e];
                if (g == kMorphPad) continue;
                const float wt = w[g];
                if (!morph_live(wt)) continue;
                const MorphF3 d = *(const MorphF3*)(A.dpos + 3 * e);
                MorphF3 dn{0.f, 0.f, 0.f};
                if (blend) dn = *(const MorphF3*)(A.dnrm + 3 * e);
                const float dp[3] = {d.x, d.y, d.z}, dnv[3] = {dn.x, dn.y, dn.z};
                morph_add(acc, wt, dp, dnv, blend);
            }
        float po[3], no[3];
        morph_end(acc, blend, pin, nin, po, no);
        *(MorphF3*)(A.out[c] + 3 * t) = MorphF3{po[0], po[1], po[2]};
        if (normals != kMorphNormalsNone) *(MorphF3*)(A.out[3 + c] + 3 * t) = MorphF3{no[0], no[1], no[2]};
    }
}

// The n rest triangles morphed into out[0..5] on `stream`: group [n], weights [num_targets], the packed planes of
// pt_morph.h (len and first [3 * ceil(n / 64)]), all on the device.  normals: 0 leaves out[3..5] alone, 1 copies the
// rest normals, 2 blends them with dnrm (which must be set).
hipError_t launch_morph(int64_t n, int32_t num_targets, const int32_t* group, const float* weights, int normals, const int32_t* len,
                        const int64_t* first, const uint16_t* target, const float* dpos, const float* dnrm, const float* const rest[6],
                        float* const out[6], hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (normals == kMorphNormalsBlend && !dnrm) return hipErrorInvalidValue;
    MorphArrays A{};
    for (int k = 0; k < 6; k++) { A.rest[k] = rest[k]; A.out[k] = out[k]; }
    A.len = len;
    A.first = first;
    A.target = target;
    A.dpos = dpos;
    A.dnrm = dnrm;
    const int64_t per_corner = morph_slices_per_corner(n);
    const int64_t tiles = (3 * per_corner + kMorphBlock / kMorphSlice - 1) / (kMorphBlock / kMorphSlice);
    const dim3 grid((unsigned)(tiles < kMorphMaxBlocks ? tiles : kMorphMaxBlocks));
    if (num_targets <= kMorphLdsTargets)
        hipLaunchKernelGGL(k_morph_meshes<true>, grid, dim3(kMorphBlock), 0, stream, n, per_corner, num_targets, group, weights, normals, A);
    else
        hipLaunchKernelGGL(k_morph_meshes<false>, grid, dim3(kMorphBlock), 0, stream, n, per_corner, num_targets, group, weights, normals, A);
    return hipGetLastError();
}

}  // namespace pt
