// pt_skin.hip — the kernel of pt_skin_meshes (gfx950): linear blend skinning of the rest pose kept on the device, four
// (bone, weight) influences per corner, one matrix per bone per call, written where the refit kernels read their staged
// arrays.  The arithmetic is pt_skin.h's skin_triangle (shared with the host check).
//   k_skin_meshes  one lane per source triangle, a block of 256 lanes per tile of 256 triangles, at most kSkinMaxBlocks
//                  blocks striding over the tiles.  A lane reads its triangle's mesh (group[t], -1: a loose triangle,
//                  copied), the 18 rest floats, and for a mesh triangle the three index rows and three weight rows of
//                  its corners, and writes 18 floats.
// Lane mapping, by the access shape: every array is per corner and per triangle ([n][3] floats for v1..n3, [n][4] for a
// corner's indices and weights), so with a lane per triangle the 64 lanes of a wave abut in every one of them: a rest or
// output array moves as one 12-byte access per lane (768 contiguous bytes per wave-instruction, six whole 128-byte
// lines), a weight row as one 16-byte access (1024 bytes), an index row, kept as four 16-bit indices, as one 8-byte
// access (512 bytes).  Every byte is used once, by the lane that loaded it; nothing is re-shaped through LDS.  A lane
// per corner would cut each wave-instruction into three runs over three arrays, read group[t] three times, and buy
// only lanes the kernel has no use for: it streams 220 B per triangle and a frame of any size fills the chip with
// waves already.
// Where the matrices live: unlike a pose, the lanes of a wave read different bones, so the reads are gathers, not
// broadcasts.  Up to kSkinLdsBones bones, each block stages the 12 doubles per bone in LDS once, before its first tile,
// and the gathers are LDS reads; above, the rows are read from global memory (they stay in L2).  Both are
// instantiations of one kernel text (kLds).  kSkinLdsBones = 128 makes the table 12 KiB: eight blocks of 256 lanes,
// the 32 waves a CU can hold at all, take 96 KiB of its 160 KiB, so the table never decides how many blocks are
// resident (the next power of two, 24 KiB, would stop at six), and filling all of it costs a block a fifth of the
// 55 KiB one tile moves.  No other value has been measured.
// A dead influence (weight +-0) is skipped by a branch, not multiplied by zero: its matrix is never read.
// Every index is 64-bit; every store is a plain vector store to the lane's own triangle, made whatever
// the data is; no atomics.  The table fill is indexed by bone and bounded by num_bones; pt_set_skin checked every bone
// index against num_bones before it stored one, so no gather leaves the table or the matrix array; a lane past the
// last triangle leaves the loop before any load of a triangle.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_skin.h"

namespace pt {

constexpr int kSkinBlock = 256;
constexpr int kSkinLdsBones = 128;      // bones whose matrices fit the LDS table; above: read from global memory
constexpr int64_t kSkinMaxBlocks = 2048;

struct SkinArrays {
    const float* rest[6];       // v1 v2 v3 n1 n2 n3 of the rest pose, [n][3]
    float* out[6];              // the refit workspace's staged arrays
    const uint16_t* bone[3];    // per corner, [n][4]
    const float* weight[3];     // per corner, [n][4]
};

namespace {
struct __attribute__((packed, aligned(4))) SkinF3 { float x, y, z; };
struct __attribute__((aligned(8))) SkinB4 { uint16_t b[4]; };
struct __attribute__((aligned(16))) SkinW4 { float w[4]; };
}

template <bool kLds>
__global__ __launch_bounds__(kSkinBlock) void k_skin_meshes(int64_t n, int32_t num_bones, const int32_t* __restrict__ group,
                                                            const double* __restrict__ matrices, int normals, SkinArrays A) {
    __shared__ double s_rows[kLds ? kSkinLdsBones * 12 : 1];
    if (kLds) {
        for (int i = threadIdx.x; i < num_bones * 12; i += kSkinBlock) s_rows[i] = matrices[(int64_t)(i / 12) * 16 + i % 12];
        __syncthreads();
    }
    const int64_t tiles = (n + kSkinBlock - 1) / kSkinBlock;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t t = tile * kSkinBlock + threadIdx.x;
        if (t >= n) return;   // the last tile's tail (no barrier follows)
        const bool moved = group[t] >= 0;
        float in[18], out[18];
        for (int k = 0; k < 6; k++) {
            const SkinF3 a = *(const SkinF3*)(A.rest[k] + 3 * t);
            in[3 * k] = a.x;
            in[3 * k + 1] = a.y;
            in[3 * k + 2] = a.z;
        }
        uint16_t bones[3 * kSkinInfluences] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        float weights[3 * kSkinInfluences] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (moved) {
            for (int c = 0; c < 3; c++) {
                const SkinB4 b = *(const SkinB4*)(A.bone[c] + kSkinInfluences * t);
                const SkinW4 w = *(const SkinW4*)(A.weight[c] + kSkinInfluences * t);
                for (int k = 0; k < kSkinInfluences; k++) {
                    bones[kSkinInfluences * c + k] = b.b[k];
                    weights[kSkinInfluences * c + k] = w.w[k];
                }
            }
        }
        if (kLds) skin_triangle(s_rows, 12, moved, normals != 0, bones, weights, in, out);
        else skin_triangle(matrices, 16, moved, normals != 0, bones, weights, in, out);
        for (int k = 0; k < 6; k++) *(SkinF3*)(A.out[k] + 3 * t) = SkinF3{out[3 * k], out[3 * k + 1], out[3 * k + 2]};
    }
}

// The n rest triangles skinned into out[0..5] on `stream`: group [n], matrices [num_bones][16] row-major, a corner's
// bone rows [n][4] (every index below num_bones) and weight rows [n][4], all on the device; normals: the blend of
// MulDirection of the rest normals (else they are copied).
hipError_t launch_skin(int64_t n, int32_t num_bones, const int32_t* group, const double* matrices, bool normals,
                       const uint16_t* const bone[3], const float* const weight[3], const float* const rest[6], float* const out[6],
                       hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    SkinArrays A{};
    for (int k = 0; k < 6; k++) { A.rest[k] = rest[k]; A.out[k] = out[k]; }
    for (int c = 0; c < 3; c++) { A.bone[c] = bone[c]; A.weight[c] = weight[c]; }
    const int64_t tiles = (n + kSkinBlock - 1) / kSkinBlock;
    const dim3 grid((unsigned)(tiles < kSkinMaxBlocks ? tiles : kSkinMaxBlocks));
    if (num_bones <= kSkinLdsBones)
        hipLaunchKernelGGL(k_skin_meshes<true>, grid, dim3(kSkinBlock), 0, stream, n, num_bones, group, matrices, normals ? 1 : 0, A);
    else
        hipLaunchKernelGGL(k_skin_meshes<false>, grid, dim3(kSkinBlock), 0, stream, n, num_bones, group, matrices, normals ? 1 : 0, A);
    return hipGetLastError();
}

}  // namespace pt
