// pt_pose.hip — the kernel of pt_pose_meshes (gfx950): Mesh.Transform of the rest pose kept on the device, one
// matrix per mesh, written where the refit kernels read their staged arrays.  The arithmetic is
// pt_pose.h's pose_triangle (shared with the host check).
//   k_pose_meshes  one lane per source triangle, a block of 256 lanes per tile of 256 triangles, at most kPoseMaxBlocks
//                  blocks striding over the tiles.  A lane reads its triangle's mesh (group[t], -1: a loose triangle),
//                  the mesh's mask word and matrix and the 18 rest floats, and writes 18 floats.
// Access shape: the arrays are [n][3] floats, so a lane's three floats of one array are 12 contiguous bytes and the 64
// lanes of a wave abut: each array is read with one 12-byte load per lane (global_load_dwordx3), a wave-instruction
// covering 768 contiguous bytes, six whole 128-byte lines, and written the same way.  Every byte is used once and by
// the lane that loaded it, so nothing is staged through LDS to re-shape it.
// Where the matrices live: neighbouring triangles share a mesh, so the lanes of a wave read the same 12 doubles.  A
// scene of at most kPoseLdsMeshes meshes keeps the rows (12 doubles per mesh) and the mask words in an LDS table that
// each block fills once, before its first tile; lanes of one mesh then read one address, a broadcast.  The table is
// 64 * (96 + 4) B = 6.25 KiB: a block's fill stays a sixth of the 37 KiB one tile moves, and the table never limits
// the blocks a CU holds.  A scene with more meshes reads the rows from global memory (they stay in L2).  Both are
// instantiations of one kernel text (kLds).
// Every index is 64-bit; every store is a plain vector store to the lane's own triangle, made whatever
// the data is; no atomics.  The table fill is indexed by mesh and bounded by num_meshes; a lane past the last triangle
// leaves the loop before any load of a triangle.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_pose.h"

namespace pt {

constexpr int kPoseBlock = 256;
constexpr int kPoseLdsMeshes = 64;      // meshes whose matrices fit the LDS table; above: read from global memory
constexpr int64_t kPoseMaxBlocks = 2048;

struct PoseArrays {
    const float* rest[6];   // v1 v2 v3 n1 n2 n3 of the rest pose, [n][3]
    float* out[6];          // the refit workspace's staged arrays
};

namespace {
struct __attribute__((packed, aligned(4))) PoseF3 { float x, y, z; };
}

template <bool kLds>
__global__ __launch_bounds__(kPoseBlock) void k_pose_meshes(int64_t n, int32_t num_meshes, const int32_t* __restrict__ group,
                                                            const int32_t* __restrict__ mask, const double* __restrict__ matrices,
                                                            int normals, PoseArrays A) {
    __shared__ double s_rows[kLds ? kPoseLdsMeshes * 12 : 1];
    __shared__ int32_t s_on[kLds ? kPoseLdsMeshes : 1];
    if (kLds) {
        for (int i = threadIdx.x; i < num_meshes * 12; i += kPoseBlock) s_rows[i] = matrices[(int64_t)(i / 12) * 16 + i % 12];
        for (int j = threadIdx.x; j < num_meshes; j += kPoseBlock) s_on[j] = mask ? (mask[j] != 0) : 1;
        __syncthreads();
    }
    const int64_t tiles = (n + kPoseBlock - 1) / kPoseBlock;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t t = tile * kPoseBlock + threadIdx.x;
        if (t >= n) return;   // the last tile's tail (no barrier follows)
        const int32_t g = group[t];
        bool moved = g >= 0 && g < num_meshes;
        double m[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (moved) {
            if (kLds) {
                moved = s_on[g] != 0;
                for (int i = 0; i < 12; i++) m[i] = s_rows[12 * g + i];
            } else {
                moved = !mask || mask[g] != 0;
                for (int i = 0; i < 12; i++) m[i] = matrices[(int64_t)g * 16 + i];
            }
        }
        float in[18], out[18];
        for (int k = 0; k < 6; k++) {
            const PoseF3 a = *(const PoseF3*)(A.rest[k] + 3 * t);
            in[3 * k] = a.x;
            in[3 * k + 1] = a.y;
            in[3 * k + 2] = a.z;
        }
        pose_triangle(m, moved, normals != 0, in, out);
        for (int k = 0; k < 6; k++) *(PoseF3*)(A.out[k] + 3 * t) = PoseF3{out[3 * k], out[3 * k + 1], out[3 * k + 2]};
    }
}

// The n rest triangles posed into out[0..5] on `stream`: group [n], matrices [num_meshes][16] row-major, mask
// [num_meshes] or NULL (all), all on the device; normals: MulDirection of the rest normals (else they are copied).
hipError_t launch_pose(int64_t n, int32_t num_meshes, const int32_t* group, const int32_t* mask, const double* matrices,
                       bool normals, const float* const rest[6], float* const out[6], hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    PoseArrays A{};
    for (int k = 0; k < 6; k++) { A.rest[k] = rest[k]; A.out[k] = out[k]; }
    const int64_t tiles = (n + kPoseBlock - 1) / kPoseBlock;
    const dim3 grid((unsigned)(tiles < kPoseMaxBlocks ? tiles : kPoseMaxBlocks));
    if (num_meshes <= kPoseLdsMeshes)
        hipLaunchKernelGGL(k_pose_meshes<true>, grid, dim3(kPoseBlock), 0, stream, n, num_meshes, group, mask, matrices,
                           normals ? 1 : 0, A);
    else
        hipLaunchKernelGGL(k_pose_meshes<false>, grid, dim3(kPoseBlock), 0, stream, n, num_meshes, group, mask, matrices,
                           normals ? 1 : 0, A);
    return hipGetLastError();
}

}  // namespace pt
