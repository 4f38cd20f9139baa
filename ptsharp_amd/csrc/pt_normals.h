// pt_normals.h — the arithmetic of pt_update_triangles_normals, shared by the device kernels (pt_normals.hip) and
// the host (tests/native/normals_check.cpp drives the same functions in the kernels' order): every function is
// `__host__ __device__ inline`, makes no HIP call and compiles with g++.  Build with -ffp-contract=off.
//
// The normals of moved triangles, from their positions alone:
//   normals_face     Triangle.Normal(): normalize(cross(V2 - V1, V3 - V1)), the fp32 sequence of pt_obj.cpp
//                    (sub, cross, normalize, each operation rounded on its own).
//   normals_key      what Mesh.SmoothNormals groups corners by: the corner's group (its mesh; kNormalsLoose for a
//                    triangle outside every mesh) and the three words of its position after `+ 0.f`, which
//                    makes -0 and +0 one key as Vector == does.  Keys are compared and ordered as raw words:
//                    only the grouping matters.
//   normals_segment  one position of the corners sorted by key, equal keys in corner order (3 * triangle + k,
//                    k = 0, 1, 2 for V1, V2, V3): the first corner of a run of equal keys sums the run's corner
//                    normals from (+0, +0, +0) in that order, normalises the sum and writes it to every corner of
//                    the run.  A run reads and writes only its own corners' slots, so runs are independent.
// A corner is a uint32 (3 * triangle + k): a caller keeps 3 * num_triangles below 2^31.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace pt {

constexpr uint32_t kNormalsLoose = 0;   // the group word of a triangle outside every mesh; mesh j is j + 1

struct NormalsKey { uint32_t g, x, y, z; };

__host__ __device__ inline uint32_t normals_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

// Vector.Normalize: len = sqrt((x·x + y·y) + z·z), then three divisions
__host__ __device__ inline void normals_normalize(float x, float y, float z, float* out) {
    const float len = sqrtf((x * x + y * y) + z * z);
    out[0] = x / len;
    out[1] = y / len;
    out[2] = z / len;
}

__host__ __device__ inline void normals_face(const float* v1, const float* v2, const float* v3, float* out) {
    const float ax = v2[0] - v1[0], ay = v2[1] - v1[1], az = v2[2] - v1[2];
    const float bx = v3[0] - v1[0], by = v3[1] - v1[1], bz = v3[2] - v1[2];
    normals_normalize(ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx, out);
}

// the group word of source triangle t: group[t] is its mesh, or -1
__host__ __device__ inline uint32_t normals_group_word(const int32_t* group, int64_t t) { return (uint32_t)(group[t] + 1); }

// the slot of corner c in the [n][3] arrays a1, a2, a3
__host__ __device__ inline const float* normals_corner(uint32_t c, const float* a1, const float* a2, const float* a3) {
    const int64_t t = (int64_t)(c / 3u);
    const uint32_t k = c - 3u * (uint32_t)t;
    return (k == 0 ? a1 : k == 1 ? a2 : a3) + 3 * t;
}
__host__ __device__ inline float* normals_corner(uint32_t c, float* a1, float* a2, float* a3) {
    return const_cast<float*>(normals_corner(c, (const float*)a1, (const float*)a2, (const float*)a3));
}

// Word w of corner c's key, the least significant first: 0 z, 1 y, 2 x, 3 the group
__host__ __device__ inline uint32_t normals_key_word(int w, uint32_t c, const int32_t* group, const float* v1, const float* v2,
                                                     const float* v3) {
    if (w == 3) return normals_group_word(group, (int64_t)(c / 3u));
    return normals_bits(normals_corner(c, v1, v2, v3)[2 - w] + 0.f);
}
__host__ __device__ inline NormalsKey normals_key(uint32_t c, const int32_t* group, const float* v1, const float* v2, const float* v3) {
    const float* p = normals_corner(c, v1, v2, v3);
    return NormalsKey{normals_group_word(group, (int64_t)(c / 3u)), normals_bits(p[0] + 0.f), normals_bits(p[1] + 0.f),
                      normals_bits(p[2] + 0.f)};
}
__host__ __device__ inline bool normals_same_key(const NormalsKey& a, const NormalsKey& b) {
    return a.g == b.g && a.x == b.x && a.y == b.y && a.z == b.z;
}
// the order the four stable passes over words 0..3 leave: by group, then x, y, z
__host__ __device__ inline bool normals_key_less(const NormalsKey& a, const NormalsKey& b) {
    if (a.g != b.g) return a.g < b.g;
    if (a.x != b.x) return a.x < b.x;
    if (a.y != b.y) return a.y < b.y;
    return a.z < b.z;
}

// Position i of `sorted` (total corners, ordered by key, equal keys in corner order).  n1..n3 hold the face normal
// of every triangle in all three arrays on entry; a run's corners hold the run's smooth normal on return.  Corners
// of loose triangles keep what they hold.
__host__ __device__ inline void normals_segment(int64_t i, int64_t total, const uint32_t* sorted, const int32_t* group,
                                                const float* v1, const float* v2, const float* v3, float* n1, float* n2,
                                                float* n3) {
    const NormalsKey key = normals_key(sorted[i], group, v1, v2, v3);
    if (key.g == kNormalsLoose) return;
    if (i > 0 && normals_same_key(key, normals_key(sorted[i - 1], group, v1, v2, v3))) return;   // not the run's first
    float sx = 0.f, sy = 0.f, sz = 0.f;
    int64_t end = i;
    do {
        const float* q = normals_corner(sorted[end], (const float*)n1, (const float*)n2, (const float*)n3);
        sx = sx + q[0];
        sy = sy + q[1];
        sz = sz + q[2];
        end++;
    } while (end < total && normals_same_key(key, normals_key(sorted[end], group, v1, v2, v3)));
    float s[3];
    normals_normalize(sx, sy, sz, s);
    for (int64_t j = i; j < end; j++) {
        float* q = normals_corner(sorted[j], n1, n2, n3);
        q[0] = s[0];
        q[1] = s[1];
        q[2] = s[2];
    }
}

}  // namespace pt
