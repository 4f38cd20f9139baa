// pt_refit.h — the arithmetic of pt_update_triangles, shared by the device kernels (pt_refit.hip) and the
// host (tests/native/refit_check.cpp drives the same functions leaves-then-levels): every function is
// `__host__ __device__ inline`, makes no HIP call and compiles with g++.  Build with -ffp-contract=off.
//
// A refit keeps the topology of the 8-wide quantized triangle BVH (pt_bvh.h Bvh8Result) and recomputes, from
// new vertices, what depends on coordinates:
//   refit_chunk  one leaf chunk: its triangles' 128-B shading records (rows 0-2 {v1, e1, e2} as pack_tri_geom
//                writes them, rows 3-5 the normals when given, the material word and the uv rows kept), the
//                chunk's geometry words, and the chunk's exact box: the union of its triangles' padded boxes
//                (pt_scene_compile.cpp tri_padded_box / pad_box: pad = max(|lo|, |hi|)·2.0e-6f + 1e-30f).
//   refit_node   one node, after every node below it: the children's exact boxes (node scratch for inner slots,
//                chunk scratch for leaf slots) requantized by refit_quantize, which the host builder calls too
//                (pt_bvh.cpp Wide8::emit, collapse_bvh8q: there is one quantizer): per
//                axis the origin is the least lower bound, the step 2^e the least power of two with every bound
//                within kRefitQMax steps (one more step when the outward rounding needs it), lower bounds
//                floored, upper bounds ceiled and clamped, empty slots +inf / -inf.  Words [3] bits 24-31 and
//                [4..7] are topology and stay.  The node's own exact box (origin, top) goes to the node scratch.
// The host builder quantizes BVH2 boxes that are exact unions of the padded triangle boxes, and min / max are
// exact and associative, so a refit with the vertices a scene was built from reproduces every byte.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif
#if defined(__clang__)
#define PT_REFIT_UNROLL _Pragma("unroll")
#else
#define PT_REFIT_UNROLL
#endif

namespace pt {

constexpr uint32_t kRefitQMax = 2047;   // child bounds as binary16 integers: 0..2047 are exact
constexpr int kRefitWords = 32;         // words per node, leaf chunk and shading record

struct alignas(16) RefitRow { uint32_t x, y, z, w; };   // one 16-B row: every store of a refit is one of these
__host__ __device__ inline uint32_t refit_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
__host__ __device__ inline float refit_float(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
__host__ __device__ inline RefitRow refit_row(float x, float y, float z, float w) {
    return RefitRow{refit_bits(x), refit_bits(y), refit_bits(z), refit_bits(w)};
}

// 2^e as a double, e in [-1022, 1023]
__host__ __device__ inline double refit_pow2(int e) {
    const uint64_t u = (uint64_t)(e + 1023) << 52;
    double d;
    __builtin_memcpy(&d, &u, 8);
    return d;
}
// an integer 0..2047 as binary16 bits (exact)
__host__ __device__ inline uint32_t refit_half_of_int(uint32_t q) {
    if (q == 0) return 0;
    const int e = 31 - __builtin_clz(q);
    return ((uint32_t)(e + 15) << 10) | ((q - (1u << e)) << (10 - e));
}

// pad_box (pt_scene_compile.cpp), each operation rounded on its own
__host__ __device__ inline void refit_pad_box(float* lo, float* hi) {
    for (int k = 0; k < 3; k++) {
        const float m = fmaxf(fabsf(lo[k]), fabsf(hi[k]));
        const float e = m * 2.0e-6f + 1e-30f;
        lo[k] = lo[k] - e;
        hi[k] = hi[k] + e;
    }
}
// tri_padded_box
__host__ __device__ inline void refit_tri_box(const float* v1, const float* v2, const float* v3, float* lo, float* hi) {
    for (int k = 0; k < 3; k++) {
        lo[k] = fminf(fminf(v1[k], v2[k]), v3[k]);
        hi[k] = fmaxf(fmaxf(v1[k], v2[k]), v3[k]);
    }
    refit_pad_box(lo, hi);
}
// pack_tri_geom: {v1, e1, e2}, e1 = v2 - v1 and e2 = v3 - v1 in fp32
__host__ __device__ inline void refit_tri_geom(const float* v1, const float* v2, const float* v3, float* g) {
    for (int k = 0; k < 3; k++) {
        g[k] = v1[k];
        g[3 + k] = v2[k] - v1[k];
        g[6 + k] = v3[k] - v1[k];
    }
}

// One leaf chunk `ci`.  chunks / recs: kRefitWords words per chunk / per BVH position; src_of_pos: the source
// triangle of each position; v1..n3: [num_triangles][3] in pt_scene_desc order (n1 NULL: the normals stay);
// chunk_box: 6 floats per chunk.  All indexing in 64 bits.
__host__ __device__ inline void refit_chunk(int64_t ci, uint32_t* chunks, uint32_t* recs, const int32_t* src_of_pos,
                                            const float* v1, const float* v2, const float* v3, const float* n1,
                                            const float* n2, const float* n3, float* chunk_box) {
    uint32_t* cw = chunks + ci * (int64_t)kRefitWords;
    const uint32_t w0 = cw[0];
    const int64_t first = (int64_t)(w0 & 0x1FFFFFFFu);
    const int cnt = (int)((w0 >> 29) & 3u) + 1;
    float line[kRefitWords];
    for (int k = 0; k < kRefitWords; k++) line[k] = 0.f;
    line[0] = refit_float(w0);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    PT_REFIT_UNROLL
    for (int t = 0; t < 3; t++) {
        if (t >= cnt) continue;
        const int64_t pos = first + t;
        const int64_t s = (int64_t)src_of_pos[pos];
        const float* a = v1 + 3 * s;
        const float* b = v2 + 3 * s;
        const float* c = v3 + 3 * s;
        float g[9], tl[3], th[3];
        refit_tri_geom(a, b, c, g);
        refit_tri_box(a, b, c, tl, th);
        for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], tl[k]); hi[k] = fmaxf(hi[k], th[k]); }
        for (int k = 0; k < 9; k++) line[1 + 9 * t + k] = g[k];
        RefitRow* r = (RefitRow*)(recs + pos * (int64_t)kRefitWords);
        r[0] = refit_row(g[0], g[1], g[2], g[3]);
        r[1] = refit_row(g[4], g[5], g[6], g[7]);
        r[2] = refit_row(g[8], 0.f, 0.f, 0.f);
        if (n1) {
            const float* p = n1 + 3 * s;
            const float* q = n2 + 3 * s;
            const float* u = n3 + 3 * s;
            const uint32_t mat = r[5].y;   // the material word stays
            r[3] = refit_row(p[0], p[1], p[2], q[0]);
            r[4] = refit_row(q[1], q[2], u[0], u[1]);
            r[5] = RefitRow{refit_bits(u[2]), mat, 0u, 0u};
        }
    }
    RefitRow* out = (RefitRow*)cw;
    PT_REFIT_UNROLL
    for (int k = 0; k < kRefitWords / 4; k++) out[k] = refit_row(line[4 * k], line[4 * k + 1], line[4 * k + 2], line[4 * k + 3]);
    float* cb = chunk_box + ci * 6;
    for (int k = 0; k < 3; k++) { cb[k] = lo[k]; cb[3 + k] = hi[k]; }
}

// Words 0-3 and 8-31 of a node from its nc children's exact boxes clo / chi ([8][3]); w3: the node's word 3, whose
// bits 24-31 stay.  The quantization of collapse_bvh8q (pt_bvh.cpp calls this); the lone-leaf root (one leaf child) takes the same form, since
// with one child the lower bound is the origin (q = 0) and the exponent search already bounds the upper one.
__host__ __device__ inline void refit_quantize(int nc, const float clo[8][3], const float chi[8][3], uint32_t w3,
                                               uint32_t out03[4], uint32_t out8[24], float box[6]) {
    uint32_t ebits = 0;
    for (int ax = 0; ax < 3; ax++) {
        float o = INFINITY, top = -INFINITY;
        for (int k = 0; k < 8; k++)
            if (k < nc) { o = fminf(o, clo[k][ax]); top = fmaxf(top, chi[k][ax]); }
        const double ext = (double)top - (double)o;
        int e = -126;
        while (e < 127 && (double)kRefitQMax * refit_pow2(e) < ext) e++;
        for (;;) {   // the outward rounding can need one more step
            bool ok = true;
            for (int k = 0; k < 8; k++)
                if (k < nc) ok = ok && ceil(((double)chi[k][ax] - (double)o) / refit_pow2(e)) <= (double)kRefitQMax;
            if (ok || e >= 127) break;
            e++;
        }
        const double step = refit_pow2(e);
        uint32_t ql[8], qh[8];
        for (int k = 0; k < 8; k++) {
            if (k >= nc) { ql[k] = 0x7C00u; qh[k] = 0xFC00u; continue; }   // +inf / -inf
            const double l = floor(((double)clo[k][ax] - (double)o) / step);
            const double h = ceil(((double)chi[k][ax] - (double)o) / step);
            ql[k] = refit_half_of_int((uint32_t)fmax(0.0, l));
            qh[k] = refit_half_of_int((uint32_t)fmin((double)kRefitQMax, fmax(0.0, h)));
        }
        for (int k = 0; k < 8; k += 2) {
            out8[8 * ax + k / 2] = ql[k] | (ql[k + 1] << 16);
            out8[8 * ax + 4 + k / 2] = qh[k] | (qh[k + 1] << 16);
        }
        out03[ax] = refit_bits(o);
        ebits |= (uint32_t)(e + 127) << (8 * ax);
        box[ax] = o;
        box[3 + ax] = top;
    }
    out03[3] = (w3 & 0xFF000000u) | ebits;
}

// One node `ni`, after every node of the levels below it.  nodes: kRefitWords words per node; node_box / chunk_box:
// 6 floats per node / chunk.
__host__ __device__ inline void refit_node(int64_t ni, uint32_t* nodes, float* node_box, const float* chunk_box) {
    uint32_t* w = nodes + ni * (int64_t)kRefitWords;
    const uint32_t w3 = w[3], w4 = w[4], w5 = w[5];
    const int nc = (int)(w3 >> 28), nin = (int)((w3 >> 24) & 15u);
    float clo[8][3], chi[8][3];
    for (int k = 0; k < 8; k++) {
        const bool used = k < nc, inner = k < nin;
        // every slot reads a valid box: an unused slot reads this node's first child again and is ignored
        const int kk = used ? k : 0;
        const bool in2 = used ? inner : nin > 0;
        const float* b = in2 ? node_box + ((int64_t)w4 + kk) * 6 : chunk_box + (int64_t)((w5 + (uint32_t)kk) & 0x7FFFFFFFu) * 6;
        for (int ax = 0; ax < 3; ax++) { clo[k][ax] = b[ax]; chi[k][ax] = b[3 + ax]; }
    }
    uint32_t o03[4], o8[24];
    float box[6];
    refit_quantize(nc, clo, chi, w3, o03, o8, box);
    RefitRow* r = (RefitRow*)w;
    r[0] = RefitRow{o03[0], o03[1], o03[2], o03[3]};
    for (int k = 0; k < 6; k++)
        r[2 + k] = RefitRow{o8[4 * k], o8[4 * k + 1], o8[4 * k + 2], o8[4 * k + 3]};
    float* nb = node_box + ni * 6;
    for (int k = 0; k < 6; k++) nb[k] = box[k];
}

}  // namespace pt
