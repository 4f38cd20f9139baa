// pt_wavefront.hip — wavefront engine for PTSharp's render hot path on gfx950.
//
// The per-pixel megakernel (pt_render.hip) carries the whole sampler state and
// both traversal stacks in one kernel, which costs ~240 VGPRs (2 waves/SIMD).
// Here the recursion of DefaultSampler.sample (Sampler.cs:55-145) is unrolled
// by depth into queues in HBM:
//
//   k_wf_camera   camera samples → extension rays, depth 0      (Renderer.cs:294-305, Camera.cs:98-119)
//   k_wf_trace    closest hit for every queued ray               (Scene.Intersect, Scene.cs:75-79)
//   k_wf_shade    Hit.Info, emission, and every child of the vertex: Ray.Bounce →
//                 next-depth extension ray; sampleLights up to the shadow query
//                 (light choice, soft-shadow point, coverage) → shadow ray
//                                                                (Sampler.cs:62-131,191-296, Ray.cs:44-85)
//   k_wf_shadow   shadow visibility (nearest-hit == light ⇔ no primitive nearer
//                 than the light's own t: any-hit, early exit)   (Sampler.cs:261-265)
//   k_wf_nee_accum  the visible shadow rays' light terms, in slot order (Sampler.cs:119-127, 292-295)
//   k_wf_finalize per-pixel mean of the pass → Welford           (Renderer.cs:308-309, Buffer.cs:33-44)
//
// The traversal kernels keep only ray + stack state, so they run at the
// occupancy the LDS stack allows.  Queue appends are wave-aggregated atomics;
// per-pixel contributions (fp64, as the reference's Colour) go into order-independent
// fixed-point accumulators (pt_accum.h), so a pass gives the same bits on every run.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "pt_device.h"
#include "pt_wavefront.h"

#pragma clang fp contract(off)

namespace pt {

constexpr int kTB = 256;   // threads per block, traversal kernels (LDS stack column stride)
// Occupancy of the FULL instantiations (textures / SDF / volume / transformed shapes),
// measured with tools/bench_scenes.py: traversal at 4 waves (spilling past the 128-VGPR
// budget) beat 2/1 by 14-33 % on sdf_zoo / volume / transformed; 5-7 were slower on the
// SDF scene; shade is fastest at 2.
#ifndef PT_FULL_TRACE_WAVES
#define PT_FULL_TRACE_WAVES 4
#endif
#ifndef PT_FULL_SHADE_WAVES
#define PT_FULL_SHADE_WAVES 2
#endif
#ifndef PT_FULL_SHADOW_WAVES
#define PT_FULL_SHADOW_WAVES 4
#endif
// Rays a traversal wave claims per fetch atomic, in 64-ray batches.  A wave waits for its
// claim's return before tracing, and the 8 partition cursors are contended: claiming one
// batch at a time cost C4 trace 106 ms and shadow 47 ms per pass, four batches 82 and 42
// (eight: the same; sixteen: a longer tail).
constexpr uint32_t kFetchBatches = 4;
using WStack = SpillStack<kTB, kLdsStack>;

// Queue traffic.  Loads are non-temporal (read once per depth; they should not displace
// the BVH from L2 / the Infinity Cache).  Stores go through the default policy: a shade
// lane writes its children to consecutive slots, one 16-B field per store instruction,
// so a 128-B line is completed over several instructions; L2 write-combines them, while
// non-temporal stores sent the partial lines on (measured: k_wf_shade 67 → 43 ms/step).
typedef float f4v __attribute__((ext_vector_type(4)));
typedef unsigned int u4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void q_store(float4* p, float4 v) { *p = v; }
__device__ __forceinline__ void q_store(uint4* p, uint4 v) { *p = v; }
__device__ __forceinline__ void q_store(double2* p, double2 v) { *p = v; }
__device__ __forceinline__ void q_store(ulonglong2* p, ulonglong2 v) { *p = v; }
// Queue stores are non-temporal: with the child-major fill every store instruction writes whole
// lines, and keeping the streamed queues out of the caches helped k_wf_shade (C4 shade 29.9 → 28.2
// ms/step, 4963 → 5040 Mrays/s; only the data read two kernels later — throughput, key, light terms:
// 29.2 ms).  Hit records go through the default policy (non-temporal measured no better).
typedef float f4s __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void q_store_nt(double2* p, double2 v) {
    __builtin_nontemporal_store(__builtin_bit_cast(f4s, v), (f4s*)p);
}
__device__ __forceinline__ void q_store_nt(ulonglong2* p, ulonglong2 v) {
    __builtin_nontemporal_store(__builtin_bit_cast(f4s, v), (f4s*)p);
}
__device__ __forceinline__ void q_store_nt(float4* p, float4 v) {
    __builtin_nontemporal_store(__builtin_bit_cast(f4s, v), (f4s*)p);
}
template <class T>
__device__ __forceinline__ void q_store_late(T* p, T v) { q_store_nt(p, v); }
template <class T>
__device__ __forceinline__ void q_store_next(T* p, T v) { q_store_nt(p, v); }
__device__ __forceinline__ void hit_store(uint4* p, uint4 v) { q_store(p, v); }
__device__ __forceinline__ float4 nt_load(const float4* p) {
    f4v x = __builtin_nontemporal_load((const f4v*)p);
    return make_float4(x.x, x.y, x.z, x.w);
}
__device__ __forceinline__ uint4 nt_load(const uint4* p) {
    u4v x = __builtin_nontemporal_load((const u4v*)p);
    return make_uint4(x.x, x.y, x.z, x.w);
}
typedef double d2v __attribute__((ext_vector_type(2)));
typedef unsigned long long u2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 nt_load(const double2* p) {
    d2v x = __builtin_nontemporal_load((const d2v*)p);
    return make_double2(x.x, x.y);
}
__device__ __forceinline__ ulonglong2 nt_load(const ulonglong2* p) {
    u2v x = __builtin_nontemporal_load((const u2v*)p);
    return make_ulonglong2(x.x, x.y);
}

__device__ __forceinline__ uint32_t* ray_count(const WfQueues& Q, int q, int g) { return Q.counts + count_word(q * kParts + g); }
__device__ __forceinline__ uint32_t* nee_count(const WfQueues& Q, int q, int g) {
    return Q.counts + count_word(q * kParts + g) + 1;
}
__device__ __forceinline__ unsigned long long* pair_word(const WfQueues& Q, int q, int g) {
    return reinterpret_cast<unsigned long long*>(Q.counts + count_word(q * kParts + g));
}

// XCD group of this block (grids are multiples of kParts): group g = b % kParts,
// local block index lb, nb blocks per group.
struct Group {
    uint32_t g, lb, nb;
};
__device__ __forceinline__ Group xcd_group() {
    return Group{blockIdx.x % (uint32_t)kParts, blockIdx.x / (uint32_t)kParts, gridDim.x / (uint32_t)kParts};
}

__device__ __forceinline__ uint32_t append(uint32_t* counter) {
    return atomicAdd(counter, 1u);  // hipcc aggregates a uniform +1 into one atomic per wave
}

constexpr uint32_t kDead = 0xFFFFFFFFu;  // queue slot reserved for a child that was not cast
// Block-wide child-major fill (k_wf_shade) up to FirstHitSamples 16: ⌊√16⌋² strata × 2 modes.
constexpr int kBlockMajorFH = 16;
constexpr int kBlockMajorChildren = 32;
constexpr int32_t kDeadKind = -2;         // hit-record kind of a dead camera slot (k_wf_trace)
#ifndef PT_SHADE_LDS
#define PT_SHADE_LDS 1     // k_wf_shade reads a small scene's materials and lights from LDS (stage_shading)
#endif
#ifndef PT_SHADE_SCAN
#define PT_SHADE_SCAN 8    // rows of 256 per SCAN claim: 16 best before claims carried their partial round, 8 since
                           // (C4 5836 / 5885 / 5743 for 16 / 8 / 32; the 1/8 share 5099 / 5208 / 4735)
#endif
constexpr int kShadeScan = PT_SHADE_SCAN;   // 256-vertex groups a SCAN shade block claims and lists
// The environment may be textured (non-black per direction) only where the shade kernel
// runs its FULL instantiation; the traversal kernels see S.env_tex either way.
#define FULL_SHADE_ENV(S) ((S).env_tex >= 0)

__device__ __forceinline__ uint32_t wave_scan(uint32_t n, int lane) {  // inclusive
    uint32_t x = n;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    return x;
}

// Reserve a lane's a slots of one queue and b of another with ONE returning atomic
// per 256-thread block: the two counters are the halves of one 64-bit word (a
// returning atomic on one word saturates near 88 per µs on MI355X,
// MI355X_MICROARCH.md "dequeue"; per-wave reservation made k_wf_shade wait on it).
// Block-uniform call sites only.  Returns each lane's first slot in both queues.
// Optionally also returns the block's first slot in both queues (blk_a, blk_b).
__device__ __forceinline__ void block_reserve2(unsigned long long* word, uint32_t a, uint32_t b, uint32_t& abase,
                                               uint32_t& bbase, uint32_t* blk_a = nullptr, uint32_t* blk_b = nullptr) {
    __shared__ uint32_t s_tot[2][4];
    __shared__ uint32_t s_base[2][4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t xa = wave_scan(a, lane), xb = wave_scan(b, lane);
    if (lane == 63) { s_tot[0][wid] = xa; s_tot[1][wid] = xb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t ta = 0, tb = 0;
        for (int w = 0; w < 4; w++) {
            s_base[0][w] = ta; s_base[1][w] = tb;
            ta += s_tot[0][w]; tb += s_tot[1][w];
        }
        unsigned long long base = 0;
        if (ta | tb) base = atomicAdd(word, ((unsigned long long)tb << 32) | ta);
        for (int w = 0; w < 4; w++) {
            s_base[0][w] += (uint32_t)base;
            s_base[1][w] += (uint32_t)(base >> 32);
        }
    }
    __syncthreads();
    if (blk_a) { *blk_a = s_base[0][0]; *blk_b = s_base[1][0]; }
    abase = s_base[0][wid] + xa - a;
    bbase = s_base[1][wid] + xb - b;
}

// Throughput (fp64) rides in two 16-B fields: {r, g} and {key, b}.
__device__ __forceinline__ void ray_store(const WfQueues& Q, int q, uint32_t i, v3 o, v3 d, const double thr[3],
                                          uint32_t pixel, uint32_t meta, uint64_t key) {
    q_store_next(&Q.q_o[q][i], make_float4(o.x, o.y, o.z, __uint_as_float(pixel)));
    q_store_next(&Q.q_d[q][i], make_float4(d.x, d.y, d.z, __uint_as_float(meta)));
    q_store_late(&Q.q_t[q][i], make_double2(thr[0], thr[1]));
    q_store_late(&Q.q_k[q][i], make_ulonglong2(key, (unsigned long long)__double_as_longlong(thr[2])));
}
__device__ __forceinline__ void ray_store_camera(const WfQueues& Q, int q, uint32_t i, v3 o, v3 d, uint32_t pixel,
                                                 uint64_t key) {
    const double one[3] = {1.0, 1.0, 1.0};
    ray_store(Q, q, i, o, d, one, pixel, 0u | (1u << 8), key);
}

// ---------------------------------------------------------------- camera
// Camera samples go to the XCD partitions in runs of `run` 256-sample blocks (deal_run: one block,
// 16 pixels' samples, so every XCD touches every tile — the finest balance), the runs dealt
// round-robin.
__global__ __launch_bounds__(256) void k_wf_camera(DevCamera cam, DevPass P, WfQueues Q, uint64_t begin,
                                                   uint32_t count, int32_t spp_launch, int32_t sample_base) {
    // The deal is fixed, so each sample's queue slot is too: no slot needs an atomic (one
    // returning atomic per wave on the partition counters held this kernel to their
    // ~88-per-µs rate: 5.9 ms per C4 pass).  Samples of pixels outside the image (edge
    // tiles) leave dead slots that k_wf_trace and k_wf_shade skip.  Every run is whole blocks
    // (a tile's samples are a multiple of 256), and a chunk may start inside a run: the deal
    // counts blocks from the chunk's start.
    const Group G = xcd_group();
    const uint32_t run = deal_run(spp_launch);
    const uint32_t nblk = (count + 255u) / 256u;
    if (blockIdx.x == 0 && threadIdx.x < kParts) {
        const uint32_t g = threadIdx.x;
        // blocks of partition g: runs g, g + kParts, ... of `run` blocks, the last one cut at nblk
        const uint32_t nruns = (nblk + run - 1u) / run;
        uint32_t c = 0;
        if (g < nruns) {
            const uint32_t mine = (nruns - 1u - g) / kParts + 1u;   // runs of partition g
            c = mine * run;
            if ((nruns - 1u) % kParts == g) c -= nruns * run - nblk;   // the cut last run
            c *= 256u;
            if ((nblk - 1u) / run % kParts == g) c -= nblk * 256u - count;   // the chunk's partial last block
        }
        if (c > Q.pcap) { *Q.overflow = 1ull; c = Q.pcap; }
        *ray_count(Q, 0, g) = c;
    }
    // this block's share of partition G.g: local blocks lb, lb + nb, ...
    for (uint32_t lblk = G.lb;; lblk += G.nb) {
        const uint32_t blk = ((lblk / run) * kParts + G.g) * run + lblk % run;   // chunk block of local block lblk
        if (blk >= nblk) break;
        const uint32_t g = blk * 256u + threadIdx.x;   // chunk-relative sample
        if (g >= count) continue;
        const uint32_t local = lblk * 256u + threadIdx.x;
        if (local >= Q.pcap) continue;   // flagged above
        const uint32_t i = G.g * Q.pcap + local;
        const uint64_t slot = begin + g;
        uint64_t pslot;
        int s;
        if (slot <= 0xFFFFFFFFull) {   // 32-bit division whenever it fits (a 64-bit one is a long call)
            const uint32_t q = (uint32_t)slot / (uint32_t)spp_launch;
            pslot = q;
            s = (int)((uint32_t)slot - q * (uint32_t)spp_launch);
        } else {
            pslot = slot / (uint64_t)spp_launch;
            s = (int)(slot % (uint64_t)spp_launch);
        }
        // a batch of passes: pass p of the batch covers pixel slots p·num_tiles·1024 ..
        uint32_t bp = 0;
        if (P.passes > 1) {
            const uint64_t per = (uint64_t)P.num_tiles * 1024u;
            bp = (uint32_t)(pslot / per);
            pslot -= (uint64_t)bp * per;
        }
        const int tile_slot = (int)(pslot >> 10);
        const int tile = P.tiles ? P.tiles[tile_slot] : tile_slot;
        int x, y;
        tile_pixel(tile, (int)(pslot & 1023), P.tiles_x, x, y);
        if (x >= P.width || y >= P.height) {
            q_store(&Q.q_d[0][i], make_float4(0.f, 0.f, 0.f, __uint_as_float(kDead)));
            continue;
        }
        const int w = P.width, h = P.height;
        const uint64_t pix = (uint64_t)y * (uint64_t)w + (uint64_t)x;
        v3 o, d;
        uint64_t K;
        if (P.stratified) {
            const int sample = sample_base + s;
            const int root = (int)sqrt((double)P.spp);
            const int u = sample / root, v = sample % root;
            K = camera_key(P.seed, P.pass_index + bp, pix, (uint32_t)sample);
            cast_ray(cam, x, y, w, h, ((double)u + 0.5) / (double)root, ((double)v + 0.5) / (double)root, K, o, d);
        } else {
            K = camera_key(P.seed, P.pass_index + bp, pix, (uint32_t)s);
            double fu = (x + draw(K, D_JX)) / w;   // RenderParallel's jitter (Renderer.cs:297-302)
            double fv = (y + draw(K, D_JY)) / h;
            cast_ray(cam, x, y, w, h, fu, fv, K, o, d);
        }
        // the queue's "pixel" word is the accumulator the path's terms go to
        ray_store_camera(Q, 0, i, o, d, (uint32_t)pix + bp * P.acc_stride, K);
    }
}

// ---------------------------------------------------------------- closest hit
// Waves per SIMD of the lockstep traversal kernels (analytic scenes: gopher3 7 > 6) and of the
// per-lane refill kernels (C4: 5 / 6 / 7 / 8 measured, 6 best: 80 VGPRs and no spills in the
// step loop, closest hit 58.3 → 49.5 ms and shadow 25.2 → 22.1 ms per pass against 7).
#ifndef PT_LANES_WAVES
#define PT_LANES_WAVES 6
#endif
#ifndef PT_TRACE_WAVES
#define PT_TRACE_WAVES 7
#endif
// SPLIT (FULL only): the analytic half of a split closest hit (pt_device.h trace_ana): the refill
// kernel left the planes' and triangles' hit in Q.hits; this pass adds the analytic BVH's.
template <bool COUNT, bool FULL, bool SPLIT = false>
__global__ __launch_bounds__(kTB, FULL ? PT_FULL_TRACE_WAVES : PT_TRACE_WAVES) void k_wf_trace(DevScene S, WfQueues Q, int qi, unsigned long long* counters) {
    __shared__ uint32_t s_stack[kLdsStack * kTB];
    const WStack stack{s_stack + threadIdx.x, Q.ovf + blockIdx.x * kTB + threadIdx.x, gridDim.x * kTB};
    if (!SPLIT && blockIdx.x == 0 && threadIdx.x < kParts) {
        *pair_word(Q, 1 - qi, threadIdx.x) = 0ull;              // consumed: free for k_wf_shade's output
        Q.counts[fetch_word(1, threadIdx.x)] = 0u;               // k_wf_shade's fetch cursors
        Q.counts[fetch_word(7, threadIdx.x)] = 0u;               // (the FULL one's of a routed shade)
    }
    const Group G = xcd_group();
    const bool route = SPLIT && S.route;   // the heavy queue's rays only (the refill half finished the others)
    const uint32_t cnt = route ? Q.counts[heavy_word((int)G.g)] : *ray_count(Q, qi, G.g);
    const uint32_t n = cnt < Q.pcap ? cnt : Q.pcap, base = G.g * Q.pcap;
    uint32_t* cursor = Q.counts + fetch_word(SPLIT ? 4 : 0, G.g);
    const uint32_t lane = threadIdx.x & 63;
    Counters ctr{0, 0, 0, 0};
    const bool env_black = (!FULL_SHADE_ENV(S)) && S.env[0] == 0.f && S.env[1] == 0.f && S.env[2] == 0.f;
    uint32_t kept = 0;   // rays with work for k_wf_shade (its SCAN choice)
    // Persistent grid (resident capacity); each wave claims kFetchBatches × 64 rays of
    // its partition with one atomic and traces them 64 at a time, so no wave waits for a
    // second dispatch round and the tail is a few traversals long.
    for (;;) {
        uint32_t kc = 0;
        if (lane == 0) kc = atomicAdd(cursor, 64u * kFetchBatches);
        kc = __shfl(kc, 0, 64);
        if (kc >= n) break;
        for (uint32_t k0 = kc; k0 < kc + 64u * kFetchBatches && k0 < n; k0 += 64u) {
            if (k0 + lane >= n) continue;
            const uint32_t i = route ? Q.hq[base + k0 + lane] : base + k0 + lane;
            // both queue loads before the dead test: one round trip per ray, not two (the pin keeps the
            // compiler from sinking the origin's load behind the test)
            float4 b = nt_load(&Q.q_d[qi][i]);
            float4 a = nt_load(&Q.q_o[qi][i]);
            PT_PIN44(b, a);
            if (__float_as_uint(b.w) == kDead) {   // a camera slot outside the image: k_wf_shade skips it
                hit_store(&Q.hits[i], make_uint4(0u, 0u, (uint32_t)kDeadKind, 0u));
                continue;
            }
            HitRec h;
            if constexpr (SPLIT) {
                const uint4 r = Q.hits[i];   // the planes' and triangles' hit (k_wf_trace_lanes, split)
                h.t = __longlong_as_double((long long)(((unsigned long long)r.y << 32) | r.x));
                h.kind = (int32_t)r.z;
                h.idx = (int32_t)r.w;
                h.tx = h.t;
                int32_t sdf = -1, vol = -1;
                int32_t* const vol_out = Q.volq ? &vol : nullptr;   // Volumes deferred to k_wf_vol_hits
                if (route) trace_heavy<COUNT>(S, v3{a.x, a.y, a.z}, v3{b.x, b.y, b.z}, ctr, h, &sdf, vol_out);
                else trace_ana<COUNT>(S, v3{a.x, a.y, a.z}, v3{b.x, b.y, b.z}, stack, ctr, h, &sdf, vol_out);
                {   // k_wf_vol_hits and k_wf_sdf_hits trace them, every lane busy (the active lanes append here)
                    const bool defer = sdf >= 0 || vol >= 0;
                    const uint64_t m = __ballot(defer);
                    if (m) {
                        const int lead = __builtin_ctzll(m);
                        uint32_t at = 0;
                        if ((int)lane == lead) at = atomicAdd(Q.counts + kSdfWord, (uint32_t)__popcll(m));
                        at = (uint32_t)__shfl((int)at, lead, 64) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                        if (defer && at < Q.cap) {
                            const unsigned long long tb = (unsigned long long)__double_as_longlong(h.t);
                            Q.sdfq[at] = make_uint4(i, (uint32_t)sdf, (uint32_t)tb, (uint32_t)(tb >> 32));
                            if (Q.volq) Q.volq[at] = (uint32_t)vol;
                        } else if (defer) {
                            *Q.overflow = 1ull;   // a dropped entry would lose the hit: the pass reports it
                        }
                    }
                }
            } else {
                h = trace<COUNT, FULL>(S, v3{a.x, a.y, a.z}, v3{b.x, b.y, b.z}, stack, ctr);
            }
            kept += (h.kind >= 0 || !env_black) ? 1u : 0u;
            // a TransformedShape hit keeps its inner object-space t, what Hit.Info needs (HitRec::tx)
            unsigned long long tb = (unsigned long long)__double_as_longlong(FULL && h.kind == KIND_XFORM ? h.tx : h.t);
            hit_store(&Q.hits[i], make_uint4((uint32_t)tb, (uint32_t)(tb >> 32), (uint32_t)h.kind, (uint32_t)h.idx));
        }
    }
    uint32_t rays = wave_sum(ctr.rays);
    if (lane == 0 && rays) atomicAdd(&counters[0], (unsigned long long)rays);
    kept = wave_sum(kept);
    if (lane == 0 && kept) atomicAdd(Q.counts + kept_word(qi), kept);
    if (COUNT) {
        uint32_t nodes = wave_sum(ctr.nodes), prims = wave_sum(ctr.prims);
        if (lane == 0) {
            atomicAdd(&counters[1], (unsigned long long)nodes);
            atomicAdd(&counters[2], (unsigned long long)prims);
        }
    }
}

// Closest hit and shadow visibility of the scenes whose shapes are a few analytic records and planes with no
// triangle BVH (lean, DevScene::ana_linear, tri_num_nodes 0: C2's gopher3).  k_wf_trace / k_wf_shadow ran them
// through the general lockstep traversal, whose registers (stack, BVH state) held them at 7 waves, parked on
// their queue loads 72 % of their wave time (profiles/r06q_wave_states.txt).  Here a ray is its queue entry
// and the record tests (trace_linear / light_visible_linear: the same tests in the same order, so the same
// results), and each wave loads its next row of 64 entries before it tests the current one.  Static deal:
// wave w of the partition's group takes rows w, w + W, ... (every ray costs the same tests).
struct LinRay { float4 b, a; };   // the queue entry: q_d / n_n and q_o / n_o
// The records and planes in LDS (at most kLinRecs / kLinPlanes, pt_pass_plan.h: the launch checks), read by every
// ray's tests: from global memory the compiler issued them as vector loads per ray (it cannot prove them unwritten).
struct LinScene { const float4* recs; const float4* planes; };
__device__ __forceinline__ LinScene stage_linear(const DevScene& S) {   // block-uniform call
    __shared__ float4 s_rec[3 * kLinRecs];
    __shared__ float4 s_pl[2 * kLinPlanes];
    for (uint32_t k = threadIdx.x; k < 3u * (uint32_t)S.ana_count; k += blockDim.x) s_rec[k] = S.ana_recs[k];
    for (uint32_t k = threadIdx.x; k < 2u * (uint32_t)S.num_planes; k += blockDim.x) s_pl[k] = S.planes[k];
    __syncthreads();
    return LinScene{s_rec, s_pl};
}
__device__ __forceinline__ LinRay lin_fetch(const float4* qb, const float4* qa, uint32_t base, uint32_t k, uint32_t n) {
    LinRay x;
    if (k < n) {
        x.b = nt_load(qb + base + k);
        x.a = nt_load(qa + base + k);
    } else {
        x.b = make_float4(0.f, 0.f, 0.f, __uint_as_float(kDead));
        x.a = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return x;
}
template <bool COUNT>
__global__ __launch_bounds__(256, 8) void k_wf_trace_linear(DevScene S, WfQueues Q, int qi, unsigned long long* counters) {
    if (blockIdx.x == 0 && threadIdx.x < kParts) {   // as k_wf_trace
        *pair_word(Q, 1 - qi, threadIdx.x) = 0ull;
        Q.counts[fetch_word(1, threadIdx.x)] = 0u;
        Q.counts[fetch_word(7, threadIdx.x)] = 0u;
    }
    const Group G = xcd_group();
    const uint32_t n = min(*ray_count(Q, qi, G.g), Q.pcap), base = G.g * Q.pcap;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t W = G.nb * 4u;
    Counters ctr{0, 0, 0, 0};
    const bool env_black = (!FULL_SHADE_ENV(S)) && S.env[0] == 0.f && S.env[1] == 0.f && S.env[2] == 0.f;
    uint32_t kept = 0;
    const LinScene L = stage_linear(S);
    uint32_t r = G.lb * 4u + (threadIdx.x >> 6);
    LinRay cur = lin_fetch(Q.q_d[qi], Q.q_o[qi], base, r * 64u + lane, n);
    for (; r * 64u < n; r += W) {   // wave-uniform
        const LinRay nxt = lin_fetch(Q.q_d[qi], Q.q_o[qi], base, (r + W) * 64u + lane, n);
        const uint32_t k = r * 64u + lane;
        if (k < n) {
            const uint32_t i = base + k;
            if (__float_as_uint(cur.b.w) == kDead) {   // a camera slot outside the image: k_wf_shade skips it
                hit_store(&Q.hits[i], make_uint4(0u, 0u, (uint32_t)kDeadKind, 0u));
            } else {
                const HitRec h = trace_linear<COUNT>(S, L.recs, L.planes, v3{cur.a.x, cur.a.y, cur.a.z},
                                                     v3{cur.b.x, cur.b.y, cur.b.z}, ctr);
                kept += (h.kind >= 0 || !env_black) ? 1u : 0u;
                const unsigned long long tb = (unsigned long long)__double_as_longlong(h.t);
                hit_store(&Q.hits[i], make_uint4((uint32_t)tb, (uint32_t)(tb >> 32), (uint32_t)h.kind, (uint32_t)h.idx));
            }
        }
        cur = nxt;
    }
    uint32_t rays = wave_sum(ctr.rays);
    if (lane == 0 && rays) atomicAdd(&counters[0], (unsigned long long)rays);
    kept = wave_sum(kept);
    if (lane == 0 && kept) atomicAdd(Q.counts + kept_word(qi), kept);
    if (COUNT) {
        const uint32_t prims = wave_sum(ctr.prims);
        if (lane == 0) atomicAdd(&counters[2], (unsigned long long)prims);
    }
}

// Closest hit with per-lane refill (lean scenes: no §8f row 4 shapes).  k_wf_trace runs
// 64 rays in lockstep until the longest is done: ~10 of 64 lanes are active per node
// fetch, and every fetch instruction pays the texture-address unit's fixed cost.  Here
// each lane keeps one ray in flight through ONE step loop: a step is one node (or leaf)
// of the analytic BVH or of the triangle BVH (the same seven-load 128-B fetch), the
// analytic phase hands over to the triangle phase at an empty stack, and a lane whose ray
// is done takes the next one when PT_REFILL_IDLE lanes of the wave are idle (one claim
// atomic per refill).  A new ray's head work is two queue loads and the planes (none in
// C4), so a refill holds the busy lanes for one load round trip.  Same visit order,
// same arithmetic as trace(): bit-identical hits.
#ifndef PT_VOL_WAVES
#define PT_VOL_WAVES 4   // the cooperative march needs ~130 VGPRs (5 / 6 / 8 waves: 37-146 spilled)
#endif
// The Volume records the analytic half of a split closest hit deferred (trace_ana / trace_heavy
// vol_out), merged before the entry's SDF record (k_wf_sdf_hits then reads the t this kernel lowered:
// the traversal's order, the Volume's march before the SDF).  A wave takes 64 entries and marches their
// Volumes one at a time with all its lanes (march_pending, the cooperative march), in a kernel that
// holds nothing else and so runs more waves than the FULL kernel that found them.
// The scene's one Volume staged in this block's LDS (DevScene::vol_lds > 0): its DevVolume, its windows and its
// uniform-cell table, so the march's table reads, window loop and the volume's fields are LDS reads (flat loads of
// LDS addresses) instead of L1 / L2 round trips; the grid's corners stay in HBM.  Returns the scene view that reads
// them there.  Block-uniform call.
static_assert(sizeof(DevVolume) <= kVolLdsHeader, "stage_vol's header");
__device__ __forceinline__ DevScene stage_vol(const DevScene& S) {
    extern __shared__ __align__(16) unsigned char s_vol[];
    DevScene V = S;
    const DevVolume src = S.volumes[0];
    DevVolume* hv = reinterpret_cast<DevVolume*>(s_vol);
    DevWindow* win = reinterpret_cast<DevWindow*>(s_vol + kVolLdsHeader);
    const uint32_t nwin_b = ((uint32_t)src.nwin * (uint32_t)sizeof(DevWindow) + 15u) & ~15u;
    int8_t* runs = reinterpret_cast<int8_t*>(s_vol + kVolLdsHeader + nwin_b);
    const uint32_t nr = (uint32_t)((src.w + 1) * (src.h + 1) * (src.d + 1));
    for (uint32_t k = threadIdx.x; k < nr; k += blockDim.x) runs[k] = src.runs[k];
    for (uint32_t k = threadIdx.x; k < (uint32_t)src.nwin; k += blockDim.x) win[k] = src.windows[k];
    if (threadIdx.x == 0) {
        DevVolume v = src;
        v.windows = win;
        v.runs = runs;
        *hv = v;
    }
    __syncthreads();
    V.volumes = hv;
    return V;
}
template <bool STAGED, bool COUNT>
__global__ __launch_bounds__(256, PT_VOL_WAVES) void k_wf_vol_hits(DevScene S0, WfQueues Q, int qi) {
    const DevScene S = STAGED ? stage_vol(S0) : S0;
    const uint32_t n = min(Q.counts[kSdfWord], Q.cap);
    const bool env_black = S.env_tex < 0 && S.env[0] == 0.f && S.env[1] == 0.f && S.env[2] == 0.f;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
    uint32_t gained = 0;   // misses that became hits: rays with work for k_wf_shade (kept_word)
    for (uint32_t k0 = w * 64u; k0 < n; k0 += nw * 64u) {   // wave-uniform: every lane takes part in the march
        const uint32_t k = k0 + lane;
        int32_t pend = k < n ? (int32_t)Q.volq[k] : -1;
        if (__ballot(pend >= 0) == 0ull) continue;
        uint4 e = make_uint4(0u, 0u, 0u, 0u);
        HitRec best{kHitInf, -1, -1};
        v3 o{0.f, 0.f, 0.f}, d{0.f, 0.f, 0.f};
        if (pend >= 0) {
            e = Q.sdfq[k];
            const uint4 hr = Q.hits[e.x];
            best.t = __longlong_as_double((long long)(((unsigned long long)e.w << 32) | e.z));
            best.kind = (int32_t)hr.z;
            best.idx = (int32_t)hr.w;
            const float4 a = nt_load(&Q.q_o[qi][e.x]), b = nt_load(&Q.q_d[qi][e.x]);
            o = v3{a.x, a.y, a.z};
            d = v3{b.x, b.y, b.z};
        }
        const int32_t kind0 = best.kind;
        march_coop<false, true, COUNT>(S, o, d, pend, best, nullptr);
        if (pend >= 0 && best.idx == pend && (best.kind == KIND_VOLUME || best.kind == KIND_XFORM)) {   // nearer
            const unsigned long long tb = (unsigned long long)__double_as_longlong(best.kind == KIND_XFORM ? best.tx : best.t);
            hit_store(&Q.hits[e.x], make_uint4((uint32_t)tb, (uint32_t)(tb >> 32), (uint32_t)best.kind, (uint32_t)pend));
            const unsigned long long tw = (unsigned long long)__double_as_longlong(best.t);
            Q.sdfq[k] = make_uint4(e.x, e.y, (uint32_t)tw, (uint32_t)(tw >> 32));   // the SDF kernel's bound
            gained += (kind0 < 0 && env_black) ? 1u : 0u;
        }
    }
    gained = wave_sum(gained);
    if (lane == 0 && gained) atomicAdd(Q.counts + kept_word(qi), gained);
}
// The Volume records split shadow rays deferred: blocked (unlit) when the march's t is nearer than
// the light; k_wf_sdf_shadow then skips the ray.
template <bool STAGED, bool COUNT>
__global__ __launch_bounds__(256, PT_VOL_WAVES) void k_wf_vol_shadow(DevScene S0, WfQueues Q, int qo) {
    const DevScene S = STAGED ? stage_vol(S0) : S0;
    const uint32_t n = min(Q.counts[sdf_sh_word(qo)], Q.s_cap);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t k0 = w * 64u; k0 < n; k0 += nw * 64u) {   // wave-uniform
        const uint32_t k = k0 + lane;
        int32_t pend = k < n ? (int32_t)Q.volq_sh[k] : -1;
        if (__ballot(pend >= 0) == 0ull) continue;
        uint4 e = make_uint4(0u, 0u, 0u, 0u);
        HitRec best{kHitInf, -1, -1};
        v3 o{0.f, 0.f, 0.f}, d{0.f, 0.f, 0.f};
        if (pend >= 0) {
            e = Q.sdfq_sh[k];
            best.t = __longlong_as_double((long long)(((unsigned long long)e.w << 32) | e.z));   // the light's t
            const float4 a = nt_load(&Q.n_o[qo][e.x]), b = nt_load(&Q.n_n[qo][e.x]);
            o = v3{a.x, a.y, a.z};
            d = v3{b.x, b.y, b.z};
        }
        bool blocked = false;
        march_coop<true, true, COUNT>(S, o, d, pend, best, &blocked);
        if (pend >= 0 && blocked) Q.n_lit[qo][e.x] = 0;
    }
}

// The SDF programs (instructions, then parameters: DevSdfIns is 8 B) staged in this block's LDS when
// small (DevScene::sdf_lds): the march reads an instruction and its parameters at every step, one
// address for the wave (one shape), from LDS instead of through the vector L1.  Returns the scene
// view that reads them there.  Block-uniform call, STAGED kernels only.
static_assert(sizeof(DevSdfIns) == 8, "stage_sdf copies 8-B words");
__device__ __forceinline__ DevScene stage_sdf(const DevScene& S) {
    extern __shared__ __align__(16) unsigned char s_sdf[];
    DevScene V = S;
    const uint32_t words = (uint32_t)S.sdf_lds / 8u;
    const unsigned long long* prog = reinterpret_cast<const unsigned long long*>(S.sdf_prog);
    const uint32_t pn = (uint32_t)S.sdf_prog_n;   // program entries (8 B each), then the parameters
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(s_sdf);
    for (uint32_t k = threadIdx.x; k < words; k += blockDim.x)
        dst[k] = k < pn ? prog[k] : reinterpret_cast<const unsigned long long*>(S.sdf_params)[k - pn];
    __syncthreads();
    V.sdf_prog = reinterpret_cast<const DevSdfIns*>(s_sdf);
    V.sdf_params = reinterpret_cast<const double*>(s_sdf + (size_t)pn * sizeof(DevSdfIns));
    return V;
}

// The SDF records the analytic half of a split closest hit queued: one lane per
// entry, so SDFShape's sphere tracing (up to 1000 dependent steps) runs with every lane busy
// instead of with the few lanes of a wave whose rays reach the shape.  Merged into the hit record
// as the traversal would have: nearer wins, and an equal t beats a triangle (the analytic BVH
// precedes the triangles in Scene.Intersect).  One entry per ray: no two lanes write one record.
template <bool STAGED>
__global__ __launch_bounds__(256, PT_FULL_TRACE_WAVES) void k_wf_sdf_hits(DevScene S0, WfQueues Q, int qi) {
    const DevScene S = STAGED ? stage_sdf(S0) : S0;
    const uint32_t n = min(Q.counts[kSdfWord], Q.cap);
    const bool env_black = S.env_tex < 0 && S.env[0] == 0.f && S.env[1] == 0.f && S.env[2] == 0.f;
    uint32_t gained = 0;   // misses that became hits: rays with work for k_wf_shade (kept_word)
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        const uint4 e = Q.sdfq[k];
        if (e.y == kNoRecord) continue;   // a Volume-only entry (k_wf_vol_hits)
        const uint32_t i = e.x;
        const double bt = __longlong_as_double((long long)(((unsigned long long)e.w << 32) | e.z));
        const float4 a = nt_load(&Q.q_o[qi][i]), b = nt_load(&Q.q_d[qi][i]);
        int32_t kind;
        double tx = 0;
        const double t = sdf_record_t(S, e.y, v3{a.x, a.y, a.z}, v3{b.x, b.y, b.z}, kind, tx);
        const int32_t hk = (int32_t)Q.hits[i].z;
        if (t < bt || (t == bt && hk == KIND_TRI)) {
            const unsigned long long tb = (unsigned long long)__double_as_longlong(kind == KIND_XFORM ? tx : t);
            hit_store(&Q.hits[i], make_uint4((uint32_t)tb, (uint32_t)(tb >> 32), (uint32_t)kind, e.y));
            gained += (hk < 0 && env_black) ? 1u : 0u;
        }
    }
    gained = wave_sum(gained);
    if ((threadIdx.x & 63) == 0 && gained) atomicAdd(Q.counts + kept_word(qi), gained);
}

// The SDF records the analytic half of split shadow rays queued: one lane per
// entry; a ray whose SDF is strictly nearer than its light is blocked.
template <bool STAGED>
__global__ __launch_bounds__(256, PT_FULL_TRACE_WAVES) void k_wf_sdf_shadow(DevScene S0, WfQueues Q, int qo) {
    const DevScene S = STAGED ? stage_sdf(S0) : S0;
    const uint32_t n = min(Q.counts[sdf_sh_word(qo)], Q.s_cap);
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        const uint4 e = Q.sdfq_sh[k];
        if (e.y == kNoRecord || Q.n_lit[qo][e.x] == 0) continue;   // Volume-only, or blocked by its Volume
        const double tl = __longlong_as_double((long long)(((unsigned long long)e.w << 32) | e.z));
        const float4 a = nt_load(&Q.n_o[qo][e.x]), b = nt_load(&Q.n_n[qo][e.x]);
        int32_t kind;
        double tx = 0;
        if (sdf_record_t(S, e.y, v3{a.x, a.y, a.z}, v3{b.x, b.y, b.z}, kind, tx) < tl) Q.n_lit[qo][e.x] = 0;
    }
}

// The register budget of the per-lane refill kernels: 512 / waves, rounded down to 8, pinned
// explicitly (the compiler would size it for the occupancy it computes from LDS).
#define PT_LANES_VGPRS ((512 / PT_LANES_WAVES) & ~7)

// Does the ray reach the triangle BVH at all (its root box within tmax)?  A child box lies inside
// the root box and the fp32 slab arithmetic is monotone in the bounds, so a miss here is a miss of
// every root child: skipping the root step changes no hit, only the step count.
__device__ __forceinline__ bool tri_reach(const DevScene& S, v3 o, v3 invd, float tmax) {
    if (S.tri_num_nodes <= 0) return false;
    return slab1(S.tri_box[0], S.tri_box[3], S.tri_box[1], S.tri_box[4], S.tri_box[2], S.tri_box[5], o, invd, tmax) !=
           __int_as_float(0x7f800000);
}

#ifndef PT_REFILL_IDLE
#define PT_REFILL_IDLE 40   // closest hit: 8 / 16 / 24 / 32 / 40 / 48 measured on C4, 40 best
#endif
#ifndef PT_SHADOW_REFILL_IDLE
#define PT_SHADOW_REFILL_IDLE 32   // shadow: 16 / 24 / 32 / 48 measured, 32 best
#endif
// The list-fed forms (every refilled ray traverses, and a refill is cheaper): thresholds of their own, and the
// list positions a wave claims per cursor atomic (a refill inside a claim is the list read and then the ray's
// loads, no atomic).  Measured on C4, closest-hit / shadow class ms per step: closest hit
// 12 / 16 / 20 / 24 / 28 / 32 / 40 / 48 idle lanes: 43.7 / 43.1 / 42.9 / 43.0 / 43.4 / 43.8 / 44.6 / 46.9; shadow
// 8 / 16 / 24 / 32 / 48: 17.6 / 17.2 / 17.3 / 17.6 / 19.6; closest-hit claims of 64 / 128 / 256 / 512 / 1024
// positions: 46.5 (at 40 idle) / 42.9 / 43.0 / 43.5 / 46.4 (at 40 idle); shadow claims of 64 / 128 / 256: 17.0 / 16.9 / 17.2.
#ifndef PT_LIST_REFILL_IDLE
#define PT_LIST_REFILL_IDLE 24
#endif
#ifndef PT_LIST_SHADOW_REFILL_IDLE
#define PT_LIST_SHADOW_REFILL_IDLE 16
#endif
#ifndef PT_LIST_CLAIM
#define PT_LIST_CLAIM 256
#endif
#ifndef PT_LIST_SHADOW_CLAIM
#define PT_LIST_SHADOW_CLAIM 128
#endif
constexpr uint32_t kListClaim = PT_LIST_CLAIM, kListShClaim = PT_LIST_SHADOW_CLAIM;

// Closest hit with per-lane refill over lean scenes (no §8f row-4 shapes; the refill half of a split
// closest hit).  See k_wf_trace for the lockstep form.  Each lane keeps one ray in flight through ONE
// step loop: a step is one node (or leaf) of the analytic BVH or of the triangle BVH (the same
// seven-load 128-B line), the analytic phase hands over to the triangle phase at an empty stack, and
// a lane whose ray is done takes the next one when PT_REFILL_IDLE lanes of the wave are idle (one
// claim atomic per refill).  A new ray's head work is two queue loads, the planes and (ana_linear /
// route) the few analytic shapes, so a refill holds the busy lanes for one load round trip.  Same
// visit order, same arithmetic as trace(): bit-identical hits.
// SPLIT: the planes, the lean analytic records (routed split) and the triangle BVH only; the FULL
// k_wf_trace<.., SPLIT> pass adds the analytic BVH (or, routed, the heavy records of the rays that
// reach their boxes) and counts the kept rays it finishes.
// Measured and not kept: a cooperative line fetch through LDS (round 2) and through
// a permlane transpose (round 4), leaf turns, a line read ahead, partition stealing, refill kernels
// for the row-4 scenes.
// LIST (unsplit, a triangles-only step loop; depth_loop decides): k_wf_trace_head ran the head work of every
// queued ray, finished the rays that do not reach the triangle BVH and listed the others (Q.tlist).  A refill
// takes list entries, kListClaim positions per cursor claim (kept in SGPRs between refills), and its rays
// start at the root with the provisional hit the head left in Q.hits; the analytic BVH4 branch and the head
// work are not in this instantiation.
template <bool COUNT, bool SPLIT = false, bool LIST = false>
__device__ __forceinline__ void trace_lanes(const DevScene& S, const WfQueues& Q, int qi, unsigned long long* counters) {
    static_assert(!(SPLIT && LIST), "the list-fed form is unsplit");
    constexpr bool split = SPLIT;   // a template flag: the unsplit kernel keeps its registers
    __shared__ uint32_t s_stack[kLdsStack * kTB];
    const WStack stack{s_stack + threadIdx.x, Q.ovf + blockIdx.x * kTB + threadIdx.x, gridDim.x * kTB};
    if (blockIdx.x == 0 && threadIdx.x < kParts) {
        *pair_word(Q, 1 - qi, threadIdx.x) = 0ull;              // consumed: free for k_wf_shade's output
        Q.counts[fetch_word(1, threadIdx.x)] = 0u;               // k_wf_shade's fetch cursors
        Q.counts[fetch_word(7, threadIdx.x)] = 0u;               // (the FULL one's of a routed shade)
    }
    const Group G = xcd_group();
    const uint32_t part = G.g;   // the XCD's own partition
    const uint32_t n = min(LIST ? Q.counts[list_word((int)part)] : *ray_count(Q, qi, part), Q.pcap), base = part * Q.pcap;
    uint32_t* const cursor = Q.counts + (LIST ? list_fetch_word((int)part) : fetch_word(0, part));
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t below = (1ull << lane) - 1ull;
    Counters ctr{0, 0, 0, 0};
    const bool env_black = (!FULL_SHADE_ENV(S)) && S.env[0] == 0.f && S.env[1] == 0.f && S.env[2] == 0.f;
    uint32_t kept = 0;
    const float inf = __int_as_float(0x7f800000);
    bool has = false, tri = LIST, more = true;   // (LIST: every ray is in the triangle phase)
    uint32_t res = 0, rend = 0;   // LIST, wave-uniform: the list positions [res, rend) of the wave's claim not yet taken
    uint32_t i = 0, ref = 0;   // i: the ray's slot; bit 31 set = the ray misses the triangle BVH's root box
    int sp = 0;
    v3 o{0.f, 0.f, 0.f}, d{0.f, 0.f, 0.f}, invd{0.f, 0.f, 0.f};
    double bt = kHitInf;
    int32_t bkind = -1, bidx = -1;
    float tmax = 0.f;
    const bool route = split && S.route;   // routed split: only rays that reach a heavy box go on (hq)
    bool hpend = false;                       // this lane's finished ray waits for the heavy-box test (at the loop top)
    auto finish = [&]() {
        unsigned long long tb = (unsigned long long)__double_as_longlong(bt);
        hit_store(&Q.hits[i & 0x7FFFFFFFu], make_uint4((uint32_t)tb, (uint32_t)(tb >> 32), (uint32_t)bkind, (uint32_t)bidx));
        if (route) hpend = true;
        else if (!split) kept += (bkind >= 0 || !env_black) ? 1u : 0u;
        has = false;
    };
    for (;;) {
        if (route) {   // wave-uniform: the finished rays that reach a heavy box, appended with one atomic per wave
            // (one call site of the box test: the step loop keeps its registers)
            if (hpend) {
                hpend = heavy_reach(S, o, invd, tmax_bound(bt));
                if (!hpend) kept += (bkind >= 0 || !env_black) ? 1u : 0u;
            }
            const uint64_t hm = __ballot(hpend);
            if (hm) {
                const int lead = __builtin_ctzll(hm);
                uint32_t at = 0;
                if ((int)lane == lead) at = atomicAdd(Q.counts + heavy_word((int)part), (uint32_t)__popcll(hm));
                at = (uint32_t)__shfl((int)at, lead, 64) + (uint32_t)__popcll(hm & below);
                if (hpend) {
                    if (at < Q.pcap) Q.hq[part * Q.pcap + at] = i & 0x7FFFFFFFu;
                    else *Q.overflow = 1ull;
                    hpend = false;
                }
            }
        }
        const uint64_t idle = __ballot(!has);
        const uint32_t nidle = (uint32_t)__popcll(idle);
        if constexpr (LIST) {
            if (more && (nidle >= PT_LIST_REFILL_IDLE || nidle == 64u)) {   // wave-uniform
                if (res == rend) {
                    uint32_t kc = 0;
                    if (lane == 0) kc = atomicAdd(cursor, kListClaim);
                    res = __builtin_amdgcn_readfirstlane(kc);   // every lane is active here
                    rend = res + kListClaim;
                }
                const uint32_t k = res + (uint32_t)__popcll(idle & below);
                const uint32_t kend = min(rend, n);
                res = min(res + nidle, rend);   // (lanes past the claim's end wait for the next refill's claim)
                if (res >= n) more = false;     // this partition's list is drained
                if (!has && k < kend) {
                    i = Q.tlist[base + k];
                    const float4 b = nt_load(&Q.q_d[qi][i]);
                    const float4 a = nt_load(&Q.q_o[qi][i]);
                    const uint4 h = nt_load(&Q.hits[i]);   // {bt, bkind, bidx} of the planes and the analytic shapes
                    has = true;
                    o = v3{a.x, a.y, a.z};
                    d = v3{b.x, b.y, b.z};
                    invd = v3{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
                    bt = __longlong_as_double((long long)(((unsigned long long)h.y << 32) | h.x));
                    bkind = (int32_t)h.z; bidx = (int32_t)h.w;
                    tmax = tmax_bound(bt);
                    sp = 0;
                    ref = 0;
                }
            }
        } else if (more && (nidle >= PT_REFILL_IDLE || nidle == 64u)) {   // wave-uniform
            uint32_t kc = 0;
            if (lane == 0) kc = atomicAdd(cursor, nidle);
            kc = __builtin_amdgcn_readfirstlane(kc);   // every lane is active here: lane 0's claim, in an SGPR
            const uint32_t k = kc + (uint32_t)__popcll(idle & below);
            if (kc + nidle >= n) more = false;   // this partition is drained
            if (!has && k < n) {
                i = base + k;
                const float4 b = nt_load(&Q.q_d[qi][i]);
                const float4 a = nt_load(&Q.q_o[qi][i]);
                if (__float_as_uint(b.w) == kDead) {   // a camera slot outside the image: k_wf_shade skips it
                    hit_store(&Q.hits[i], make_uint4(0u, 0u, (uint32_t)kDeadKind, 0u));
                } else {
                    has = true;
                    ctr.rays++;
                    o = v3{a.x, a.y, a.z};
                    d = v3{b.x, b.y, b.z};
                    invd = v3{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
                    bt = kHitInf; bkind = -1; bidx = -1;
                    for (int p = 0; p < S.num_planes; p++) {   // Scene.Intersect order: planes, analytic BVH, triangles
                        const float4 pa = S.planes[2 * p], pb = S.planes[2 * p + 1];
                        const double t = isect_plane(v3{pa.x, pa.y, pa.z}, v3{pb.x, pb.y, pb.z}, o, d);
                        if (t < bt) { bt = t; bkind = KIND_PLANE; bidx = p; }
                    }
                    if (S.ana_linear || route) {   // a few analytic shapes: every lane the same record (one line per load)
                        for (int p = 0; p < S.ana_count; p++) {
                            if (route && f2u(S.ana_recs[3 * p].w) > (uint32_t)KIND_CUBE) continue;   // heavy: its box at finish
                            if (COUNT) ctr.prims++;
                            int32_t kind;
                            const double t = prim_t<false, false>(S, S.ana_recs, (uint32_t)p, o, d, kind);
                            if (t < bt) { bt = t; bkind = kind; bidx = p; }
                        }
                    }
                    tmax = tmax_bound(bt);
                    sp = 0;
                    ref = 0;
                    // tested at the refill's bound (planes only), kept as a bit of i: no register for it
                    if (!tri_reach(S, o, invd, tmax)) i |= 0x80000000u;
                    tri = split || S.ana_linear || S.ana_num_nodes <= 0;
                    if (tri && (i >> 31)) finish();
                }
            }
        }
        if (!more && __ballot(has || hpend) == 0ull) break;   // (a ray finished at refill may wait for the append)
        if (!has) continue;
        // one step: inner node or leaf of the current BVH, one 128-B line of seven 16-B pieces, by a
        // 32-bit offset into the one allocation of all traversal lines (no per-BVH 64-bit base: the
        // step loop then holds its state without spilling).  An analytic leaf reads its records in
        // prim_t; its line is not used.
        const bool leaf = (ref & 0x80000000u) != 0;
        float4 q0, q1, q2, q3, q4, q5, q6, q7;
        {
            const uint32_t at = 8u * (tri ? (leaf ? S.tri_chunk_line0 : S.tri_node_line0) + (ref & 0x1FFFFFFFu)
                                          : (leaf ? 0u : ref));
            q0 = S.lines[at]; q1 = S.lines[at + 1u]; q2 = S.lines[at + 2u]; q3 = S.lines[at + 3u];
            q4 = S.lines[at + 4u]; q5 = S.lines[at + 5u]; q6 = S.lines[at + 6u]; q7 = S.lines[at + 7u];
        }
        PT_PIN4(q0); PT_PIN4(q1); PT_PIN4(q2); PT_PIN4(q3); PT_PIN4(q4); PT_PIN4(q5); PT_PIN4(q6); PT_PIN4(q7);
        bool pop = true;
        if (!leaf) {
            if (COUNT) ctr.nodes++;
            if (tri) {   // the triangle BVH: 8-wide quantized nodes (pt_device.h node8_step)
                pop = !node8_step<true>(q0, q1, q2, q3, q4, q5, q6, q7, o, invd, tmax, stack, sp, ref, S.stack_key_mask);
            } else {     // the analytic BVH4
                float k0, k1, k2, k3;
                uint32_t v0, v1, v2, v3r;
                node4_test(q0, q1, q2, q3, q4, q5, q6, o, invd, tmax, k0, k1, k2, k3, v0, v1, v2, v3r);
                cswap(k0, v0, k1, v1);
                cswap(k2, v2, k3, v3r);
                cswap(k0, v0, k2, v2);
                cswap(k1, v1, k3, v3r);
                cswap(k1, v1, k2, v2);
                if (k0 != inf) {
                    push_hits(stack, sp, 1 + (k1 != inf) + (k2 != inf) + (k3 != inf), v1, v2, v3r);
                    ref = v0;
                    pop = false;
                }
            }
        } else if (tri) {
            const uint32_t w0 = __float_as_uint(q0.x), cntl = (w0 >> 29) + 1u, first = w0 & 0x1FFFFFFFu;   // chunk word 0
            PT_CHUNK_TRIS(q0, q1, q2, q3, q4, q5, q6);
#pragma unroll 1
            for (uint32_t k = 0; k < cntl; k++) {
                if (COUNT) ctr.prims++;
                const double t = isect_tri(a0, a1, a2, o, d);
                if (t < bt) {
                    bt = t; bkind = KIND_TRI; bidx = (int32_t)(first + k);
                    tmax = tmax_bound(t);
                }
                a0 = b0; a1 = b1; a2 = b2;
                b0 = c0; b1 = c1; b2 = c2;
            }
        } else {
            const uint32_t first = ref & 0x1FFFFFFFu, cntl = ((ref >> 29) & 3u) + 1u;
            for (uint32_t k = 0; k < cntl; k++) {
                if (COUNT) ctr.prims++;
                int32_t kind;
                const double t = prim_t<false, false>(S, S.ana_recs, first + k, o, d, kind);
                if (t < bt) {
                    bt = t; bkind = kind; bidx = (int32_t)(first + k);
                    tmax = tmax_bound(t);
                }
            }
        }
        if (pop) {
            if (tri) {
                // Keyed entries (pt_stack_key.h): an entry pushed under an earlier bound whose entry distance
                // is beyond the bound of now is dropped here, and the lane pops again, instead of spending a
                // step on a line none of whose children (or triangles) can win.  The bound is recomputed
                // here, not held across the step (a register).  The analytic phase's stack is empty when a
                // lane enters this phase, so every entry met here is a keyed one.
                const uint32_t km = S.stack_key_mask, bound = stack_bound_bits(tmax);
                uint32_t e = 0u;
                bool got = false;
                while (sp > 0) {
                    sp--;
                    e = stack.get(sp);
                    if (!stack_entry_culled(e, km, bound)) { got = true; break; }
                }
                if (got) ref = stack_entry_ref(e, km);
                else finish();
            } else if (sp > 0) {   // the analytic BVH4's bare refs (their leaf refs use bits 29-30)
                sp--;
                ref = stack.get(sp);
            } else if (!(i >> 31)) {
                tri = true;
                ref = 0;
            } else {
                finish();
            }
        }
    }
    uint32_t rays = wave_sum(ctr.rays);
    if (lane == 0 && rays) atomicAdd(&counters[0], (unsigned long long)rays);
    kept = wave_sum(kept);
    if (lane == 0 && kept) atomicAdd(Q.counts + kept_word(qi), kept);
    if (COUNT) {
        uint32_t nodes = wave_sum(ctr.nodes), prims = wave_sum(ctr.prims);
        if (lane == 0) {
            atomicAdd(&counters[1], (unsigned long long)nodes);
            atomicAdd(&counters[2], (unsigned long long)prims);
        }
    }
}
template <bool COUNT, bool SPLIT = false, bool LIST = false>
__global__ __launch_bounds__(kTB, PT_LANES_WAVES) __attribute__((amdgpu_num_vgpr(PT_LANES_VGPRS))) void k_wf_trace_lanes(DevScene S, WfQueues Q, int qi, unsigned long long* counters) {
    trace_lanes<COUNT, SPLIT, LIST>(S, Q, qi, counters);
}

// Head pass of the list-fed closest hit: one lane per queued slot of the XCD's own partition, every wave full.
// The head work of k_wf_trace_lanes' refill (the same operations in the same order): the dead-slot record, the
// planes, the few analytic shapes (S.ana_linear), the bound, the root-box test.  A ray that does not reach the
// triangle BVH gets its final hit record here and counts as kept like a ray k_wf_trace_lanes finishes; a ray
// that reaches it gets its provisional hit in Q.hits and its slot in the partition's list, in slot order
// inside the block's claim of kHeadRows rows of 256 slots (the child-major order of 64-ray batches survives
// within a claim), reserved with one atomic per claim.
// STATS (PT_HEAD_STATS=1, never a timed run): the rays decided here as a miss with nothing to shade, added to
// counters[kEscapeStatCounter].
constexpr uint32_t kHeadRows = 4;
constexpr int kEscapeStatCounter = 16;   // DevBuffer::counters word (no other kernel's; not read back by the pass)
template <bool COUNT, bool STATS = false>
__global__ __launch_bounds__(256) void k_wf_trace_head(DevScene S, WfQueues Q, int qi, unsigned long long* counters) {
    const Group G = xcd_group();
    const uint32_t n = min(*ray_count(Q, qi, G.g), Q.pcap), base = G.g * Q.pcap;
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    const bool env_black = (!FULL_SHADE_ENV(S)) && S.env[0] == 0.f && S.env[1] == 0.f && S.env[2] == 0.f;
    Counters ctr{0, 0, 0, 0};
    uint32_t kept = 0;
    uint32_t escaped = 0;   // STATS
    __shared__ uint32_t s_wcnt[kHeadRows * 4];
    __shared__ uint32_t s_at;
    for (uint32_t k0 = G.lb * (256u * kHeadRows); k0 < n; k0 += G.nb * (256u * kHeadRows)) {   // block-uniform
        uint32_t listed = 0;   // bit j: this lane's ray of row j enters the triangle BVH
#pragma unroll 1
        for (uint32_t j = 0; j < kHeadRows; j++) {
            const uint32_t k = k0 + j * 256u + threadIdx.x;
            if (k >= n) continue;
            const uint32_t i = base + k;
            const float4 b = nt_load(&Q.q_d[qi][i]);
            const float4 a = nt_load(&Q.q_o[qi][i]);
            if (__float_as_uint(b.w) == kDead) {   // a camera slot outside the image: k_wf_shade skips it
                hit_store(&Q.hits[i], make_uint4(0u, 0u, (uint32_t)kDeadKind, 0u));
                continue;
            }
            ctr.rays++;
            const v3 o{a.x, a.y, a.z}, d{b.x, b.y, b.z};
            const v3 invd{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
            double bt = kHitInf;
            int32_t bkind = -1, bidx = -1;
            for (int p = 0; p < S.num_planes; p++) {   // Scene.Intersect order: planes, analytic shapes, triangles
                const float4 pa = S.planes[2 * p], pb = S.planes[2 * p + 1];
                const double t = isect_plane(v3{pa.x, pa.y, pa.z}, v3{pb.x, pb.y, pb.z}, o, d);
                if (t < bt) { bt = t; bkind = KIND_PLANE; bidx = p; }
            }
            if (S.ana_linear) {
                for (int p = 0; p < S.ana_count; p++) {
                    if (COUNT) ctr.prims++;
                    int32_t kind;
                    const double t = prim_t<false, false>(S, S.ana_recs, (uint32_t)p, o, d, kind);
                    if (t < bt) { bt = t; bkind = kind; bidx = p; }
                }
            }
            const bool reach = tri_reach(S, o, invd, tmax_bound(bt));
            const unsigned long long tb = (unsigned long long)__double_as_longlong(bt);
            hit_store(&Q.hits[i], make_uint4((uint32_t)tb, (uint32_t)(tb >> 32), (uint32_t)bkind, (uint32_t)bidx));
            if (reach) listed |= 1u << j;
            else kept += (bkind >= 0 || !env_black) ? 1u : 0u;
            if (STATS && !reach && bkind < 0 && env_black) escaped++;
        }
        uint64_t bal[kHeadRows];
#pragma unroll
        for (uint32_t j = 0; j < kHeadRows; j++) {
            bal[j] = __ballot((listed >> j) & 1u);
            if (lane == 0) s_wcnt[j * 4 + wid] = (uint32_t)__popcll(bal[j]);
        }
        __syncthreads();
        uint32_t pre[kHeadRows], total = 0;
#pragma unroll
        for (uint32_t q = 0; q < kHeadRows * 4; q++) {
            if ((q & 3) == wid) pre[q >> 2] = total;
            total += s_wcnt[q];
        }
        if (threadIdx.x == 0 && total) s_at = atomicAdd(Q.counts + list_word((int)G.g), total);
        __syncthreads();   // (s_wcnt and s_at are rewritten only behind the next claim's barriers)
        if (listed) {
            const uint32_t at = base + s_at;   // at most n entries: every listed ray is one of the partition's n slots
#pragma unroll
            for (uint32_t j = 0; j < kHeadRows; j++)
                if ((listed >> j) & 1u)
                    Q.tlist[at + pre[j] + (uint32_t)__popcll(bal[j] & below)] = base + k0 + j * 256u + threadIdx.x;
        }
    }
    uint32_t rays = wave_sum(ctr.rays);
    if (lane == 0 && rays) atomicAdd(&counters[0], (unsigned long long)rays);
    kept = wave_sum(kept);
    if (lane == 0 && kept) atomicAdd(Q.counts + kept_word(qi), kept);
    if (COUNT) {
        uint32_t prims = wave_sum(ctr.prims);
        if (lane == 0 && prims) atomicAdd(&counters[2], (unsigned long long)prims);
    }
    if (STATS) {
        escaped = wave_sum(escaped);
        if (lane == 0 && escaped) atomicAdd(&counters[kEscapeStatCounter], (unsigned long long)escaped);
    }
}

// Would k_wf_trace_head turn the ray (o, d), as ray_store is about to write it, into a miss and list nothing?  The
// head's own operations in the head's order: no plane hit, no hit among the linear analytic records, and the
// triangle BVH's root box not reached within tmax_bound(kHitInf) (nothing was hit).  True: the head would write
// {kHitInf, -1, -1} to Q.hits; under a black, untextured environment no later kernel has work for that ray.
__device__ __forceinline__ bool head_misses(const DevScene& S, v3 o, v3 d) {
    const v3 invd{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
    for (int p = 0; p < S.num_planes; p++) {
        const float4 pa = S.planes[2 * p], pb = S.planes[2 * p + 1];
        if (isect_plane(v3{pa.x, pa.y, pa.z}, v3{pb.x, pb.y, pb.z}, o, d) < kHitInf) return false;
    }
    if (S.ana_linear) {
        for (int p = 0; p < S.ana_count; p++) {
            int32_t kind;
            if (prim_t<false, false>(S, S.ana_recs, (uint32_t)p, o, d, kind) < kHitInf) return false;
        }
    }
    return !tri_reach(S, o, invd, tmax_bound(kHitInf));
}

// ---------------------------------------------------------------- shade / bounce
#ifndef PT_SHADE_WAVES
#define PT_SHADE_WAVES 3
#endif
// One thread per queued ray: Hit.Info, emission, then every child of the vertex
// (the u/v/mode loop of Sampler.cs:96-131).  Which children are reflected / live
// depends only on the vertex' Fresnel p and one draw per Any-mode child, so each
// lane counts its extension rays and NEE requests before computing any bounce, and
// the block reserves both queues with ONE atomic (a returning atomic on one
// word saturates near 88 per µs on MI355X, MI355X_MICROARCH.md "dequeue").  Light
// sampling up to the shadow query runs here too, so k_wf_shadow is a lean
// traversal kernel (ray + stack state only).
// One queued vertex (slot i of partition G.g; `alive` false: the lane only takes part in
// the block's reservation and ballots).  Block-uniform call.
template <bool FULL, bool DROP, bool HOLD>
__device__ __forceinline__ void shade_children(const DevScene& S, const DevSampler& smp, const WfQueues& Q, int qi,
                                               const Group& G, const Shade& sh, v3 d, int depth, uint64_t node,
                                               uint32_t pixel, const double (&t2)[3], double pv, double n1, double n2,
                                               int nn, int nm, int nch, uint32_t& dropped);
template <bool COUNT, bool FULL, bool DROP, bool HOLD = false>
__device__ __forceinline__ void shade_vertex(const DevScene& S, const DevSampler& smp, const WfQueues& Q, int qi,
                                             const Group& G, uint32_t i, bool alive, Counters& ctr,
                                             const uint4* hl = nullptr) {   // hl: the hit record, already in LDS
    float4 ro = make_float4(0.f, 0.f, 0.f, 0.f), rd = ro;
    double2 rt = make_double2(0.0, 0.0);
    ulonglong2 rk = make_ulonglong2(0ull, 0ull);
    uint4 hr = make_uint4(0, 0, 0, 0);
    uint32_t meta = kDead;
    if (alive) {  // all loads issued together: one memory round trip
        rd = nt_load(&Q.q_d[qi][i]);
        ro = nt_load(&Q.q_o[qi][i]);
        rt = nt_load(&Q.q_t[qi][i]);
        hr = hl ? *hl : nt_load(&Q.hits[i]);
        rk = nt_load(&Q.q_k[qi][i]);
        meta = __float_as_uint(rd.w);
        alive = meta != kDead;
    }
    const uint64_t node = rk.x;
    const uint32_t pixel = __float_as_uint(ro.w);
    const int depth = (int)(meta & 0xFF);
    const bool emission = (meta >> 8) & 1;
    HitRec h;
    h.t = __longlong_as_double((long long)(((unsigned long long)hr.y << 32) | hr.x));
    h.kind = (int32_t)hr.z;
    h.idx = (int32_t)hr.w;
    h.tx = h.t;   // a TransformedShape hit's record holds its inner object-space t (k_wf_trace)
    const double thr[3] = {rt.x, rt.y, __longlong_as_double((long long)rk.y)};
    const v3 o{ro.x, ro.y, ro.z}, d{rd.x, rd.y, rd.z};
    Shade sh{};
    int mat = 0, nn = 1, nm = 1, nch = 0;
    double t2[3] = {0.0, 0.0, 0.0};
    double pv = 0.0, n1 = 1.0, n2 = 1.0;
    bool has_c = false;   // this vertex' own term: environment (miss) or emission
    double cc[3] = {0.0, 0.0, 0.0};
    if (alive && !(h.t < kHitInf)) {  // sampleEnvironment (Sampler.cs:64-67, 177-189)
        const double3 env = environment<FULL>(S, d);
        cc[0] = thr[0] * env.x; cc[1] = thr[1] * env.y; cc[2] = thr[2] * env.z;
        has_c = true;
        alive = false;
    }
    if (alive) {
        sh = hit_info<COUNT, FULL>(S, h, o, d, ctr);
        mat = sh.mat;
        const DevMaterial& m = S.mats[mat];
        const int samples = depth == 0 ? smp.fh : 1;
        nn = (int)sqrt((double)samples);
        const double rsq = strata_recip(nn * nn);   // result.DivScalar(n * n) (Sampler.cs:144): 1 / (n·n) when exact
        if (m.emittance > 0) {
            if (smp.dl && !emission) {
                alive = false;  // Sampler.cs:75-78
            } else {
                const double e = m.emittance * samples;   // Color.MulScalar(Emittance * samples) (Sampler.cs:79)
                for (int k = 0; k < 3; k++) cc[k] = thr[k] * div_strata(sh.col[k] * e, nn * nn, rsq);
                has_c = true;
            }
        }
        nm = (smp.spec_mode == 2 || (depth == 0 && smp.spec_mode == 1)) ? 2 : 1;
        nch = alive ? nn * nn * nm : 0;
        for (int k = 0; k < 3; k++) t2[k] = div_strata(thr[k], nn * nn, rsq);
        pv = vertex_p(m, sh, d, n1, n2);
    }
    fix_add_wave(Q.acc, pixel, has_c, cc[0], cc[1], cc[2]);
    shade_children<FULL, DROP, HOLD>(S, smp, Q, qi, G, sh, d, depth, node, pixel, t2, pv, n1, n2, nn, nm, nch, ctr.rays);
}
// The children of a shaded vertex (Sampler.cs:96-131): mode, reflect decision and liveness, the block's
// child-major reservation of extension rays and NEE requests, sampleLights up to the shadow query, Ray.Bounce.
// nch 0: the lane only takes part in the block's reservation and ballots.  Block-uniform call.
// DROP (lean only; choose_kernels says where: WfChoice::escape_drop): the slots are reserved before any bounce is
// computed, so the first sweep also computes each extension child's ray and asks head_misses of it.  A child it
// answers for is one Scene.Intersect call (added to `dropped`; the kernel adds them to the pass' counters) and
// nothing else: it is in no count, so the reservation, the child-major order and every store see the survivors
// only.  The second sweep computes a survivor's ray again (keyed draws: the same bits), except in a wave of one
// child per vertex (every depth >= 1), which keeps the first sweep's ray.  A dropped diffuse child's NEE requests
// are made as ever.
// HOLD (the direct form, whose block has the LDS for it): the first sweep leaves the directions of a lane's first
// kDropHold children in LDS and the second sweep takes a survivor's from there (its origin is the vertex, or
// bounce_origin's offset one): no ray is computed twice.  Each lane reads its own words only.
constexpr int kDropHold = 8;
template <bool HOLD>
__device__ __forceinline__ float* drop_hold() {
    if constexpr (HOLD) {
        __shared__ float s_nd[3 * kDropHold * 256];
        return s_nd;
    } else {
        return nullptr;
    }
}
template <bool FULL, bool DROP, bool HOLD>
__device__ __forceinline__ void shade_children(const DevScene& S, const DevSampler& smp, const WfQueues& Q, int qi,
                                               const Group& G, const Shade& sh, v3 d, int depth, uint64_t node,
                                               uint32_t pixel, const double (&t2)[3], double pv, double n1, double n2,
                                               int nn, int nm, int nch, uint32_t& dropped) {
    static_assert(!(FULL && DROP), "the dropping form is a lean shade");
    static_assert(DROP || !HOLD, "only the dropping form holds directions");
    float* const hold = drop_hold<HOLD>();
    const int qo = 1 - qi;
    const bool nee_on = smp.dl && S.num_lights > 0;
    const int nl = S.num_lights;
    const bool all_lights = smp.light_mode == 1;
    const uint32_t rays_per_nee = all_lights ? (uint32_t)nl : 1u;   // shadow rays of one sampleLights call
    const DevMaterial& m = S.mats[sh.mat];
    const int ma = nm == 2 ? 1 : 0;
    const bool ext_on = depth + 1 <= smp.mb;   // deeper samples return black without an Intersect
    const double rn = strata_recip(nn);        // 1 / nn when exact (pt_math.h div_strata)
    const int lg = rn != 0.0 ? __builtin_ctz((unsigned)nn) : 0;
    // child c: mode, reflect decision, liveness (p > 0 after the Any-mode override)
    // Block-wide child-major slots (below): each wave's count of child c's extension rays
    // and NEE requests goes to LDS here, ahead of the reservation's barriers.
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    int cmax = nch;
    for (int off = 32; off > 0; off >>= 1) cmax = max(cmax, __shfl_xor(cmax, off, 64));
    __shared__ uint32_t s_cc[kBlockMajorChildren][4][2];
    const bool block_major = smp.fh <= kBlockMajorFH;   // kernel-uniform: every depth's children fit s_cc
    uint32_t n_ext = 0, n_nee = 0;
    uint64_t rbits = 0;   // the reflect decisions of children 0..63, kept for the second loop (one draw each)
    uint64_t dbits = 0;   // DROP: the children 0..63 whose extension ray is dropped
    v3 no1 = zero3(), nd1 = zero3();   // DROP: the first sweep's last ray (the second sweep's, when cmax is 1)
    // child c's extension ray (Ray.Bounce with the stratum's jittered u, v)
    auto child_ray = [&](int c, uint64_t E, bool refl, v3& no, v3& nd) {
        const int stratum = nm == 2 ? c >> 1 : c;
        const int u = rn != 0.0 ? stratum >> lg : stratum / nn, v = rn != 0.0 ? stratum & (nn - 1) : stratum % nn;
        const double fu = div_strata((double)u + draw(E, D_STRATUM_U), nn, rn);
        const double fv = div_strata((double)(float)v + draw(E, D_STRATUM_V), nn, rn);
        bounce_dir(m, sh, d, fu, fv, refl, n1, n2, E, no, nd);
    };
    for (int c = 0; c < cmax; c++) {   // wave-uniform trip count: the ballots need every lane
        const int mode = ma + (nm == 2 ? c & 1 : 0);   // nm is 1 or 2
        const bool refl = mode == 2 || (mode == 0 && c < nch && draw(child_key(node, (uint32_t)c), D_REFLECT) < pv);
        rbits |= refl && c < 64 ? 1ull << c : 0ull;
        const bool live = c < nch && (mode == 0 || (refl ? pv > 0 : (1 - pv) > 0));
        bool ee = live && ext_on;
        const bool en = live && !refl && !m.transparent && nee_on;
        if (DROP && ee) {
            child_ray(c, child_key(node, (uint32_t)c), refl, no1, nd1);
            if (head_misses(S, no1, nd1)) {
                ee = false;
                dbits |= c < 64 ? 1ull << c : 0ull;
                dropped++;
            } else if (HOLD && c < kDropHold) {
                hold[(3 * c + 0) * 256 + threadIdx.x] = nd1.x;
                hold[(3 * c + 1) * 256 + threadIdx.x] = nd1.y;
                hold[(3 * c + 2) * 256 + threadIdx.x] = nd1.z;
            }
        }
        n_ext += ee ? 1u : 0u;
        n_nee += en ? rays_per_nee : 0u;
        if (block_major) {
            const uint64_t be = __ballot(ee), bn = __ballot(en);
            if (lane == 0) { s_cc[c][wid][0] = (uint32_t)__popcll(be); s_cc[c][wid][1] = (uint32_t)__popcll(bn); }
        }
    }
    if (block_major && lane >= cmax && lane < kBlockMajorChildren) { s_cc[lane][wid][0] = 0u; s_cc[lane][wid][1] = 0u; }
    uint32_t ebase, nbase, blk_e, blk_n;
    block_reserve2(pair_word(Q, qo, G.g), n_ext, n_nee, ebase, nbase, &blk_e, &blk_n);
    if (ebase + n_ext > Q.pcap || nbase + n_nee > Q.spcap) *Q.overflow = 1ull;
    // Child-major slots: the block's reservation is filled child index by child index,
    // child c of every lane of the block on consecutive slots (waves in order, a ballot
    // prefix within each), then child c + 1.  A 64-ray batch of the next depth then holds
    // the same stratum and mode of neighbouring camera samples (one direction quadrant,
    // origins of a few pixels) rather than all children of one sample, the depth after it
    // inherits runs of one stratum from 16 pixels, and every store instruction writes
    // whole lines.  Which children exist is unchanged, so is every child's key.  With
    // more children per vertex than s_cc holds, each wave fills its own share that way.
    uint32_t ej = block_major ? blk_e : __shfl(ebase, 0, 64), nj = block_major ? blk_n : __shfl(nbase, 0, 64);
    for (int c = 0; c < cmax; c++) {   // wave-uniform trip count: the ballots need every lane
        const int mode = ma + (nm == 2 ? c & 1 : 0);
        const uint64_t E = child_key(node, (uint32_t)c);
        const bool refl = c < 64 ? ((rbits >> c) & 1ull) != 0
                                 : mode == 2 || (mode == 0 && c < nch && draw(E, D_REFLECT) < pv);
        const bool live = c < nch && (mode == 0 || (refl ? pv > 0 : (1 - pv) > 0));
        const bool reflected = refl || m.transparent;                 // specular branch (Sampler.cs:109-115)
        const bool emit_nee = live && !reflected && nee_on;
        bool emit_ext = live && ext_on;
        v3 no, nd;
        bool have_ray = false;   // DROP, children >= 64: the ray, computed here for the decision
        if (DROP && emit_ext) {
            if (c < 64) {
                emit_ext = !((dbits >> c) & 1ull);
            } else {
                child_ray(c, E, refl, no, nd);
                have_ray = true;
                emit_ext = !head_misses(S, no, nd);
            }
        }
        const uint64_t bn = __ballot(emit_nee), be = __ballot(emit_ext);
        uint32_t pe = 0, pn = 0, te = (uint32_t)__popcll(be), tn = (uint32_t)__popcll(bn);
        if (block_major) {   // waves before this one, and the whole block's total, at child c
            te = tn = 0;
            for (int w = 0; w < 4; w++) {
                const uint32_t ce = s_cc[c][w][0], cn = s_cc[c][w][1];
                if (w < wid) { pe += ce; pn += cn; }
                te += ce; tn += cn;
            }
        }
        const uint32_t my_n = nj + (pn + (uint32_t)__popcll(bn & below)) * rays_per_nee;
        const uint32_t my_e = ej + pe + (uint32_t)__popcll(be & below);
        nj += tn * rays_per_nee;
        ej += te;
        if (!live) continue;
        const double fp = mode == 0 ? 1.0 : (refl ? pv : 1 - pv);
        double w[3];
        if (reflected) {   // indirect.Mix(Color·indirect, Tint)·p (Sampler.cs:112-114)
            for (int k = 0; k < 3; k++) w[k] = fp * ((1.0 - m.tint) + m.tint * sh.col[k]);
        } else {           // Color·(direct + indirect)·p (Sampler.cs:119-127)
            for (int k = 0; k < 3; k++) w[k] = fp * sh.col[k];
            if (nee_on) {
                // diffuse child: sampleLights from the normal ray (Sampler.cs:191-296) up to the
                // shadow query — light choice, soft-shadow point, coverage — here, so the
                // visibility kernel carries only ray + stack state.  One shadow-ray slot per
                // light considered; a light with diffuse <= 0 casts no ray (dead slot).
                const int first = all_lights ? 0 : min((int)(draw(E, D_LIGHT) * nl), nl - 1);
                for (uint32_t j = 0; j < rays_per_nee; j++) {
                    const int li = first + (int)j;
                    v3 ldir;
                    double3 lc;
                    const bool cast = light_setup<FULL>(S, smp, S.lights[li], sh.pos, sh.nrm,
                                                  all_lights ? light_key(E, (uint32_t)li) : E, ldir, lc);
                    // sampleLights: ÷ nLights (LightModeAll) or × nLights (random light), Sampler.cs:199-209
                    if (all_lights) { lc.x /= nl; lc.y /= nl; lc.z /= nl; }
                    else { lc.x *= nl; lc.y *= nl; lc.z *= nl; }
                    if (my_n + j < Q.spcap) {
                        const uint32_t at = G.g * Q.spcap + my_n + j;
                        q_store_next(&Q.n_o[qo][at], make_float4(sh.pos.x, sh.pos.y, sh.pos.z, __uint_as_float(pixel)));
                        q_store_next(&Q.n_n[qo][at], make_float4(ldir.x, ldir.y, ldir.z, __uint_as_float(cast ? (uint32_t)li : kDead)));
                        q_store_late(&Q.n_w[qo][2 * (size_t)at], make_double2((t2[0] * w[0]) * lc.x, (t2[1] * w[1]) * lc.y));
                        q_store_late(&Q.n_w[qo][2 * (size_t)at + 1],   // {b, pixel}: k_wf_nee_accum reads only n_w
                                     make_double2((t2[2] * w[2]) * lc.z, __longlong_as_double((long long)pixel)));
                    }
                }
            }
        }
        if (DROP ? !emit_ext : !ext_on) continue;
        if (HOLD && c < kDropHold) {
            no = bounce_origin(m, sh, d, refl, n1, n2);
            nd = v3{hold[(3 * c + 0) * 256 + threadIdx.x], hold[(3 * c + 1) * 256 + threadIdx.x], hold[(3 * c + 2) * 256 + threadIdx.x]};
        } else if (DROP && cmax == 1) {   // (wave-uniform)
            no = no1; nd = nd1;
        } else if (!(DROP && have_ray)) {
            child_ray(c, E, refl, no, nd);
        }
        if (my_e < Q.pcap) {
            const double nthr[3] = {t2[0] * w[0], t2[1] * w[1], t2[2] * w[2]};
            ray_store(Q, qo, G.g * Q.pcap + my_e, no, nd, nthr, pixel, (uint32_t)(depth + 1) | ((reflected ? 1u : 0u) << 8),
                      E);
        }
    }
}

// SCAN (one of the two instantiations launched per depth runs; the other returns at
// once): k_wf_trace counted the rays with work for shade (hits, and misses when the
// environment is not black; kept_word).  Where fewer than half of the queued rays have
// work (C4's first bounce: ~77 % escape), a block claims kShadeScan × 256 vertices, reads
// their hit records and lists the ones with work in slot order, then shades the list 256
// at a time: each round trip of the chain (claim, queue loads, triangle record,
// reservation) serves four times as many vertices.  Otherwise the block shades every
// claimed slot (no extra read of the hit records, fewer live registers).
// A scene's materials and lights, when few, staged in the shade block's LDS (and its analytic records and planes,
// when few): a vertex' material (after its
// triangle record), its light (after the light draw) and that light's material are dependent loads of the
// shading chain; from LDS each costs an LDS round trip instead of an L1 / L2 one.  Returns the scene view
// that reads them there (flat loads).  Block-uniform call.
constexpr int kLdsMats = 32;   // (kLdsLights: pt_pass_plan.h)
static_assert(sizeof(DevMaterial) % 8 == 0 && sizeof(DevLight) % 8 == 0, "stage_shading copies 8-B words");
__device__ __forceinline__ DevScene stage_shading(const DevScene& S0) {
    __shared__ unsigned long long s_mats[kLdsMats * sizeof(DevMaterial) / 8];
    __shared__ unsigned long long s_lights[kLdsLights * sizeof(DevLight) / 8];
    __shared__ float4 s_ana[3 * kLinRecs];     // a few analytic records (a sphere or cube hit's record in hit_info)
    __shared__ float4 s_pln[2 * kLinPlanes];   // and planes
    DevScene S = S0;
    if (S0.num_mats > kLdsMats || S0.num_lights > kLdsLights) return S;
    const bool ana = S0.ana_count > 0 && S0.ana_count <= kLinRecs, pln = S0.num_planes > 0 && S0.num_planes <= kLinPlanes;
    if (ana)
        for (uint32_t k = threadIdx.x; k < 3u * (uint32_t)S0.ana_count; k += blockDim.x) s_ana[k] = S0.ana_recs[k];
    if (pln)
        for (uint32_t k = threadIdx.x; k < 2u * (uint32_t)S0.num_planes; k += blockDim.x) s_pln[k] = S0.planes[k];
    const uint32_t nm = (uint32_t)S0.num_mats * (uint32_t)(sizeof(DevMaterial) / 8);
    const uint32_t nl = (uint32_t)S0.num_lights * (uint32_t)(sizeof(DevLight) / 8);
    const unsigned long long* gm = reinterpret_cast<const unsigned long long*>(S0.mats);
    const unsigned long long* gl = reinterpret_cast<const unsigned long long*>(S0.lights);
    for (uint32_t k = threadIdx.x; k < nm; k += blockDim.x) s_mats[k] = gm[k];
    for (uint32_t k = threadIdx.x; k < nl; k += blockDim.x) s_lights[k] = gl[k];
    __syncthreads();
    S.mats = reinterpret_cast<const DevMaterial*>(s_mats);
    S.lights = reinterpret_cast<const DevLight*>(s_lights);
    if (ana) S.ana_recs = s_ana;
    if (pln) S.planes = s_pln;
    return S;
}

template <bool COUNT, bool FULL, bool SCAN, bool DROP = false>
__global__ __launch_bounds__(256, FULL ? PT_FULL_SHADE_WAVES : PT_SHADE_WAVES) void k_wf_shade(DevScene S0, DevSampler smp, WfQueues Q, int qi,
                                                                  unsigned long long* counters, int form) {
    const DevScene& S = S0;   // the kernel argument until the block knows it runs (stage_shading below)
    uint32_t queued = 0;
    for (int g = 0; g < kParts; g++) queued += min(*ray_count(Q, qi, g), Q.pcap);
    // SCAN unless (nearly) every queued ray has work: with its partial rounds carried over it
    // beat the direct form down to ~92 % kept in the lean kernels (C4 +1.6 %, C2 +9.8 %); the
    // FULL kernels keep the round-1 rule (SCAN below half kept; forcing it cost them 8-10 %).
    const unsigned long long kept = Q.counts[kept_word(qi)];
    // routed shade: the lean and the FULL kernel each list their own vertices (SCAN only)
    const bool routed = S.shade_route != 0;
    const bool scan = routed ? true
                    : form ? form == 2
                           // (the dropping form: its direct kernel holds the children's directions in LDS, which the
                           // SCAN kernel's lists leave no room for, so it stays direct down to half kept)
                           : FULL || DROP ? 2ull * kept < (unsigned long long)queued
                                                     : 32ull * kept < 31ull * (unsigned long long)queued;
    if (scan != SCAN) return;
    const DevScene Sv = PT_SHADE_LDS ? stage_shading(S0) : S0;
    if (blockIdx.x == 0 && threadIdx.x < kParts) {
        Q.counts[fetch_word(2 + (1 - qi), threadIdx.x)] = 0u;   // the fetch cursors of the shadow rays it writes
        Q.counts[fetch_word(0, threadIdx.x)] = 0u;              // the next k_wf_trace's (it may run beside k_wf_shadow)
        Q.counts[fetch_word(4, threadIdx.x)] = 0u;              // its analytic half's (split)
        if (threadIdx.x == 0) Q.counts[kSdfWord] = 0u;          // and that half's SDF queue
        Q.counts[heavy_word(threadIdx.x)] = 0u;                 // and the routed split's heavy queue
        Q.counts[heavy_sh_word(1 - qi, threadIdx.x)] = 0u;      // the shadow set it writes: its heavy queue
        if (threadIdx.x == 0) Q.counts[sdf_sh_word(1 - qi)] = 0u;   // and its SDF queue
        Q.counts[fetch_word(5 + (1 - qi), threadIdx.x)] = 0u;   // the split shadow rays' analytic half
        if (threadIdx.x == 0) Q.counts[kept_word(1 - qi)] = 0u;   // the next k_wf_trace's kept count
        Q.counts[list_word(threadIdx.x)] = 0u;                  // the next closest hit's list (k_wf_trace_head)
        Q.counts[list_fetch_word(threadIdx.x)] = 0u;            // and its cursor
        Q.counts[list_sh_word(1 - qi, threadIdx.x)] = 0u;       // the shadow set it writes: its list (k_wf_shadow_head)
        Q.counts[list_sh_fetch_word(1 - qi, threadIdx.x)] = 0u;
    }
    const Group G = xcd_group();
    const uint32_t cnt = *ray_count(Q, qi, G.g);
    const uint32_t n = cnt < Q.pcap ? cnt : Q.pcap, base = G.g * Q.pcap;
    Counters ctr{0, 0, 0, 0};
    __shared__ uint32_t s_k0;
    if constexpr (!SCAN) {
        for (;;) {  // block-uniform: the block takes 256 vertices of its partition at a time
            if (threadIdx.x == 0) s_k0 = atomicAdd(Q.counts + fetch_word(1, G.g), 256u);
            __syncthreads();
            const uint32_t k0 = s_k0;  // thread 0 rewrites it only after block_reserve2's barriers
            if (k0 >= n) break;
            shade_vertex<COUNT, FULL, DROP, DROP>(Sv, smp, Q, qi, G, base + k0 + threadIdx.x, k0 + threadIdx.x < n, ctr);
        }
    } else {
        const bool env_black = (!FULL || S.env_tex < 0) && S.env[0] == 0.f && S.env[1] == 0.f && S.env[2] == 0.f;
        // routed: the lean kernel takes the hits on spheres, cubes, planes and triangles, and the misses unless the
        // environment is textured (then k_wf_shade_miss takes them); the FULL kernel takes the rest
        const bool env_lean = S.env_tex < 0;
        uint32_t* const shade_cursor = Q.counts + fetch_word(routed && FULL ? 7 : 1, G.g);
        const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
        const uint64_t below = (1ull << lane) - 1ull;
        __shared__ uint32_t s_wcnt[kShadeScan * 4];
        // the listed vertices (partition-local slots) of this claim, after the < 256 held over from
        // the last one: every round but the kernel's last shades a full 256 (round 1 shaded each
        // claim's partial last round, a quarter to a half of the rounds at C4's first bounce)
        __shared__ uint32_t s_list[kShadeScan * 256 + 256];
        __shared__ uint4 s_hit[kShadeScan * 256 + 256];   // their hit records (read once, by the scan)
        uint32_t carry = 0;   // block-uniform
        // rows of 256 slots per claim: kShadeScan, fewer when the partition would not give every block a
        // claim (small chunks: one rank's share of a multi-GPU frame; 4 or 8 claims per block: no better)
        const uint32_t rows = max(1u, min((uint32_t)kShadeScan, n / (G.nb * 256u)));
        for (;;) {
            if (threadIdx.x == 0) s_k0 = atomicAdd(shade_cursor, 256u * rows);
            __syncthreads();
            const uint32_t k0 = s_k0;  // thread 0 rewrites it only after the barriers below
            const bool last = k0 >= n;   // block-uniform: nothing claimed, shade what is held over
            uint32_t total = carry;
            if (!last) {
                uint32_t keep = 0;
                uint4 hv[kShadeScan];
#pragma unroll
                for (int j = 0; j < kShadeScan; j++) {
                    const uint32_t sl = k0 + (uint32_t)j * 256u + threadIdx.x;
                    hv[j] = make_uint4(0u, 0u, (uint32_t)kDeadKind, 0u);
                    if ((uint32_t)j < rows && sl < n) hv[j] = nt_load(&Q.hits[base + sl]);
                    const int32_t kind = (int32_t)hv[j].z;
                    bool k = kind != kDeadKind && (kind >= 0 || !env_black);
                    if (routed) k = k && (kind >= 0 ? (kind <= KIND_TRI) != FULL : PT_SHADE_MISS ? env_lean && !FULL : env_lean != FULL);
                    keep |= k ? 1u << j : 0u;
                }
                uint64_t bal[kShadeScan];
#pragma unroll
                for (int j = 0; j < kShadeScan; j++) {
                    bal[j] = __ballot((keep >> j) & 1u);
                    if (lane == 0) s_wcnt[j * 4 + wid] = (uint32_t)__popcll(bal[j]);
                }
                __syncthreads();
                uint32_t pre[kShadeScan];
#pragma unroll
                for (int q = 0; q < kShadeScan * 4; q++) {
                    const uint32_t w = s_wcnt[q];
                    if ((q & 3) == wid) pre[q >> 2] = total;
                    total += w;
                }
#pragma unroll
                for (int j = 0; j < kShadeScan; j++)
                    if ((keep >> j) & 1u) {
                        const uint32_t at = pre[j] + (uint32_t)__popcll(bal[j] & below);
                        s_list[at] = k0 + (uint32_t)j * 256u + threadIdx.x;
                        s_hit[at] = hv[j];
                    }
                __syncthreads();
            }
            const uint32_t full = last ? total : total & ~255u;
            for (uint32_t r = 0; r < full; r += 256u) {   // block-uniform
                const bool listed = r + threadIdx.x < full;
                shade_vertex<COUNT, FULL, DROP>(Sv, smp, Q, qi, G, base + (listed ? s_list[r + threadIdx.x] : 0u), listed, ctr,
                                          &s_hit[r + threadIdx.x]);
                __syncthreads();   // the next round rewrites shade_vertex's LDS child counts
            }
            if (last) break;
            carry = total - full;   // < 256: to the front of the list
            const uint32_t held = threadIdx.x < carry ? s_list[full + threadIdx.x] : 0u;
            const uint4 hheld = threadIdx.x < carry ? s_hit[full + threadIdx.x] : make_uint4(0u, 0u, 0u, 0u);
            __syncthreads();
            if (threadIdx.x < carry) { s_list[threadIdx.x] = held; s_hit[threadIdx.x] = hheld; }
            __syncthreads();
        }
    }
    if (COUNT) {
        uint32_t shades = wave_sum(ctr.shades);
        if ((threadIdx.x & 63) == 0) atomicAdd(&counters[3], (unsigned long long)shades);
    }
    if (DROP) {   // the dropped children: Scene.Intersect calls, each with the head's analytic tests
        const uint32_t rays = wave_sum(ctr.rays);
        if ((threadIdx.x & 63) == 0 && rays) {
            atomicAdd(&counters[0], (unsigned long long)rays);
            if (COUNT && S.ana_linear) atomicAdd(&counters[2], (unsigned long long)rays * (unsigned long long)S.ana_count);
        }
    }
}

// The misses of a routed shade under a textured environment (DevScene::shade_route, S.env_tex >= 0):
// sampleEnvironment (Sampler.cs:64-67, 177-189), throughput · Scene.Texture lookup, added to the
// vertex' pixel; a miss has no children.  The SCAN shades skip these vertices, so the texture lookup
// runs here at a small kernel's occupancy instead of in the FULL shade (2 waves).
__global__ __launch_bounds__(256) void k_wf_shade_miss(DevScene S, WfQueues Q, int qi) {
    const Group G = xcd_group();
    const uint32_t cnt = *ray_count(Q, qi, G.g);
    const uint32_t n = cnt < Q.pcap ? cnt : Q.pcap, base = G.g * Q.pcap;
    for (uint32_t k0 = G.lb * 256u; k0 < n; k0 += G.nb * 256u) {   // block-uniform: fix_add_wave takes every lane
        const uint32_t sl = k0 + threadIdx.x;
        bool has = false;
        uint32_t pixel = 0;
        double c[3] = {0.0, 0.0, 0.0};
        // a miss, by shade_vertex's own test (t = Hit.INF; a dead slot has kind kDeadKind and t 0).  Every hit
        // store writes kind -1 exactly with t = kHitInf (trace / refill kernels: HitRec{kHitInf, -1, -1} until
        // a hit; k_wf_vol_hits / k_wf_sdf_hits write hits only), so this agrees with the SCAN listing's
        // kind < 0 that routes these vertices here and not to the FULL shade.
        const uint4 hr = sl < n ? nt_load(&Q.hits[base + sl]) : make_uint4(0u, 0u, (uint32_t)kDeadKind, 0u);
        const double ht = __longlong_as_double((long long)(((unsigned long long)hr.y << 32) | hr.x));
        if ((int32_t)hr.z != kDeadKind && !(ht < kHitInf)) {
            const size_t i = base + sl;
            const float4 rd = nt_load(&Q.q_d[qi][i]), ro = nt_load(&Q.q_o[qi][i]);
            const double2 rt = nt_load(&Q.q_t[qi][i]);
            const ulonglong2 rk = nt_load(&Q.q_k[qi][i]);
            const double3 env = environment<true>(S, v3{rd.x, rd.y, rd.z});
            c[0] = rt.x * env.x;
            c[1] = rt.y * env.y;
            c[2] = __longlong_as_double((long long)rk.y) * env.z;
            pixel = __float_as_uint(ro.w);
            has = true;
        }
        fix_add_wave(Q.acc, pixel, has, c[0], c[1], c[2]);
    }
}

// ---------------------------------------------------------------- shadow rays
#ifndef PT_SHADOW_WAVES
#define PT_SHADOW_WAVES 7   // lockstep shadow kernel; the refill one runs PT_LANES_WAVES
#endif
// The lean shadow kernels' lights in LDS (LDSL: the scene has at most kLdsLights lights; the kernels
// run their LDSL = false form otherwise): each light and its own record, the one light_t intersects.  A
// shadow ray's light index comes from its queue entry, so the light and then its record were two dependent
// loads ahead of the ray's first traversal step.
template <bool LDSL>
struct LightLds {
    const DevLight* l;   // LDSL: kLdsLights lights in LDS
    const float4* r;     // LDSL: 3 float4 per light, its ana_recs record
    __device__ __forceinline__ const DevLight& light(const DevScene& S, uint32_t li) const { return LDSL ? l[li] : S.lights[li]; }
    __device__ __forceinline__ const float4* rec(uint32_t li) const { return LDSL ? r + 3 * li : nullptr; }   // null: ana_recs
};
template <bool LDSL>
__device__ __forceinline__ LightLds<LDSL> stage_lights(const DevScene& S) {   // block-uniform call
    if constexpr (!LDSL) {
        return LightLds<false>{nullptr, nullptr};
    } else {
        __shared__ DevLight s_l[kLdsLights];
        __shared__ float4 s_r[kLdsLights * 3];
        for (uint32_t k = threadIdx.x; k < (uint32_t)S.num_lights; k += blockDim.x) {
            const DevLight L = S.lights[k];
            s_l[k] = L;
            if (L.kind != KIND_PLANE && !L.phantom)
                for (int j = 0; j < 3; j++) s_r[3 * k + j] = S.ana_recs[3 * (size_t)L.index + j];
        }
        __syncthreads();
        return LightLds<true>{s_l, s_r};
    }
}

// One thread per shadow ray that k_wf_shade set up (light, direction, the colour the
// light adds if it is the nearest hit): the visibility query of Sampler.cs:261-265.
// SPLIT (FULL only): the analytic half of split shadow rays: the rays the refill kernel left lit.
template <bool COUNT, bool FULL, bool SPLIT, bool LDSL>
__device__ __forceinline__ void shadow_rays(const DevScene& S, const WfQueues& Q, int qo, unsigned long long* counters) {
    __shared__ uint32_t s_stack[kLdsStack * kTB];
    const WStack stack{s_stack + threadIdx.x, Q.ovf_sh + blockIdx.x * kTB + threadIdx.x, gridDim.x * kTB};
    const Group G = xcd_group();
    const bool route = SPLIT && S.route;   // the heavy queue's rays only (the refill half decided the others)
    const uint32_t cnt = route ? Q.counts[heavy_sh_word(qo, (int)G.g)] : *nee_count(Q, qo, G.g);
    const uint32_t n = cnt < Q.spcap ? cnt : Q.spcap, base = G.g * Q.spcap;
    uint32_t* cursor = Q.counts + fetch_word(SPLIT ? 5 + qo : 2 + qo, G.g);
    const uint32_t lane = threadIdx.x & 63;
    Counters ctr{0, 0, 0, 0};
    const LightLds<LDSL> LL = stage_lights<LDSL>(S);
    for (;;) {  // kFetchBatches × 64 rays per claim, 64 at a time (see k_wf_trace)
        uint32_t kc = 0;
        if (lane == 0) kc = atomicAdd(cursor, 64u * kFetchBatches);
        kc = __shfl(kc, 0, 64);
        if (kc >= n) break;
        for (uint32_t k0 = kc; k0 < kc + 64u * kFetchBatches && k0 < n; k0 += 64u) {
            if (k0 + lane >= n) continue;
            const uint32_t i = route ? Q.hq_sh[base + k0 + lane] : base + k0 + lane;
            if (SPLIT && Q.n_lit[qo][i] == 0) continue;   // blocked (or dead) in the refill half
            bool lit = false;
            float4 b = nt_load(&Q.n_n[qo][i]);
            float4 a = nt_load(&Q.n_o[qo][i]);   // with n_n, before the dead test: one round trip per ray
            PT_PIN44(b, a);
            const uint32_t li = __float_as_uint(b.w);
            if (SPLIT) {
                int32_t sdf = -1, vol = -1;
                int32_t* const vol_out = Q.volq_sh ? &vol : nullptr;   // Volumes deferred to k_wf_vol_shadow
                double tl = 0;
                const bool blocked =
                    route ? heavy_blocked<COUNT>(S, S.lights[li], v3{a.x, a.y, a.z}, v3{b.x, b.y, b.z}, ctr,
                                                 &sdf, &tl, vol_out)
                          : ana_blocked<COUNT>(S, S.lights[li], v3{a.x, a.y, a.z}, v3{b.x, b.y, b.z}, stack, ctr,
                                               &sdf, &tl, vol_out);
                {   // k_wf_vol_shadow and k_wf_sdf_shadow test them, every lane busy
                    const bool defer = !blocked && (sdf >= 0 || vol >= 0);
                    const uint64_t m = __ballot(defer);
                    if (m) {
                        const int lead = __builtin_ctzll(m);
                        uint32_t at = 0;
                        if ((int)lane == lead) at = atomicAdd(Q.counts + sdf_sh_word(qo), (uint32_t)__popcll(m));
                        at = (uint32_t)__shfl((int)at, lead, 64) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                        if (defer && at < Q.s_cap) {
                            const unsigned long long tb = (unsigned long long)__double_as_longlong(tl);
                            Q.sdfq_sh[at] = make_uint4(i, (uint32_t)sdf, (uint32_t)tb, (uint32_t)(tb >> 32));
                            if (Q.volq_sh) Q.volq_sh[at] = (uint32_t)vol;
                        } else if (defer) {
                            *Q.overflow = 1ull;
                        }
                    }
                }
                if (!blocked) continue;
            } else if (li != kDead) {
                const DevLight L = LL.light(S, li);
                lit = light_visible<COUNT, FULL>(S, L, v3{a.x, a.y, a.z}, v3{b.x, b.y, b.z}, stack, ctr,
                                                 LL.rec(li));
            }
            Q.n_lit[qo][i] = lit ? 1 : 0;   // k_wf_nee_accum adds the lit rays' terms
        }
    }
    uint32_t rays = wave_sum(ctr.rays);
    if (lane == 0 && rays) atomicAdd(&counters[4], (unsigned long long)rays);
    if (COUNT) {
        uint32_t nodes = wave_sum(ctr.nodes), prims = wave_sum(ctr.prims);
        if (lane == 0) {
            atomicAdd(&counters[5], (unsigned long long)nodes);
            atomicAdd(&counters[6], (unsigned long long)prims);
        }
    }
}
// LDSL (lean, at most kLdsLights lights; the launch decides): the lights in LDS (stage_lights)
template <bool COUNT, bool FULL, bool SPLIT = false, bool LDSL = false>
__global__ __launch_bounds__(kTB, FULL ? PT_FULL_SHADOW_WAVES : PT_SHADOW_WAVES) void k_wf_shadow(DevScene S, WfQueues Q, int qo, unsigned long long* counters) {
    shadow_rays<COUNT, FULL, SPLIT, LDSL && !FULL>(S, Q, qo, counters);
}

// The shadow rays of the same scenes (see k_wf_trace_linear).
template <bool COUNT, bool LDSL>
__global__ __launch_bounds__(256, 8) void k_wf_shadow_linear(DevScene S, WfQueues Q, int qo, unsigned long long* counters) {
    const Group G = xcd_group();
    const uint32_t n = min(*nee_count(Q, qo, G.g), Q.spcap), base = G.g * Q.spcap;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t W = G.nb * 4u;
    Counters ctr{0, 0, 0, 0};
    const LightLds<LDSL> LL = stage_lights<LDSL>(S);
    const LinScene L = stage_linear(S);
    uint32_t r = G.lb * 4u + (threadIdx.x >> 6);
    LinRay cur = lin_fetch(Q.n_n[qo], Q.n_o[qo], base, r * 64u + lane, n);
    for (; r * 64u < n; r += W) {   // wave-uniform
        const LinRay nxt = lin_fetch(Q.n_n[qo], Q.n_o[qo], base, (r + W) * 64u + lane, n);
        const uint32_t k = r * 64u + lane;
        if (k < n) {
            const uint32_t li = __float_as_uint(cur.b.w);
            bool lit = false;
            if (li != kDead)
                lit = light_visible_linear<COUNT>(S, L.recs, L.planes, LL.light(S, li), v3{cur.a.x, cur.a.y, cur.a.z},
                                                  v3{cur.b.x, cur.b.y, cur.b.z}, ctr, LL.rec(li));
            Q.n_lit[qo][base + k] = lit ? 1 : 0;   // k_wf_nee_accum adds the lit rays' terms
        }
        cur = nxt;
    }
    uint32_t rays = wave_sum(ctr.rays);
    if (lane == 0 && rays) atomicAdd(&counters[4], (unsigned long long)rays);
    if (COUNT) {
        const uint32_t prims = wave_sum(ctr.prims);
        if (lane == 0) atomicAdd(&counters[6], (unsigned long long)prims);
    }
}

// Shadow visibility with per-lane refill (triangle scenes; see k_wf_trace_lanes): the
// light's own t and the planes at refill, then one step loop over the analytic BVH and
// the triangle BVH, any-hit (a primitive strictly nearer than the light ends the ray
// unlit).  The outcome goes to n_lit; k_wf_nee_accum adds the lit rays' terms.
// split: the planes, the lean analytic records (routed split) and the triangle BVH only; the FULL
// k_wf_shadow<.., SPLIT> pass then tests the analytic BVH (routed: the heavy records) of the rays
// left lit.
// The tail (queue drained): idle lanes take stack entries of busy lanes' rays and traverse those
// subtrees (any-hit: the ray is blocked iff some subtree holds a blocker, in any order).
// s_help[root]: helpers still running on root's ray, bit 31 = blocked.  A root that ends its own
// traversal waits for its helpers before it reports the ray lit.
// EARLY (Q.tail_early, tests; its own instantiation: a runtime flag cost the render kernel 22 SGPR spills): a
// wave refills only when every lane is idle — then no helper and no waiting root is
// left, so the refill may reset s_help — and hands stack entries to idle lanes from its first claim on.
// Uncounted passes add the hand-offs to counters[11].
// LIST (unsplit, a triangles-only step loop; depth_loop decides): k_wf_shadow_head ran the head work, decided
// the rays that do not reach the triangle BVH and listed the others with their light's t (Q.slist); a refill
// takes list entries as the list-fed k_wf_trace_lanes does, and no light is read here.
template <bool COUNT, bool SPLIT, bool EARLY, bool LDSL, bool LIST = false>
__device__ __forceinline__ void shadow_lanes(const DevScene& S, const WfQueues& Q, int qo, unsigned long long* counters) {
    static_assert(!(LIST && (SPLIT || LDSL)), "the list-fed form is unsplit and reads no light");
    constexpr bool split = SPLIT;
    __shared__ uint32_t s_stack[kLdsStack * kTB];
    const WStack stack{s_stack + threadIdx.x, Q.ovf_sh + blockIdx.x * kTB + threadIdx.x, gridDim.x * kTB};
    const Group G = xcd_group();
    const uint32_t part = G.g;   // the XCD's own partition
    const uint32_t n = min(LIST ? Q.counts[list_sh_word(qo, (int)part)] : *nee_count(Q, qo, part), Q.spcap), base = part * Q.spcap;
    uint32_t* const cursor = Q.counts + (LIST ? list_sh_fetch_word(qo, (int)part) : fetch_word(2 + qo, part));
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t below = (1ull << lane) - 1ull;
    Counters ctr{0, 0, 0, 0};
    const float inf = __int_as_float(0x7f800000);
    bool has = false, tri = LIST, more = true, phantom = false;   // (LIST: every ray is in the triangle phase)
    uint32_t res = 0, rend = 0;   // LIST, wave-uniform: the list positions [res, rend) of the wave's claim not yet taken
    uint32_t i = 0, ref = 0;
    int sp = 0;
    v3 o{0.f, 0.f, 0.f}, d{0.f, 0.f, 0.f}, invd{0.f, 0.f, 0.f};
    double tl = kHitInf;
    float tmax = 0.f;
    bool waiting = false;   // a root whose traversal is done, waiting for its tail helpers
    __shared__ uint32_t s_help[kTB];
    __shared__ uint32_t s_map[kTB];   // per wave: donor lane by rank
    __shared__ uint32_t s_handoffs[kTB / 64];   // per wave: tail hand-offs
    if (lane == 0) s_handoffs[threadIdx.x >> 6] = 0u;
    const LightLds<LDSL> LL = stage_lights<LDSL>(S);
    bool helper = false;
    uint32_t root = threadIdx.x;
    const uint32_t wbase = threadIdx.x & ~63u;
    const bool route = split && S.route;   // routed split: lit rays that reach a heavy box go on (hq_sh)
    constexpr bool early = EARLY && !COUNT;
    constexpr uint32_t refill_at = early ? 64u : (uint32_t)(LIST ? PT_LIST_SHADOW_REFILL_IDLE : PT_SHADOW_REFILL_IDLE);
    bool hpend = false;
    // a root ray found nothing nearer than its light: lit (a phantom light never is); under the routed
    // split, provisionally when the ray reaches a heavy box (the FULL half decides: k_wf_shadow<.., SPLIT>)
    // (the box test runs here, on this lane's own ray: in the tail a lane that reported may turn helper and
    // take another root's ray into o / invd before the loop top)
    auto report_lit = [&]() {
        Q.n_lit[qo][i] = phantom ? 0 : 1;
        if (route && !phantom) hpend = heavy_reach(S, o, invd, tmax);
    };
    for (;;) {
        if (route) {   // wave-uniform: the provisionally lit rays that reach a heavy box, one atomic per wave
            const uint64_t hm = __ballot(hpend);
            if (hm) {
                const int lead = __builtin_ctzll(hm);
                uint32_t at = 0;
                if ((int)lane == lead) at = atomicAdd(Q.counts + heavy_sh_word(qo, (int)part), (uint32_t)__popcll(hm));
                at = (uint32_t)__shfl((int)at, lead, 64) + (uint32_t)__popcll(hm & below);
                if (hpend) {
                    if (at < Q.spcap) Q.hq_sh[part * Q.spcap + at] = i;
                    else *Q.overflow = 1ull;
                    hpend = false;
                }
            }
        }
        const uint64_t idle = __ballot(!has);
        const uint32_t nidle = (uint32_t)__popcll(idle);
        if constexpr (LIST) {
            if (more && (nidle >= refill_at || nidle == 64u)) {   // wave-uniform
                if (res == rend) {
                    uint32_t kc = 0;
                    if (lane == 0) kc = atomicAdd(cursor, kListShClaim);
                    res = __builtin_amdgcn_readfirstlane(kc);   // every lane is active here
                    rend = res + kListShClaim;
                }
                const uint32_t k = res + (uint32_t)__popcll(idle & below);
                const uint32_t kend = min(rend, n);
                res = min(res + nidle, rend);   // (lanes past the claim's end wait for the next refill's claim)
                if (res >= n) more = false;
                if (!has && k < kend) {
                    const uint4 e = nt_load(&Q.slist[base + k]);
                    i = e.x;
                    if (early) {   // a former helper is a root again
                        root = threadIdx.x;
                        helper = false;
                        waiting = false;
                    }
                    const float4 b = nt_load(&Q.n_n[qo][i]);
                    const float4 a = nt_load(&Q.n_o[qo][i]);
                    o = v3{a.x, a.y, a.z};
                    d = v3{b.x, b.y, b.z};
                    invd = v3{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
                    phantom = e.y != 0u;
                    tl = __longlong_as_double((long long)(((unsigned long long)e.w << 32) | e.z));
                    tmax = tmax_bound(tl);
                    sp = 0;
                    ref = 0;
                    has = true;
                    s_help[threadIdx.x] = 0u;
                }
            }
        } else if (more && (nidle >= refill_at || nidle == 64u)) {   // wave-uniform
            uint32_t kc = 0;
            if (lane == 0) kc = atomicAdd(cursor, nidle);
            kc = __builtin_amdgcn_readfirstlane(kc);   // every lane is active here: lane 0's claim, in an SGPR
            const uint32_t k = kc + (uint32_t)__popcll(idle & below);
            if (kc + nidle >= n) more = false;
            if (!has && k < n) {
                i = base + k;
                if (early) {   // a former helper is a root again (without EARLY no lane refills after the tail began)
                    root = threadIdx.x;
                    helper = false;
                    waiting = false;
                }
                const float4 b = nt_load(&Q.n_n[qo][i]);
                const float4 a = nt_load(&Q.n_o[qo][i]);
                const uint32_t li = __float_as_uint(b.w);
                if (li == kDead) {
                    Q.n_lit[qo][i] = 0;
                } else {   // light_visible (pt_device.h), head part
                    ctr.rays++;
                    const DevLight L = LL.light(S, li);
                    o = v3{a.x, a.y, a.z};
                    d = v3{b.x, b.y, b.z};
                    invd = v3{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
                    phantom = L.phantom != 0;
                    bool run;
                    if (phantom) {
                        tl = kHitInf;   // traced like the reference, never lit
                        run = S.tri_num_nodes > 0;
                        tri = true;
                    } else {
                        tl = light_t<false>(S, L, o, d, LL.rec(li));
                        run = tl < kHitInf;
                        for (int p = 0; run && p < S.num_planes; p++) {
                            const float4 pa = S.planes[2 * p], pb = S.planes[2 * p + 1];
                            if (isect_plane(v3{pa.x, pa.y, pa.z}, v3{pb.x, pb.y, pb.z}, o, d) < tl) run = false;
                        }
                        if (S.ana_linear || route)   // the light itself gives t == tl, never nearer
                            for (int p = 0; p < S.ana_count; p++) {
                                if (route && f2u(S.ana_recs[3 * p].w) > (uint32_t)KIND_CUBE) continue;   // heavy: its box at the end
                                if (COUNT) ctr.prims++;
                                int32_t kind;
                                if (prim_t<false, false>(S, S.ana_recs, (uint32_t)p, o, d, kind) < tl) run = false;
                            }
                        tri = split || S.ana_linear || S.ana_num_nodes <= 0;
                    }
                    tmax = tmax_bound(tl);
                    sp = 0;
                    ref = 0;
                    if (run && tri && !tri_reach(S, o, invd, tmax)) {   // nothing of the mesh before the light
                        run = false;
                        report_lit();
                    } else if (!run) {
                        Q.n_lit[qo][i] = 0;
                    }
                    has = run;
                    s_help[threadIdx.x] = 0u;
                }
            }
        }
        if (!more && __ballot(has || hpend) == 0ull) break;   // (a ray finished at refill may wait for the append)
        if (!COUNT && (!more || early)) {   // wave-uniform: the tail (not in the counting pass: its node counts stay sequential)
            if (has) {
                const uint32_t st = s_help[root];
                if (st & 0x80000000u) {   // a helper found a blocker: the root ends unlit, its helpers stop
                    if (!helper) Q.n_lit[qo][i] = 0;
                    has = false;
                } else if (waiting && st == 0u) {   // the root's own traversal and every helper done
                    report_lit();
                    has = false;
                }
            }
            const uint64_t idle = __ballot(!has), don = __ballot(has && !waiting && sp > 0);
            if (idle != 0ull && don != 0ull) {
                const uint32_t nd = min((uint32_t)__popcll(idle), (uint32_t)__popcll(don));
                const uint32_t rd = (uint32_t)__popcll(don & below), ri = (uint32_t)__popcll(idle & below);
                uint32_t top = 0;
                if (has && !waiting && sp > 0 && rd < nd) {   // give the top entry (what this lane would pop next)
                    sp--;
                    top = stack.get(sp);
                    s_map[wbase + rd] = lane;
                    atomicAdd(&s_help[root], 1u);
                }
                __builtin_amdgcn_s_waitcnt(0xC07F);
                __builtin_amdgcn_wave_barrier();
                const bool take = !has && ri < nd;
                if (lane == 0) s_handoffs[threadIdx.x >> 6] += nd;   // (to counters[11] at the end: the pointer
                                                                     // live in the loop cost 26 SGPR spills)
                const int src = take ? (int)s_map[wbase + ri] : (int)lane;
                const float ox = __shfl(o.x, src, 64), oy = __shfl(o.y, src, 64), oz = __shfl(o.z, src, 64);
                const float dx = __shfl(d.x, src, 64), dy = __shfl(d.y, src, 64), dz = __shfl(d.z, src, 64);
                const double tls = __shfl(tl, src, 64);
                const uint32_t rt = __shfl(root, src, 64), tp = __shfl(top, src, 64);
                const int fl = __shfl((tri ? 1 : 0) | (phantom ? 2 : 0), src, 64);
                if (take) {
                    o = v3{ox, oy, oz};
                    d = v3{dx, dy, dz};
                    invd = v3{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
                    tl = tls;
                    tmax = tmax_bound(tl);
                    root = rt;
                    ref = tp;
                    sp = 0;
                    tri = (fl & 1) != 0;
                    phantom = (fl & 2) != 0;
                    helper = true;
                    waiting = false;
                    has = true;
                }
            }
        }
        if (!has || waiting) continue;
        // one step: inner node or leaf of the current BVH (one 128-B line; see k_wf_trace_lanes)
        const bool leaf = (ref & 0x80000000u) != 0;
        float4 q0, q1, q2, q3, q4, q5, q6, q7;
        {
            const uint32_t at = 8u * (tri ? (leaf ? S.tri_chunk_line0 : S.tri_node_line0) + (ref & 0x1FFFFFFFu)
                                          : (leaf ? 0u : ref));
            q0 = S.lines[at]; q1 = S.lines[at + 1u]; q2 = S.lines[at + 2u]; q3 = S.lines[at + 3u];
            q4 = S.lines[at + 4u]; q5 = S.lines[at + 5u]; q6 = S.lines[at + 6u]; q7 = S.lines[at + 7u];
        }
        PT_PIN4(q0); PT_PIN4(q1); PT_PIN4(q2); PT_PIN4(q3); PT_PIN4(q4); PT_PIN4(q5); PT_PIN4(q6); PT_PIN4(q7);
        bool pop = true, blocked = false;
        if (!leaf) {
            if (COUNT) ctr.nodes++;
            if (tri) {   // the triangle BVH: 8-wide quantized nodes (pt_device.h node8_step)
                pop = !node8_step(q0, q1, q2, q3, q4, q5, q6, q7, o, invd, tmax, stack, sp, ref);
            } else {     // the analytic BVH4
                float k0, k1, k2, k3;
                uint32_t v0, v1, v2, v3r;
                node4_test(q0, q1, q2, q3, q4, q5, q6, o, invd, tmax, k0, k1, k2, k3, v0, v1, v2, v3r);
                cswap(k0, v0, k1, v1);
                cswap(k2, v2, k3, v3r);
                cswap(k0, v0, k2, v2);
                cswap(k1, v1, k3, v3r);
                cswap(k1, v1, k2, v2);
                if (k0 != inf) {
                    push_hits(stack, sp, 1 + (k1 != inf) + (k2 != inf) + (k3 != inf), v1, v2, v3r);
                    ref = v0;
                    pop = false;
                }
            }
        } else if (tri) {
            const uint32_t cntl = (__float_as_uint(q0.x) >> 29) + 1u;   // chunk word 0
            PT_CHUNK_TRIS(q0, q1, q2, q3, q4, q5, q6);
#pragma unroll 1
            for (uint32_t k = 0; k < cntl; k++) {
                if (COUNT) ctr.prims++;
                if (isect_tri(a0, a1, a2, o, d) < tl) { blocked = true; break; }
                a0 = b0; a1 = b1; a2 = b2;
                b0 = c0; b1 = c1; b2 = c2;
            }
        } else {
            const uint32_t first = ref & 0x1FFFFFFFu, cntl = ((ref >> 29) & 3u) + 1u;
            for (uint32_t k = 0; k < cntl; k++) {
                if (COUNT) ctr.prims++;
                int32_t kind;
                if (prim_t<false, false>(S, S.ana_recs, first + k, o, d, kind) < tl) { blocked = true; break; }
            }
        }
        if (blocked) {
            has = false;
            if (helper) atomicOr(&s_help[root], 0x80000000u);
            else {
                Q.n_lit[qo][i] = 0;
                if (!more || early) atomicOr(&s_help[root], 0x80000000u);   // its helpers stop
            }
        } else if (pop) {
            if (sp > 0) {
                sp--;
                ref = stack.get(sp);
            } else if (helper) {   // a donated subtree done, nothing nearer than the light in it
                has = false;
                atomicSub(&s_help[root], 1u);
            } else if (!tri && tri_reach(S, o, invd, tmax)) {
                tri = true;
                ref = 0;
            } else if (s_help[root] == 0u) {   // no primitive nearer than the light
                has = false;
                report_lit();
            } else {
                waiting = true;   // the tail block above decides once the helpers are done
            }
        }
    }
    uint32_t rays = wave_sum(ctr.rays);
    if (lane == 0 && rays) atomicAdd(&counters[4], (unsigned long long)rays);
    if (!COUNT && lane == 0 && s_handoffs[threadIdx.x >> 6])
        atomicAdd(&counters[11], (unsigned long long)s_handoffs[threadIdx.x >> 6]);
    if (COUNT) {
        uint32_t nodes = wave_sum(ctr.nodes), prims = wave_sum(ctr.prims);
        if (lane == 0) {
            atomicAdd(&counters[5], (unsigned long long)nodes);
            atomicAdd(&counters[6], (unsigned long long)prims);
        }
    }
}
// LDSL (at most kLdsLights lights; the launch decides): the lights in LDS (stage_lights)
template <bool COUNT, bool SPLIT = false, bool EARLY = false, bool LDSL = false, bool LIST = false>
__global__ __launch_bounds__(kTB, PT_LANES_WAVES) __attribute__((amdgpu_num_vgpr(PT_LANES_VGPRS))) void k_wf_shadow_lanes(DevScene S, WfQueues Q, int qo, unsigned long long* counters) {
    shadow_lanes<COUNT, SPLIT, EARLY, LDSL, LIST>(S, Q, qo, counters);
}

// Head pass of the list-fed shadow kernel (see k_wf_trace_head): the head work of k_wf_shadow_lanes' refill in
// the same order: a dead slot is unlit, the light's own t, the planes, the few analytic shapes (S.ana_linear),
// the root-box test (a ray that does not reach the mesh before its light is lit; a phantom light never is).  A
// ray that goes on is listed with its light's t and the phantom flag, so the traversal kernel reads no light.
template <bool COUNT, bool LDSL>
__global__ __launch_bounds__(256) void k_wf_shadow_head(DevScene S, WfQueues Q, int qo, unsigned long long* counters) {
    const Group G = xcd_group();
    const uint32_t n = min(*nee_count(Q, qo, G.g), Q.spcap), base = G.g * Q.spcap;
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    Counters ctr{0, 0, 0, 0};
    const LightLds<LDSL> LL = stage_lights<LDSL>(S);
    __shared__ uint32_t s_wcnt[kHeadRows * 4];
    __shared__ uint32_t s_at;
    __shared__ double s_tl[kHeadRows * 256];   // each lane's own listed rays' light t (read back by the same lane)
    for (uint32_t k0 = G.lb * (256u * kHeadRows); k0 < n; k0 += G.nb * (256u * kHeadRows)) {   // block-uniform
        uint32_t listed = 0;   // bit j: this lane's ray of row j goes on into the triangle BVH; bit 8 + j: phantom light
#pragma unroll 1
        for (uint32_t j = 0; j < kHeadRows; j++) {
            const uint32_t k = k0 + j * 256u + threadIdx.x;
            if (k >= n) continue;
            const uint32_t i = base + k;
            const float4 b = nt_load(&Q.n_n[qo][i]);
            const float4 a = nt_load(&Q.n_o[qo][i]);
            const uint32_t li = __float_as_uint(b.w);
            if (li == kDead) {
                Q.n_lit[qo][i] = 0;
                continue;
            }
            ctr.rays++;
            const DevLight L = LL.light(S, li);
            const v3 o{a.x, a.y, a.z}, d{b.x, b.y, b.z};
            const v3 invd{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
            const bool phantom = L.phantom != 0;
            double tl;
            bool run;
            if (phantom) {
                tl = kHitInf;   // traced like the reference, never lit
                run = S.tri_num_nodes > 0;
            } else {
                tl = light_t<false>(S, L, o, d, LL.rec(li));
                run = tl < kHitInf;
                for (int p = 0; run && p < S.num_planes; p++) {
                    const float4 pa = S.planes[2 * p], pb = S.planes[2 * p + 1];
                    if (isect_plane(v3{pa.x, pa.y, pa.z}, v3{pb.x, pb.y, pb.z}, o, d) < tl) run = false;
                }
                if (S.ana_linear)   // the light itself gives t == tl, never nearer
                    for (int p = 0; p < S.ana_count; p++) {
                        if (COUNT) ctr.prims++;
                        int32_t kind;
                        if (prim_t<false, false>(S, S.ana_recs, (uint32_t)p, o, d, kind) < tl) run = false;
                    }
            }
            if (run && !tri_reach(S, o, invd, tmax_bound(tl))) {   // nothing of the mesh before the light
                run = false;
                Q.n_lit[qo][i] = phantom ? 0 : 1;
            } else if (!run) {
                Q.n_lit[qo][i] = 0;
            }
            if (run) {
                listed |= (1u << j) | (phantom ? 256u << j : 0u);
                s_tl[j * 256u + threadIdx.x] = tl;
            }
        }
        uint64_t bal[kHeadRows];
#pragma unroll
        for (uint32_t j = 0; j < kHeadRows; j++) {
            bal[j] = __ballot((listed >> j) & 1u);
            if (lane == 0) s_wcnt[j * 4 + wid] = (uint32_t)__popcll(bal[j]);
        }
        __syncthreads();
        uint32_t pre[kHeadRows], total = 0;
#pragma unroll
        for (uint32_t q = 0; q < kHeadRows * 4; q++) {
            if ((q & 3) == wid) pre[q >> 2] = total;
            total += s_wcnt[q];
        }
        if (threadIdx.x == 0 && total) s_at = atomicAdd(Q.counts + list_sh_word(qo, (int)G.g), total);
        __syncthreads();   // (s_wcnt and s_at are rewritten only behind the next claim's barriers)
        if (listed) {
            const uint32_t at = base + s_at;   // at most n entries: every listed ray is one of the partition's n slots
#pragma unroll
            for (uint32_t j = 0; j < kHeadRows; j++)
                if ((listed >> j) & 1u) {
                    const unsigned long long tb = (unsigned long long)__double_as_longlong(s_tl[j * 256u + threadIdx.x]);
                    Q.slist[at + pre[j] + (uint32_t)__popcll(bal[j] & below)] =
                        make_uint4(base + k0 + j * 256u + threadIdx.x, (listed >> (8 + j)) & 1u, (uint32_t)tb, (uint32_t)(tb >> 32));
                }
        }
    }
    uint32_t rays = wave_sum(ctr.rays);
    if (lane == 0 && rays) atomicAdd(&counters[4], (unsigned long long)rays);
    if (COUNT) {
        uint32_t prims = wave_sum(ctr.prims);
        if (lane == 0 && prims) atomicAdd(&counters[6], (unsigned long long)prims);
    }
}

// ---------------------------------------------------------------- direct-light terms
// The light terms (throughput·weight·light colour·coverage, set up by k_wf_shade) of the
// shadow rays the visibility kernels found lit, added in slot order after each shadow pass
// (a pixel's rays sit in runs of consecutive slots, so fix_add_wave sums most of them in
// registers).  Keeping the accumulation out of the traversal kernels keeps their refill path
// and registers lean.  Group g takes partition g (written on its XCD by k_wf_shade).
#ifndef PT_ACC_WIN
#define PT_ACC_WIN 16
#endif
constexpr uint32_t kAccWin = PT_ACC_WIN;   // 256-slot rows per block window (one shade block's child-major region
                                      // of FirstHitSamples 16 children)
constexpr uint32_t kAccTable = 512;   // LDS table entries (a power of two)
template <bool COUNT>
__global__ __launch_bounds__(256) void k_wf_nee_accum(WfQueues Q, int qo, unsigned long long* counters) {
    const Group G = xcd_group();
    const uint32_t cnt = *nee_count(Q, qo, G.g);
    const uint32_t n = cnt < Q.spcap ? cnt : Q.spcap;
    const size_t base = (size_t)G.g * Q.spcap;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t lit_n = 0, runs = 0;
    // One slot's flag and weights.  The weights are loaded with the flag, not after it (an unlit slot's are
    // read and dropped: one round trip per row instead of two), and the window's next row is loaded before
    // this row's sums run.
    struct Slot { bool lit; double2 w01, w2; };
    auto fetch = [&](uint32_t j) {
        Slot x{false, make_double2(0.0, 0.0), make_double2(0.0, 0.0)};
        if (j < n) {
            const size_t i = base + j;
            x.lit = Q.n_lit[qo][i] != 0;
            x.w01 = nt_load(&Q.n_w[qo][2 * i]);
            x.w2 = nt_load(&Q.n_w[qo][2 * i + 1]);
        }
        return x;
    };
    auto row = [&](const Slot& x, const LdsFix* T) {   // one row of 64 slots of this wave (wave-uniform)
        const uint32_t pixel = x.lit ? (uint32_t)__double_as_longlong(x.w2.y) : 0u;
        const uint32_t r = fix_add_wave(Q.acc, pixel, x.lit, x.w01.x, x.w01.y, x.w2.x, T);
        if (COUNT) { runs += r; lit_n += (uint32_t)__popcll(__ballot(x.lit)); }
    };
    // A pixel's light terms of one depth sit in runs of consecutive slots, one run per child index
    // of its vertex (the child-major fill): a block takes windows of kAccWin·256 slots, sums the
    // wave runs of a window per pixel in LDS and flushes one atomic set per pixel (for
    // FirstHitSamples 16, 16 runs of a pixel become one).  Integer sums: the order is free.
    __shared__ uint32_t s_key[kAccTable];
    __shared__ unsigned long long s_sum[kAccTable * 3];
    const LdsFix T{s_key, s_sum, kAccTable - 1u};
    for (uint32_t e = threadIdx.x; e < kAccTable; e += 256u) {
        s_key[e] = kLdsFree;
        s_sum[3 * e] = 0ull; s_sum[3 * e + 1] = 0ull; s_sum[3 * e + 2] = 0ull;
    }
    __syncthreads();
    for (uint32_t w0 = G.lb * 256u * kAccWin; w0 < n; w0 += G.nb * 256u * kAccWin) {   // block-uniform
        Slot cur = fetch(w0 + threadIdx.x);
        for (uint32_t r = 0; r < kAccWin; r++) {
            const Slot nxt = r + 1 < kAccWin ? fetch(w0 + (r + 1) * 256u + threadIdx.x) : Slot{false, {0.0, 0.0}, {0.0, 0.0}};
            row(cur, &T);
            cur = nxt;
        }
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < kAccTable; e += 256u) {
            const uint32_t k = s_key[e];
            if (k == kLdsFree) continue;
            for (int c = 0; c < 3; c++) {
                const long long v = (long long)s_sum[3 * e + c];
                if (v) fix_atomic(Q.acc, k, c, v);
                s_sum[3 * e + c] = 0ull;
            }
            s_key[e] = kLdsFree;
        }
        __syncthreads();
    }
    if (COUNT && lane == 0) {
        atomicAdd(&counters[7], (unsigned long long)lit_n);
        atomicAdd(&counters[8], (unsigned long long)runs);
    }
}

// ---------------------------------------------------------------- Welford
__global__ __launch_bounds__(256) void k_wf_finalize(DevPass P, DevBuffer B, WfQueues Q, double spp) {
    const uint32_t total = (uint32_t)P.num_tiles * 1024u;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < total; s += gridDim.x * blockDim.x) {
        const int tile = P.tiles ? P.tiles[s >> 10] : (int)(s >> 10);
        int x, y;
        tile_pixel(tile, (int)(s & 1023), P.tiles_x, x, y);
        if (x >= P.width || y >= P.height) continue;
        const size_t pix = (size_t)y * (size_t)P.width + (size_t)x;
        for (int p = 0; p < P.passes; p++) {   // a batch's passes in order: the Welford sequence of separate passes
            double c[3];
            fix_take(Q.acc, pix + (size_t)p * P.acc_stride, c);
            // c /= spp (Renderer.cs:308) then Buffer.AddSample
            welford(B, pix, c[0] / spp, c[1] / spp, c[2] / spp);
        }
    }
}

// ---------------------------------------------------------------- adaptive / firefly phases
// Entry e of a phase is one pixel with K individually accumulated samples
// (Renderer.cs:340-470): the adaptive phase walks the pass' pixels in tile order,
// the extra phases the pixel lists of k_wf_select.  A camera ray's
// accumulator index is its chunk-relative slot e·K + j, not its pixel.
__device__ __forceinline__ bool entry_pixel(const DevPass& P, const uint32_t* plist, uint64_t e, int& x, int& y) {
    if (plist) {
        const uint32_t pix = plist[e];
        x = (int)(pix % (uint32_t)P.width);
        y = (int)(pix / (uint32_t)P.width);
        return true;
    }
    const int tile = P.tiles ? P.tiles[e >> 10] : (int)(e >> 10);
    tile_pixel(tile, (int)(e & 1023), P.tiles_x, x, y);
    return x < P.width && y < P.height;
}

// The order of an extra-phase chunk's samples (ne entries, K samples each): entries in groups of kExtraGroup,
// a group's slots sample-major (sample j of its w entries, then sample j + 1), the last group w = ne mod
// kExtraGroup entries wide.  A wave of camera rays is then a few samples of neighbouring pixels (the ray
// coherence of entry-major slots), and the finalize's lanes read whole runs of a group's accumulators.
#ifndef PT_EXTRA_GROUP
#define PT_EXTRA_GROUP 8
#endif
constexpr uint32_t kExtraGroup = PT_EXTRA_GROUP;
static_assert(kExtraGroup >= 1, "kExtraGroup");
// (slots are < ne · K, a uint32 count; a group's span kExtraGroup · K is taken in 64 bits)
__device__ __forceinline__ uint32_t extra_slot(uint32_t el, uint32_t j, uint32_t ne, uint32_t K) {
    const uint32_t b = el / kExtraGroup, w = min(kExtraGroup, ne - b * kExtraGroup);
    return (uint32_t)((uint64_t)b * kExtraGroup * K) + j * w + (el - b * kExtraGroup);
}
__device__ __forceinline__ void extra_entry(uint32_t g, uint32_t ne, uint32_t K, uint32_t& el, uint32_t& j) {
    const uint64_t span = (uint64_t)kExtraGroup * K;
    const uint32_t b = (uint32_t)(g / span), w = min(kExtraGroup, ne - b * kExtraGroup);
    const uint32_t off = (uint32_t)(g - b * span);
    j = off / w;
    el = b * kExtraGroup + (off - j * w);
}
__global__ __launch_bounds__(256) void k_wf_camera_extra(DevCamera cam, DevPass P, WfQueues Q, uint64_t begin,
                                                         uint32_t count, int32_t K, uint32_t sample_base,
                                                         const uint32_t* plist, int scaled) {
    // Camera samples are dealt to the XCD groups in interleaved 256-slot blocks
    // (one sample of 256 pixels): every group gets an even share of sky, floor and mesh.
    // Slot g of the chunk is sample j of entry e (extra_slot's order: groups of kExtraGroup entries, sample-major
    // within a group), and it is the sample's accumulator too, so k_wf_finalize_extra's lanes, one entry each,
    // read sample j of a group's entries together.
    const Group G = xcd_group();
    const uint32_t ne = count / (uint32_t)K;
    const uint64_t e0 = begin / (uint64_t)K;
    for (uint32_t g = (G.g + kParts * G.lb) * 256u + threadIdx.x; g < count; g += kParts * G.nb * 256u) {
        uint32_t el, j;
        extra_entry(g, ne, (uint32_t)K, el, j);
        const uint64_t e = e0 + el;
        int x, y;
        if (!entry_pixel(P, plist, e, x, y)) continue;
        const uint64_t pix = (uint64_t)y * (uint64_t)P.width + (uint64_t)x;
        const uint64_t Kc = camera_key(P.seed, P.pass_index, pix, sample_base + j);
        v3 o, d;
        // CastRay(x, y, w, h, NextDouble(), NextDouble()): no jitter bug in these loops; Render's
        // firefly loop passes (x + NextDouble()) · invWidth, invWidth = 1.0f / w in float
        // (Renderer.cs:98-99, 184-185)
        double fu = draw(Kc, D_JX), fv = draw(Kc, D_JY);
        if (scaled) {
            fu = ((double)x + fu) * (double)(1.0f / (float)P.width);
            fv = ((double)y + fv) * (double)(1.0f / (float)P.height);
        }
        cast_ray(cam, x, y, P.width, P.height, fu, fv, Kc, o, d);
        const uint32_t i = append(ray_count(Q, 0, G.g));
        if (i >= Q.pcap) { *Q.overflow = 1ull; continue; }
        ray_store_camera(Q, 0, G.g * Q.pcap + i, o, d, g, Kc);
    }
}

// One thread per entry: the K samples in order — AddSample each (adaptive), or stop
// at the first IsFirefly sample (firefly; a pixel that did not stop goes on next_list for
// the next round).  Clears the entry's accumulators (sample j of entry e at extra_slot's place,
// k_wf_camera_extra).  The pixel's Welford state stays in registers across
// the K samples (welford's arithmetic, in the same order) and is written once.
__global__ __launch_bounds__(256) void k_wf_finalize_extra(DevPass P, DevBuffer B, FixAcc acc,
                                                           uint64_t begin_entry, uint32_t entries, int32_t K,
                                                           const uint32_t* plist, int firefly,
                                                           const double* __restrict__ snap, uint32_t* next_list,
                                                           uint32_t* next_count) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < entries; e += gridDim.x * blockDim.x) {
        int x, y;
        const bool in = entry_pixel(P, plist, begin_entry + e, x, y);
        const size_t pix = (size_t)y * (size_t)P.width + (size_t)x;
        bool stop = !in;
        int32_t n = 0;
        double M[3] = {0.0, 0.0, 0.0}, V[3] = {0.0, 0.0, 0.0};
        if (in) {
            n = B.n[pix];
            for (int k = 0; k < 3; k++) { M[k] = B.m[3 * pix + k]; V[k] = B.v[3 * pix + k]; }
        }
        const int32_t n0 = n;
        for (int j = 0; j < K; j++) {
            double c[3];
            fix_take(acc, extra_slot(e, (uint32_t)j, entries, (uint32_t)K), c);
            if (stop) continue;
            if (firefly && is_firefly(c[0], c[1], c[2], x, y, P.width, P.height, snap, M)) { stop = true; continue; }
            n++;   // welford (pt_device.h), Buffer.AddSample
            if (n == 1) {
                M[0] = c[0]; M[1] = c[1]; M[2] = c[2];
                continue;
            }
            for (int k = 0; k < 3; k++) {
                const double mo = M[k];
                const double mn = mo + (c[k] - mo) / (double)n;
                V[k] = V[k] + (c[k] - mo) * (c[k] - mn);
                M[k] = mn;
            }
        }
        if (n != n0) {
            B.n[pix] = n;
            for (int k = 0; k < 3; k++) { B.m[3 * pix + k] = M[k]; B.v[3 * pix + k] = V[k]; }
        }
        if (next_list && !stop) next_list[atomicAdd(next_count, 1u)] = (uint32_t)pix;
    }
}

// Pixels of the pass whose standard deviation exceeds FireflyThreshold (kind 0, Renderer.cs:179,
// 426), or reaches AdaptiveThreshold in Render's adaptive branch (kind 1, Renderer.cs:155-158).
// List order is irrelevant: every later step is per pixel.
__global__ __launch_bounds__(256) void k_wf_select(DevPass P, DevBuffer B, int kind, uint32_t* plist, uint32_t* count) {
    const uint32_t total = (uint32_t)P.num_tiles * 1024u;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < total; s += gridDim.x * blockDim.x) {
        int x, y;
        if (!entry_pixel(P, nullptr, s, x, y)) continue;
        const uint32_t pix = (uint32_t)y * (uint32_t)P.width + (uint32_t)x;
        if (kind ? adaptive_serial_candidate(B, pix) : firefly_candidate(B, pix)) plist[atomicAdd(count, 1u)] = pix;
    }
}

// ---------------------------------------------------------------- host driver
// Grid for `items` work items; a multiple of kParts (XCD groups), at most cap_blocks.
static unsigned grid_for(uint64_t items, unsigned block, unsigned cap_blocks) {
    uint64_t g = (items + block - 1) / block;
    g = (g + kParts - 1) / kParts * kParts;
    if (g < (uint64_t)kParts) g = kParts;
    if (g > cap_blocks) g = cap_blocks / kParts * kParts;
    return (unsigned)g;
}

// What choose_kernels (pt_pass_plan.h) reads of a pass.
static WfChoiceInput choice_input(const DevScene& S, const WfQueues& Q, const WfPlan& plan, bool count) {
    WfChoiceInput in;
    in.full = S.full; in.full_geom = S.full_geom; in.tri_num_nodes = S.tri_num_nodes; in.ana_num_nodes = S.ana_num_nodes;
    in.ana_count = S.ana_count; in.ana_linear = S.ana_linear; in.num_planes = S.num_planes; in.num_sdf = S.num_sdf;
    in.num_vol = S.num_vol; in.num_lights = S.num_lights; in.lights_lean = S.lights_lean; in.shade_route = S.shade_route;
    in.env_tex = S.env_tex; in.sdf_lds = S.sdf_lds; in.vol_lds = S.vol_lds;
    in.volq = Q.volq != nullptr; in.volq_sh = Q.volq_sh != nullptr;
    in.env_black = S.env[0] == 0.f && S.env[1] == 0.f && S.env[2] == 0.f;
    in.knobs = plan;
    in.knobs.tail_early = Q.tail_early;
    in.counted = count;
    return in;
}

// Trace / shade / shadow for every depth of one chunk whose camera rays are queued.  Which kernels: choose_kernels
// (pt_pass_plan.cpp), once per call.
template <bool COUNT>
static hipError_t depth_loop(const DevScene& S, const DevSampler& smp, const DevBuffer& B, const WfQueues& Q,
                             const WfPlan& plan, hipStream_t stream, LaunchTimer* timer, uint64_t bound) {
    auto begin_k = [&](int cls, hipStream_t s) { if (timer) timer->begin(cls, s); };
    auto end_k = [&](int cls, hipStream_t s) { if (timer) timer->end(cls, s); };
    const WfChoice ch = choose_kernels(choice_input(S, Q, plan, COUNT));
    const bool head = ch.trace == WF_HEAD;   // (then the shadow family is WF_HEAD too)
    const hipStream_t side = plan.side ? plan.side : stream;
    // PT_HEAD_STATS=1 (a diagnostic, not for timed runs: it waits for both streams at every depth): the listed
    // share of each depth's closest-hit and shadow rays, from the list counts, to stderr; of the closest-hit rays,
    // those the head decided as a miss with nothing to shade (k_wf_trace_head<.., STATS>); and the child rays the
    // dropping shade of that depth's vertices did not queue (what it added to the rays counted since the head)
    unsigned long long stat_escaped = 0, stat_rays = 0;   // counters[kEscapeStatCounter] and [0] at the last closest hit
    auto list_stats = [&](int depth, int q, bool shadow) {   // after the closest hit of queue q / the shadow pass of set q
        if (!head || !plan.head_stats) return;
        (void)hipStreamSynchronize(stream);
        (void)hipStreamSynchronize(side);
        std::vector<uint32_t> w(kCountWords);
        if (hipMemcpy(w.data(), Q.counts, kCountWords * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return;
        unsigned long long c[kEscapeStatCounter + 1];
        if (hipMemcpy(c, B.counters, sizeof c, hipMemcpyDeviceToHost) != hipSuccess) return;
        unsigned long long rays = 0, listed = 0;
        for (int g = 0; g < kParts; g++) {
            rays += shadow ? std::min(w[count_word(q * kParts + g) + 1], Q.spcap) : std::min(w[count_word(q * kParts + g)], Q.pcap);
            listed += shadow ? w[list_sh_word(q, g)] : w[list_word(g)];
        }
        std::fprintf(stderr, "head depth %d: %s %llu listed of %llu\n", depth, shadow ? "shadow" : "closest hit", listed, rays);
        if (shadow) {
            std::fprintf(stderr, "head depth %d: shade dropped %llu child rays\n", depth, c[0] - stat_rays);
        } else {
            std::fprintf(stderr, "head depth %d: closest hit %llu of %llu missed with nothing to shade\n", depth,
                         c[kEscapeStatCounter] - stat_escaped, rays);
            stat_escaped = c[kEscapeStatCounter];
            stat_rays = c[0];
        }
    };
    using RayKernel = void (*)(DevScene, WfQueues, int, unsigned long long*);
    using QueueKernel = void (*)(DevScene, WfQueues, int);
    // over the (at most) n rays of queue / shadow set q: a traversal kernel; a head kernel, 256 · kHeadRows rays a
    // block; a linear kernel, its resident grid whatever n is
    auto traverse = [&](RayKernel kernel, uint64_t n, WfGrid cap, hipStream_t s, int q) {
        hipLaunchKernelGGL(kernel, dim3(grid_for(n, kTB, plan.blocks[cap])), dim3(kTB), 0, s, S, Q, q, B.counters);
    };
    auto head_pass = [&](RayKernel kernel, uint64_t n, WfGrid cap, hipStream_t s, int q) {
        hipLaunchKernelGGL(kernel, dim3(grid_for(n, 256u * kHeadRows, plan.blocks[cap])), dim3(256), 0, s, S, Q, q, B.counters);
    };
    auto linear = [&](RayKernel kernel, WfGrid blocks, hipStream_t s, int q) {
        hipLaunchKernelGGL(kernel, dim3(plan.blocks[blocks]), dim3(256), 0, s, S, Q, q, B.counters);
    };
    // a split step's queue kernel: the Volume or SDF records its refill half deferred, staged in `lds` bytes of LDS or not
    auto queue = [&](WfQueueKernel k, QueueKernel plain, QueueKernel staged, uint64_t n, unsigned cap, int32_t lds, hipStream_t s, int q) {
        const dim3 g(grid_for(n, 256, cap));
        if (k == WF_Q_STAGED) hipLaunchKernelGGL(staged, g, dim3(256), (size_t)lds, s, S, Q, q);
        else if (k == WF_Q_PLAIN) hipLaunchKernelGGL(plain, g, dim3(256), 0, s, S, Q, q);
    };
    auto trace = [&](int qi, uint64_t n) {
        const WfGrid g0 = ch.trace_grid[0], g1 = ch.trace_grid[1];
        begin_k(1, stream);
        switch (ch.trace) {
        case WF_SPLIT:   // (a counted pass times the Volume march)
            traverse(k_wf_trace_lanes<COUNT, true>, n, g0, stream, qi);
            traverse(k_wf_trace<COUNT, true, true>, n, g1, stream, qi);
            queue(ch.vol_hits, k_wf_vol_hits<false, COUNT>, k_wf_vol_hits<true, COUNT>, n, 2048, S.vol_lds, stream, qi);
            queue(ch.sdf_hits, k_wf_sdf_hits<false>, k_wf_sdf_hits<true>, n, 8192, S.sdf_lds, stream, qi);
            break;
        case WF_HEAD:
            head_pass(plan.head_stats ? k_wf_trace_head<COUNT, true> : k_wf_trace_head<COUNT, false>, n, g0, stream, qi);
            traverse(k_wf_trace_lanes<COUNT, false, true>, n, g1, stream, qi);
            break;
        case WF_FULL: traverse(k_wf_trace<COUNT, true>, n, g0, stream, qi); break;
        case WF_LANES: traverse(k_wf_trace_lanes<COUNT>, n, g0, stream, qi); break;
        case WF_LINEAR: linear(k_wf_trace_linear<COUNT>, g0, stream, qi); break;
        case WF_LOCKSTEP: traverse(k_wf_trace<COUNT, false>, n, g0, stream, qi); break;
        }
        end_k(1, stream);
    };
    // (ch.early, ch.ldsl and ch.head_ldsl are never set in a counted pass: those forms have no counted instantiation)
    auto shadow = [&](int q, uint64_t n) {   // shadow set q, n rays at most
        const WfGrid g0 = ch.shadow_grid[0], g1 = ch.shadow_grid[1];
        begin_k(3, side);
        switch (ch.shadow) {
        case WF_SPLIT:
            traverse(ch.early ? k_wf_shadow_lanes<false, true, true> : k_wf_shadow_lanes<COUNT, true>, n, g0, side, q);
            traverse(k_wf_shadow<COUNT, true, true>, n, g1, side, q);
            queue(ch.vol_shadow, k_wf_vol_shadow<false, COUNT>, k_wf_vol_shadow<true, COUNT>, n, 2048, S.vol_lds, side, q);
            queue(ch.sdf_shadow, k_wf_sdf_shadow<false>, k_wf_sdf_shadow<true>, n, 8192, S.sdf_lds, side, q);
            break;
        case WF_HEAD:
            head_pass(ch.head_ldsl ? k_wf_shadow_head<false, true> : k_wf_shadow_head<COUNT, false>, n, g0, side, q);
            traverse(ch.early ? k_wf_shadow_lanes<false, false, true, false, true> : k_wf_shadow_lanes<COUNT, false, false, false, true>,
                     n, g1, side, q);
            break;
        case WF_FULL: traverse(k_wf_shadow<COUNT, true>, n, g0, side, q); break;
        case WF_LANES:
            traverse(ch.early ? k_wf_shadow_lanes<false, false, true> : ch.ldsl ? k_wf_shadow_lanes<false, false, false, true>
                                                                               : k_wf_shadow_lanes<COUNT>, n, g0, side, q);
            break;
        case WF_LINEAR: linear(ch.ldsl ? k_wf_shadow_linear<false, true> : k_wf_shadow_linear<COUNT, false>, g0, side, q); break;
        case WF_LOCKSTEP: traverse(ch.ldsl ? k_wf_shadow<false, false, false, true> : k_wf_shadow<COUNT, false>, n, g0, side, q); break;
        }
        end_k(3, side);
    };
    int qi = 0;
    if (head && plan.head_stats) {   // (a pass' later chunks: the head's count so far)
        (void)hipStreamSynchronize(stream);
        (void)hipStreamSynchronize(side);
        (void)hipMemcpy(&stat_escaped, B.counters + kEscapeStatCounter, sizeof stat_escaped, hipMemcpyDeviceToHost);
    }
    trace(qi, bound);
    list_stats(0, qi, false);
    for (int depth = 0; depth <= smp.mb; depth++) {
        const unsigned sg = grid_for(bound, 256, plan.blocks[G_SHADE]);
        auto shade = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(sg), dim3(256), 0, stream, S, smp, Q, qi, B.counters, plan.shade_form);
        };
        begin_k(2, stream);
        // both forms (the one the kept count selects runs, the other returns at once); a routed shade runs
        // the lean and the FULL SCAN kernels, each on its own vertices
        switch (ch.shade) {
        case WF_SHADE_ROUTED: shade(k_wf_shade<COUNT, false, true>); shade(k_wf_shade<COUNT, true, true>); break;
        case WF_SHADE_FULL: shade(k_wf_shade<COUNT, true, false>); shade(k_wf_shade<COUNT, true, true>); break;
        case WF_SHADE_LEAN:
            if (ch.escape_drop(depth)) { shade(k_wf_shade<COUNT, false, false, true>); shade(k_wf_shade<COUNT, false, true, true>); }
            else { shade(k_wf_shade<COUNT, false, false>); shade(k_wf_shade<COUNT, false, true>); }
            break;
        }
        if (ch.shade_miss)   // a routed shade's misses of a textured environment
            hipLaunchKernelGGL(k_wf_shade_miss, dim3(grid_for(bound, 256, 8192)), dim3(256), 0, stream, S, Q, qi);
        end_k(2, stream);
        if (plan.side) {
            (void)hipEventRecord(plan.ev_main, stream);
            (void)hipStreamWaitEvent(side, plan.ev_main, 0);
        }
        const uint64_t children = bound * (uint64_t)(depth == 0 ? plan.root_children : plan.children);
        shadow(1 - qi, children * plan.lights_per_child);
        begin_k(6, side);   // PT_K_ACCUM
        const unsigned ag = grid_for(children * plan.lights_per_child, 256u * kAccWin, 4096);
        hipLaunchKernelGGL((k_wf_nee_accum<COUNT>), dim3(ag), dim3(256), 0, side, Q, 1 - qi, B.counters);
        end_k(6, side);
        if (plan.side) (void)hipEventRecord(plan.ev_side[1 - qi], side);
        list_stats(depth, 1 - qi, true);
        bound = children < Q.cap ? children : Q.cap;
        qi = 1 - qi;
        // trace(d + 1) frees pair word 1 - qi and shade(d + 1) rewrites shadow set 1 - qi: the
        // shadow pass and the light-term accumulation of depth d - 1 read both
        if (plan.side && depth >= 1) (void)hipStreamWaitEvent(stream, plan.ev_side[1 - qi], 0);
        if (depth < smp.mb) {
            trace(qi, bound);
            list_stats(depth + 1, qi, false);
        }
    }
    if (plan.side) {   // the chunk ends with its last two shadow passes
        (void)hipStreamWaitEvent(stream, plan.ev_side[0], 0);
        (void)hipStreamWaitEvent(stream, plan.ev_side[1], 0);
    }
    return hipSuccess;
}
static hipError_t depth_loop(const DevScene& S, const DevSampler& smp, const DevBuffer& B, const WfQueues& Q, const WfPlan& plan,
                             bool count, hipStream_t stream, LaunchTimer* timer, uint64_t bound) {
    return count ? depth_loop<true>(S, smp, B, Q, plan, stream, timer, bound)
                 : depth_loop<false>(S, smp, B, Q, plan, stream, timer, bound);
}

hipError_t wavefront_pass(const DevScene& S, const DevCamera& cam, const DevSampler& smp, const DevPass& P,
                          const DevBuffer& B, const WfQueues& Q, const WfPlan& plan, bool count, hipStream_t stream,
                          LaunchTimer* timer) {
    // Every persistent grid is launched as planned: a zero grid (a kernel whose occupancy query was never made)
    // would fail only at its launch, as "invalid configuration argument" with no kernel named (VERDICT r05 #7a)
    if (!plan.complete() || !plan.chunk) return hipErrorInvalidConfiguration;
    const uint64_t pix_slots = (uint64_t)P.num_tiles * 1024u;
    const int rounds = P.stratified ? P.spp : 1;        // stratified: one Welford sample per sample index
    const int spp_launch = P.stratified ? 1 : P.spp;
    const double spp_d = (double)spp_launch;
    const uint64_t total = pix_slots * (uint64_t)spp_launch * (uint64_t)(P.passes > 1 ? P.passes : 1);
    auto begin_k = [&](int cls) { if (timer) timer->begin(cls, stream); };
    auto end_k = [&](int cls) { if (timer) timer->end(cls, stream); };
    for (int r = 0; r < rounds; r++) {
        for (uint64_t begin = 0; begin < total; begin += plan.chunk) {
            const uint32_t cnt = (uint32_t)((total - begin) < plan.chunk ? (total - begin) : plan.chunk);
            hipError_t e = hipMemsetAsync(Q.counts, 0, kChunkResetWords * sizeof(uint32_t), stream);
            if (e != hipSuccess) return e;
            begin_k(0);
            hipLaunchKernelGGL(k_wf_camera, dim3(grid_for(cnt, 256, 4096)), dim3(256), 0, stream, cam, P, Q, begin,
                               cnt, spp_launch, r);
            end_k(0);
            if ((e = depth_loop(S, smp, B, Q, plan, count, stream, timer, cnt)) != hipSuccess) return e;
        }
        begin_k(4);
        hipLaunchKernelGGL(k_wf_finalize, dim3(grid_for(pix_slots, 256, 4096)), dim3(256), 0, stream, P, B, Q, spp_d);
        end_k(4);
    }
    return hipGetLastError();
}

hipError_t wavefront_extra(const DevScene& S, const DevCamera& cam, const DevSampler& smp, const DevPass& P,
                           const DevBuffer& B, const WfQueues& Q, const WfPlan& plan, bool count, hipStream_t stream,
                           LaunchTimer* timer, int firefly, int32_t K, uint32_t sample_base, uint64_t entries,
                           const uint32_t* plist, const double* snap, uint32_t* next_list, uint32_t* next_count) {
    if (K <= 0 || entries == 0) return hipSuccess;
    auto begin_k = [&](int cls) { if (timer) timer->begin(cls, stream); };
    auto end_k = [&](int cls) { if (timer) timer->end(cls, stream); };
    WfQueues Qx = Q;
    Qx.acc = Q.acc_s;  // per-sample accumulators
    // entries per chunk (whole pixels; smaller extra-phase chunks measured slower)
    uint64_t per_chunk = std::max(plan.chunk, plan.chunk_extra) / (uint64_t)K;
    if (per_chunk < 1) per_chunk = 1;
    for (uint64_t e0 = 0; e0 < entries; e0 += per_chunk) {
        const uint64_t ne = (entries - e0) < per_chunk ? (entries - e0) : per_chunk;
        const uint32_t cnt = (uint32_t)(ne * (uint64_t)K);
        hipError_t e = hipMemsetAsync(Q.counts, 0, kChunkResetWords * sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
        begin_k(0);
        hipLaunchKernelGGL(k_wf_camera_extra, dim3(grid_for(cnt, 256, 4096)), dim3(256), 0, stream, cam, P, Qx,
                           e0 * (uint64_t)K, cnt, K, sample_base, plist, firefly == EXTRA_ADD_SCALED ? 1 : 0);
        end_k(0);
        if ((e = depth_loop(S, smp, B, Qx, plan, count, stream, timer, cnt)) != hipSuccess) return e;
        begin_k(4);
        hipLaunchKernelGGL(k_wf_finalize_extra, dim3(grid_for(ne, 256, 4096)), dim3(256), 0, stream, P, B, Q.acc_s,
                           e0, (uint32_t)ne, K, plist, firefly == EXTRA_FIREFLY_STOP ? 1 : 0, snap, next_list,
                           next_count);
        end_k(4);
    }
    return hipGetLastError();
}

hipError_t wavefront_grids(WfGrids& grids) {
    // every persistent grid: the kernel whose resident capacity sizes it (its family's widest form), block size, cap
    static const struct { WfGrid grid; const void* kernel; int block; uint32_t cap; } kGrids[] = {
        {G_TRACE, (const void*)k_wf_trace<false, false>, kTB, kWfMaxBlocks},
        {G_SHADE, (const void*)k_wf_shade<false, false, false>, 256, 1u << 20},
        {G_SHADOW, (const void*)k_wf_shadow<false, false>, kTB, kWfMaxBlocks},
        {G_LANES_TRACE, (const void*)k_wf_trace_lanes<false>, kTB, kWfMaxBlocks},
        {G_LANES_SHADOW, (const void*)k_wf_shadow_lanes<false>, kTB, kWfMaxBlocks},
        {G_FULL_TRACE, (const void*)k_wf_trace<false, true>, kTB, kWfMaxBlocks},
        {G_FULL_SHADOW, (const void*)k_wf_shadow<false, true>, kTB, kWfMaxBlocks},
        {G_LINEAR_TRACE, (const void*)k_wf_trace_linear<false>, 256, 1u << 20},
        {G_LINEAR_SHADOW, (const void*)k_wf_shadow_linear<false, true>, 256, 1u << 20},
        {G_HEAD_TRACE, (const void*)k_wf_trace_head<false>, 256, 1u << 20},
        {G_HEAD_SHADOW, (const void*)k_wf_shadow_head<false, true>, 256, 1u << 20},
        {G_LIST_TRACE, (const void*)k_wf_trace_lanes<false, false, true>, kTB, kWfMaxBlocks},
        {G_LIST_SHADOW, (const void*)k_wf_shadow_lanes<false, false, false, false, true>, kTB, kWfMaxBlocks},
    };
    static_assert(sizeof kGrids / sizeof kGrids[0] == kWfGridCount, "one row per WfGrid");
    int dev = 0, cus = 0, nb = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    for (const auto& g : kGrids) {
        if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, g.kernel, g.block, 0);
        if (e != hipSuccess) break;
        uint64_t blocks = (uint64_t)nb * (uint64_t)cus / kParts * kParts;
        if (blocks < (uint64_t)kParts) blocks = kParts;
        grids.blocks[g.grid] = (uint32_t)(blocks < g.cap ? blocks : g.cap / kParts * kParts);
    }
    return e;
}

hipError_t select_pixels(const DevPass& P, const DevBuffer& B, int kind, uint32_t* plist, uint32_t* count,
                         hipStream_t stream) {
    hipError_t e = hipMemsetAsync(count, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const uint64_t pix_slots = (uint64_t)P.num_tiles * 1024u;
    hipLaunchKernelGGL(k_wf_select, dim3(grid_for(pix_slots, 256, 4096)), dim3(256), 0, stream, P, B, kind, plist,
                       count);
    return hipGetLastError();
}

}  // namespace pt
