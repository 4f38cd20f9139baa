// pt_pass_plan.h — how a render pass runs, decided on the host before anything is allocated or launched
// (pt_pass_plan.cpp): engine, chunk sizes, queue capacities, batch split, side stream (plan_pass), and which kernels
// every depth of a wavefront pass launches (choose_kernels).  Plain arithmetic over
// plain values: no HIP header, no HIP call, no environment (pt_api.hip reads the switches into PassKnobs and
// the device's memory into wf_max_cap / batch_passes_max), so tests/native/pass_plan_check.cpp drives it on
// the CPU.  The deal functions below are shared with the device code (pt_wavefront.h includes this header).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ptsharp_hip.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define PT_PLAN_HD __host__ __device__
#else
#define PT_PLAN_HD
#endif

namespace pt {

// Partitions of every wavefront queue, one per XCD group (pt_wavefront.h WfQueues).
constexpr int kParts = 8;

// k_wf_camera deals a chunk's camera samples to the partitions in runs of deal_run 256-sample
// blocks, the runs round-robin (pt_wavefront.hip): one block (16 pixels' samples) per run.  Runs of
// one 32x32 tile's samples, so that each XCD traces compact patches of the scene, measured slower
// (C4 5899 → 5831 Mrays/s; profiles/r03e_ab_deal.txt).
PT_PLAN_HD inline uint32_t deal_run(int32_t) { return 1u; }
// Camera samples the fullest partition receives from a chunk of `samples`.
PT_PLAN_HD inline uint64_t deal_group_max(uint64_t samples, int32_t spp_launch) {
    const uint64_t run = deal_run(spp_launch), nblk = (samples + 255) / 256, nruns = (nblk + run - 1) / run;
    return (nruns + kParts - 1) / kParts * run * 256;
}

// Queue capacity bound (entries per queue).  A pass is rendered in chunks of camera
// samples whose widest depth fits the queues; every chunk pays the fill and drain of
// 16 persistent launches, so fewer, larger chunks are faster (C4, 16 spp per pass: 8
// chunks of 32M-entry queues 2574 Mrays/s, 2 chunks 2809, one chunk 2853).  The bound is
// the largest power of two in [2^20, 2^29] whose queues, at kWfBytesPerEntry, fit the budget: half of the
// device's memory and half of what is free at the context's first pass (2^29: 123 GB of the MI355X's 288 GB:
// C2's 33M camera samples × 16 children in one chunk).  kWfBytesPerEntry, 229 B, counts what every scene
// allocates per entry (pt_api.hip ensure_wavefront): two extension queues of o, d, throughput r g,
// key + throughput b (2 × 64 B), the hits (16 B), one shadow set (o, n, two weights, lit: 65 B) and the head
// pass' two lists (4 B per extension ray, 16 B per shadow ray).  Not counted, so on top of the budget:
//   * the second shadow set of a context that has run a side-stream pass (65 B per shadow entry; it stays
//     allocated for the context's later passes);
//   * for row-4 scenes only (counted in, they halved C4-sized queues from 2^28 to 2^27 entries and split the
//     pass in two chunks, -3 %): the two deferred-record queues of a scene with SDF shapes or Volumes (sdfq,
//     sdfq_sh: 32 B per entry), with Volumes their record words (volq, volq_sh: 8 B), and under the routed
//     split the heavy queues (hq, hq_sh: 8 B): at most 48 B per entry, 25.8 GB at 2^29 entries;
//   * the per-pixel accumulators (72 B per pixel and pass of a batch, batch_passes_for) and the adaptive /
//     firefly phases' per-sample accumulators (72 B per camera sample of chunk_extra).
// All of it comes out of the half of the device the budget leaves free.
constexpr uint32_t kWfMinCapLimit = 1u << 20, kWfMaxCapLimit = 1u << 29;
constexpr size_t kWfBytesPerEntry = 2 * (16 + 16 + 16 + 16) + 16 + (64 + 1) + (4 + 16);
uint32_t wf_cap_for_budget(size_t budget_bytes);
// PT_WF_MAX_CAP (entries; tests use it to force many chunks): the largest power of two up to it, at least one
// 1024-entry block per partition.
uint32_t wf_cap_for_limit(unsigned long long entries);

// Passes one batch may hold: its accumulator sets (bytes_per_pass each) within an eighth of the device's
// memory; knob_max_passes (PassKnobs::batch_max_passes, 0: none) lowers it.
int32_t batch_passes_for(size_t total_bytes, size_t bytes_per_pass, int64_t knob_max_passes);

#ifndef PT_EXTRA_CHUNK_MAX
#define PT_EXTRA_CHUNK_MAX (64ull << 20)   // camera samples per chunk of the adaptive / firefly phases, at most (round 6: 32M → 64M with the 2^29-entry queues, C5 +1.8 %, profiles/r06ec_ab_extra_chunk.txt)
#endif
constexpr double kSideStreamMaxRays = (double)(64ull << 20);   // a chunk's widest depth, extension rays

// The debug / test switches of a pass, as pt_api.hip read_pass_knobs() finds them in the environment at each
// pt_render_pass call (tests flip them between the passes of one process).
struct PassKnobs {
    int32_t shade_form = 0;     // PT_SHADE_FORM=direct|scan: 1, 2; else 0, chosen per depth from the kept count
    int32_t lanes = -1;         // PT_LANES=0|1: refill traversal kernels never / always; else -1, by BVH size
    int32_t head = 1;           // PT_HEAD=0: no head pass and list-fed refill kernels; else 1, where they apply
    int32_t head_stats = 0;     // PT_HEAD_STATS=1: the lists' counts per depth to stderr (it synchronizes)
    int32_t linear = -1;        // PT_LINEAR=0: no linear kernels; else -1, where they apply
    int32_t side_stream = -1;   // PT_SIDE_STREAM=0|1: one stream / the side stream; else -1, by the chunk's rays
    int32_t tail_early = 0;     // PT_SHADOW_TAIL=early: 1 (WfQueues::tail_early)
    int32_t escape_drop = 1;    // PT_ESCAPE_DROP=0: shade queues every child; all: 2, the dropping shade at every depth;
                                // else 1, where choose_kernels finds it applies (WfChoice::escape_drop)
    int64_t batch_max_passes = 0;          // PT_BATCH_MAX_PASSES: its value, at least 1; 0: not set
    bool wf_max_cap_set = false;           // PT_WF_MAX_CAP is set, to
    unsigned long long wf_max_cap = 0;     // this many entries (read once per context: wf_max_cap() in pt_api.hip)
};

struct PassPlanInput {
    int32_t width = 0, height = 0;   // the image
    int32_t num_tiles = 0;           // 32x32 tiles of this pass: its tile list's, or all of the image's
    // pt_pass_params
    int32_t spp = 0, stratified = 0, engine = 0, flags = 0, adaptive_samples = 0, firefly_samples = 0, passes = 0;
    // pt_sampler
    int32_t first_hit_samples = 0, max_bounces = 0, light_mode = 0, specular_mode = 0;
    int32_t num_lights = 0;          // of the uploaded scene (LightModeAll: shadow-ray slots per child)
    bool counted = false;            // pt_render_pass_counted
    uint32_t wf_max_cap = 0;         // queue capacity bound of the context (wf_cap_for_budget / wf_cap_for_limit)
    int32_t batch_passes_max = 1;    // batch_passes_for; read only when passes > 1
    PassKnobs knobs;
};

struct PassPlan {
    int rc = PT_OK;                  // a pt_status; when not PT_OK the pass is refused with `message` and
    const char* message = "";        // no other field means anything
    int32_t engine = 0;              // PT_ENGINE_WAVEFRONT or PT_ENGINE_MEGAKERNEL
    uint64_t chunk = 0;              // camera samples per chunk
    uint64_t chunk_extra = 0;        // camera samples per chunk of the adaptive / firefly phases (>= chunk: their
                                     // queues and per-sample accumulators are sized for it)
    uint32_t root_children = 0;      // ⌊√FH⌋² · modes at depth 0
    uint32_t children = 0;           // modes at depth >= 1 (1, or 2 under SpecularModeAll)
    uint32_t lights_per_child = 0;   // shadow-ray slots per diffuse child: 1, or #lights under LightModeAll
    int32_t passes_per_launch = 1;   // > 1: the call's K passes as one batch (one launch sequence, one accumulator
                                     // set per pass)
    // > 0: the call's K passes do not run as one batch but as consecutive calls of split_step passes each (1: pass
    // by pass; more: sub-batches); each of those is planned again: passes_per_launch then means nothing, and cap,
    // scap and use_side below stay unset
    int32_t split_step = 0;
    uint32_t cap = 0, scap = 0;      // wavefront engine: entries of a ray queue and of a shadow-ray set
    bool use_side = false;           // wavefront engine: shadow passes on the side stream
};

// The checks of a pass' parameters that come before anything else is looked at (plan_pass makes them first; a
// caller with refusals of its own in between calls this ahead of them to keep their order).
PassPlan check_pass_params(const PassPlanInput& in);

// Never fails otherwise than by a refusal in the result; every input is allowed.
PassPlan plan_pass(const PassPlanInput& in);

// ---- Which kernels every depth of a wavefront pass launches (choose_kernels; DESIGN.md §4 has the rules as a table).
// The limits and build switches the choice shares with the kernels of pt_wavefront.hip:
#ifndef PT_SHADE_MISS
#define PT_SHADE_MISS 1   // routed shade: a textured environment's misses in k_wf_shade_miss (0: in the FULL shade)
#endif
#ifndef PT_LINEAR
#define PT_LINEAR 1        // k_wf_trace_linear / k_wf_shadow_linear for a few analytic records and no triangles
#endif
#ifndef PT_SHADOW_LDS
#define PT_SHADOW_LDS 1    // the lean shadow kernels read a small scene's lights and their records from LDS (stage_lights)
#endif
// Scenes with a Volume take the split traversal whatever their triangle count, for the Volume queue kernels
// (k_wf_vol_*: full waves, the Volume in LDS): the Volume-only scene 495 -> 528 Mrays/s
#ifndef PT_SPLIT_VOL
#define PT_SPLIT_VOL 1
#endif
// The refill kernels run on scenes whose triangle BVH has more than this many nodes (gopher3's five
// analytic shapes: trace 16.0 → 23.5 ms with refill).
constexpr int kLanesMinNodes = 64;
// The linear kernels' records and planes in LDS, at most (stage_linear); k_wf_shade stages as many (stage_shading).
constexpr int kLinRecs = 8, kLinPlanes = 8;
constexpr int kLdsLights = 16;   // lights in LDS, at most (stage_shading, stage_lights: the LDSL shadow kernels)

// The persistent grids of WfGrids (pt_wavefront.h), in the order of wavefront_grids' table.
enum WfGrid : int32_t {
    G_TRACE, G_SHADE, G_SHADOW, G_LANES_TRACE, G_LANES_SHADOW, G_FULL_TRACE, G_FULL_SHADOW, G_LINEAR_TRACE, G_LINEAR_SHADOW,
    G_HEAD_TRACE, G_HEAD_SHADOW, G_LIST_TRACE, G_LIST_SHADOW, kWfGridCount
};
// A traversal step's kernels.  Lockstep: k_wf_trace / k_wf_shadow<.., false>.  Full: their FULL forms (row-4 shapes).
// Lanes: the per-lane refill kernels.  Head: k_wf_*_head, then the list-fed refill kernels.  Linear: k_wf_*_linear.
// Split: the lean refill kernels (<.., SPLIT>), then the FULL lockstep kernels' analytic half, then the queue kernels.
enum WfFamily : int32_t { WF_LOCKSTEP, WF_FULL, WF_LANES, WF_HEAD, WF_LINEAR, WF_SPLIT };
// Lean / full: the direct and the SCAN form of k_wf_shade<COUNT, FULL>.  Routed: the lean SCAN and the FULL SCAN form.
enum WfShade : int32_t { WF_SHADE_LEAN, WF_SHADE_FULL, WF_SHADE_ROUTED };
enum WfQueueKernel : int32_t { WF_Q_NONE, WF_Q_PLAIN, WF_Q_STAGED };   // staged: its records in dynamic LDS

struct WfChoiceInput {
    // of the uploaded scene (DevScene's members of these names)
    int32_t full = 0, full_geom = 0, tri_num_nodes = 0, ana_num_nodes = 0, ana_count = 0, ana_linear = 0, num_planes = 0;
    int32_t num_sdf = 0, num_vol = 0, num_lights = 0, lights_lean = 0, shade_route = 0, env_tex = -1, sdf_lds = 0, vol_lds = 0;
    bool volq = false, volq_sh = false;   // WfQueues::volq / volq_sh are allocated (they outlive a scene without Volumes)
    bool env_black = false;               // DevScene::env is {0, 0, 0} (with env_tex < 0: a miss adds nothing)
    PassKnobs knobs;                      // lanes, head, linear, tail_early, escape_drop
    bool counted = false;
};

struct WfChoice {
    WfFamily trace = WF_LOCKSTEP, shadow = WF_LOCKSTEP;
    // the shadow family's traversal kernel (its list-fed one under WF_HEAD): the EARLY and LDSL forms, never both and
    // never counted; head_ldsl: k_wf_shadow_head's LDSL form
    bool early = false, ldsl = false, head_ldsl = false;
    WfShade shade = WF_SHADE_LEAN;
    bool shade_miss = false;              // k_wf_shade_miss after a routed shade
    WfQueueKernel vol_hits = WF_Q_NONE, sdf_hits = WF_Q_NONE;       // after a split closest hit, in this order
    WfQueueKernel vol_shadow = WF_Q_NONE, sdf_shadow = WF_Q_NONE;   // after split shadow rays
    // what caps each launch's grid: [0] the step's first kernel, [1] its second (WF_HEAD: the list-fed kernel,
    // WF_SPLIT: the FULL half; otherwise as [0]).  The linear kernels launch exactly their member's blocks.
    WfGrid trace_grid[2] = {G_TRACE, G_TRACE}, shadow_grid[2] = {G_SHADOW, G_SHADOW};
    // The dropping form of the lean shade (k_wf_shade<.., DROP>: a child ray that k_wf_trace_head would turn into a
    // miss with nothing to shade is counted and not queued) runs at the depths below this one; 0: at none.
    int32_t escape_drop_depths = 0;
    bool escape_drop(int depth) const { return depth < escape_drop_depths; }
};
// Depths of the dropping shade under the default rule (PassKnobs::escape_drop 1): the camera hits only.  Their
// children are the first bounce, where most rays leave the scene; deeper, the head lists 84-94 % of the rays
// (DESIGN.md §8 has both rules measured).
constexpr int32_t kEscapeDropDepths = 1;
constexpr int32_t kEscapeDropEveryDepth = 1 << 30;

WfChoice choose_kernels(const WfChoiceInput& in);

}  // namespace pt
