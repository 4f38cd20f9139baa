// pt_pass_plan.cpp — the render-pass plan (pt_pass_plan.h): host arithmetic only.
#include "pt_pass_plan.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace pt {

uint32_t wf_cap_for_budget(size_t budget_bytes) {
    uint32_t cap = kWfMaxCapLimit;
    while (cap > kWfMinCapLimit && (size_t)cap * kWfBytesPerEntry > budget_bytes) cap >>= 1;
    return cap;
}

uint32_t wf_cap_for_limit(unsigned long long entries) {
    uint32_t cap = kWfMaxCapLimit;
    while (cap > (uint32_t)kParts * 1024u && cap > entries) cap >>= 1;
    return cap;
}

int32_t batch_passes_for(size_t total_bytes, size_t bytes_per_pass, int64_t knob_max_passes) {
    int64_t k = (int64_t)std::max<size_t>(1, (total_bytes / 8) / std::max<size_t>(bytes_per_pass, 1));
    if (knob_max_passes > 0) k = std::min(k, knob_max_passes);
    return (int32_t)std::min<int64_t>(k, INT32_MAX);
}

namespace {

PassPlan refuse(int rc, const char* message) {
    PassPlan p;
    p.rc = rc;
    p.message = message;
    return p;
}

// What decides a chunk's size: the partition's entries and what one camera sample can put into them.
struct Fit {
    double pmax;             // entries of one partition, at most (wf_max_cap / kParts)
    double per_sample_nee;   // shadow-ray slots per camera sample: the widest a sample gets
    int32_t spp_launch;
    double group_max(uint64_t samples) const { return (double)deal_group_max(samples, spp_launch); }
};

// The largest chunk of at most `want` camera samples whose fullest partition fits.  Queues are kParts
// partitions.  Camera samples are dealt to the XCD groups in 256-sample blocks, so a group gets at most
// ceil(ceil(chunk/256)/kParts)·256 of them, and everything it appends stays in its own partition.
uint64_t fit_chunk(const Fit& f, uint64_t want) {
    uint64_t chunk = (uint64_t)std::min<double>((double)want, std::floor(f.pmax / f.per_sample_nee / 256.0) * 256.0 * kParts);
    // the deal's runs can give one partition a little more than an eighth: shrink until it fits
    const uint64_t step = (uint64_t)deal_run(f.spp_launch) * 256u * kParts;
    while (chunk > step && f.group_max(chunk) * std::max(1.0, f.per_sample_nee) > f.pmax) chunk -= step;
    while (chunk > 256 && f.group_max(chunk) * std::max(1.0, f.per_sample_nee) > f.pmax) chunk -= 256;
    return chunk;
}

}  // namespace

PassPlan check_pass_params(const PassPlanInput& in) {
    if (in.spp <= 0) return refuse(PT_ERR_INVALID_ARG, "spp must be >= 1");
    if (in.first_hit_samples <= 0 || in.max_bounces < 0) return refuse(PT_ERR_INVALID_ARG, "bad sampler");
    if (in.specular_mode == PT_SPEC_ALL && in.max_bounces > 32)
        return refuse(PT_ERR_UNSUPPORTED, "SpecularModeAll with MaxBounces > 32");
    if (in.light_mode < 0 || in.light_mode > 1 || in.specular_mode < 0 || in.specular_mode > 2)
        return refuse(PT_ERR_INVALID_ARG, "bad light/specular mode");
    return PassPlan{};
}

PassPlan plan_pass(const PassPlanInput& in) {
    PassPlan plan = check_pass_params(in);
    if (plan.rc != PT_OK) return plan;
    const int n_root = (int)std::sqrt((double)in.first_hit_samples);
    const int nm_root = (in.specular_mode != PT_SPEC_NAIVE) ? 2 : 1;
    const int nm = in.specular_mode == PT_SPEC_ALL ? 2 : 1;
    plan.root_children = (uint32_t)std::max<int64_t>(1, (int64_t)n_root * n_root * nm_root);
    plan.children = (uint32_t)nm;
    plan.lights_per_child = (uint32_t)(in.light_mode == PT_LIGHT_ALL ? std::max(1, in.num_lights) : 1);
    const bool extra = in.adaptive_samples > 0 || in.firefly_samples > 0;
    const bool serial = (in.flags & PT_PASS_SERIAL) != 0;   // Renderer.Render's extra phases (NumCPU == 1)
    // pt_pass_params.passes: K consecutive passes.  Plain RenderParallel passes run as one batch
    // (one launch sequence over all K passes' camera samples, so a small share — one rank's tiles
    // of a multi-GPU frame — fills the GPU like a whole frame); the others pass by pass.
    const int32_t batch = in.passes > 1 ? in.passes : 1;
    if (batch > 1 && in.counted) return refuse(PT_ERR_INVALID_ARG, "counted passes run one at a time (passes = 1)");
    const uint32_t acc_stride = (uint32_t)((size_t)in.width * (size_t)in.height);   // DevPass::acc_stride
    const bool batchable = batch > 1 && !extra && !serial && !in.stratified && in.engine != PT_ENGINE_MEGAKERNEL &&
                           (uint64_t)acc_stride * (uint64_t)batch <= 0xFFFFFFFFull;
    // A batch keeps one set of per-pixel accumulators per pass (72 B per pixel): the sets of one launch
    // sequence stay within an eighth of the device's memory; a larger K runs as consecutive sub-batches,
    // each bit-identical to its passes run one by one (4K at K = 500 would ask for ~300 GB).
    const int32_t sub = batchable ? std::min(batch, in.batch_passes_max) : 1;
    if (batchable && sub == batch) plan.passes_per_launch = batch;
    const int32_t spp_launch = in.stratified ? 1 : in.spp;
    const uint64_t cam_samples = (uint64_t)in.num_tiles * 1024u * (uint64_t)spp_launch * (uint64_t)plan.passes_per_launch;
    double growth = 1.0;   // queue growth beyond depth 1 (SpecularModeAll doubles every depth)
    if (nm == 2) growth = std::ldexp(1.0, std::min(std::max(in.max_bounces - 1, 0), 60));
    const double per_sample = (double)plan.root_children * growth;   // extension rays per camera sample (widest depth)
    const Fit fit{(double)(in.wf_max_cap / kParts), per_sample * (double)plan.lights_per_child, spp_launch};
    plan.chunk = fit_chunk(fit, cam_samples);
    const uint64_t tile = (uint64_t)deal_run(spp_launch) * 256u;   // chunks of whole tiles where they fit
    if (plan.chunk < cam_samples && plan.chunk >= tile) plan.chunk = plan.chunk / tile * tile;
    if (in.adaptive_samples < 0 || in.firefly_samples < 0) return refuse(PT_ERR_INVALID_ARG, "negative extra samples");
    // The adaptive / firefly phases' chunks: as many of their camera samples as the queues may hold (the main
    // loop's chunk is bounded by its own samples: C5's 1-spp pass at 4K gave the 32-sample adaptive phase 32
    // chunks of 8.3M), up to PT_EXTRA_CHUNK_MAX samples, whole tiles' worth of entries.
    plan.chunk_extra = plan.chunk;
    if (extra && !serial) {
        const uint64_t k = (uint64_t)std::max(in.adaptive_samples, 1);
        const uint64_t all = (uint64_t)in.num_tiles * 1024u * k;
        const uint64_t ce = fit_chunk(fit, std::min<uint64_t>(all, (uint64_t)PT_EXTRA_CHUNK_MAX)) / (1024u * k) * (1024u * k);
        if (ce > plan.chunk_extra) plan.chunk_extra = ce;
    }
    plan.engine = in.engine;
    if (plan.engine == PT_ENGINE_AUTO)
        plan.engine = extra || plan.chunk >= 4096 || plan.chunk >= cam_samples ? PT_ENGINE_WAVEFRONT : PT_ENGINE_MEGAKERNEL;
    if (plan.engine == PT_ENGINE_MEGAKERNEL && extra)
        return refuse(PT_ERR_UNSUPPORTED, "adaptive / firefly phases run on the wavefront engine");
    if (plan.engine == PT_ENGINE_WAVEFRONT && plan.chunk < 1)
        return refuse(PT_ERR_UNSUPPORTED, "wavefront queues cannot hold one camera sample of this sampler (use the megakernel)");
    if (plan.engine != PT_ENGINE_WAVEFRONT && plan.engine != PT_ENGINE_MEGAKERNEL) return refuse(PT_ERR_INVALID_ARG, "bad engine");
    if (batch > 1 && !(plan.passes_per_launch > 1 && plan.engine == PT_ENGINE_WAVEFRONT)) {
        // not one batch: the K passes one after another, or sub-batches of `sub` passes
        plan.split_step = (sub > 1 && plan.engine == PT_ENGINE_WAVEFRONT) ? sub : 1;
        return plan;
    }
    if (plan.engine != PT_ENGINE_WAVEFRONT) return plan;
    // Shadow passes on the side stream, beside the next depth's closest-hit pass, when a
    // chunk's widest depth is small enough for the launches' fill and drain to matter (one
    // rank's 1/8 share of C4 passed one at a time, 33M rays: +6.5 %); a full C4 frame (265M)
    // runs 0.3 % slower that way and C2's 16-child chunks (268M) 6.2 % slower (10632 vs 11332
    // Mrays/s, profiles/r03c_c2_*.json): they keep one stream.  The bound is on rays, not
    // camera samples (round 2 used 20M camera samples, which sent C2 to the side stream).
    // PassKnobs::side_stream forces one stream or the side stream.
    plan.use_side = in.knobs.side_stream < 0 ? (double)plan.chunk * per_sample <= kSideStreamMaxRays : in.knobs.side_stream == 1;
    const double group_samples = fit.group_max(plan.chunk_extra);   // (>= chunk's)
    const double need = group_samples * per_sample;   // a partition's widest depth
    const uint32_t pcap = (uint32_t)std::min(fit.pmax, std::max(8192.0, std::max(group_samples, need)));
    const uint32_t spcap = (uint32_t)std::min(fit.pmax, std::max(8192.0, group_samples * fit.per_sample_nee));
    plan.cap = pcap * kParts;
    plan.scap = spcap * kParts;
    if ((uint64_t)in.adaptive_samples > plan.chunk)
        return refuse(PT_ERR_UNSUPPORTED, "adaptive samples exceed one wavefront chunk");
    if (serial && (uint64_t)in.firefly_samples > plan.chunk)
        return refuse(PT_ERR_UNSUPPORTED, "firefly samples exceed one wavefront chunk");
    return plan;
}

WfChoice choose_kernels(const WfChoiceInput& in) {
    const PassKnobs& k = in.knobs;
    const bool full = in.full != 0;        // shade: textures or row-4 shapes
    const bool fullg = in.full_geom != 0;  // traversal: row-4 shapes only
    // Per-lane refill traversal (k_wf_trace_lanes, k_wf_shadow_lanes) where rays are long
    // enough to pay for it: lean scenes with a triangle BVH of more than kLanesMinNodes nodes.
    const bool lanes = !fullg && (k.lanes >= 0 ? k.lanes == 1 : in.tri_num_nodes > kLanesMinNodes);
    const bool ldsl = PT_SHADOW_LDS && in.num_lights <= kLdsLights;   // the lean shadow kernels' lights in LDS
    // a few analytic records and planes, no triangles: k_wf_trace_linear / k_wf_shadow_linear
    const bool linear = PT_LINEAR && k.linear != 0 && !fullg && !lanes && in.ana_linear && in.tri_num_nodes <= 0 && in.num_sdf <= 0 &&
                        in.num_vol <= 0 && in.ana_count <= kLinRecs && in.num_planes <= kLinPlanes;
    // Split traversal (row-4 scenes with a triangle BVH, or with a Volume: PT_SPLIT_VOL): the lean refill kernels take
    // the planes and the triangles at their occupancy, then the FULL lockstep kernels add the analytic BVH (where
    // the §8f row-4 shapes live) from that result.  Shadow rays split only when every light's own t is a lean
    // intersect (spheres, cubes, planes); otherwise the unsplit FULL shadow kernel.
    const bool split = k.lanes < 0 && fullg && (in.tri_num_nodes > kLanesMinNodes || (PT_SPLIT_VOL && in.num_vol > 0));
    const bool split_sh = split && in.lights_lean;
    // Head pass and list-fed refill kernels (k_wf_trace_head / k_wf_shadow_head, then the <.., LIST> forms): where
    // the unsplit refill kernels run and their step loop is triangles only.  Every other scene keeps its kernels.
    const bool head = k.head != 0 && lanes && !split && (in.ana_linear || in.ana_num_nodes <= 0);
    auto family = [&](bool split_here) {
        return split_here ? WF_SPLIT : head ? WF_HEAD : fullg ? WF_FULL : lanes ? WF_LANES : linear ? WF_LINEAR : WF_LOCKSTEP;
    };
    auto queue = [](bool run, int32_t lds) { return !run ? WF_Q_NONE : lds > 0 ? WF_Q_STAGED : WF_Q_PLAIN; };
    static constexpr WfGrid kTraceGrid[][2] = {{G_TRACE, G_TRACE}, {G_FULL_TRACE, G_FULL_TRACE}, {G_LANES_TRACE, G_LANES_TRACE},
                                               {G_HEAD_TRACE, G_LIST_TRACE}, {G_LINEAR_TRACE, G_LINEAR_TRACE}, {G_LANES_TRACE, G_FULL_TRACE}};
    static constexpr WfGrid kShadowGrid[][2] = {{G_SHADOW, G_SHADOW}, {G_FULL_SHADOW, G_FULL_SHADOW}, {G_LANES_SHADOW, G_LANES_SHADOW},
                                                {G_HEAD_SHADOW, G_LIST_SHADOW}, {G_LINEAR_SHADOW, G_LINEAR_SHADOW}, {G_LANES_SHADOW, G_FULL_SHADOW}};
    WfChoice c;
    c.trace = family(split);
    c.shadow = family(split_sh);
    for (int i = 0; i < 2; i++) {
        c.trace_grid[i] = kTraceGrid[c.trace][i];
        c.shadow_grid[i] = kShadowGrid[c.shadow][i];
    }
    // a counted pass takes no EARLY or LDSL form (none is instantiated); EARLY (a test switch) beats LDSL; the
    // refill kernels have the EARLY forms, the unsplit lean kernels and the head kernel the LDSL forms
    c.early = !in.counted && k.tail_early && (c.shadow == WF_SPLIT || c.shadow == WF_HEAD || c.shadow == WF_LANES);
    c.ldsl = !in.counted && ldsl && !c.early && (c.shadow == WF_LANES || c.shadow == WF_LINEAR || c.shadow == WF_LOCKSTEP);
    c.head_ldsl = !in.counted && ldsl && c.shadow == WF_HEAD;
    c.shade = full && in.shade_route ? WF_SHADE_ROUTED : full ? WF_SHADE_FULL : WF_SHADE_LEAN;
    c.shade_miss = c.shade == WF_SHADE_ROUTED && PT_SHADE_MISS && in.env_tex >= 0;
    // the deferred Volume and SDF records of a split step, staged in LDS when they fit (DevScene::vol_lds / sdf_lds)
    c.vol_hits = queue(split && in.volq && in.num_vol > 0, in.vol_lds);
    c.sdf_hits = queue(split && in.num_sdf > 0, in.sdf_lds);
    c.vol_shadow = queue(split_sh && in.volq_sh && in.num_vol > 0, in.vol_lds);
    c.sdf_shadow = queue(split_sh && in.num_sdf > 0, in.sdf_lds);
    // The dropping shade: only where k_wf_trace_head decides the child rays (so the analytic shapes are linear or
    // absent, no row-4 kind, no split), the shade is the lean one, and a miss adds nothing (the head's env_black).
    const bool drop = k.escape_drop != 0 && c.trace == WF_HEAD && c.shade == WF_SHADE_LEAN && in.env_black && in.env_tex < 0;
    c.escape_drop_depths = !drop ? 0 : k.escape_drop == 2 ? kEscapeDropEveryDepth : kEscapeDropDepths;
    return c;
}

}  // namespace pt
