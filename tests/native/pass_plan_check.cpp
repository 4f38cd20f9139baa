// pass_plan_check.cpp — the render-pass plan and the kernel choice (ptsharp_amd/csrc/pt_pass_plan.cpp) on the CPU.
//
//   pass_plan_check            a dense sweep of valid inputs; every plan is checked against what the queues must
//                              hold, worked out here from the sampler alone (not with the plan's own helpers); then
//                              every choice of the grid of tests/test_wf_choice_host.py against what must hold of it
//   pass_plan_check --rows     reads requests from stdin, one per line, and prints one answer line each
//                              (tests/test_pass_plan_host.py feeds it tests/golden/pass_plan_v1.json):
//       plan <19 inputs in the golden table's column order>
//            -> rc engine chunk chunk_extra root_children children lights_per_child cap scap side
//               passes_per_launch split_step <tab> message      (a refusal: rc, zeros, the message)
//       budget <bytes>                            -> wf_cap_for_budget
//       limit <entries>                           -> wf_cap_for_limit
//       batch <total bytes> <bytes per pass> <knob>  -> batch_passes_for
//       choice <22 inputs in the column order of tests/golden/wf_kernel_choice_v1.json>
//            -> trace shadow early ldsl head_ldsl shade shade_miss vol_hits sdf_hits vol_shadow sdf_shadow
//               and the four grids (closest hit, shadow; first and second launch), all by name
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <set>

#include "../../ptsharp_amd/csrc/pt_pass_plan.h"

static long g_fail = 0, g_plans = 0, g_wavefront = 0, g_refused = 0, g_split = 0, g_multi_chunk = 0;

static void print_input(const pt::PassPlanInput& in) {
    std::printf("  tiles %d spp %d strat %d engine %d flags %d adaptive %d firefly %d passes %d fh %d mb %d light %d spec %d lights %d "
                "cap %u bpm %d side %d\n", in.num_tiles, in.spp, in.stratified, in.engine, in.flags, in.adaptive_samples, in.firefly_samples,
                in.passes, in.first_hit_samples, in.max_bounces, in.light_mode, in.specular_mode, in.num_lights, in.wf_max_cap,
                in.batch_passes_max, in.knobs.side_stream);
}

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (g_fail++ < 20) { std::printf("FAILED %s (line %d)\n", #cond, __LINE__); print_input(in); } \
        }                                                                    \
    } while (0)

// Camera samples the fullest of the 8 partitions gets: 256-sample blocks dealt round-robin.
static uint64_t fullest(uint64_t samples) { return ((samples + 255) / 256 + 7) / 8 * 256; }

static void check_plan(const pt::PassPlanInput& in) {
    const pt::PassPlan p = pt::plan_pass(in);
    g_plans++;
    if (p.rc != PT_OK) { g_refused++; CHECK(p.message && p.message[0]); return; }
    // what one camera sample can put into the queues (Sampler.cs: ⌊√FH⌋² first-hit samples, every specular mode but
    // Naive splits the first hit in two, SpecularModeAll every later one too; LightModeAll one shadow ray per light)
    const int n_root = (int)std::floor(std::sqrt((double)in.first_hit_samples));
    const double root = (double)(n_root * n_root > 0 ? n_root * n_root : 1) * (in.specular_mode != PT_SPEC_NAIVE ? 2.0 : 1.0);
    const double growth = in.specular_mode == PT_SPEC_ALL ? std::ldexp(1.0, in.max_bounces > 1 ? in.max_bounces - 1 : 0) : 1.0;
    const double per_sample = root * growth;
    const double per_sample_nee = per_sample * (in.light_mode == PT_LIGHT_ALL ? (double)(in.num_lights > 1 ? in.num_lights : 1) : 1.0);
    const uint64_t part = in.wf_max_cap / pt::kParts;
    const uint64_t spp_launch = in.stratified ? 1 : (uint64_t)in.spp;
    const uint64_t total = (uint64_t)in.num_tiles * 1024u * spp_launch * (uint64_t)p.passes_per_launch;
    CHECK(p.engine == PT_ENGINE_WAVEFRONT || p.engine == PT_ENGINE_MEGAKERNEL);
    CHECK(in.engine == PT_ENGINE_AUTO || p.engine == in.engine);
    CHECK(p.root_children == (uint32_t)root && p.children == (in.specular_mode == PT_SPEC_ALL ? 2u : 1u));
    CHECK(p.lights_per_child == (uint32_t)(per_sample_nee / per_sample));
    CHECK(p.passes_per_launch >= 1 && p.passes_per_launch <= (in.passes > 1 ? in.passes : 1));
    CHECK(p.split_step >= 0 && p.split_step <= (in.passes > 1 ? in.passes : 1));
    CHECK(p.split_step == 0 || in.passes > 1);
    CHECK(p.passes_per_launch == 1 || p.passes_per_launch <= in.batch_passes_max);
    CHECK(p.split_step <= 1 || p.split_step <= in.batch_passes_max);
    CHECK(p.chunk <= total);
    if (p.chunk > 256) CHECK((double)fullest(p.chunk) * (per_sample_nee > 1.0 ? per_sample_nee : 1.0) <= (double)part);
    if (p.chunk < total) CHECK(p.chunk % 256 == 0);
    CHECK(p.chunk_extra >= p.chunk);
    if (p.chunk_extra > p.chunk) CHECK(p.chunk_extra % (1024u * (uint64_t)(in.adaptive_samples > 1 ? in.adaptive_samples : 1)) == 0);
    if (p.split_step > 0) { g_split++; return; }
    if (p.engine != PT_ENGINE_WAVEFRONT) return;
    g_wavefront++;
    if (p.chunk < total) g_multi_chunk++;
    CHECK(p.chunk >= 1);
    CHECK(p.cap % pt::kParts == 0 && p.scap % pt::kParts == 0 && p.cap <= in.wf_max_cap && p.scap <= in.wf_max_cap);
    CHECK((double)fullest(p.chunk_extra) * per_sample <= (double)(p.cap / pt::kParts));       // the widest depth
    CHECK((double)fullest(p.chunk_extra) <= (double)(p.cap / pt::kParts));                    // the camera rays
    CHECK((double)fullest(p.chunk_extra) * per_sample_nee <= (double)(p.scap / pt::kParts));  // its shadow slots
    if (in.knobs.side_stream < 0) CHECK(p.use_side == ((double)p.chunk * per_sample <= pt::kSideStreamMaxRays));
    else CHECK(p.use_side == (in.knobs.side_stream == 1));
    CHECK((uint64_t)in.adaptive_samples <= p.chunk);
}

// The bounds keep every product an exact integer in a double (below 2^53) and inside the integer it is converted
// to: at most 8160 tiles x 17 spp x 8 passes camera samples (1.1e9), 32 first-hit children, growth 2^15, 40 lights.
static void sweep() {
    pt::PassPlanInput in;
    in.width = 3840; in.height = 2160;
    const int light_cases[4][2] = {{PT_LIGHT_RANDOM, 1}, {PT_LIGHT_ALL, 0}, {PT_LIGHT_ALL, 3}, {PT_LIGHT_ALL, 40}};
    for (int tiles : {1, 2, 3, 13, 64, 255, 2040, 8160})
    for (int spp : {1, 2, 3, 16, 17})
    for (int strat = 0; strat < 2; strat++)
    for (int passes : {1, 8})
    for (int fh : {1, 5, 16})
    for (int mb : {0, 1, 4, 16})
    for (int spec = 0; spec < 3; spec++)
    for (const auto& lc : light_cases)
    for (int adaptive : {0, 4, 32})
    for (int firefly : {0, 3})
    for (int serial = 0; serial < 2; serial++)
    for (int lg = 13; lg <= 29; lg++) {
        in.num_tiles = tiles; in.spp = spp; in.stratified = strat; in.passes = passes;
        in.first_hit_samples = fh; in.max_bounces = mb; in.specular_mode = spec; in.light_mode = lc[0]; in.num_lights = lc[1];
        in.adaptive_samples = adaptive; in.firefly_samples = firefly; in.flags = serial ? PT_PASS_SERIAL : 0;
        in.wf_max_cap = 1u << lg;
        // the remaining inputs change with the others rather than multiply them: every value meets every value of
        // each loop above many times over
        const unsigned mix = (unsigned)(tiles + spp + fh + mb + lg + adaptive);
        in.engine = (int)(mix % 3u);
        in.batch_passes_max = (mix / 3u) % 3u == 0 ? 1 : (mix / 3u) % 3u == 1 ? 3 : 1000;
        in.knobs.side_stream = (int)((mix / 9u) % 3u) - 1;
        check_plan(in);
    }
}

// ---- the kernel choice (pt::choose_kernels)
static const char* const kFamilyNames[] = {"lockstep", "full", "lanes", "head", "linear", "split"};
static const char* const kShadeNames[] = {"lean", "full", "routed"};
static const char* const kQueueNames[] = {"none", "plain", "staged"};
static const char* const kGridNames[] = {"trace", "shade", "shadow", "lanes_trace", "lanes_shadow", "full_trace", "full_shadow",
                                         "linear_trace", "linear_shadow", "head_trace", "head_shadow", "list_trace", "list_shadow"};
static_assert(sizeof kGridNames / sizeof kGridNames[0] == pt::kWfGridCount, "the 13 grids");

static bool in_range(int v, int n) { return v >= 0 && v < n; }

// The choice's value as one number (every field in range: check_choice looks first), for counting distinct outcomes.
static uint64_t choice_key(const pt::WfChoice& c) {
    uint64_t k = 0;
    for (int v : {(int)c.trace, (int)c.shadow, (int)c.early, (int)c.ldsl, (int)c.head_ldsl, (int)c.shade, (int)c.shade_miss, (int)c.vol_hits,
                  (int)c.sdf_hits, (int)c.vol_shadow, (int)c.sdf_shadow, (int)c.trace_grid[0], (int)c.trace_grid[1], (int)c.shadow_grid[0],
                  (int)c.shadow_grid[1]})
        k = k * 16 + (uint64_t)v;
    return k;
}

#define CHECK_CHOICE(cond)                                                   \
    do {                                                                     \
        if (!(cond) && g_fail++ < 20) std::printf("FAILED %s (line %d) at choice %ld\n", #cond, __LINE__, g_choices); \
    } while (0)

static long g_choices = 0, g_family[2][6];
static std::set<uint64_t> g_outcomes;
static uint64_t g_last_outcome = 0;

// What must hold of every choice, from the inputs alone (none of choose_kernels' own predicates is used).
static void check_choice(const pt::WfChoiceInput& in) {
    using namespace pt;
    const WfChoice c = choose_kernels(in);
    g_choices++;
    // exactly one closest-hit family, one shadow family, one shade family; every grid named is one of the 13
    const bool ranges = in_range(c.trace, 6) && in_range(c.shadow, 6) && in_range(c.shade, 3) && in_range(c.vol_hits, 3) &&
                        in_range(c.sdf_hits, 3) && in_range(c.vol_shadow, 3) && in_range(c.sdf_shadow, 3) &&
                        in_range(c.trace_grid[0], kWfGridCount) && in_range(c.trace_grid[1], kWfGridCount) &&
                        in_range(c.shadow_grid[0], kWfGridCount) && in_range(c.shadow_grid[1], kWfGridCount);
    CHECK_CHOICE(ranges);
    if (!ranges) return;
    g_family[0][c.trace]++;
    g_family[1][c.shadow]++;
    if (g_outcomes.empty() || choice_key(c) != g_last_outcome) g_outcomes.insert(g_last_outcome = choice_key(c));
    // a counted pass has no LDSL and no EARLY form; the two never combine
    if (in.counted) CHECK_CHOICE(!c.early && !c.ldsl && !c.head_ldsl);
    CHECK_CHOICE(!(c.early && c.ldsl));
    if (c.early) CHECK_CHOICE(in.knobs.tail_early != 0);
    if (c.ldsl || c.head_ldsl) CHECK_CHOICE(in.num_lights <= kLdsLights);
    if (c.head_ldsl) CHECK_CHOICE(c.shadow == WF_HEAD);
    // head: the refill kernels run (a lean scene; forced, or by its BVH's size), unsplit, for both kinds of ray
    const bool refill = !in.full_geom && (in.knobs.lanes == 1 || (in.knobs.lanes < 0 && in.tri_num_nodes > kLanesMinNodes));
    CHECK_CHOICE((c.trace == WF_HEAD) == (c.shadow == WF_HEAD));
    if (c.trace == WF_HEAD) CHECK_CHOICE(refill && in.knobs.head != 0);
    if (c.trace == WF_LANES || c.shadow == WF_LANES) CHECK_CHOICE(refill);
    if (in.knobs.lanes == 0) CHECK_CHOICE(c.trace != WF_LANES && c.trace != WF_HEAD && c.trace != WF_SPLIT);
    // row-4 shapes are traversed by the FULL kernels only, whole or as the second half of a split
    CHECK_CHOICE((in.full_geom != 0) == (c.trace == WF_FULL || c.trace == WF_SPLIT));
    CHECK_CHOICE((in.full_geom != 0) == (c.shadow == WF_FULL || c.shadow == WF_SPLIT));
    if (c.shadow == WF_SPLIT) CHECK_CHOICE(c.trace == WF_SPLIT && in.lights_lean);
    if (c.trace == WF_SPLIT) CHECK_CHOICE(in.knobs.lanes < 0);
    // linear: no triangles, no SDF, no Volume, what fits its LDS
    if (c.trace == WF_LINEAR || c.shadow == WF_LINEAR)
        CHECK_CHOICE(c.trace == c.shadow && in.tri_num_nodes <= 0 && in.num_sdf <= 0 && in.num_vol <= 0 && in.ana_count <= kLinRecs &&
                     in.num_planes <= kLinPlanes && in.ana_linear && in.knobs.linear != 0);
    // each launch's grid is its own kernel's
    const int tg[6][2] = {{G_TRACE, G_TRACE}, {G_FULL_TRACE, G_FULL_TRACE}, {G_LANES_TRACE, G_LANES_TRACE}, {G_HEAD_TRACE, G_LIST_TRACE},
                          {G_LINEAR_TRACE, G_LINEAR_TRACE}, {G_LANES_TRACE, G_FULL_TRACE}};
    const int sg[6][2] = {{G_SHADOW, G_SHADOW}, {G_FULL_SHADOW, G_FULL_SHADOW}, {G_LANES_SHADOW, G_LANES_SHADOW}, {G_HEAD_SHADOW, G_LIST_SHADOW},
                          {G_LINEAR_SHADOW, G_LINEAR_SHADOW}, {G_LANES_SHADOW, G_FULL_SHADOW}};
    CHECK_CHOICE(c.trace_grid[0] == tg[c.trace][0] && c.trace_grid[1] == tg[c.trace][1]);
    CHECK_CHOICE(c.shadow_grid[0] == sg[c.shadow][0] && c.shadow_grid[1] == sg[c.shadow][1]);
    // the queue kernels: after a split step only, where the scene has such records (and the Volume queue exists)
    CHECK_CHOICE((c.vol_hits != WF_Q_NONE) == (c.trace == WF_SPLIT && in.volq && in.num_vol > 0));
    CHECK_CHOICE((c.sdf_hits != WF_Q_NONE) == (c.trace == WF_SPLIT && in.num_sdf > 0));
    CHECK_CHOICE((c.vol_shadow != WF_Q_NONE) == (c.shadow == WF_SPLIT && in.volq_sh && in.num_vol > 0));
    CHECK_CHOICE((c.sdf_shadow != WF_Q_NONE) == (c.shadow == WF_SPLIT && in.num_sdf > 0));
    for (pt::WfQueueKernel q : {c.vol_hits, c.vol_shadow}) CHECK_CHOICE(q == WF_Q_NONE || (q == WF_Q_STAGED) == (in.vol_lds > 0));
    for (pt::WfQueueKernel q : {c.sdf_hits, c.sdf_shadow}) CHECK_CHOICE(q == WF_Q_NONE || (q == WF_Q_STAGED) == (in.sdf_lds > 0));
    // shade
    CHECK_CHOICE((c.shade == WF_SHADE_LEAN) == !in.full && (c.shade == WF_SHADE_ROUTED) == (in.full && in.shade_route));
    CHECK_CHOICE(c.shade_miss == (c.shade == WF_SHADE_ROUTED && in.env_tex >= 0));
}

// The grid of tests/test_wf_choice_host.py, whole (the test feeds every kChoiceStride-th row of it through --rows).
static void sweep_choices() {
    pt::WfChoiceInput in;
    for (int tri : {0, 1, pt::kLanesMinNodes, pt::kLanesMinNodes + 1})
    for (int recs : {0, pt::kLinRecs, pt::kLinRecs + 1})
    for (int planes : {0, pt::kLinPlanes, pt::kLinPlanes + 1})
    for (int lights : {1, pt::kLdsLights, pt::kLdsLights + 1})
    for (int ana_nodes : {0, 3})
    for (int full = 0; full < 2; full++)
    for (int full_geom = 0; full_geom <= full; full_geom++)
    for (int bits = 0; bits < 1 << 14; bits++)
    for (int lanes = -1; lanes <= 1; lanes++) {
        auto bit = [&](int b) { return (bits >> b) & 1; };
        in.tri_num_nodes = tri; in.ana_count = recs; in.num_planes = planes; in.num_lights = lights; in.ana_num_nodes = ana_nodes;
        in.full = full; in.full_geom = full_geom; in.knobs.lanes = lanes;
        in.ana_linear = bit(0); in.lights_lean = bit(1); in.shade_route = bit(2); in.env_tex = bit(3) - 1;
        in.sdf_lds = 64 * bit(4); in.vol_lds = 64 * bit(5); in.num_sdf = 2 * bit(6); in.num_vol = bit(7);
        in.volq = bit(8) != 0; in.volq_sh = bit(9) != 0; in.knobs.head = bit(10); in.knobs.linear = bit(11) - 1;
        in.knobs.tail_early = bit(12); in.counted = bit(13) != 0;
        check_choice(in);
    }
}

static int rows() {
    char line[1024];
    while (std::fgets(line, sizeof line, stdin)) {
        unsigned long long a = 0, b = 0;
        long long k = 0;
        pt::PassPlanInput in;
        pt::WfChoiceInput ci;
        int counted = 0, volq = 0, volq_sh = 0;
        if (std::sscanf(line, "choice %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &ci.full, &ci.full_geom,
                        &ci.tri_num_nodes, &ci.ana_num_nodes, &ci.ana_count, &ci.ana_linear, &ci.num_planes, &ci.num_sdf, &ci.num_vol,
                        &ci.num_lights, &ci.lights_lean, &ci.shade_route, &ci.env_tex, &ci.sdf_lds, &ci.vol_lds, &volq, &volq_sh,
                        &ci.knobs.lanes, &ci.knobs.head, &ci.knobs.linear, &ci.knobs.tail_early, &counted) == 22) {
            ci.volq = volq != 0; ci.volq_sh = volq_sh != 0; ci.counted = counted != 0;
            const pt::WfChoice c = pt::choose_kernels(ci);
            std::printf("%s %s %d %d %d %s %d %s %s %s %s %s %s %s %s\n", kFamilyNames[c.trace], kFamilyNames[c.shadow], (int)c.early, (int)c.ldsl,
                        (int)c.head_ldsl, kShadeNames[c.shade], (int)c.shade_miss, kQueueNames[c.vol_hits], kQueueNames[c.sdf_hits],
                        kQueueNames[c.vol_shadow], kQueueNames[c.sdf_shadow], kGridNames[c.trace_grid[0]], kGridNames[c.trace_grid[1]],
                        kGridNames[c.shadow_grid[0]], kGridNames[c.shadow_grid[1]]);
        } else if (std::sscanf(line, "budget %llu", &a) == 1) std::printf("%u\n", pt::wf_cap_for_budget((size_t)a));
        else if (std::sscanf(line, "limit %llu", &a) == 1) std::printf("%u\n", pt::wf_cap_for_limit(a));
        else if (std::sscanf(line, "batch %llu %llu %lld", &a, &b, &k) == 3)
            std::printf("%d\n", pt::batch_passes_for((size_t)a, (size_t)b, (int64_t)k));
        else if (std::sscanf(line, "plan %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %u %d %d", &in.width, &in.height, &in.num_tiles,
                             &in.spp, &in.stratified, &in.engine, &in.flags, &in.adaptive_samples, &in.firefly_samples, &in.passes,
                             &in.first_hit_samples, &in.max_bounces, &in.light_mode, &in.specular_mode, &in.num_lights, &counted,
                             &in.wf_max_cap, &in.batch_passes_max, &in.knobs.side_stream) == 19) {
            in.counted = counted != 0;
            pt::PassPlan p = pt::plan_pass(in);
            if (p.rc != PT_OK) {
                const pt::PassPlan refused = p;
                p = pt::PassPlan{};
                p.rc = refused.rc; p.message = refused.message; p.passes_per_launch = 0;
            }
            std::printf("%d %d %" PRIu64 " %" PRIu64 " %u %u %u %u %u %d %d %d\t%s\n", p.rc, p.engine, p.chunk, p.chunk_extra, p.root_children,
                        p.children, p.lights_per_child, p.cap, p.scap, p.use_side ? 1 : 0, p.passes_per_launch, p.split_step, p.message);
        } else {
            std::printf("bad request: %s", line);
            return 2;
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--rows")) return rows();
    sweep();
    sweep_choices();
    std::printf("choices %ld: distinct %zu; closest hit", g_choices, g_outcomes.size());
    for (int f = 0; f < 6; f++) std::printf(" %s %ld", kFamilyNames[f], g_family[0][f]);
    std::printf("; shadow");
    for (int f = 0; f < 6; f++) std::printf(" %s %ld", kFamilyNames[f], g_family[1][f]);
    std::printf("\nplans %ld: wavefront %ld (in several chunks %ld), split %ld, refused %ld\n", g_plans, g_wavefront, g_multi_chunk,
                g_split, g_refused);
    std::printf("pass_plan_check: %ld failures\n", g_fail);
    return g_fail ? 1 : 0;
}
