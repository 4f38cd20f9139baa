// pass_plan_check.cpp — the render-pass plan (ptsharp_amd/csrc/pt_pass_plan.cpp) on the CPU.
//
//   pass_plan_check            a dense sweep of valid inputs; every plan is checked against what the queues must
//                              hold, worked out here from the sampler alone (not with the plan's own helpers)
//   pass_plan_check --rows     reads requests from stdin, one per line, and prints one answer line each
//                              (tests/test_pass_plan_host.py feeds it tests/golden/pass_plan_v1.json):
//       plan <19 inputs in the golden table's column order>
//            -> rc engine chunk chunk_extra root_children children lights_per_child cap scap side
//               passes_per_launch split_step <tab> message      (a refusal: rc, zeros, the message)
//       budget <bytes>                            -> wf_cap_for_budget
//       limit <entries>                           -> wf_cap_for_limit
//       batch <total bytes> <bytes per pass> <knob>  -> batch_passes_for
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>

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

static int rows() {
    char line[1024];
    while (std::fgets(line, sizeof line, stdin)) {
        unsigned long long a = 0, b = 0;
        long long k = 0;
        pt::PassPlanInput in;
        int counted = 0;
        if (std::sscanf(line, "budget %llu", &a) == 1) std::printf("%u\n", pt::wf_cap_for_budget((size_t)a));
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
    std::printf("plans %ld: wavefront %ld (in several chunks %ld), split %ld, refused %ld\n", g_plans, g_wavefront, g_multi_chunk,
                g_split, g_refused);
    std::printf("pass_plan_check: %ld failures\n", g_fail);
    return g_fail ? 1 : 0;
}
