// escape_plan_check.cpp — where the dropping shade runs (pt::choose_kernels' WfChoice::escape_drop_depths,
// ptsharp_amd/csrc/pt_pass_plan.cpp) on the CPU: the grid of pass_plan_check.cpp's choice sweep, thinned, times the
// environment's colour and the PT_ESCAPE_DROP knob.  Checked from the inputs alone:
//   * depths > 0 only where the closest-hit family is the head's, the shade the lean one, the environment black and
//     untextured and the knob not 0; and everywhere that holds;
//   * knob 1: the camera hits only (depth 0); knob 2: every depth;
//   * the new inputs change no other field of the choice.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../ptsharp_amd/csrc/pt_pass_plan.h"

static long g_fail = 0, g_rows = 0, g_on = 0;

#define CHECK(cond)                                                                                        \
    do {                                                                                                   \
        if (!(cond) && g_fail++ < 20) std::printf("FAILED %s (line %d) at row %ld\n", #cond, __LINE__, g_rows); \
    } while (0)

static bool same_but_drop(pt::WfChoice a, pt::WfChoice b) {
    a.escape_drop_depths = b.escape_drop_depths = 0;
    return a.trace == b.trace && a.shadow == b.shadow && a.early == b.early && a.ldsl == b.ldsl && a.head_ldsl == b.head_ldsl &&
           a.shade == b.shade && a.shade_miss == b.shade_miss && a.vol_hits == b.vol_hits && a.sdf_hits == b.sdf_hits &&
           a.vol_shadow == b.vol_shadow && a.sdf_shadow == b.sdf_shadow && !std::memcmp(a.trace_grid, b.trace_grid, sizeof a.trace_grid) &&
           !std::memcmp(a.shadow_grid, b.shadow_grid, sizeof a.shadow_grid);
}

int main() {
    using namespace pt;
    {   // the defaults: a choice input that says nothing of the environment drops nothing
        WfChoiceInput in;
        in.tri_num_nodes = kLanesMinNodes + 1;
        CHECK(in.knobs.escape_drop == 1 && !in.env_black);
        CHECK(choose_kernels(in).trace == WF_HEAD && choose_kernels(in).escape_drop_depths == 0);
        CHECK(!WfChoice{}.escape_drop(0));
    }
    WfChoiceInput in;
    for (int tri : {0, kLanesMinNodes, kLanesMinNodes + 1})
    for (int recs : {0, kLinRecs, kLinRecs + 1})
    for (int ana_nodes : {0, 3})
    for (int full = 0; full < 2; full++)
    for (int full_geom = 0; full_geom <= full; full_geom++)
    for (int bits = 0; bits < 1 << 9; bits++)
    for (int lanes = -1; lanes <= 1; lanes++)
    for (int knob = 0; knob <= 2; knob++)
    for (int black = 0; black < 2; black++) {
        auto bit = [&](int b) { return (bits >> b) & 1; };
        in.tri_num_nodes = tri; in.ana_count = recs; in.ana_num_nodes = ana_nodes; in.full = full; in.full_geom = full_geom;
        in.num_planes = 1; in.num_lights = 2; in.knobs.lanes = lanes;
        in.ana_linear = bit(0); in.lights_lean = bit(1); in.shade_route = bit(2); in.env_tex = bit(3) - 1;
        in.num_sdf = 2 * bit(4); in.num_vol = bit(5); in.volq = in.volq_sh = bit(5) != 0; in.knobs.head = bit(6);
        in.knobs.tail_early = bit(7); in.counted = bit(8) != 0;
        in.knobs.escape_drop = knob; in.env_black = black != 0;
        const WfChoice c = choose_kernels(in);
        g_rows++;
        const bool applies = c.trace == WF_HEAD && c.shade == WF_SHADE_LEAN && black && in.env_tex < 0 && knob != 0;
        CHECK((c.escape_drop_depths > 0) == applies);
        if (applies) {
            g_on++;
            // the head's own conditions, from the inputs: lean geometry, linear or no analytic shapes, untextured
            CHECK(!in.full_geom && !in.full && (in.ana_linear || in.ana_num_nodes <= 0) && in.knobs.head != 0);
            CHECK(c.escape_drop(0));
            CHECK(c.escape_drop(1) == (knob == 2) && c.escape_drop(255) == (knob == 2));
        } else {
            CHECK(!c.escape_drop(0) && !c.escape_drop(1));
        }
        WfChoiceInput base = in;   // as a caller from before the field and the knob existed fills it
        base.env_black = false;
        base.knobs.escape_drop = PassKnobs{}.escape_drop;
        CHECK(same_but_drop(c, choose_kernels(base)) && choose_kernels(base).escape_drop_depths == 0);
    }
    CHECK(g_on > 0 && g_on < g_rows);
    std::printf("rows %ld, dropping shade in %ld\n", g_rows, g_on);
    std::printf("escape_plan_check: %ld failures\n", g_fail);
    return g_fail ? 1 : 0;
}
