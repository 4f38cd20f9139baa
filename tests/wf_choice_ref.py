"""Which kernels a depth of a wavefront pass launches: depth_loop's predicates and launch ladders (pt_wavefront.hip) as
they stood before the choice moved into pt_pass_plan.cpp (choose_kernels), restated expression for expression and rung
for rung.  tests/test_wf_choice_host.py holds the C++ choice to it.

`choose(*row)` takes a row in COLUMNS' order and gives the answer line of `pass_plan_check --rows` to a `choice`
request: the closest-hit and the shadow family, the shadow traversal kernel's EARLY and LDSL forms, k_wf_shadow_head's
LDSL form, the shade family, k_wf_shade_miss, the four queue kernels (none / plain / staged) and the grid that caps the
first and the second launch of the closest hit and of the shadow step (a step of one launch names its grid twice)."""
from __future__ import annotations

K_LANES_MIN_NODES, K_LIN_RECS, K_LIN_PLANES, K_LDS_LIGHTS = 64, 8, 8, 16   # pt_wavefront.hip's limits
PT_LINEAR = PT_SHADOW_LDS = PT_SHADE_MISS = PT_SPLIT_VOL = 1                # and its build switches' defaults

COLUMNS = ("full", "full_geom", "tri_num_nodes", "ana_num_nodes", "ana_count", "ana_linear", "num_planes", "num_sdf",
           "num_vol", "num_lights", "lights_lean", "shade_route", "env_tex", "sdf_lds", "vol_lds", "volq", "volq_sh",
           "lanes", "head", "linear", "tail_early", "counted")
OUT_COLUMNS = ("trace", "shadow", "early", "ldsl", "head_ldsl", "shade", "shade_miss", "vol_hits", "sdf_hits",
               "vol_shadow", "sdf_shadow", "trace_grid0", "trace_grid1", "shadow_grid0", "shadow_grid1")
GRIDS = ("trace", "shade", "shadow", "lanes_trace", "lanes_shadow", "full_trace", "full_shadow", "linear_trace",
         "linear_shadow", "head_trace", "head_shadow", "list_trace", "list_shadow")


def choose(full, full_geom, tri_num_nodes, ana_num_nodes, ana_count, ana_linear, num_planes, num_sdf, num_vol,
           num_lights, lights_lean, shade_route, env_tex, sdf_lds, vol_lds, volq, volq_sh, knob_lanes, knob_head,
           knob_linear, tail_early, count):
    full = full != 0
    fullg = full_geom != 0
    lanes = (not fullg) and ((knob_lanes == 1) if knob_lanes >= 0 else tri_num_nodes > K_LANES_MIN_NODES)
    ldsl = bool(PT_SHADOW_LDS) and num_lights <= K_LDS_LIGHTS
    linear = bool(PT_LINEAR and knob_linear != 0 and (not fullg) and (not lanes) and ana_linear and tri_num_nodes <= 0
                  and num_sdf <= 0 and num_vol <= 0 and ana_count <= K_LIN_RECS and num_planes <= K_LIN_PLANES)
    split = bool(knob_lanes < 0 and fullg and (tri_num_nodes > K_LANES_MIN_NODES or (PT_SPLIT_VOL and num_vol > 0)))
    split_sh = bool(split and lights_lean)
    head = bool(knob_head != 0 and lanes and (not split) and (ana_linear or ana_num_nodes <= 0))

    # trace(qi, n)
    vol_hits = sdf_hits = "none"
    if split:
        trace, tg = "split", ("lanes_trace", "full_trace")
        if volq and num_vol > 0:
            vol_hits = "staged" if vol_lds > 0 else "plain"
        if num_sdf > 0 and sdf_lds > 0:
            sdf_hits = "staged"
        elif num_sdf > 0:
            sdf_hits = "plain"
    elif head:
        trace, tg = "head", ("head_trace", "list_trace")
    else:
        cap = "full_trace" if fullg else "lanes_trace" if lanes else "trace"
        if fullg:
            trace = "full"
        elif lanes:
            trace = "lanes"
        elif linear:
            trace, cap = "linear", "linear_trace"   # plan.linear_trace_blocks blocks, not grid_for
        else:
            trace = "lockstep"
        tg = (cap, cap)

    # the shade step
    shade_miss = 0
    if full and shade_route:
        shade = "routed"
        if PT_SHADE_MISS and env_tex >= 0:
            shade_miss = 1
    elif full:
        shade = "full"
    else:
        shade = "lean"

    # the shadow step
    hg = "full_shadow" if fullg else "lanes_shadow" if lanes else "shadow"
    early = ldsl_form = head_ldsl = 0
    vol_shadow = sdf_shadow = "none"
    if split_sh:
        shadow, sg = "split", ("lanes_shadow", "full_shadow")
        sq = num_sdf > 0
        if count:
            pass
        elif tail_early:
            early = 1
        if volq_sh and num_vol > 0:
            vol_shadow = "staged" if vol_lds > 0 else "plain"
        if sq and sdf_lds > 0:
            sdf_shadow = "staged"
        elif sq:
            sdf_shadow = "plain"
    elif head:
        shadow, sg = "head", ("head_shadow", "list_shadow")
        if count:
            pass
        elif ldsl:
            head_ldsl = 1
        if count:
            pass
        elif tail_early:
            early = 1
    elif fullg:
        shadow, sg = "full", (hg, hg)
    elif lanes:
        shadow, sg = "lanes", (hg, hg)
        if count:
            pass
        elif tail_early:
            early = 1
        elif ldsl:
            ldsl_form = 1
    elif linear:
        shadow, sg = "linear", ("linear_shadow", "linear_shadow")
        if count:
            pass
        elif ldsl:
            ldsl_form = 1
    else:
        shadow, sg = "lockstep", (hg, hg)
        if count:
            pass
        elif ldsl:
            ldsl_form = 1
    return (f"{trace} {shadow} {early} {ldsl_form} {head_ldsl} {shade} {shade_miss} {vol_hits} {sdf_hits} {vol_shadow} "
            f"{sdf_shadow} {tg[0]} {tg[1]} {sg[0]} {sg[1]}")
