// Host-only probe of vidtome_amd/csrc/match_plan.h for tests/test_match_plan_host.py: one call = one plan, flattened.
#include "match_plan.h"

using namespace vtm_match_plan;

// in: B C Ns Nd align mode scout_steps seed_N ordered cus | kp5 kp nsplit seed_dry nsplit_r4 no_xprune   (16 values)
extern "C" void match_plan_probe(const int64_t *in, int64_t *out) {
    const DebugEnv dbg{(int)in[10], (int)in[11], (int)in[12], in[13] != 0, in[14] != 0, in[15] != 0};
    const Layout L = make_layout(in[0], in[1], in[2], in[3], (int)in[4]);
    const FilterPlan P = plan_filter(L, in[0], in[1], in[2], in[3], (int)in[4], (int)in[5], (int)in[6], in[7], in[8] != 0, (int)in[9], dbg);
    const int64_t v[] = {P.KT, P.KP, P.KPS, P.prune, P.cut, P.cut2, P.ns_tiles, P.nd_tiles, P.total_src_tiles, P.patch_tiles,
                         P.ngroups, P.nsplit, P.tiles_per_split, P.grid, P.range_plan, P.tps_r, P.nsplit_r, P.grid_r, P.map_words,
                         P.xsplit, P.xtps, P.xgrid, P.KX, P.refine_grid, P.prep_grid, P.seed_grid, (int64_t)L.total};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) out[i] = v[i];
}
