// The host side of vtm_match_filtered* as VALUES: the workspace layout and the launch plan (pruning depths, XCD patch
// geometry, split counts, the scout + range decision, the escape's split, every grid), computed from the call's sizes
// alone.  match_filter.hip launches from it; nothing here includes HIP, so tests/test_match_plan_host.py compiles this
// header as host C++ and pins the plans of every BASELINE level shape.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace vtm_match_plan {

// ---- the tile constants of the kernels in match_filter.hip ----
constexpr int FBD = 128;      // dst rows per tile (MFMA A operand, LDS)
constexpr int FBS = 256;      // src rows per workgroup (B operand, registers), 64 per wave
constexpr int FBK = 64;       // channels per pipeline step = 4 MFMA k-steps = 8 panels
constexpr int CAP = 64;       // candidate slots per src row
// Which products the filter accumulates (the refine pass is exact whatever the filter does; fewer products = less
// MFMA work and operand traffic, wider window = more candidates for the refine pass):
//   SRC_LO && DST_LO : 3 products  hi*hi + hi*lo + lo*hi
//   DST_LO only      : 2 products  (hi_dst + lo_dst) * hi_src
//   neither          : 1 product   hi_dst * hi_src                                  <- shipped
// (the error budget and the window of each: match_filter.hip)
#ifndef VTM_FILTER_PRODUCTS
#define VTM_FILTER_PRODUCTS 1   // build-time choice (1, 2 or 3); the shipped library uses 1
#endif
constexpr bool SRC_LO = VTM_FILTER_PRODUCTS >= 3;
constexpr bool DST_LO = VTM_FILTER_PRODUCTS >= 2;
static_assert(DST_LO || !SRC_LO, "the src lo half is only used together with the dst lo half");
#ifndef VTM_PREP_WAVES
#define VTM_PREP_WAVES 4        // (A/B build switch)
#endif
constexpr int PREP_WAVES = VTM_PREP_WAVES;   // waves per prep_operand workgroup, 64 gathered rows each
#ifndef VTM_RROWS
#define VTM_RROWS 64        // (A/B build switch: 256 = rounds 1-4)
#endif
constexpr int RROWS = VTM_RROWS;   // rows per refine workgroup (256 threads)
#ifndef VTM_XS
#define VTM_XS 128          // (A/B build switch: 256 = 64 src rows per wave, one workgroup per CU: profiles/r04_escape_tile.txt)
#endif
constexpr int XS = VTM_XS;   // listed src rows per workgroup: 32 (or two 32-row MFMA blocks) per wave
constexpr int XD = 128;   // dst rows per tile
constexpr int XK = 32;    // channels per step
constexpr int MODE_SCOUT_RANGE = 1;   // = VTM_MATCH_SCOUT_RANGE of include/vidtome_hip.h (asserted in match_filter.hip)

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct Layout {
    size_t na, nb, ah, al, bh, bl, amax, cnt, seedlb, tilemap, cand, flags, ovf_cnt, ovf, pairs, rest_a, rest_bt, rest_a2, rest_bt2, total;
    int64_t Ns_pad, Nd_pad, C64;
};

inline Layout make_layout(int64_t B, int64_t C, int64_t Ns, int64_t Nd, int align) {
    Layout L;
    L.Ns_pad = cdiv(Ns, FBS) * FBS;
    L.Nd_pad = cdiv(Nd, FBS) * FBS;
    L.C64 = cdiv(C, 64) * 64;
    const int64_t rows_out = align ? Ns : B * Ns;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += align_up(bytes); return at; };
    L.na = take((size_t)B * Ns * 4);
    L.nb = take((size_t)B * Nd * 4);
    L.ah = take((size_t)B * L.C64 * L.Ns_pad * 2);
    L.al = take(SRC_LO ? (size_t)B * L.C64 * L.Ns_pad * 2 : 0);
    L.bh = take((size_t)B * L.C64 * L.Nd_pad * 2);
    L.bl = take(DST_LO ? (size_t)B * L.C64 * L.Nd_pad * 2 : 0);
    L.amax = take((size_t)rows_out * 4);      // amax, cnt and flags are contiguous: cleared together
    L.cnt = take((size_t)rows_out * 4);
    L.seedlb = take((size_t)rows_out * 4);    // certified lower bounds of the rows' exact maxima (seed_kernel -> exact_rows_kernel)
    // the scout's map of live (src tile, dst tile) pairs: one bit per dst tile (inside the cleared range)
    L.tilemap = take((size_t)B * (L.Ns_pad / FBS) * ((L.Nd_pad / FBD + 31) / 32) * 4);
    L.flags = take(256);
    L.ovf_cnt = take((size_t)B * 4);          // per-sample overflow-list lengths (inside the cleared range)
    L.cand = take((size_t)rows_out * CAP * 8);
    L.ovf = take((size_t)rows_out * 4);
    L.pairs = take((size_t)rows_out * CAP * 8);
    L.rest_a = take((size_t)B * L.Ns_pad * 4);
    L.rest_bt = take((size_t)B * (L.Nd_pad / FBD) * 4);
    L.rest_a2 = take((size_t)B * L.Ns_pad * 4);              // ... for the shallow scout's cut
    L.rest_bt2 = take((size_t)B * (L.Nd_pad / FBD) * 4);
    L.total = o;
    return L;
}

// Tuning / A-B hooks of the host side, read from the environment ONCE per process (they were getenv calls on
// every matcher call).  Every one of them is result-preserving: they move launch shapes and pruning depths, never what
// `best` holds.  (A hook that changes results belongs behind a VTM_EXP_* build switch of ablate.h, where it sets a bit of
// VTM_ABLATIONS and the Python binding refuses to load the library.)
struct DebugEnv {
    int kp5, kp, nsplit;              // -1 = unset
    bool seed_dry, nsplit_r4, no_xprune;
};
inline const DebugEnv &debug_env() {
    static const DebugEnv e = [] {
        auto num = [](const char *name) {
            const char *v = getenv(name);
            return v ? atoi(v) : -1;
        };
        DebugEnv d;
        d.kp5 = num("VTM_DEBUG_KP5");
        d.kp = num("VTM_DEBUG_KP");
        d.nsplit = num("VTM_DEBUG_NSPLIT");
        d.seed_dry = getenv("VTM_DEBUG_SEED_DRY") != nullptr;
        d.nsplit_r4 = getenv("VTM_DEBUG_NSPLIT_R4") != nullptr;
        d.no_xprune = getenv("VTM_DEBUG_NOXPRUNE") != nullptr;
        return d;
    }();
    return e;
}

// Every number the launches of one vtm_match_filtered* call use.
struct FilterPlan {
    int KT, KP, KPS;            // channel steps; the filter's pruning test comes after KP of them, the scout's after KPS <= KP
    bool prune;                 // false: no test at all
    int64_t cut, cut2;          // the first channel behind the filter's / the scout's test (rest norms start there)
    int ns_tiles, nd_tiles, total_src_tiles, patch_tiles, ngroups;   // XCD patch geometry of filter_kernel's grid
    int nsplit, tiles_per_split;                                      // dst splits of the one launch (or of the scout)
    int64_t grid;
    bool range_plan;            // scout + range: a second launch of nsplit_r splits (0 without the plan)
    int tps_r, nsplit_r;
    int64_t grid_r;
    int map_words;              // words per src tile of the scout's tile map
    int xsplit, xtps, KX;       // exact_rows_kernel: dst splits, pruning depth in XK-channel steps (0 = off)
    unsigned xgrid, refine_grid, prep_grid, seed_grid;   // (seed_grid 0: no seeds, no launch)
};

// workgroups one XCD has to run (2 per CU at a time) for a split count; patch_wgs = its patches x their src tiles
inline int wgs_per_xcd(int nd_tiles, int patch_wgs, int ns) {
    const int tps = (int)cdiv(nd_tiles, ns);
    return patch_wgs * (int)cdiv(nd_tiles, tps);
}

// rounds 1-4: enough workgroups to fill the chip, >= 4 dst tiles each, at most 8 (every split contributes >= 1
// candidate per row), 8 whenever the dst axis is long enough, 7 or 6 when that saves a round (A/B hook)
inline int nsplit_rounds_1_4(int nd_tiles, int patch_wgs, int ns_tiles, int64_t B, int cus) {
    int64_t want = cdiv(1536, (int64_t)ns_tiles * B);
    int nsplit = (int)(want < 1 ? 1 : want);
    if (nd_tiles >= 32) nsplit = 8;
    if (nsplit > nd_tiles / 4) nsplit = nd_tiles / 4 > 0 ? nd_tiles / 4 : 1;
    if (nsplit > 8) nsplit = 8;
    if (nsplit == 8) {
        const int slots = cus / 8 * 2;
        for (int ns = 7; ns >= 6; --ns)
            if (wgs_per_xcd(nd_tiles, patch_wgs, 8) > slots && wgs_per_xcd(nd_tiles, patch_wgs, ns) <= slots) return ns;
    }
    return nsplit;
}

// Round 5: the split count that minimises  rounds x (tiles per split + 1.5) + 0.25 splits  -- an XCD runs its workgroups in
// rounds of its CUs x 2, a workgroup costs its dst tiles plus ~1.5 tiles of prologue / flush, and every split adds
// candidates to the rows' lists.  Reproduces the best of tools/sweep_nsplit.py's 2..14 sweep on all six cfg-2 shapes
// (profiles/r05_h_sweeps.txt): level 2 takes 5 splits instead of 8 (768 workgroups = 1.5 rounds -> 480 = one round:
// -6 %), the mid levels 5 / 14 instead of 8 (-7 % / -10 %), the top global level 7.
inline int nsplit_round_5(int nd_tiles, int patch_wgs, int cus) {
    const int slots = cus / 8 * 2;
    double best_cost = 1e30;
    int nsplit = 1;
    for (int ns = 1; ns <= 16 && ns <= nd_tiles; ++ns) {
        const int tps = (int)cdiv(nd_tiles, ns);
        if ((int)cdiv(nd_tiles, tps) != ns) continue;          // same workgroups as a smaller count
        if (tps < 4 && ns > 1) continue;   // >= 4 dst tiles per split (rounds 1-4's rule: every split starts its rows' running maxima and lists anew)
        const int wgs = wgs_per_xcd(nd_tiles, patch_wgs, ns);
        // (a single round must leave a few slots free: 63 workgroups on 64 slots measured as two rounds)
        const double rounds = (wgs <= slots && wgs > slots - slots / 16) ? 2.0 : (double)cdiv(wgs, slots);
        const double cost = rounds * (tps + 1.5) + 0.25 * ns;
        if (cost < best_cost - 1e-9) {
            best_cost = cost;
            nsplit = ns;
        }
    }
    return nsplit;
}

// The plan of one call: a pure function of its arguments (`cus` = compute units of the device the call runs on;
// `scout_steps` = VTM_MATCH_SCOUT_STEPS of the mode word, `mode` the rest of it; `ordered` = a position-ordered call).
inline FilterPlan plan_filter(const Layout &L, int64_t B, int64_t /*C: L.C64*/, int64_t Ns, int64_t Nd, int align, int mode,
                              int scout_steps, int64_t seed_N, bool ordered, int cus, const DebugEnv &dbg) {
    FilterPlan P;
    // partial-sum pruning: check after KP of the KT channel steps; off for short rows and for the 2- / 3-product
    // builds (their lo products are not covered by the hi rest norms)
    const int KT = P.KT = (int)(L.C64 / FBK);
    int KP = (VTM_FILTER_PRODUCTS == 1 && KT >= 4) ? (2 * KT + 2) / 5 : 0;   // 40 % depth (profiles/r04_kp_sweep.txt)
    if (VTM_FILTER_PRODUCTS == 1 && KT == 5 && dbg.kp5 >= 0 && dbg.kp5 < KT) KP = dbg.kp5;   // the C = 320 levels alone (KT = 5)
    if (VTM_FILTER_PRODUCTS == 1 && dbg.kp >= 0 && dbg.kp < KT) KP = dbg.kp;                 // 0 = off, else the step after which blocks are tested
    P.KP = KP;
    P.prune = KP > 0 && KP < KT;
    P.cut = P.prune ? (int64_t)KP * FBK : L.C64;
    // the scout of the scout + range plan may test EARLIER than the filter proper (its own rest norms): a low-noise clip's
    // dead tiles are dead after one step already, and the scout's cost is its steps
    P.KPS = (P.prune && mode == MODE_SCOUT_RANGE && scout_steps > 0 && scout_steps < KP) ? scout_steps : KP;
    P.cut2 = P.KPS < KP ? (int64_t)P.KPS * FBK : P.cut;

    const int ns_tiles = P.ns_tiles = (int)(L.Ns_pad / FBS), nd_tiles = P.nd_tiles = (int)(L.Nd_pad / FBD);
    P.total_src_tiles = (int)(B * ns_tiles);
    // patch size: at most 16 src tiles while their (hi) operands fit comfortably in one L2 (16 x 256 rows x C x
    // 2 B <= 3 MiB), else 8 -- and balanced: patch g runs on XCD g % 8, so the tiles are cut into equal patches
    // whose number per XCD is the same for all XCDs (17 patches of 16 tiles would keep one XCD busy for three
    // patches while the other seven idle after two)
    const int max_patch = (int64_t)16 * FBS * L.C64 * 2 <= (3 << 20) ? 16 : 8;
    const int tiles_per_xcd = (int)cdiv(P.total_src_tiles, 8);
    const int patches_per_xcd = (int)cdiv(tiles_per_xcd, max_patch);
    P.patch_tiles = (int)cdiv(tiles_per_xcd, patches_per_xcd);
    P.ngroups = (int)cdiv(P.total_src_tiles, P.patch_tiles);
    const int patch_wgs = patches_per_xcd * P.patch_tiles;
    int nsplit = dbg.nsplit_r4 ? nsplit_rounds_1_4(nd_tiles, patch_wgs, ns_tiles, B, cus) : nsplit_round_5(nd_tiles, patch_wgs, cus);
    if (dbg.nsplit >= 1 && dbg.nsplit <= 16 && dbg.nsplit <= nd_tiles) nsplit = dbg.nsplit;   // tuning hook (tools/sweep_nsplit.py)
    P.tiles_per_split = (int)cdiv(nd_tiles, nsplit);
    P.nsplit = (int)cdiv(nd_tiles, P.tiles_per_split);
    P.grid = (int64_t)8 * cdiv(P.ngroups, 8) * P.patch_tiles * P.nsplit;
    // scout + range plan (see filter_kernel): needs the pruning test, the seeds (without a starting maximum nothing is
    // dead) and dst frames of whole tiles -- one split per dst frame, so that a span is the live tiles of ONE frame
    // (position-ordered call: the whole dst axis is ONE position-major run; the splits stay the one-launch plan's -- a src
    // tile's span then lies in one or two of them and the other workgroups leave at once, while a level whose spans are long
    // keeps its parallelism: with a single split corr05's top global level took 2.9 ms instead of 1.3)
    P.map_words = (nd_tiles + 31) / 32;
    P.range_plan = mode == MODE_SCOUT_RANGE && P.prune &&
                   (ordered ? seed_N > 0 && nd_tiles >= 2 : seed_N >= 2 * FBD && seed_N % FBD == 0);
    P.tps_r = !P.range_plan ? 0 : ordered ? P.tiles_per_split : (int)(seed_N / FBD);
    P.nsplit_r = P.range_plan ? (int)cdiv(nd_tiles, P.tps_r) : 0;
    P.grid_r = (int64_t)8 * cdiv(P.ngroups, 8) * P.patch_tiles * P.nsplit_r;

    // the escape: a fixed grid strides over the (device-side) lists of overflowed rows -- normally empty, then the
    // workgroups leave at once; dst splits of >= 8 tiles so that a short list still spreads over the chip
    const int xd_tiles = (int)cdiv(Nd, XD);
    int xsplit = xd_tiles / 8;
    xsplit = xsplit < 1 ? 1 : xsplit > 16 ? 16 : xsplit;
    P.xtps = (int)cdiv(xd_tiles, xsplit);
    P.xsplit = (int)cdiv(xd_tiles, P.xtps);
    P.xgrid = (unsigned)((XS == 128 ? 2 : 1) * cus);
    // exact_rows_kernel's tile pruning: the rest norms prep_operand wrote for the filter's cut, in 32-channel steps
    P.KX = dbg.no_xprune ? 0 : (int)(P.cut / XK);

    P.refine_grid = (unsigned)cdiv(align ? Ns : B * Ns, RROWS);
    P.prep_grid = (unsigned)cdiv(B * (L.Ns_pad + L.Nd_pad), 64 * PREP_WAVES);
    P.seed_grid = seed_N > 0 ? (unsigned)cdiv(B * Ns * 8, 256) : 0u;
    return P;
}

}  // namespace vtm_match_plan
