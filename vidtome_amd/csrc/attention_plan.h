// How an attention launch is planned and issued, once for the five kernel families (attention_kernel in attention.hip,
// attention16s_kernel in attention16.hip, attention16g_kernel in attention16g.hip, attention_f32_kernel in
// attention_f32.hip, attention_sets_kernel in attention_sets.hip): the host tail plan, the device plan of query-bounded launches, the family descriptor, the launch
// driver, the workspace size and the head-dim dispatch -- and the device side of the same plan: how a workgroup of a main or
// combine kernel finds its work item (decode_work_item, decode_combine_item).  Header-only; host code apart from those and
// attention16_plan_kernel.
#pragma once
#include "attention_common.h"

#include <algorithm>
#include <type_traits>

namespace vtm_att {

struct TailPlan {
    int64_t nqb, total, full;   // query blocks per (sample, head), all workgroups, workgroups in whole rounds
    int nsplit;                 // splits of each remaining work item (1 = none)
    size_t ws_bytes;
    bool split_all;             // every item is split (launches with a device-side query bound)
};

// Tail plan.  All workgroups of a launch take the same time, so the launch runs in "rounds" of as many workgroups
// as the chip holds (slots); the last, partly filled round leaves most CUs idle for a whole workgroup time (cfg-2
// mid blocks: 272 workgroups on 256 slots -> two rounds for 6 % more work than one; top blocks: 4.25 rounds).  The
// work items of that last round are therefore split along the key axis into `nsplit` shorter workgroups that fill
// the chip -- in the SAME launch, behind the whole ones, so they start as the slots of the last whole round free
// up -- and merged by a combine kernel.
// `bounded`: the launch carries a device-side query count (vtm_attention_kv_bounded: compacted live queries).  How many
// of its workgroups do real work is not known when it is launched -- the cfg-2 top block launches 2 176 for ~1 800 live
// ones, 3.5 rounds of 512 that cost 4 -- so the round structure cannot be planned.  It is made finer instead: EVERY
// work item is split in two along the key axis (split-major order), the live ones then fill 7 half-length rounds
// (profiles/r04_attention_split_all.txt); the price is one partial record per workgroup for the combine kernel.
// B_items: samples the grid runs over; QB: query rows per workgroup; wg_per_cu: resident workgroups per CU (launch
// bounds / LDS); rec_bytes: the partial record of one key-split workgroup.
inline TailPlan plan_tail(int64_t B_items, int64_t h, int64_t Mq, int64_t Mk, int64_t QB, int wg_per_cu, size_t rec_bytes,
                          bool bounded) {
    TailPlan p;
    p.nqb = vtm::cdiv(Mq, QB);
    p.total = p.nqb * h * B_items;
    const int64_t slots = (int64_t)vtm::device_cus() * wg_per_cu;
    p.full = p.total / slots * slots;
    const int64_t rem = p.total - p.full, ntiles = vtm::cdiv(Mk, KV);
    p.nsplit = 1;
    p.ws_bytes = 0;
    p.split_all = false;
    if (bounded && p.total >= 2 * slots && ntiles >= 64 && p.total % 8 == 0) {
        p.full = 0;
        p.nsplit = 2;
        p.split_all = true;
        p.ws_bytes = (size_t)p.total * 2 * rec_bytes;
        return p;
    }
    // worth it only behind at least one whole round, for long key axes, and when the last round is at most a
    // quarter full (a workgroup that has its CU to itself already runs about twice as fast as in a full round;
    // measured: 128 of 512 -> -7 %, 16 of 256 -> -18 %, 192 or 256 of 512 -> no gain)
    if (p.full > 0 && rem > 0 && rem * 4 <= slots && ntiles >= 32) {
        int64_t ns = slots / rem;
        if (ns > 16) ns = 16;
        if (ns > ntiles / 8) ns = ntiles / 8;
        if (ns >= 2) {
            p.nsplit = (int)ns;
            p.ws_bytes = (size_t)rem * ns * rec_bytes;
        }
    }
    if (p.nsplit == 1) p.full = p.total;
    return p;
}

// ---- one attention call, as the exports (attention.hip) hand it to the families ----
struct Call {
    const void *q; int64_t ldq; const void *k; int64_t ldk; const void *vt; int64_t ldvt; void *out; int64_t ldo;
    int dtype; int64_t B, h, M, Mp, Mk, Mkp; float scale; int share_groups; void *ws; size_t ws_bytes;
    const int32_t *q_count; hipStream_t s; bool fold; const int32_t *k_count; const uint32_t *k_bias; int64_t ldkb;
    const struct KeySets *sets = nullptr;   // vtm_attention_kv_sets only: the key ranges, each with a softmax of its own
    const struct SetMasks *set_masks = nullptr;   // vtm_attention_kv_sets_masked only: the per-query weights of the sets
    const struct KeyBias *key_bias = nullptr;     // vtm_attention_kv_bias only: the per-key score bias (attention_bias.hip)
    const struct SetSrc *set_src = nullptr;       // vtm_attention_kv_sets_src only: the second query operand of the sets
    const struct QuerySegments *segments = nullptr;   // vtm_attention_kv_segments only: the query segments (attention_segments.hip)
};

// ---- the key sets of one vtm_attention_kv_sets call (attention_sets.hip): set s = keys [start[s], start[s] + len[s]) ----
constexpr int MAX_KEY_SETS = 8;
struct KeySets {
    int n;
    int start[MAX_KEY_SETS], len[MAX_KEY_SETS];
    float w[MAX_KEY_SETS];
};
// ---- the per-query weights of a vtm_attention_kv_sets_masked call: set s is weighted by w[s] * table[b * batch_stride +
// row[s] * ld + query] (row[s] = -1: by w[s] alone); one table for all heads ----
struct SetMasks {
    const float *table;
    int64_t ld, batch_stride;
    int row[MAX_KEY_SETS];
};
// ---- the second query operand of a vtm_attention_kv_sets_src call: set s takes the query row (b * Mp + i) * ld of `q`
// here when bit s of `from_src` is set, else the call's own q ----
struct SetSrc {
    const void *q;
    int64_t ld, Mp;
    unsigned from_src;
};

// ---- what planned_launch computed, for a family's launch thunks ----
struct Launch {
    int64_t wgs;                // main kernel grid
    int64_t split_items;        // combine kernel grid: the items that run key-split
    int64_t nqb, whole;         // query blocks per (sample, head); items in front of the split ones, one workgroup each
    int nsplit;                 // pieces per split item (a device plan: its tiers say)
    float *partial;             // partial records of the key-split workgroups
    int xcd_groups;             // see item_of
    int64_t split_major;        // items split in split-major order (plan_tail's split_all)
    const void *plan;           // the DevPlan of a device-planned launch, else nullptr (DevPlan is internal to each file)
    float scale_log2e;
    int64_t src_batch;          // B / share_groups
};

// ---- the constants of one kernel family, and its two launch thunks ----
struct Family {
    const char *name = "vtm_attention";   // (error messages)
    int qb = 0;                 // query rows per workgroup
    int wg_per_cu = 1;          // resident workgroups per CU (launch bounds / LDS)
    size_t rec_bytes = 0;       // the partial record of one key-split workgroup
    int share = 1;              // the grid runs over B / share samples (attention16g: the source samples)
    int key_tile = KV;          // keys per tile (a device plan keeps >= 8 of them per piece)
    int xcd_min_nqb = 0;        // query blocks per (sample, head) from which the pairs are pinned to XCDs
    bool host_split_all = true; // a query-bounded launch without a device plan may split every item (plan_tail's `bounded`)
    int64_t ws_devplan_min_tiles = 0;   // ws_bytes counts a device plan from this many 64-key tiles (the launch takes one
                                        // whenever the workspace holds it)
    hipError_t (*lds_opt_in)() = nullptr;   // lets the main kernel use more than 64 KB of dynamic LDS (nullptr: not needed)
    void (*main)(const Call &, const Launch &) = nullptr;
    void (*combine)(const Call &, const Launch &) = nullptr;
};

// Calls fn(std::integral_constant<int, D>{}) for the head dim d the kernels are built for.  For another d a launch fails
// (VTM_EINVAL) and a workspace size (fn returns size_t) is 0.
template <typename Fn>
auto with_head_dim(int64_t d, Fn &&fn) {
    switch (d) {
        case 40: return fn(std::integral_constant<int, 40>{});
        case 64: return fn(std::integral_constant<int, 64>{});
        case 80: return fn(std::integral_constant<int, 80>{});
        case 160: return fn(std::integral_constant<int, 160>{});
        case 8: return fn(std::integral_constant<int, 8>{});
        case 16: return fn(std::integral_constant<int, 16>{});
        case 32: return fn(std::integral_constant<int, 32>{});
        case 96: return fn(std::integral_constant<int, 96>{});
        case 128: return fn(std::integral_constant<int, 128>{});
    }
    using R = decltype(fn(std::integral_constant<int, 8>{}));
    if constexpr (std::is_same_v<R, size_t>)
        return size_t(0);
    else
        return vtm::fail(VTM_EINVAL, "vtm_attention: unsupported head dim %lld (have 8,16,32,40,64,80,96,128,160)",
                         (long long)d);
}

// attention16.hip: self-attention or folded keys at d = 40 (attention16s_kernel); dtype VTM_F16 or VTM_BF16
Family family16s(int dtype, bool fold);
int attention16(const Call &c);
// attention16g.hip: shared probabilities of ng = 2, 3 value groups at d = 40 (attention16g_kernel); dtype VTM_F16 or VTM_BF16
Family family16g(int dtype, int ng);
int attention16g(const Call &c, int ng);
// attention_f32.hip: dtype VTM_F32, every head dim (attention_f32_kernel; never folded)
int attention_f32(const Call &c, int64_t d);
// ... and the workspace of the largest plan its family can take for a call of this shape (qb, wg_per_cu and rec_bytes differ
// from the 16-bit families', so neither size bounds the other)
size_t ws_bytes_f32(int64_t B, int64_t h, int64_t Mq, int64_t Mk, int64_t d, bool bounded);

}  // namespace vtm_att

namespace {

using namespace vtm_att;

// ---- device-side launch plan for QUERY-BOUNDED launches (vtm_attention_kv_bounded: compacted live queries) ----
// How many query blocks are live is a device value (q_count), so the host cannot cut the launch into whole rounds plus a
// key-split tail the way plan_tail does for a known length; rounds 4-5 split EVERY item in two instead (finer rounds).
// Measured in round 6 (profiles/r06_d_attention16_ab.txt): 912 live items on 256 slots are 3.56 rounds of work and took the
// time of 4 (4.81 ms against 4.31).  One thread now plans on the device, in front of the launch, from the counts -- a
// GEOMETRIC tail: workgroups are dispatched in index order as slots free up, so pieces that shrink towards the end of the
// grid pack like longest-first list scheduling and the idle tail is one SMALLEST piece long:
//   L live items (the longest sample's blocks x heads x samples), S slots;
//   tier 0: the items of the whole rounds, L - L % S of them, one workgroup each (a last round >= 0.8 full, or the only round of a
//   launch that fills more than half of the chip, counts as whole);
//   then, while items remain: the next tier takes S / n of them (or what is left), n = the smallest power of two >= 2 with
//   S / n <= remaining (at most MAX_SPLIT), each split n ways along the key axis -- S pieces, one short round.
// 912 items on 256 slots: 768 whole, 128 in halves, 16 in sixteenths = 3 + 0.5 + 1/16 rounds -- the work there is.  The
// launch itself is sized for the host-known upper bound; workgroups the plan has no role for leave at once.
constexpr int PLAN_TIERS = 8;
constexpr int PLAN_MAX_SPLIT = 16;
struct DevTier {
    int wg0, item0, items, nsplit, rec0;   // first workgroup, first item, items, pieces per item, first partial record
};
struct DevPlan {
    int nqb, ntiers, split_items, pad;     // live query blocks per (sample, head); tiers in use; items behind tier 0
    DevTier tier[PLAN_TIERS];
};

// ---- the planning arguments of a launch: ONE by-value argument of every main and combine kernel (plan_args below) ----
struct PlanArgs {
    int64_t nqb, nwhole;         // query blocks per (sample, head); the items in front of the split ones, one workgroup each
    int64_t split_major_items;   // host plan: the items split in split-major order (plan_tail's split_all), else 0
    float *partial_base;         // partial records of the key-split workgroups
    const int32_t *q_count;      // device-side query bound of every sample the grid runs over, or nullptr
    const DevPlan *dev_plan;     // a device-planned launch: nqb and the roles come from it (the host values are upper bounds)
    int nsplit_tail, xcd_groups; // host plan: pieces per split item; see item_of
};

// what one workgroup does, decoded from its index and the PlanArgs (all of it wave-uniform)
struct WorkItem {
    int64_t b, h, q0;   // sample of the grid, head, first query row of the item's query block
    int64_t rec;        // main kernel: the partial record this key-split workgroup leaves (-1: a whole item, it writes the
                        // output); combine kernel: the first record of the item.  In records: the caller knows their size
    int nsplit, split;  // pieces of the item along the key axis, and which one this workgroup is
    bool leave;         // no role in the plan, or a query block at or beyond q_count[b]: return at once
};

// work item `lin` (query blocks fastest, then heads, then samples) -> its coordinates and the q_count exit
template <int QB>
__device__ __forceinline__ WorkItem item_coords(int64_t lin, int64_t nqb, int64_t H, const int32_t *q_count = nullptr) {
    WorkItem w{};
    w.b = lin / (nqb * H);
    w.h = (lin / nqb) % H;
    w.q0 = (lin % nqb) * QB;
    w.rec = -1;
    w.nsplit = 1;
    // device-side query bound (compacted live queries, vtm_compact_queries): the launch is sized for the host-known upper
    // bound; a query block that starts at or beyond its sample's count has nothing anybody reads (and leaves no record)
    w.leave = q_count != nullptr && w.q0 >= (int64_t)q_count[w.b];
    return w;
}

// Main kernels: workgroup `wg` of the grid.  Workgroups [0, nwhole) take one item each and all its key tiles; the ones
// behind them share the remaining items nsplit ways along the key axis, split-minor (a partly filled last round: the
// pieces of an item sit next to each other) or split-MAJOR (all first pieces, then all second pieces ..., so that workgroup
// p and its item still share p % 8 = the XCD the item's (sample, head) pair is pinned to: a host plan that splits EVERY
// item, and every tier of a device plan).  A device plan (one thread made it from the live counts: whole items, then tiers
// split 2, 4, 8, 16 ways) overrides the host's upper bounds; workgroups behind its last tier leave.
// QB: query rows per workgroup; XCD_MIN_NQB: the family's Family::xcd_min_nqb, which a device plan checks here.
template <int QB, int XCD_MIN_NQB>
__device__ __forceinline__ WorkItem decode_work_item(const PlanArgs &p, int64_t H, int64_t wg) {
    int64_t nqb = p.nqb, nwhole = p.nwhole, split_major_items = p.split_major_items;
    int nsplit_tail = p.nsplit_tail, xcd_groups = p.xcd_groups;
    int64_t tier_item0 = nwhole, tier_wg0 = nwhole, tier_rec0 = 0;   // (host plan: one tier behind the whole items)
    if (p.dev_plan != nullptr) {
        nqb = p.dev_plan->nqb;
        xcd_groups = nqb >= XCD_MIN_NQB ? xcd_groups : 0;
        int ti = 0;
        while (ti + 1 < p.dev_plan->ntiers && (int)wg >= p.dev_plan->tier[ti + 1].wg0) ++ti;
        const DevTier tr = p.dev_plan->tier[ti];
        if (wg >= (int64_t)tr.wg0 + (int64_t)tr.items * tr.nsplit) {   // behind the last tier
            WorkItem w{};
            w.leave = true;
            return w;
        }
        nwhole = p.dev_plan->tier[0].items;
        nsplit_tail = tr.nsplit;
        split_major_items = tr.items;
        tier_item0 = tr.item0;
        tier_wg0 = tr.wg0;
        tier_rec0 = tr.rec0;
    }
    const bool tail_wg = wg >= nwhole;
    const int64_t tail_id = wg - tier_wg0;
    const int nsplit = tail_wg ? nsplit_tail : 1;
    const int64_t tail_item = split_major_items ? tail_id % split_major_items : tail_id / nsplit;
    const int split = !tail_wg ? 0 : split_major_items ? (int)(tail_id / split_major_items) : (int)(tail_id % nsplit);
    WorkItem w = item_coords<QB>(item_of(tail_wg ? tier_item0 + tail_item : wg, nqb, xcd_groups), nqb, H, p.q_count);
    w.rec = tail_wg ? tier_rec0 + tail_item * nsplit + split : -1;
    w.nsplit = nsplit;
    w.split = split;
    return w;
}

// Combine kernels: split item `idx` of the launch (a device-planned launch is sized for the most items a plan can split).
// It must see the items exactly as decode_work_item does -- same QB, same XCD_MIN_NQB -- or it merges other items' records.
template <int QB, int XCD_MIN_NQB>
__device__ __forceinline__ WorkItem decode_combine_item(const PlanArgs &p, int64_t H, int64_t idx) {
    int64_t nqb = p.nqb, pos = p.nwhole + idx, rec0 = idx * p.nsplit_tail;
    int nsplit = p.nsplit_tail, xcd_groups = p.xcd_groups;
    if (p.dev_plan != nullptr) {
        if ((int)idx >= p.dev_plan->split_items) {
            WorkItem w{};
            w.leave = true;
            return w;
        }
        nqb = p.dev_plan->nqb;
        xcd_groups = nqb >= XCD_MIN_NQB ? xcd_groups : 0;
        pos = p.dev_plan->tier[0].items + idx;
        int ti = 1;
        while (ti + 1 < p.dev_plan->ntiers && pos >= p.dev_plan->tier[ti + 1].item0) ++ti;
        const DevTier tr = p.dev_plan->tier[ti];
        nsplit = tr.nsplit;
        rec0 = tr.rec0 + (pos - tr.item0) * tr.nsplit;
    }
    WorkItem w = item_coords<QB>(item_of(pos, nqb, xcd_groups), nqb, H, p.q_count);   // (dead block: its records were never written)
    w.rec = rec0;
    w.nsplit = nsplit;
    return w;
}

// upper bounds of a plan on S slots: workgroups behind the whole items / partial records, items that are split
constexpr int64_t plan_tail_wgs(int slots) { return (int64_t)(PLAN_TIERS - 1) * slots; }
constexpr int64_t plan_split_items(int slots) { return slots; }

__global__ void attention16_plan_kernel(const int32_t *__restrict__ q_count, int B, int H, int QB, int slots, int ntiles,
                                        DevPlan *__restrict__ plan) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int nqb = 1;
    for (int b = 0; b < B; ++b) {
        const int n = (q_count[b] + QB - 1) / QB;
        nqb = n > nqb ? n : nqb;
    }
    const int L = nqb * H * B, S = slots;
    int max_ns = ntiles / 8;                     // a piece keeps >= 8 key tiles
    max_ns = max_ns > PLAN_MAX_SPLIT ? PLAN_MAX_SPLIT : max_ns < 1 ? 1 : max_ns;
    DevPlan p;
    p.nqb = nqb;
    p.pad = 0;
    int nt = 0, wg = 0, item = 0, rec = 0;
    // what runs whole: the full rounds; ALSO a last round that is at least 0.8 full, or the one round of a launch that fills
    // more than half of the chip (splitting those moves more partial records than the idle slots are worth)
    int whole = L - L % S;
    if (max_ns < 2 || (L % S) * 5 >= S * 4 || (L < S && L * 2 > S)) whole = L;
    p.tier[nt++] = DevTier{0, 0, whole, 1, 0};
    wg = item = whole;
    while (item < L && nt < PLAN_TIERS) {
        const int rem = L - item;
        int n = 2;
        while (n < max_ns && S / n > rem) n *= 2;
        if (n > max_ns) n = max_ns;
        int take = S / n < rem ? S / n : rem;
        if (nt == PLAN_TIERS - 1) take = rem;    // (never with S = 256: 2, 4, 8, 16, 16 ...: the last tier takes what is left)
        p.tier[nt++] = DevTier{wg, item, take, n, rec};
        wg += take * n;
        rec += take * n;
        item += take;
    }
    p.ntiers = nt;
    p.split_items = L - whole;
    for (int i = nt; i < PLAN_TIERS; ++i) p.tier[i] = DevTier{wg, item, 0, 1, rec};
    *plan = p;
}

// workspace of a device-planned launch: the plan (one cache line) + the records of the largest tail a plan can have
constexpr size_t DEVPLAN_HEADER = 256;
static_assert(sizeof(DevPlan) <= 256, "the plan lives in the workspace header");
inline size_t devplan_ws_bytes(int slots, size_t rec_bytes) { return DEVPLAN_HEADER + (size_t)plan_tail_wgs(slots) * rec_bytes; }

// the PlanArgs of a planned launch, for a family's launch thunks
inline PlanArgs plan_args(const Call &c, const Launch &g) {
    return {g.nqb, g.whole, g.split_major, g.partial, c.q_count, static_cast<const DevPlan *>(g.plan), g.nsplit, g.xcd_groups};
}

// The launch protocol of every family.  A query-bounded launch of at least two rounds is planned ON THE DEVICE from the
// live counts (attention16_plan_kernel) when the workspace holds the plan and the records of the largest tail a plan can
// have: whole items, then tiers split 2 .. 16 ways.  (A one-round launch does not get back the 50-70 us the oversized grid
// and the two small launches of a plan cost -- profiles/r06_k_devplan_attention_kernel.txt.)  Otherwise the host plans
// (plan_tail): split every item of a bounded launch in two (split_all) if the family allows it and the workspace holds the
// records, else a key-split tail behind the whole rounds if the workspace holds it, else one plain launch.
inline int planned_launch(const Call &c, const Family &f) {
    if (f.lds_opt_in) {
        const hipError_t e = f.lds_opt_in();
        if (e != hipSuccess) return vtm::fail(VTM_ELAUNCH, "%s: LDS attribute: %s", f.name, hipGetErrorString(e));
    }
    const int64_t B = c.B / f.share;   // the samples the grid runs over
    const int slots = vtm::device_cus() * f.wg_per_cu;
    // (sample, head) pairs pinned to XCDs when they divide evenly and every pair has enough query blocks to keep an XCD's
    // share of the chip busy (see item_of): xcd_min_nqb, checked here for a host plan and on the device for a device plan
    const int xcd_pairs = (B * c.h) % 8 == 0 ? (int)(B * c.h / 8) : 0;
    Launch g;
    g.scale_log2e = c.scale * 1.4426950408889634f;
    g.src_batch = c.B / c.share_groups;
    const int64_t nqb_max = vtm::cdiv(c.M, f.qb);
    if (c.q_count != nullptr && c.ws != nullptr && c.ws_bytes >= devplan_ws_bytes(slots, f.rec_bytes) &&
        nqb_max * c.h * B >= 2 * slots) {
        DevPlan *plan = reinterpret_cast<DevPlan *>(c.ws);
        const int64_t total = nqb_max * c.h * B, tail_max = plan_tail_wgs(slots);
        VTM_REQUIRE(total + tail_max < (1ll << 31) / 16, "vtm_attention: grid too large");
        hipLaunchKernelGGL(attention16_plan_kernel, dim3(1), dim3(64), 0, c.s, c.q_count, (int)B, (int)c.h, f.qb, slots,
                           (int)vtm::cdiv(c.Mk, f.key_tile), plan);
        g.wgs = total + tail_max;
        g.split_items = plan_split_items(slots);
        g.nqb = nqb_max;
        g.whole = total;
        g.nsplit = 1;
        g.partial = reinterpret_cast<float *>(static_cast<char *>(c.ws) + DEVPLAN_HEADER);
        g.xcd_groups = xcd_pairs;
        g.split_major = 0;
        g.plan = plan;
        f.main(c, g);
        f.combine(c, g);
        return vtm::launch_status(f.name);
    }
    TailPlan p = plan_tail(B, c.h, c.M, c.Mk, f.qb, f.wg_per_cu, f.rec_bytes, c.q_count != nullptr && f.host_split_all);
    if (p.split_all && (!c.ws || c.ws_bytes < p.ws_bytes))   // not enough workspace: the plain plan
        p = plan_tail(B, c.h, c.M, c.Mk, f.qb, f.wg_per_cu, f.rec_bytes, false);
    if (p.nsplit > 1 && (!c.ws || c.ws_bytes < p.ws_bytes)) {   // no workspace: plain single launch
        p.nsplit = 1;
        p.full = p.total;
        p.split_all = false;
    }
    VTM_REQUIRE(p.total < (1ll << 31) / 16, "vtm_attention: grid too large");
    // one launch: the whole workgroups first, the key-split ones of the last round behind them (they start as the
    // slots of the last whole round free up -- no launch boundary to drain)
    const int64_t rem = p.total - p.full;
    g.wgs = p.full + rem * p.nsplit;
    g.split_items = rem;
    g.nqb = p.nqb;
    g.whole = p.full;
    g.nsplit = p.nsplit;
    g.partial = static_cast<float *>(c.ws);
    g.xcd_groups = p.nqb >= f.xcd_min_nqb ? xcd_pairs : 0;
    g.split_major = p.split_all ? rem : 0;
    g.plan = nullptr;
    f.main(c, g);
    if (p.nsplit > 1) f.combine(c, g);
    return vtm::launch_status(f.name);
}

// the workspace the largest plan of family f can take for a call of this shape
inline size_t ws_bytes(const Family &f, int64_t B, int64_t h, int64_t Mq, int64_t Mk, bool bounded) {
    size_t n = plan_tail(B / f.share, h, Mq, Mk, f.qb, f.wg_per_cu, f.rec_bytes, bounded && f.host_split_all).ws_bytes;
    if (bounded && vtm::cdiv(Mk, KV) >= f.ws_devplan_min_tiles)
        n = std::max(n, devplan_ws_bytes(vtm::device_cus() * f.wg_per_cu, f.rec_bytes));
    return n;
}

}  // namespace
