// Internal pieces shared by the two wide-tile d = 40 translation units (attention16.hip, attention16g.hip): the partial record of a
// key-split workgroup and the kernel that combines the records.
#pragma once
#include "attention_plan.h"

namespace {

using namespace vtm_att;

// per-(query sub-tile, value group) record a key-split workgroup leaves for attention16_combine_kernel: the PV16 record of
// attention.hip (24 accumulators at d = 40, one running max per 16-query half, one unused denominator slot)
template <int D> constexpr int rec16() { return (D + 16) / 16 * 8 + 2 + 1; }

template <typename T, int D, int NQ, int NG, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void attention16_combine_kernel(
    const float *__restrict__ partial, T *__restrict__ out, int64_t ldo, int64_t H, int64_t M, int64_t Mp, int64_t nqb,
    int64_t id0, int nsplit, int xcd_groups, const int32_t *__restrict__ q_count, int64_t src_batch,
    const DevPlan *__restrict__ dev_plan) {
    constexpr int NT = WAVES * 64, QB = WAVES * QW * NQ, NV = NQ * NG;
    constexpr int NA = (D + 16) / 16 * 8, REC = rec16<D>();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int v = blockIdx.y, sub = v / NG, g = v % NG;
    int64_t rec0 = (int64_t)blockIdx.x * nsplit;   // first partial record of this item
    int64_t pos = id0 + blockIdx.x;
    if (dev_plan != nullptr) {        // (the launch is sized for the most items a plan can split)
        if ((int)blockIdx.x >= dev_plan->split_items) return;
        nqb = dev_plan->nqb;
        xcd_groups = nqb >= 32 ? xcd_groups : 0;
        pos = dev_plan->tier[0].items + blockIdx.x;
        int ti = 1;
        while (ti + 1 < dev_plan->ntiers && pos >= dev_plan->tier[ti + 1].item0) ++ti;
        const DevTier tr = dev_plan->tier[ti];
        nsplit = tr.nsplit;
        rec0 = tr.rec0 + (pos - tr.item0) * tr.nsplit;
    }
    const int64_t lin = item_of(pos, nqb, xcd_groups);
    const int64_t b = lin / (nqb * H), h = (lin / nqb) % H;
    const int64_t q0 = (lin % nqb) * QB + (wave * NQ + sub) * QW;
    if (q_count != nullptr && (lin % nqb) * QB >= (int64_t)q_count[b]) return;   // its partial records were never written
    float acc[NA], m[2] = {-INFINITY, -INFINITY};
#pragma unroll
    for (int r = 0; r < NA; ++r) acc[r] = 0.0f;
    for (int sp = 0; sp < nsplit; ++sp) {
        const float *pp = partial + ((rec0 + sp) * NV + v) * REC * NT + tid;
        float fa[2], fb[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float ms = pp[(NA + j) * NT];
            const float mn = fmaxf(m[j], ms);
            fa[j] = mn == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(m[j] - mn);   // exp2(-inf) = 0; (-inf) - (-inf) is not
            fb[j] = mn == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(ms - mn);
            m[j] = mn;
        }
#pragma unroll
        for (int r = 0; r < NA; ++r) {
            const int j = (r >> 2) & 1;   // accumulator (dv, qh, e) is register (dv * 2 + qh) * 4 + e
            acc[r] = acc[r] * fa[j] + pp[r * NT] * fb[j];
        }
    }
    f32x4 o[(D + 16) / 16][2];
#pragma unroll
    for (int r = 0; r < NA; ++r) o[r >> 3][(r >> 2) & 1][r & 3] = acc[r];
    write_output16<T, D>(o, out, ldo, b + g * src_batch, h, q0, M, Mp, lane);
}

}  // namespace
