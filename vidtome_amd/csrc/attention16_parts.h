// Internal pieces shared by the two wide-tile d = 40 translation units (attention16.hip, attention16g.hip): the partial record of a
// key-split workgroup and the kernel that combines the records.
#pragma once
#include "attention_plan.h"

namespace {

using namespace vtm_att;

// per-(query sub-tile, value group) record a key-split workgroup leaves for attention16_combine_kernel: the PV16 record of
// attention.hip (24 accumulators at d = 40, one running max per 16-query half, one unused denominator slot)
template <int D> constexpr int rec16() { return (D + 16) / 16 * 8 + 2 + 1; }
// the constants both wide-tile families share, for their kernels and their Family: workgroups of 8 waves, the XCD threshold
// (Family::xcd_min_nqb), the query rows of a workgroup (NQ sub-tiles of 32 rows per wave), the floats of its partial records
// (NV of them: query sub-tiles x value groups)
constexpr int WAVES16 = 8, NT16 = WAVES16 * 64;
constexpr int XCD_MIN_NQB16 = 32;
constexpr int qb16(int NQ) { return WAVES16 * QW * NQ; }
template <int D> constexpr int64_t rec16_size(int NV) { return (int64_t)NV * rec16<D>() * NT16; }

template <typename T, int D, int NQ, int NG>
__global__ __launch_bounds__(NT16) void attention16_combine_kernel(
    T *__restrict__ out, int64_t ldo, int64_t H, int64_t M, int64_t Mp, int64_t src_batch, PlanArgs plan) {
    constexpr int NT = NT16, NV = NQ * NG;
    constexpr int NA = (D + 16) / 16 * 8, REC = rec16<D>();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int v = blockIdx.y, sub = v / NG, g = v % NG;
    const WorkItem w = decode_combine_item<qb16(NQ), XCD_MIN_NQB16>(plan, H, blockIdx.x);
    if (w.leave) return;
    const int64_t b = w.b, h = w.h, q0 = w.q0 + (wave * NQ + sub) * QW;
    const int nsplit = w.nsplit;
    const float *partial = plan.partial_base + w.rec * rec16_size<D>(NV);
    float acc[NA], m[2] = {-INFINITY, -INFINITY};
#pragma unroll
    for (int r = 0; r < NA; ++r) acc[r] = 0.0f;
    for (int sp = 0; sp < nsplit; ++sp) {
        const float *pp = partial + ((int64_t)sp * NV + v) * REC * NT + tid;
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
