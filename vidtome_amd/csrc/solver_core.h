// What the multistep solver's step (solver_step.hip) and its inverse (invert_step.hip) share beyond step_core.h: the launch's
// scalars (Solve), the combined model output m (combine), the fp32 history accesses, and the deterministic part of the update
//     mu = c_x x + c_x0 x0 + c_h1 h1 + c_h2 h2
// (solver_sum).  The forward step adds c_noise * noise to mu; the inverse solves that line for the noise.  Both go through
// the one expression below, compiled with -ffp-contract=off, so what the inverse corrects its target to is what the forward
// step computes from the stored noise, bit for bit.
#pragma once
#include "common.h"
#include "step_core.h"

namespace vtm {

constexpr int SOLVER_MAX_GROUPS = VTM_SOLVER_MAX_GROUPS;

struct Solve {
    int pred, g_ref, terms;                   // terms: the groups of non-zero weight,
    int g[SOLVER_MAX_GROUPS];                 // ... ascending,
    float w[SOLVER_MAX_GROUPS];               // ... and their weights
    float rescale, sqrt_alpha, sqrt_beta, c_x, c_x0, c_h1, c_h2, c_noise;
};

// Solve from the export's arguments: a group of weight 0 is never read
inline Solve make_solve(int pred_type, float rescale, int64_t g_ref, int64_t groups, const float *w, float sqrt_alpha,
                        float sqrt_beta, float c_x, float c_x0, float c_h1, float c_h2, float c_noise) {
    Solve s{pred_type, rescale > 0.0f ? (int)g_ref : 0, 0, {}, {}, rescale, sqrt_alpha, sqrt_beta, c_x, c_x0, c_h1, c_h2, c_noise};
    for (int g = 0; g < groups; ++g)
        if (w[g] != 0.0f) {
            s.g[s.terms] = g;
            s.w[s.terms++] = w[g];
        }
    return s;
}

// the chunk's n <= N fp32 history elements: N / 4 chunks of fp32
template <int N, bool VEC>
__device__ __forceinline__ void load_history(const float *p, int n, float *v) {
#pragma unroll
    for (int q = 0; q < N; q += 4) load_chunk<float, VEC>(p + q, n - q, v + q);
}

template <int N, bool VEC>
__device__ __forceinline__ void store_history(float *p, int n, const float *v) {
#pragma unroll
    for (int q = 0; q < N; q += 4) store_chunk<float, VEC>(p + q, n - q, v + q);
}

// m = sum of w[g] * model_out[g] over the groups of non-zero weight, ascending, from 0: the same operations wherever m is
// needed, so every pass sees the same m.  mo points at the chunk in group 0; group g lies g * stride elements further.
template <typename T, bool VEC>
__device__ __forceinline__ void combine(const Solve &s, const T *mo, int64_t stride, int n, float *m) {
    constexpr int N = 16 / sizeof(T);
    float v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) m[k] = 0.0f;
#pragma unroll 1
    for (int t = 0; t < s.terms; ++t) {
        const float w = s.w[t];
        load_chunk<T, VEC>(mo + s.g[t] * stride, n, v);
#pragma unroll
        for (int k = 0; k < N; ++k) m[k] = m[k] + w * v[k];
    }
}

// mu, from 0 in the order written.  A term whose coefficient is 0 (c_x, c_x0) or whose operand is absent (has1, has2: the
// export passes no history where the coefficient is 0) is not added; p1 / p2 are not looked at then.
__device__ __forceinline__ float solver_sum(const Solve &s, float xv, float x0, bool has1, float p1, bool has2, float p2) {
    float acc = 0.0f;
    if (s.c_x != 0.0f) acc = acc + s.c_x * xv;
    if (s.c_x0 != 0.0f) acc = acc + s.c_x0 * x0;
    if (has1) acc = acc + s.c_h1 * p1;
    if (has2) acc = acc + s.c_h2 * p2;
    return acc;
}

// the requirements vtm_solver_step and vtm_invert_step share, in the order vtm_solver_step always made them
inline int check_solver_sizes(const char *who, const void *x, const void *model_out, const float *w, int64_t F, int64_t E,
                              int64_t groups, float rescale, int64_t g_ref) {
    VTM_REQUIRE(x && model_out && w, "%s: x, model_out and w are required", who);
    // (F bounds the grid of the per-frame launch: 1024 F threads must stay below 2^32)
    VTM_REQUIRE(F >= 0 && F <= (1 << 20) && E >= 1 && groups >= 1 && groups <= SOLVER_MAX_GROUPS,
                "%s: bad sizes F = %lld, E = %lld, groups = %lld (1 .. %d)", who, (long long)F, (long long)E, (long long)groups,
                SOLVER_MAX_GROUPS);
    VTM_REQUIRE(!(rescale < 0.0f) && rescale == rescale, "%s: rescale = %g is negative or NaN", who, (double)rescale);
    VTM_REQUIRE(!(rescale > 0.0f) || (g_ref >= 0 && g_ref < groups && w[g_ref] != 0.0f && E >= 2),
                "%s: rescale > 0 needs g_ref = %lld inside [0, %lld) with a non-zero weight, and E >= 2", who, (long long)g_ref,
                (long long)groups);
    return VTM_OK;
}

}  // namespace vtm
