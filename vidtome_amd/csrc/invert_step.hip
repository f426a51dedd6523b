// vtm_invert_step: edit-friendly DDPM inversion (Huberman-Spiegelglas et al.; LEDITS++), the inverse of vtm_solver_step for one
// chunk in one launch.  The forward step computes x' = mu + c_noise noise with mu = c_x x + c_x0 x0 + c_h1 h1 + c_h2 h2; here x
// (the current level) and the next level `target` are given and the line is solved for the noise:
//     z       = (target - mu) / c_noise          -> z_out, rounded once to the model dtype T
//     target' = mu + c_noise * fp32(round_T(z))  -> target, in place, rounded once
// so the stored noise reproduces the corrected level exactly: m (combine), mu (solver_sum) and the last line are the forward
// step's own operations (solver_core.h, -ffp-contract=off), and sampling with z_out gives target' bit for bit.
//
// vtm_noise_levels: the levels the inversion starts from, levels[k] = sqrt_alpha[k] x0 + sqrt_beta[k] levels[k], in place on
// independent N(0, 1) draws, all levels in one launch.
//
// The cut into 16-byte chunks, the two launch shapes and the reduction order are step_core.h's.
#include "common.h"
#include "solver_core.h"

namespace {

using vtm::combine;
using vtm::load_chunk;
using vtm::load_history;
using vtm::Solve;
using vtm::store_chunk;
using vtm::store_history;

// step_core.h's policy: the launch's operands.  x, target, z_out and the history are whole-video (rows frame_ids), model_out,
// eps_out and x0_out chunk-local.  target is null when c_noise == 0: there is no noise to solve for, z_out is +0 and the
// next level is left alone.  h_out may be h1 or h2: a chunk is read before it is written, by the same thread.
template <typename T>
struct Inverter {
    static constexpr int N = 16 / sizeof(T);
    const Solve &s;
    const T *x, *model_out;
    const float *h1, *h2;
    int64_t stride;
    T *target, *z_out;
    float *h_out;
    T *eps_out, *x0_out;

    template <bool VEC>
    __device__ __forceinline__ void m(int64_t local, int n, float *out) const {
        combine<T, VEC>(s, model_out + local, stride, n, out);
    }

    template <bool VEC>
    __device__ __forceinline__ void ref(int64_t local, int n, float *r) const {
        load_chunk<T, VEC>(model_out + s.g_ref * stride + local, n, r);
    }

    // factor: the frame's rescale factor (1 and unused without rescale)
    template <bool VEC, bool RESCALE>
    __device__ __forceinline__ void update(float factor, int64_t local, int64_t video, int n, int64_t, int64_t) const {
        float mk[N], xv[N], tv[N], p1[N], p2[N], x0[N], ep[N], z[N], tn[N];
        m<VEC>(local, n, mk);
        load_chunk<T, VEC>(x + video, n, xv);
        if (target) load_chunk<T, VEC>(target + video, n, tv);
        if (h1) load_history<N, VEC>(h1 + video, n, p1);
        if (h2) load_history<N, VEC>(h2 + video, n, p2);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            float mv = mk[k];
            if constexpr (RESCALE) mv = mv * factor;
            vtm::predict(s.pred, s.sqrt_alpha, s.sqrt_beta, xv[k], mv, x0[k], ep[k]);
            const float mu = vtm::solver_sum(s, xv[k], x0[k], h1 != nullptr, p1[k], h2 != nullptr, p2[k]);
            z[k] = 0.0f;
            if (target) {
                z[k] = (tv[k] - mu) / s.c_noise;
                // what the forward step reads back from z_out (store_chunk rounds z the same way), then its own last line
                const float zr = vtm::to_f32(vtm::from_f32<T>(z[k]));
                tn[k] = mu + s.c_noise * zr;
            }
        }
        store_chunk<T, VEC>(z_out + video, n, z);
        if (target) store_chunk<T, VEC>(target + video, n, tn);
        if (h_out) store_history<N, VEC>(h_out + video, n, x0);
        if (eps_out) store_chunk<T, VEC>(eps_out + local, n, ep);
        if (x0_out) store_chunk<T, VEC>(x0_out + local, n, x0);
    }
};

template <typename T, bool VEC>
__global__ __launch_bounds__(vtm::EW_THREADS) void invert_step_kernel(const T *__restrict__ x, const T *__restrict__ model_out,
                                                                      const float *h1, const float *h2, int64_t F, int64_t E,
                                                                      const int32_t *__restrict__ frame_ids, Solve s, T *target,
                                                                      T *__restrict__ z_out, float *h_out,
                                                                      T *__restrict__ eps_out, T *__restrict__ x0_out) {
    vtm::step_elementwise<T, VEC>(Inverter<T>{s, x, model_out, h1, h2, F * E, target, z_out, h_out, eps_out, x0_out}, F, E,
                                  frame_ids);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(vtm::STEP_THREADS) void invert_step_rescale_kernel(
    const T *__restrict__ x, const T *__restrict__ model_out, const float *h1, const float *h2, int64_t F, int64_t E,
    const int32_t *__restrict__ frame_ids, Solve s, T *target, T *__restrict__ z_out, float *h_out, T *__restrict__ eps_out,
    T *__restrict__ x0_out) {
    vtm::step_rescale<T, VEC>(Inverter<T>{s, x, model_out, h1, h2, F * E, target, z_out, h_out, eps_out, x0_out}, E, frame_ids);
}

// levels (n, P), x0 (P), coef (n, 2) = (sqrt_alpha, sqrt_beta) per level: one chunk of one level per iteration
template <typename T, bool VEC>
__global__ __launch_bounds__(vtm::EW_THREADS) void noise_levels_kernel(const T *__restrict__ x0, T *__restrict__ levels,
                                                                       const float *__restrict__ coef, int64_t n, int64_t P) {
    constexpr int N = 16 / sizeof(T);
    const int64_t chunks = (P + N - 1) / N, total = n * chunks;
    for (int64_t i = (int64_t)blockIdx.x * vtm::EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * vtm::EW_THREADS) {
        const int64_t k = i / chunks, e = (i - k * chunks) * N;
        const int cnt = (int)std::min<int64_t>(N, P - e);
        const float sqrt_alpha = coef[2 * k], sqrt_beta = coef[2 * k + 1];
        float xv[N], nz[N], out[N];
        load_chunk<T, VEC>(x0 + e, cnt, xv);
        load_chunk<T, VEC>(levels + k * P + e, cnt, nz);
#pragma unroll
        for (int j = 0; j < N; ++j) out[j] = sqrt_alpha * xv[j] + sqrt_beta * nz[j];
        store_chunk<T, VEC>(levels + k * P + e, cnt, out);
    }
}

}  // namespace

VTM_EXPORT int vtm_invert_step(const void *x, const void *model_out, const float *h1, const float *h2, int dtype, int64_t F,
                               int64_t E, int64_t groups, const float *w, int64_t g_ref, const int32_t *frame_ids, int pred_type,
                               float rescale, float sqrt_alpha, float sqrt_beta, float c_x, float c_x0, float c_h1, float c_h2,
                               float c_noise, void *target, void *z_out, float *h_out, void *eps_out, void *x0_out,
                               vtm_stream_t stream) {
    const char *who = "vtm_invert_step";
    if (const int rc = vtm::check_dtype_pred(who, dtype, pred_type)) return rc;
    if (const int rc = vtm::check_solver_sizes(who, x, model_out, w, F, E, groups, rescale, g_ref)) return rc;
    VTM_REQUIRE(c_noise == 0.0f ? true : target != nullptr, "%s: c_noise != 0 needs target", who);
    VTM_REQUIRE(c_h1 == 0.0f ? true : h1 != nullptr, "%s: c_h1 != 0 needs h1", who);
    VTM_REQUIRE(c_h2 == 0.0f ? true : h2 != nullptr, "%s: c_h2 != 0 needs h2", who);
    VTM_REQUIRE(z_out != nullptr, "%s: z_out is required", who);
    VTM_REQUIRE(target != x && z_out != x && z_out != target, "%s: x, target and z_out must be three buffers", who);
    if (F == 0) return VTM_OK;

    const Solve s = vtm::make_solve(pred_type, rescale, g_ref, groups, w, sqrt_alpha, sqrt_beta, c_x, c_x0, c_h1, c_h2, c_noise);
    // a coefficient of 0: the term is absent, its operand is not read; without c_noise the next level is not touched
    void *target_used = c_noise != 0.0f ? target : nullptr;
    const float *h1_used = c_h1 != 0.0f ? h1 : nullptr, *h2_used = c_h2 != 0.0f ? h2 : nullptr;
    const int rc = vtm::with_dtype(dtype, who, [&](auto t) {
        using T = decltype(t);
        vtm::launch_step<T>(rescale > 0.0f, {invert_step_kernel<T, false>, invert_step_kernel<T, true>},
                            {invert_step_rescale_kernel<T, false>, invert_step_rescale_kernel<T, true>}, F, E,
                            {x, model_out, h1_used, h2_used, target_used, z_out, h_out, eps_out, x0_out}, vtm::as_stream(stream),
                            (const T *)x, (const T *)model_out, h1_used, h2_used, F, E, frame_ids, s, (T *)target_used,
                            (T *)z_out, h_out, (T *)eps_out, (T *)x0_out);
        return (int)VTM_OK;
    });
    if (rc != VTM_OK) return rc;
    return vtm::launch_status(who);
}

VTM_EXPORT int vtm_noise_levels(const void *x0, void *levels, const float *coef, int dtype, int64_t n, int64_t P,
                                vtm_stream_t stream) {
    const char *who = "vtm_noise_levels";
    VTM_REQUIRE(dtype == VTM_F32 || dtype == VTM_F16 || dtype == VTM_BF16, "%s: unsupported dtype %d", who, dtype);
    VTM_REQUIRE(x0 && levels && coef, "%s: x0, levels and coef are required", who);
    VTM_REQUIRE(n >= 0 && n <= (1 << 20) && P >= 1 && P <= ((int64_t)1 << 40), "%s: bad sizes n = %lld, P = %lld", who,
                (long long)n, (long long)P);
    VTM_REQUIRE(x0 != levels, "%s: levels must not be x0", who);
    if (n == 0) return VTM_OK;
    const int rc = vtm::with_dtype(dtype, who, [&](auto t) {
        using T = decltype(t);
        constexpr int N = 16 / sizeof(T);
        const bool vec = P % N == 0 && vtm::aligned16(x0) && vtm::aligned16(levels);
        const dim3 grid((unsigned)std::min<int64_t>(vtm::cdiv(n * vtm::cdiv(P, N), vtm::EW_THREADS), vtm::EW_GRID_CAP));
        auto *const kernel = vec ? noise_levels_kernel<T, true> : noise_levels_kernel<T, false>;
        hipLaunchKernelGGL(kernel, grid, dim3(vtm::EW_THREADS), 0, vtm::as_stream(stream), (const T *)x0, (T *)levels, coef, n, P);
        return (int)VTM_OK;
    });
    if (rc != VTM_OK) return rc;
    return vtm::launch_status(who);
}
