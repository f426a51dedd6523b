// vtm_solver_step: the caller-side step of one chunk in one launch for a multistep solver (DPM-Solver++, sampler.py's
// GuidedDPMSolver) -- the weighted sum over the groups of the UNet output (classifier-free guidance and its three-term
// relatives), Diffusers' guidance rescale, the prediction type, and the update
//     x' = c_x x + c_x0 x0 + c_h1 h1 + c_h2 h2 + c_noise noise
// whose history h1 / h2 (the clean-sample predictions of the two previous steps) lives per frame in whole-video fp32 buffers;
// this step's x0 goes to h_out.  Everything is fp32 and every stored value is rounded once.
//
// The cut into 16-byte chunks of the model dtype, the two launch shapes and the reduction order are step_core.h's; this file
// says what the update adds up (Solver::update); what m is (combine) and the deterministic part of the sum (solver_sum) are
// solver_core.h's, shared with the inverse step (invert_step.hip).  A chunk of the fp32 history is 16 or 32 bytes (4 / 8
// elements): one or two 16-byte accesses.
#include "common.h"
#include "solver_core.h"

namespace {

using vtm::combine;
using vtm::load_chunk;
using vtm::load_history;
using vtm::Solve;
using vtm::store_chunk;
using vtm::store_history;

constexpr int SS_THREADS = 1024;              // rescale: threads of a frame's workgroup (_lib.SOLVER_STEP_THREADS)
static_assert(SS_THREADS == vtm::STEP_THREADS, "the per-frame launch is step_core.h's");

// step_core.h's policy: the launch's operands.  Group g of model_out lies g * stride elements behind group 0; all but
// model_out and x may be null.  x_out may be x and h_out may be h1 or h2: a chunk is read before it is written, by the same
// thread.  KEYED (vtm_solver_step_keyed): there is no noise tensor, the chunk's noise is drawn from kn where it is used.
template <typename T, bool KEYED = false>
struct Solver {
    static constexpr int N = 16 / sizeof(T);
    const Solve &s;
    const T *x, *model_out, *noise;
    const float *h1, *h2;
    int64_t stride;
    T *x_out;
    float *h_out;
    T *eps_out, *x0_out;
    vtm::KeyedNoise kn{};

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
    __device__ __forceinline__ void update(float factor, int64_t local, int64_t video, int n, int64_t row, int64_t e) const {
        float mk[N], xv[N], nz[N], p1[N], p2[N], x0[N], ep[N], xn[N];
        m<VEC>(local, n, mk);
        load_chunk<T, VEC>(x + video, n, xv);
        if constexpr (KEYED) vtm::normal_chunk<T>(kn, row, e, nz);
        else if (noise) load_chunk<T, VEC>(noise + local, n, nz);
        if (h1) load_history<N, VEC>(h1 + video, n, p1);
        if (h2) load_history<N, VEC>(h2 + video, n, p2);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            float mv = mk[k];
            if constexpr (RESCALE) mv = mv * factor;
            vtm::predict(s.pred, s.sqrt_alpha, s.sqrt_beta, xv[k], mv, x0[k], ep[k]);
            float acc = vtm::solver_sum(s, xv[k], x0[k], h1 != nullptr, p1[k], h2 != nullptr, p2[k]);
            if (KEYED || noise) acc = acc + s.c_noise * nz[k];
            xn[k] = acc;
        }
        if (x_out) store_chunk<T, VEC>(x_out + video, n, xn);
        if (h_out) store_history<N, VEC>(h_out + video, n, x0);
        if (eps_out) store_chunk<T, VEC>(eps_out + local, n, ep);
        if (x0_out) store_chunk<T, VEC>(x0_out + local, n, x0);
    }
};

template <typename T, bool VEC>
__global__ __launch_bounds__(vtm::EW_THREADS) void solver_step_kernel(const T *x, const T *__restrict__ model_out,
                                                                      const T *__restrict__ noise, const float *h1,
                                                                      const float *h2, int64_t F, int64_t E,
                                                                      const int32_t *__restrict__ frame_ids, Solve s, T *x_out,
                                                                      float *h_out, T *__restrict__ eps_out,
                                                                      T *__restrict__ x0_out) {
    vtm::step_elementwise<T, VEC>(Solver<T>{s, x, model_out, noise, h1, h2, F * E, x_out, h_out, eps_out, x0_out}, F, E,
                                  frame_ids);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(SS_THREADS) void solver_step_rescale_kernel(const T *x, const T *__restrict__ model_out,
                                                                         const T *__restrict__ noise, const float *h1,
                                                                         const float *h2, int64_t F, int64_t E,
                                                                         const int32_t *__restrict__ frame_ids, Solve s,
                                                                         T *x_out, float *h_out, T *__restrict__ eps_out,
                                                                         T *__restrict__ x0_out) {
    vtm::step_rescale<T, VEC>(Solver<T>{s, x, model_out, noise, h1, h2, F * E, x_out, h_out, eps_out, x0_out}, E, frame_ids);
}

// the keyed forms of the two kernels: the noise pointer gives way to the key
template <typename T, bool VEC>
__global__ __launch_bounds__(vtm::EW_THREADS) void solver_keyed_kernel(const T *x, const T *__restrict__ model_out,
                                                                       vtm::KeyedNoise kn, const float *h1, const float *h2,
                                                                       int64_t F, int64_t E,
                                                                       const int32_t *__restrict__ frame_ids, Solve s, T *x_out,
                                                                       float *h_out, T *__restrict__ eps_out,
                                                                       T *__restrict__ x0_out) {
    vtm::step_elementwise<T, VEC>(Solver<T, true>{s, x, model_out, nullptr, h1, h2, F * E, x_out, h_out, eps_out, x0_out, kn},
                                  F, E, frame_ids);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(SS_THREADS) void solver_keyed_rescale_kernel(const T *x, const T *__restrict__ model_out,
                                                                          vtm::KeyedNoise kn, const float *h1, const float *h2,
                                                                          int64_t F, int64_t E,
                                                                          const int32_t *__restrict__ frame_ids, Solve s,
                                                                          T *x_out, float *h_out, T *__restrict__ eps_out,
                                                                          T *__restrict__ x0_out) {
    vtm::step_rescale<T, VEC>(Solver<T, true>{s, x, model_out, nullptr, h1, h2, F * E, x_out, h_out, eps_out, x0_out, kn}, E,
                              frame_ids);
}

// the body of both exports; kn: the keyed export's noise (noise is then null), null for the tensor form
int solver_step(const char *who, const void *x, const void *model_out, const void *noise, const vtm::KeyedNoise *kn,
                const float *h1, const float *h2, int dtype, int64_t F, int64_t E, int64_t groups, const float *w,
                int64_t g_ref, const int32_t *frame_ids, int pred_type, float rescale, float sqrt_alpha, float sqrt_beta,
                float c_x, float c_x0, float c_h1, float c_h2, float c_noise, void *x_out, float *h_out, void *eps_out,
                void *x0_out, vtm_stream_t stream) {
    if (const int rc = vtm::check_dtype_pred(who, dtype, pred_type)) return rc;
    if (const int rc = vtm::check_solver_sizes(who, x, model_out, w, F, E, groups, rescale, g_ref)) return rc;
    VTM_REQUIRE(c_noise == 0.0f ? true : (noise != nullptr || kn), "%s: c_noise != 0 needs noise", who);
    VTM_REQUIRE(c_h1 == 0.0f ? true : h1 != nullptr, "%s: c_h1 != 0 needs h1", who);
    VTM_REQUIRE(c_h2 == 0.0f ? true : h2 != nullptr, "%s: c_h2 != 0 needs h2", who);
    VTM_REQUIRE(x_out || h_out || eps_out || x0_out, "%s: no output", who);
    if (F == 0) return VTM_OK;

    const Solve s = vtm::make_solve(pred_type, rescale, g_ref, groups, w, sqrt_alpha, sqrt_beta, c_x, c_x0, c_h1, c_h2, c_noise);
    // a coefficient of 0: the term is absent, its operand is not read
    const void *noise_used = c_noise != 0.0f ? noise : nullptr;
    const float *h1_used = c_h1 != 0.0f ? h1 : nullptr, *h2_used = c_h2 != 0.0f ? h2 : nullptr;
    const int rc = vtm::with_dtype(dtype, who, [&](auto t) {
        using T = decltype(t);
        if (kn && c_noise != 0.0f)
            vtm::launch_step<T>(rescale > 0.0f, {solver_keyed_kernel<T, false>, solver_keyed_kernel<T, true>},
                                {solver_keyed_rescale_kernel<T, false>, solver_keyed_rescale_kernel<T, true>}, F, E,
                                {x, model_out, h1_used, h2_used, x_out, h_out, eps_out, x0_out}, vtm::as_stream(stream),
                                (const T *)x, (const T *)model_out, *kn, h1_used, h2_used, F, E, frame_ids, s, (T *)x_out,
                                h_out, (T *)eps_out, (T *)x0_out);
        else
            vtm::launch_step<T>(rescale > 0.0f, {solver_step_kernel<T, false>, solver_step_kernel<T, true>},
                                {solver_step_rescale_kernel<T, false>, solver_step_rescale_kernel<T, true>}, F, E,
                                {x, model_out, noise_used, h1_used, h2_used, x_out, h_out, eps_out, x0_out},
                                vtm::as_stream(stream), (const T *)x, (const T *)model_out, (const T *)noise_used, h1_used,
                                h2_used, F, E, frame_ids, s, (T *)x_out, h_out, (T *)eps_out, (T *)x0_out);
        return (int)VTM_OK;
    });
    if (rc != VTM_OK) return rc;
    return vtm::launch_status(who);
}

}  // namespace

VTM_EXPORT int vtm_solver_step(const void *x, const void *model_out, const void *noise, const float *h1, const float *h2,
                               int dtype, int64_t F, int64_t E, int64_t groups, const float *w, int64_t g_ref,
                               const int32_t *frame_ids, int pred_type, float rescale, float sqrt_alpha, float sqrt_beta,
                               float c_x, float c_x0, float c_h1, float c_h2, float c_noise, void *x_out, float *h_out,
                               void *eps_out, void *x0_out, vtm_stream_t stream) {
    return solver_step("vtm_solver_step", x, model_out, noise, nullptr, h1, h2, dtype, F, E, groups, w, g_ref, frame_ids,
                       pred_type, rescale, sqrt_alpha, sqrt_beta, c_x, c_x0, c_h1, c_h2, c_noise, x_out, h_out, eps_out, x0_out,
                       stream);
}

VTM_EXPORT int vtm_solver_step_keyed(const void *x, const void *model_out, uint64_t seed, uint32_t step, uint32_t tag,
                                     int64_t frame0, const float *h1, const float *h2, int dtype, int64_t F, int64_t E,
                                     int64_t groups, const float *w, int64_t g_ref, const int32_t *frame_ids, int pred_type,
                                     float rescale, float sqrt_alpha, float sqrt_beta, float c_x, float c_x0, float c_h1,
                                     float c_h2, float c_noise, void *x_out, float *h_out, void *eps_out, void *x0_out,
                                     vtm_stream_t stream) {
    const char *who = "vtm_solver_step_keyed";
    if (const int rc = vtm::check_keyed(who, frame0, E)) return rc;
    const vtm::KeyedNoise kn{vtm::noise_key(seed, step, tag), (uint32_t)frame0};
    return solver_step(who, x, model_out, nullptr, &kn, h1, h2, dtype, F, E, groups, w, g_ref, frame_ids, pred_type, rescale,
                       sqrt_alpha, sqrt_beta, c_x, c_x0, c_h1, c_h2, c_noise, x_out, h_out, eps_out, x0_out, stream);
}
