// vtm_guided_step: the caller-side step of one chunk in one launch -- pick the two guidance groups out of the UNet output
// (generate.py:276 `eps.chunk(batch_size)[-2:]`), classifier-free guidance (generate.py:278), Diffusers' guidance rescale
// (`rescale_noise_cfg`: the guided prediction brought back to the conditional prediction's per-frame standard deviation),
// the prediction type (epsilon / v / sample), the DDIM update of `pred_next_x` (generate.py:281-311) with the stochastic
// term sigma * noise, and the store of the chunk's frames into the whole-video latents (`noises[chunk] = ...` followed by
// the whole-video update, generate.py:239-311 / invert.py:181-211).  Unlike vtm_cfg_ddim (ddim.hip), which reproduces the
// reference's per-operation rounding to the tensor dtype, everything here is fp32 and every stored value is rounded once.
//
// The cut into 16-byte chunks, the two launch shapes (elementwise; with rescale one 1024-thread workgroup per frame: a frame
// of E = 2^17 fp16 elements is 512 KB and at most 128 additions per lane) and the reduction order are step_core.h's.  This
// file says what m is (guide) and what the update adds up (Guided::update).
#include "common.h"
#include "step_core.h"

namespace {

constexpr int GS_THREADS = 1024;              // rescale: threads of a frame's workgroup (_lib.GUIDED_STEP_THREADS)
constexpr int EW_THREADS = 256;               // elementwise: threads per block,
constexpr int64_t EW_GRID_CAP = 4096;         // ... and the most blocks of its grid-stride launch
// (restated for the tests that size their shapes from this file; the launch is step_core.h's)
static_assert(GS_THREADS == vtm::STEP_THREADS && EW_THREADS == vtm::EW_THREADS && EW_GRID_CAP == vtm::EW_GRID_CAP,
              "the launch shapes are step_core.h's");

struct Step {
    int pred;
    bool guided;                              // g_cond >= 0
    float guidance, rescale, sqrt_alpha, sqrt_beta, c_x0, c_eps, sigma;
};

using vtm::load_chunk;
using vtm::store_chunk;

// m = m_u + guidance (m_c - m_u): the same three operations wherever m is needed, so every pass sees the same m
__device__ __forceinline__ float guide(const Step &s, float mu, float mc) { return s.guided ? mu + s.guidance * (mc - mu) : mu; }

// step_core.h's policy: the launch's operands.  mu / mc: the unconditional and the conditional group of model_out (mc null
// without guidance); noise and any output may be null.  x_out may be x: a chunk is read before it is written, by the same
// thread.  KEYED (vtm_guided_step_keyed): there is no noise tensor, the chunk's noise is drawn from kn where it is used.
template <typename T, bool KEYED = false>
struct Guided {
    static constexpr int N = 16 / sizeof(T);
    const Step &s;
    const T *x, *mu, *mc, *noise;
    T *x_out, *eps_out, *x0_out;
    vtm::KeyedNoise kn{};

    template <bool VEC>
    __device__ __forceinline__ void m(int64_t local, int n, float *out) const {
        float u[N], c[N];
        load_chunk<T, VEC>(mu + local, n, u);
        if (s.guided) load_chunk<T, VEC>(mc + local, n, c);
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] = guide(s, u[k], s.guided ? c[k] : 0.0f);
    }

    template <bool VEC>
    __device__ __forceinline__ void ref(int64_t local, int n, float *r) const {
        load_chunk<T, VEC>(mc + local, n, r);
    }

    // factor: the frame's rescale factor (1 and unused without rescale)
    template <bool VEC, bool RESCALE>
    __device__ __forceinline__ void update(float factor, int64_t local, int64_t video, int n, int64_t row, int64_t e) const {
        float mk[N], xv[N], nz[N], x0[N], ep[N], xn[N];
        m<VEC>(local, n, mk);
        load_chunk<T, VEC>(x + video, n, xv);
        if constexpr (KEYED) vtm::normal_chunk<T>(kn, row, e, nz);
        else if (noise) load_chunk<T, VEC>(noise + local, n, nz);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            float mv = mk[k];
            if constexpr (RESCALE) mv = mv * factor;
            vtm::predict(s.pred, s.sqrt_alpha, s.sqrt_beta, xv[k], mv, x0[k], ep[k]);
            xn[k] = s.c_x0 * x0[k] + s.c_eps * ep[k];
            if (KEYED || noise) xn[k] = xn[k] + s.sigma * nz[k];
        }
        if (x_out) store_chunk<T, VEC>(x_out + video, n, xn);
        if (eps_out) store_chunk<T, VEC>(eps_out + local, n, ep);
        if (x0_out) store_chunk<T, VEC>(x0_out + local, n, x0);
    }
};

template <typename T, bool VEC>
__global__ __launch_bounds__(EW_THREADS) void guided_step_kernel(const T *x, const T *__restrict__ model_out,
                                                                 const T *__restrict__ noise, int64_t F, int64_t E,
                                                                 int64_t g_uncond, int64_t g_cond,
                                                                 const int32_t *__restrict__ frame_ids, Step s, T *x_out,
                                                                 T *__restrict__ eps_out, T *__restrict__ x0_out) {
    vtm::step_elementwise<T, VEC>(Guided<T>{s, x, model_out + g_uncond * F * E, s.guided ? model_out + g_cond * F * E : nullptr,
                                            noise, x_out, eps_out, x0_out},
                                  F, E, frame_ids);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(GS_THREADS) void guided_step_rescale_kernel(const T *x, const T *__restrict__ model_out,
                                                                         const T *__restrict__ noise, int64_t F, int64_t E,
                                                                         int64_t g_uncond, int64_t g_cond,
                                                                         const int32_t *__restrict__ frame_ids, Step s,
                                                                         T *x_out, T *__restrict__ eps_out,
                                                                         T *__restrict__ x0_out) {
    vtm::step_rescale<T, VEC>(Guided<T>{s, x, model_out + g_uncond * F * E, model_out + g_cond * F * E, noise, x_out, eps_out,
                                        x0_out},
                              E, frame_ids);
}

// the keyed forms of the two kernels: the noise pointer gives way to the key
template <typename T, bool VEC>
__global__ __launch_bounds__(EW_THREADS) void guided_keyed_kernel(const T *x, const T *__restrict__ model_out,
                                                                  vtm::KeyedNoise kn, int64_t F, int64_t E, int64_t g_uncond,
                                                                  int64_t g_cond, const int32_t *__restrict__ frame_ids, Step s,
                                                                  T *x_out, T *__restrict__ eps_out, T *__restrict__ x0_out) {
    vtm::step_elementwise<T, VEC>(Guided<T, true>{s, x, model_out + g_uncond * F * E,
                                                  s.guided ? model_out + g_cond * F * E : nullptr, nullptr, x_out, eps_out,
                                                  x0_out, kn},
                                  F, E, frame_ids);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(GS_THREADS) void guided_keyed_rescale_kernel(const T *x, const T *__restrict__ model_out,
                                                                          vtm::KeyedNoise kn, int64_t F, int64_t E,
                                                                          int64_t g_uncond, int64_t g_cond,
                                                                          const int32_t *__restrict__ frame_ids, Step s,
                                                                          T *x_out, T *__restrict__ eps_out,
                                                                          T *__restrict__ x0_out) {
    vtm::step_rescale<T, VEC>(Guided<T, true>{s, x, model_out + g_uncond * F * E, model_out + g_cond * F * E, nullptr, x_out,
                                              eps_out, x0_out, kn},
                              E, frame_ids);
}

// the body of both exports; kn: the keyed export's noise (noise is then null), null for the tensor form
int guided_step(const char *who, const void *x, const void *model_out, const void *noise, const vtm::KeyedNoise *kn, int dtype,
                int64_t F, int64_t E, int64_t groups, int64_t g_uncond, int64_t g_cond, const int32_t *frame_ids, int pred_type,
                float guidance, float rescale, float sqrt_alpha, float sqrt_beta, float c_x0, float c_eps, float sigma,
                void *x_out, void *eps_out, void *x0_out, vtm_stream_t stream) {
    if (const int rc = vtm::check_dtype_pred(who, dtype, pred_type)) return rc;
    VTM_REQUIRE(x && model_out, "%s: x and model_out are required", who);
    // (F bounds the grid of the per-frame launch: 1024 F threads must stay below 2^32)
    VTM_REQUIRE(F >= 0 && F <= (1 << 20) && E >= 1 && groups >= 1, "%s: bad sizes F = %lld, E = %lld, groups = %lld", who,
                (long long)F, (long long)E, (long long)groups);
    VTM_REQUIRE(g_uncond >= 0 && g_uncond < groups, "%s: g_uncond = %lld outside [0, %lld)", who, (long long)g_uncond,
                (long long)groups);
    VTM_REQUIRE(g_cond >= -1 && g_cond < groups, "%s: g_cond = %lld outside [0, %lld) and not -1", who, (long long)g_cond,
                (long long)groups);
    VTM_REQUIRE(g_cond != g_uncond, "%s: g_uncond == g_cond == %lld", who, (long long)g_cond);
    VTM_REQUIRE(sigma == 0.0f ? true : (noise != nullptr || kn), "%s: sigma != 0 needs noise", who);
    VTM_REQUIRE(!(rescale < 0.0f) && rescale == rescale, "%s: rescale = %g is negative or NaN", who, (double)rescale);
    VTM_REQUIRE(!(rescale > 0.0f) || (g_cond >= 0 && E >= 2), "%s: rescale > 0 needs a conditional group and E >= 2", who);
    VTM_REQUIRE(x_out || eps_out || x0_out, "%s: no output", who);
    if (F == 0) return VTM_OK;

    const Step s{pred_type, g_cond >= 0, guidance, rescale, sqrt_alpha, sqrt_beta, c_x0, c_eps, sigma};
    const void *noise_used = sigma != 0.0f ? noise : nullptr;       // sigma == 0: the term is absent, noise is not read
    const int rc = vtm::with_dtype(dtype, who, [&](auto t) {
        using T = decltype(t);
        if (kn && sigma != 0.0f)
            vtm::launch_step<T>(rescale > 0.0f, {guided_keyed_kernel<T, false>, guided_keyed_kernel<T, true>},
                                {guided_keyed_rescale_kernel<T, false>, guided_keyed_rescale_kernel<T, true>}, F, E,
                                {x, model_out, x_out, eps_out, x0_out}, vtm::as_stream(stream), (const T *)x,
                                (const T *)model_out, *kn, F, E, g_uncond, g_cond, frame_ids, s, (T *)x_out, (T *)eps_out,
                                (T *)x0_out);
        else
            vtm::launch_step<T>(rescale > 0.0f, {guided_step_kernel<T, false>, guided_step_kernel<T, true>},
                            {guided_step_rescale_kernel<T, false>, guided_step_rescale_kernel<T, true>}, F, E,
                            {x, model_out, noise_used, x_out, eps_out, x0_out}, vtm::as_stream(stream), (const T *)x,
                            (const T *)model_out, (const T *)noise_used, F, E, g_uncond, g_cond, frame_ids, s, (T *)x_out,
                            (T *)eps_out, (T *)x0_out);
        return (int)VTM_OK;
    });
    if (rc != VTM_OK) return rc;
    return vtm::launch_status(who);
}

}  // namespace

VTM_EXPORT int vtm_guided_step(const void *x, const void *model_out, const void *noise, int dtype, int64_t F, int64_t E,
                               int64_t groups, int64_t g_uncond, int64_t g_cond, const int32_t *frame_ids, int pred_type,
                               float guidance, float rescale, float sqrt_alpha, float sqrt_beta, float c_x0, float c_eps,
                               float sigma, void *x_out, void *eps_out, void *x0_out, vtm_stream_t stream) {
    return guided_step("vtm_guided_step", x, model_out, noise, nullptr, dtype, F, E, groups, g_uncond, g_cond, frame_ids,
                       pred_type, guidance, rescale, sqrt_alpha, sqrt_beta, c_x0, c_eps, sigma, x_out, eps_out, x0_out, stream);
}

VTM_EXPORT int vtm_guided_step_keyed(const void *x, const void *model_out, uint64_t seed, uint32_t step, uint32_t tag,
                                     int64_t frame0, int dtype, int64_t F, int64_t E, int64_t groups, int64_t g_uncond,
                                     int64_t g_cond, const int32_t *frame_ids, int pred_type, float guidance, float rescale,
                                     float sqrt_alpha, float sqrt_beta, float c_x0, float c_eps, float sigma, void *x_out,
                                     void *eps_out, void *x0_out, vtm_stream_t stream) {
    const char *who = "vtm_guided_step_keyed";
    if (const int rc = vtm::check_keyed(who, frame0, E)) return rc;
    const vtm::KeyedNoise kn{vtm::noise_key(seed, step, tag), (uint32_t)frame0};
    return guided_step(who, x, model_out, nullptr, &kn, dtype, F, E, groups, g_uncond, g_cond, frame_ids, pred_type, guidance,
                       rescale, sqrt_alpha, sqrt_beta, c_x0, c_eps, sigma, x_out, eps_out, x0_out, stream);
}
