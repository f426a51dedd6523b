// vtm_guided_step: the caller-side step of one chunk in one launch -- pick the two guidance groups out of the UNet output
// (generate.py:276 `eps.chunk(batch_size)[-2:]`), classifier-free guidance (generate.py:278), Diffusers' guidance rescale
// (`rescale_noise_cfg`: the guided prediction brought back to the conditional prediction's per-frame standard deviation),
// the prediction type (epsilon / v / sample), the DDIM update of `pred_next_x` (generate.py:281-311) with the stochastic
// term sigma * noise, and the store of the chunk's frames into the whole-video latents (`noises[chunk] = ...` followed by
// the whole-video update, generate.py:239-311 / invert.py:181-211).  Unlike vtm_cfg_ddim (ddim.hip), which reproduces the
// reference's per-operation rounding to the tensor dtype, everything here is fp32 and every stored value is rounded once.
//
// Work is cut into 16-byte CHUNKS of a frame (4 fp32 / 8 16-bit elements; a frame whose E is no multiple ends in a short
// chunk, chunks never straddle frames).  A chunk is moved with one 16-byte access when E is a multiple of the chunk and every
// pointer is 16-byte aligned, and element by element otherwise; which of the two it is changes no bit of the result: the
// per-element arithmetic is the same, and the statistics below assign chunks to lanes and add in the same order either way.
//
//   rescale == 0   elementwise: a grid-stride loop over the F * chunks-per-frame chunks.
//   rescale  > 0   one 1024-thread workgroup per frame, three passes over the frame's two groups (after the first they come
//                  from L2: a frame of E = 2^17 fp16 elements is 512 KB): the means of m_c and of the guided m; their
//                  squared deviations; the update.  Lane t adds its chunks t, t + 1024, ... serially (E <= 2^17: at most
//                  128 additions), then a 64-lane butterfly, then a binary tree over the 16 wave sums -- an order that depends
//                  on E alone, so a frame's bits depend neither on the other frames of the launch nor on the run.
// One launch, no workspace, no atomics.
#include "common.h"
#include "step_chunk.h"

#include <algorithm>

namespace {

constexpr int GS_THREADS = 1024;              // rescale: threads of a frame's workgroup (_lib.GUIDED_STEP_THREADS)
constexpr int GS_WAVES = GS_THREADS / 64;
constexpr int EW_THREADS = 256;               // elementwise: threads per block,
constexpr int64_t EW_GRID_CAP = 4096;         // ... and the most blocks of its grid-stride launch

struct Step {
    int pred;
    bool guided;                              // g_cond >= 0
    float guidance, rescale, sqrt_alpha, sqrt_beta, c_x0, c_eps, sigma;
};

using vtm::aligned16;
using vtm::from_f32;
using vtm::load_chunk;
using vtm::store_chunk;

// m = m_u + guidance (m_c - m_u): the same three operations wherever m is needed, so every pass sees the same m
__device__ __forceinline__ float guide(const Step &s, float mu, float mc) { return s.guided ? mu + s.guidance * (mc - mu) : mu; }

// One chunk of the update.  mu / mc / x / noise / the outputs point at the chunk's first element (mc, noise and any output
// may be null); factor is the frame's rescale factor (1 and unused without rescale).  x_out may be x: the chunk is read
// before it is written, by the same thread.
template <typename T, bool VEC, bool RESCALE>
__device__ __forceinline__ void step_chunk(const Step &s, float factor, const T *mu, const T *mc, const T *x, const T *noise,
                                           T *x_out, T *eps_out, T *x0_out, int n) {
    constexpr int N = 16 / sizeof(T);
    float u[N], c[N], xv[N], nz[N], x0[N], ep[N], xn[N];
    load_chunk<T, VEC>(mu, n, u);
    if (s.guided) load_chunk<T, VEC>(mc, n, c);
    load_chunk<T, VEC>(x, n, xv);
    if (noise) load_chunk<T, VEC>(noise, n, nz);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        float m = guide(s, u[k], s.guided ? c[k] : 0.0f);
        if constexpr (RESCALE) m = m * factor;
        if (s.pred == VTM_PRED_EPSILON) {
            ep[k] = m;
            x0[k] = (xv[k] - s.sqrt_beta * m) / s.sqrt_alpha;
        } else if (s.pred == VTM_PRED_V) {
            x0[k] = s.sqrt_alpha * xv[k] - s.sqrt_beta * m;
            ep[k] = s.sqrt_alpha * m + s.sqrt_beta * xv[k];
        } else {
            x0[k] = m;
            ep[k] = (xv[k] - s.sqrt_alpha * m) / s.sqrt_beta;
        }
        xn[k] = s.c_x0 * x0[k] + s.c_eps * ep[k];
        if (noise) xn[k] = xn[k] + s.sigma * nz[k];
    }
    if (x_out) store_chunk<T, VEC>(x_out, n, xn);
    if (eps_out) store_chunk<T, VEC>(eps_out, n, ep);
    if (x0_out) store_chunk<T, VEC>(x0_out, n, x0);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(EW_THREADS) void guided_step_kernel(const T *x, const T *__restrict__ model_out,
                                                                 const T *__restrict__ noise, int64_t F, int64_t E,
                                                                 int64_t g_uncond, int64_t g_cond,
                                                                 const int32_t *__restrict__ frame_ids, Step s, T *x_out,
                                                                 T *__restrict__ eps_out, T *__restrict__ x0_out) {
    constexpr int N = 16 / sizeof(T);
    const int64_t chunks = (E + N - 1) / N, total = F * chunks;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * EW_THREADS) {
        const int64_t f = i / chunks, e = (i - f * chunks) * N;
        const int n = (int)std::min<int64_t>(N, E - e);
        const int64_t row = frame_ids ? (int64_t)frame_ids[f] : f;
        const int64_t local = f * E + e, video = row * E + e;
        step_chunk<T, VEC, false>(s, 1.0f, model_out + g_uncond * F * E + local,
                                  s.guided ? model_out + g_cond * F * E + local : nullptr, x + video,
                                  noise ? noise + local : nullptr, x_out ? x_out + video : nullptr,
                                  eps_out ? eps_out + local : nullptr, x0_out ? x0_out + local : nullptr, n);
    }
}

// the workgroup's sums of a and b in every thread: 64-lane butterfly, then a binary tree over the wave sums
__device__ __forceinline__ void block_sum2(float &a, float &b, float (*scratch)[GS_WAVES]) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        scratch[0][threadIdx.x >> 6] = a;
        scratch[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    float wa[GS_WAVES], wb[GS_WAVES];
#pragma unroll
    for (int w = 0; w < GS_WAVES; ++w) {
        wa[w] = scratch[0][w];
        wb[w] = scratch[1][w];
    }
#pragma unroll
    for (int h = GS_WAVES / 2; h > 0; h >>= 1)
#pragma unroll
        for (int w = 0; w < h; ++w) {
            wa[w] += wa[w + h];
            wb[w] += wb[w + h];
        }
    a = wa[0];
    b = wb[0];
}

template <typename T, bool VEC>
__global__ __launch_bounds__(GS_THREADS) void guided_step_rescale_kernel(const T *x, const T *__restrict__ model_out,
                                                                         const T *__restrict__ noise, int64_t F, int64_t E,
                                                                         int64_t g_uncond, int64_t g_cond,
                                                                         const int32_t *__restrict__ frame_ids, Step s,
                                                                         T *x_out, T *__restrict__ eps_out,
                                                                         T *__restrict__ x0_out) {
    constexpr int N = 16 / sizeof(T);
    __shared__ float scratch[2][2][GS_WAVES];     // one pair of rows per pass: no barrier between a read and the next write
    const int64_t f = blockIdx.x, chunks = (E + N - 1) / N;
    const T *mu = model_out + (g_uncond * F + f) * E, *mc = model_out + (g_cond * F + f) * E;
    float u[N], c[N];

    float sum_c = 0.0f, sum_m = 0.0f;
    for (int64_t i = threadIdx.x; i < chunks; i += GS_THREADS) {
        const int n = (int)std::min<int64_t>(N, E - i * N);
        load_chunk<T, VEC>(mu + i * N, n, u);
        load_chunk<T, VEC>(mc + i * N, n, c);
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < n) {
                sum_c += c[k];
                sum_m += guide(s, u[k], c[k]);
            }
    }
    block_sum2(sum_c, sum_m, scratch[0]);
    const float mean_c = sum_c / (float)E, mean_m = sum_m / (float)E;

    float dev_c = 0.0f, dev_m = 0.0f;
    for (int64_t i = threadIdx.x; i < chunks; i += GS_THREADS) {
        const int n = (int)std::min<int64_t>(N, E - i * N);
        load_chunk<T, VEC>(mu + i * N, n, u);
        load_chunk<T, VEC>(mc + i * N, n, c);
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < n) {
                const float dc = c[k] - mean_c, dm = guide(s, u[k], c[k]) - mean_m;
                dev_c += dc * dc;
                dev_m += dm * dm;
            }
    }
    block_sum2(dev_c, dev_m, scratch[1]);
    // torch.std: unbiased.  std(m) == 0 divides by zero as IEEE says (no special case)
    const float std_c = sqrtf(dev_c / (float)(E - 1)), std_m = sqrtf(dev_m / (float)(E - 1));
    const float factor = s.rescale * (std_c / std_m) + (1.0f - s.rescale);

    const int64_t row = frame_ids ? (int64_t)frame_ids[f] : f;
    for (int64_t i = threadIdx.x; i < chunks; i += GS_THREADS) {
        const int64_t e = i * N, local = f * E + e, video = row * E + e;
        const int n = (int)std::min<int64_t>(N, E - e);
        step_chunk<T, VEC, true>(s, factor, mu + e, mc + e, x + video, noise ? noise + local : nullptr,
                                 x_out ? x_out + video : nullptr, eps_out ? eps_out + local : nullptr,
                                 x0_out ? x0_out + local : nullptr, n);
    }
}

}  // namespace

VTM_EXPORT int vtm_guided_step(const void *x, const void *model_out, const void *noise, int dtype, int64_t F, int64_t E,
                               int64_t groups, int64_t g_uncond, int64_t g_cond, const int32_t *frame_ids, int pred_type,
                               float guidance, float rescale, float sqrt_alpha, float sqrt_beta, float c_x0, float c_eps,
                               float sigma, void *x_out, void *eps_out, void *x0_out, vtm_stream_t stream) {
    const char *who = "vtm_guided_step";
    VTM_REQUIRE(dtype == VTM_F32 || dtype == VTM_F16 || dtype == VTM_BF16, "%s: unsupported dtype %d", who, dtype);
    VTM_REQUIRE(pred_type == VTM_PRED_EPSILON || pred_type == VTM_PRED_V || pred_type == VTM_PRED_SAMPLE,
                "%s: unknown pred_type %d", who, pred_type);
    VTM_REQUIRE(x && model_out, "%s: x and model_out are required", who);
    // (F bounds the grid of the per-frame launch: 1024 F threads must stay below 2^32)
    VTM_REQUIRE(F >= 0 && F <= (1 << 20) && E >= 1 && groups >= 1, "%s: bad sizes F = %lld, E = %lld, groups = %lld", who,
                (long long)F, (long long)E, (long long)groups);
    VTM_REQUIRE(g_uncond >= 0 && g_uncond < groups, "%s: g_uncond = %lld outside [0, %lld)", who, (long long)g_uncond,
                (long long)groups);
    VTM_REQUIRE(g_cond >= -1 && g_cond < groups, "%s: g_cond = %lld outside [0, %lld) and not -1", who, (long long)g_cond,
                (long long)groups);
    VTM_REQUIRE(g_cond != g_uncond, "%s: g_uncond == g_cond == %lld", who, (long long)g_cond);
    VTM_REQUIRE(sigma == 0.0f ? true : noise != nullptr, "%s: sigma != 0 needs noise", who);
    VTM_REQUIRE(!(rescale < 0.0f) && rescale == rescale, "%s: rescale = %g is negative or NaN", who, (double)rescale);
    VTM_REQUIRE(!(rescale > 0.0f) || (g_cond >= 0 && E >= 2), "%s: rescale > 0 needs a conditional group and E >= 2", who);
    VTM_REQUIRE(x_out || eps_out || x0_out, "%s: no output", who);
    if (F == 0) return VTM_OK;

    const Step s{pred_type, g_cond >= 0, guidance, rescale, sqrt_alpha, sqrt_beta, c_x0, c_eps, sigma};
    const void *noise_used = sigma != 0.0f ? noise : nullptr;       // sigma == 0: the term is absent, noise is not read
    hipStream_t st = vtm::as_stream(stream);
    const int rc = vtm::with_dtype(dtype, who, [&](auto t) {
        using T = decltype(t);
        constexpr int N = 16 / sizeof(T);
        const bool vec = E % N == 0 && aligned16(x) && aligned16(model_out) && aligned16(noise_used) && aligned16(x_out) &&
                         aligned16(eps_out) && aligned16(x0_out);
        auto launch = [&](auto kernel, dim3 grid, dim3 block) {
            hipLaunchKernelGGL(kernel, grid, block, 0, st, (const T *)x, (const T *)model_out, (const T *)noise_used, F, E,
                               g_uncond, g_cond, frame_ids, s, (T *)x_out, (T *)eps_out, (T *)x0_out);
        };
        if (rescale > 0.0f) {
            const dim3 grid((unsigned)F), block(GS_THREADS);
            if (vec) launch(guided_step_rescale_kernel<T, true>, grid, block);
            else launch(guided_step_rescale_kernel<T, false>, grid, block);
        } else {
            const dim3 grid((unsigned)std::min<int64_t>(vtm::cdiv(F * vtm::cdiv(E, N), EW_THREADS), EW_GRID_CAP)),
                block(EW_THREADS);
            if (vec) launch(guided_step_kernel<T, true>, grid, block);
            else launch(guided_step_kernel<T, false>, grid, block);
        }
        return (int)VTM_OK;
    });
    if (rc != VTM_OK) return rc;
    return vtm::launch_status(who);
}
