// vtm_solver_step: the caller-side step of one chunk in one launch for a multistep solver (DPM-Solver++, sampler.py's
// GuidedDPMSolver) -- the weighted sum over the groups of the UNet output (classifier-free guidance and its three-term
// relatives), Diffusers' guidance rescale, the prediction type, and the update
//     x' = c_x x + c_x0 x0 + c_h1 h1 + c_h2 h2 + c_noise noise
// whose history h1 / h2 (the clean-sample predictions of the two previous steps) lives per frame in whole-video fp32 buffers;
// this step's x0 goes to h_out.  Everything is fp32 and every stored value is rounded once.
//
// The cut into 16-byte chunks of the model dtype, the two launch shapes and the reduction order are guided_step.hip's:
//   rescale == 0   elementwise: a grid-stride loop over the F * chunks-per-frame chunks.
//   rescale  > 0   one 1024-thread workgroup per frame, three passes over the frame's groups: the means of the reference
//                  group and of m; their squared deviations; the update.  Lane t adds its chunks t, t + 1024, ... serially,
//                  then a 64-lane butterfly, then a binary tree over the 16 wave sums.
// A chunk of the fp32 history is 16 or 32 bytes (4 / 8 elements): one or two 16-byte accesses.  One launch, no workspace, no
// atomics.
#include "common.h"
#include "step_chunk.h"

#include <algorithm>

namespace {

using vtm::aligned16;
using vtm::load_chunk;
using vtm::store_chunk;

constexpr int SS_THREADS = 1024;              // rescale: threads of a frame's workgroup (_lib.SOLVER_STEP_THREADS)
constexpr int SS_WAVES = SS_THREADS / 64;
constexpr int EW_THREADS = 256;               // elementwise: threads per block,
constexpr int64_t EW_GRID_CAP = 4096;         // ... and the most blocks of its grid-stride launch
constexpr int MAX_GROUPS = VTM_SOLVER_MAX_GROUPS;

struct Solve {
    int pred, g_ref, terms;                   // terms: the groups of non-zero weight,
    int g[MAX_GROUPS];                        // ... ascending,
    float w[MAX_GROUPS];                      // ... and their weights
    float rescale, sqrt_alpha, sqrt_beta, c_x, c_x0, c_h1, c_h2, c_noise;
};

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

// One chunk of the update.  Every pointer points at the chunk's first element (all but mo and x may be null); factor is the
// frame's rescale factor.  x_out may be x and h_out may be h1 or h2: the chunk is read before it is written, by this thread.
template <typename T, bool VEC, bool RESCALE>
__device__ __forceinline__ void step_chunk(const Solve &s, float factor, const T *mo, int64_t stride, const T *x, const T *noise,
                                           const float *h1, const float *h2, T *x_out, float *h_out, T *eps_out, T *x0_out,
                                           int n) {
    constexpr int N = 16 / sizeof(T);
    float m[N], xv[N], nz[N], p1[N], p2[N], x0[N], ep[N], xn[N];
    combine<T, VEC>(s, mo, stride, n, m);
    load_chunk<T, VEC>(x, n, xv);
    if (noise) load_chunk<T, VEC>(noise, n, nz);
    if (h1) load_history<N, VEC>(h1, n, p1);
    if (h2) load_history<N, VEC>(h2, n, p2);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        float mk = m[k];
        if constexpr (RESCALE) mk = mk * factor;
        if (s.pred == VTM_PRED_EPSILON) {
            ep[k] = mk;
            x0[k] = (xv[k] - s.sqrt_beta * mk) / s.sqrt_alpha;
        } else if (s.pred == VTM_PRED_V) {
            x0[k] = s.sqrt_alpha * xv[k] - s.sqrt_beta * mk;
            ep[k] = s.sqrt_alpha * mk + s.sqrt_beta * xv[k];
        } else {
            x0[k] = mk;
            ep[k] = (xv[k] - s.sqrt_alpha * mk) / s.sqrt_beta;
        }
        float acc = 0.0f;
        if (s.c_x != 0.0f) acc = acc + s.c_x * xv[k];
        if (s.c_x0 != 0.0f) acc = acc + s.c_x0 * x0[k];
        if (h1) acc = acc + s.c_h1 * p1[k];
        if (h2) acc = acc + s.c_h2 * p2[k];
        if (noise) acc = acc + s.c_noise * nz[k];
        xn[k] = acc;
    }
    if (x_out) store_chunk<T, VEC>(x_out, n, xn);
    if (h_out) store_history<N, VEC>(h_out, n, x0);
    if (eps_out) store_chunk<T, VEC>(eps_out, n, ep);
    if (x0_out) store_chunk<T, VEC>(x0_out, n, x0);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(EW_THREADS) void solver_step_kernel(const T *x, const T *__restrict__ model_out,
                                                                 const T *__restrict__ noise, const float *h1, const float *h2,
                                                                 int64_t F, int64_t E, const int32_t *__restrict__ frame_ids,
                                                                 Solve s, T *x_out, float *h_out, T *__restrict__ eps_out,
                                                                 T *__restrict__ x0_out) {
    constexpr int N = 16 / sizeof(T);
    const int64_t chunks = (E + N - 1) / N, total = F * chunks;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * EW_THREADS) {
        const int64_t f = i / chunks, e = (i - f * chunks) * N;
        const int n = (int)std::min<int64_t>(N, E - e);
        const int64_t row = frame_ids ? (int64_t)frame_ids[f] : f;
        const int64_t local = f * E + e, video = row * E + e;
        step_chunk<T, VEC, false>(s, 1.0f, model_out + local, F * E, x + video, noise ? noise + local : nullptr,
                                  h1 ? h1 + video : nullptr, h2 ? h2 + video : nullptr, x_out ? x_out + video : nullptr,
                                  h_out ? h_out + video : nullptr, eps_out ? eps_out + local : nullptr,
                                  x0_out ? x0_out + local : nullptr, n);
    }
}

// the workgroup's sums of a and b in every thread: 64-lane butterfly, then a binary tree over the wave sums
// (guided_step.hip's block_sum2: the same order)
__device__ __forceinline__ void block_sum2(float &a, float &b, float (*scratch)[SS_WAVES]) {
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
    float wa[SS_WAVES], wb[SS_WAVES];
#pragma unroll
    for (int w = 0; w < SS_WAVES; ++w) {
        wa[w] = scratch[0][w];
        wb[w] = scratch[1][w];
    }
#pragma unroll
    for (int h = SS_WAVES / 2; h > 0; h >>= 1)
#pragma unroll
        for (int w = 0; w < h; ++w) {
            wa[w] += wa[w + h];
            wb[w] += wb[w + h];
        }
    a = wa[0];
    b = wb[0];
}

template <typename T, bool VEC>
__global__ __launch_bounds__(SS_THREADS) void solver_step_rescale_kernel(const T *x, const T *__restrict__ model_out,
                                                                         const T *__restrict__ noise, const float *h1,
                                                                         const float *h2, int64_t F, int64_t E,
                                                                         const int32_t *__restrict__ frame_ids, Solve s,
                                                                         T *x_out, float *h_out, T *__restrict__ eps_out,
                                                                         T *__restrict__ x0_out) {
    constexpr int N = 16 / sizeof(T);
    __shared__ float scratch[2][2][SS_WAVES];     // one pair of rows per pass: no barrier between a read and the next write
    const int64_t f = blockIdx.x, chunks = (E + N - 1) / N, stride = F * E;
    const T *mo = model_out + f * E, *ref = mo + s.g_ref * stride;
    float r[N], m[N];

    float sum_r = 0.0f, sum_m = 0.0f;
    for (int64_t i = threadIdx.x; i < chunks; i += SS_THREADS) {
        const int n = (int)std::min<int64_t>(N, E - i * N);
        load_chunk<T, VEC>(ref + i * N, n, r);
        combine<T, VEC>(s, mo + i * N, stride, n, m);
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < n) {
                sum_r += r[k];
                sum_m += m[k];
            }
    }
    block_sum2(sum_r, sum_m, scratch[0]);
    const float mean_r = sum_r / (float)E, mean_m = sum_m / (float)E;

    float dev_r = 0.0f, dev_m = 0.0f;
    for (int64_t i = threadIdx.x; i < chunks; i += SS_THREADS) {
        const int n = (int)std::min<int64_t>(N, E - i * N);
        load_chunk<T, VEC>(ref + i * N, n, r);
        combine<T, VEC>(s, mo + i * N, stride, n, m);
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < n) {
                const float dr = r[k] - mean_r, dm = m[k] - mean_m;
                dev_r += dr * dr;
                dev_m += dm * dm;
            }
    }
    block_sum2(dev_r, dev_m, scratch[1]);
    // torch.std: unbiased.  std(m) == 0 divides by zero as IEEE says (no special case)
    const float std_r = sqrtf(dev_r / (float)(E - 1)), std_m = sqrtf(dev_m / (float)(E - 1));
    const float factor = s.rescale * (std_r / std_m) + (1.0f - s.rescale);

    const int64_t row = frame_ids ? (int64_t)frame_ids[f] : f;
    for (int64_t i = threadIdx.x; i < chunks; i += SS_THREADS) {
        const int64_t e = i * N, local = f * E + e, video = row * E + e;
        const int n = (int)std::min<int64_t>(N, E - e);
        step_chunk<T, VEC, true>(s, factor, mo + e, stride, x + video, noise ? noise + local : nullptr,
                                 h1 ? h1 + video : nullptr, h2 ? h2 + video : nullptr, x_out ? x_out + video : nullptr,
                                 h_out ? h_out + video : nullptr, eps_out ? eps_out + local : nullptr,
                                 x0_out ? x0_out + local : nullptr, n);
    }
}

}  // namespace

VTM_EXPORT int vtm_solver_step(const void *x, const void *model_out, const void *noise, const float *h1, const float *h2,
                               int dtype, int64_t F, int64_t E, int64_t groups, const float *w, int64_t g_ref,
                               const int32_t *frame_ids, int pred_type, float rescale, float sqrt_alpha, float sqrt_beta,
                               float c_x, float c_x0, float c_h1, float c_h2, float c_noise, void *x_out, float *h_out,
                               void *eps_out, void *x0_out, vtm_stream_t stream) {
    const char *who = "vtm_solver_step";
    VTM_REQUIRE(dtype == VTM_F32 || dtype == VTM_F16 || dtype == VTM_BF16, "%s: unsupported dtype %d", who, dtype);
    VTM_REQUIRE(pred_type == VTM_PRED_EPSILON || pred_type == VTM_PRED_V || pred_type == VTM_PRED_SAMPLE,
                "%s: unknown pred_type %d", who, pred_type);
    VTM_REQUIRE(x && model_out && w, "%s: x, model_out and w are required", who);
    // (F bounds the grid of the per-frame launch: 1024 F threads must stay below 2^32)
    VTM_REQUIRE(F >= 0 && F <= (1 << 20) && E >= 1 && groups >= 1 && groups <= MAX_GROUPS,
                "%s: bad sizes F = %lld, E = %lld, groups = %lld (1 .. %d)", who, (long long)F, (long long)E, (long long)groups,
                MAX_GROUPS);
    VTM_REQUIRE(!(rescale < 0.0f) && rescale == rescale, "%s: rescale = %g is negative or NaN", who, (double)rescale);
    VTM_REQUIRE(!(rescale > 0.0f) || (g_ref >= 0 && g_ref < groups && w[g_ref] != 0.0f && E >= 2),
                "%s: rescale > 0 needs g_ref = %lld inside [0, %lld) with a non-zero weight, and E >= 2", who, (long long)g_ref,
                (long long)groups);
    VTM_REQUIRE(c_noise == 0.0f ? true : noise != nullptr, "%s: c_noise != 0 needs noise", who);
    VTM_REQUIRE(c_h1 == 0.0f ? true : h1 != nullptr, "%s: c_h1 != 0 needs h1", who);
    VTM_REQUIRE(c_h2 == 0.0f ? true : h2 != nullptr, "%s: c_h2 != 0 needs h2", who);
    VTM_REQUIRE(x_out || h_out || eps_out || x0_out, "%s: no output", who);
    if (F == 0) return VTM_OK;

    Solve s{pred_type, rescale > 0.0f ? (int)g_ref : 0, 0, {}, {}, rescale, sqrt_alpha, sqrt_beta, c_x, c_x0, c_h1, c_h2, c_noise};
    for (int g = 0; g < groups; ++g)
        if (w[g] != 0.0f) {                                         // a group of weight 0 is never read
            s.g[s.terms] = g;
            s.w[s.terms++] = w[g];
        }
    // a coefficient of 0: the term is absent, its operand is not read
    const void *noise_used = c_noise != 0.0f ? noise : nullptr;
    const float *h1_used = c_h1 != 0.0f ? h1 : nullptr, *h2_used = c_h2 != 0.0f ? h2 : nullptr;
    hipStream_t st = vtm::as_stream(stream);
    const int rc = vtm::with_dtype(dtype, who, [&](auto t) {
        using T = decltype(t);
        constexpr int N = 16 / sizeof(T);
        const bool vec = E % N == 0 && aligned16(x) && aligned16(model_out) && aligned16(noise_used) && aligned16(h1_used) &&
                         aligned16(h2_used) && aligned16(x_out) && aligned16(h_out) && aligned16(eps_out) && aligned16(x0_out);
        auto launch = [&](auto kernel, dim3 grid, dim3 block) {
            hipLaunchKernelGGL(kernel, grid, block, 0, st, (const T *)x, (const T *)model_out, (const T *)noise_used, h1_used,
                               h2_used, F, E, frame_ids, s, (T *)x_out, h_out, (T *)eps_out, (T *)x0_out);
        };
        if (rescale > 0.0f) {
            const dim3 grid((unsigned)F), block(SS_THREADS);
            if (vec) launch(solver_step_rescale_kernel<T, true>, grid, block);
            else launch(solver_step_rescale_kernel<T, false>, grid, block);
        } else {
            const dim3 grid((unsigned)std::min<int64_t>(vtm::cdiv(F * vtm::cdiv(E, N), EW_THREADS), EW_GRID_CAP)),
                block(EW_THREADS);
            if (vec) launch(solver_step_kernel<T, true>, grid, block);
            else launch(solver_step_kernel<T, false>, grid, block);
        }
        return (int)VTM_OK;
    });
    if (rc != VTM_OK) return rc;
    return vtm::launch_status(who);
}
