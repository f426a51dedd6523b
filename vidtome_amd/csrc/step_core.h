// The shared core of the caller-side step kernels (guided_step.hip, solver_step.hip; sag.hip, semantic.hip and freeu.hip take
// its chunk accesses, sag.hip its prediction formulas too).
//
// Work is cut into 16-byte CHUNKS of a frame: 4 fp32 / 8 16-bit elements, moved with one 16-byte access (VEC) or element by
// element; which of the two changes no bit of what is computed.  A step kernel is one of two bodies over a POLICY P, a view
// of the launch's operands that says what only that step knows:
//     p.m<VEC>(local, n, m)                       the chunk's combined model output m
//     p.ref<VEC>(local, n, r)                     the chunk of the group whose per-frame std the rescale restores
//     p.update<VEC, RESCALE>(factor, local, video, n, row, e)   one chunk of the update: predict(), the step's own sum, the stores
//     p.s.rescale                                 Diffusers' guidance_rescale
// local = f * E + e is the chunk's offset in a chunk-local (F, E) operand, video = row * E + e in a whole-video one, whose row
// is frame_ids[f] (f without ids).
//   step_elementwise   rescale == 0: a grid-stride loop over the F * chunks-per-frame chunks.
//   step_rescale       rescale  > 0: one STEP_THREADS workgroup per frame, three passes over the frame (after the first they come
//                      from L2): the means of ref and m; their squared deviations; the update.  Lane t adds its chunks t,
//                      t + 1024, ... serially, then a 64-lane butterfly, then a binary tree over the 16 wave sums -- an order
//                      that depends on E alone, so a frame's bits depend neither on the launch's other frames nor on the run.
// One launch (launch_step), no workspace, no atomics.  Everything is fp32 and every stored value is rounded once.
#pragma once
#include "common.h"
#include "philox.h"

#include <algorithm>
#include <initializer_list>

namespace vtm {

constexpr int STEP_THREADS = 1024;            // rescale: threads of a frame's workgroup
constexpr int STEP_WAVES = STEP_THREADS / 64;
constexpr int EW_THREADS = 256;               // elementwise: threads per block,
constexpr int64_t EW_GRID_CAP = 4096;         // ... and the most blocks of its grid-stride launch

template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ __half from_f32<__half>(float v) { return __float2half_rn(v); }
template <> __device__ __forceinline__ vtm_bf16 from_f32<vtm_bf16>(float v) { return __float2bfloat16(v); }

// the n <= N elements of the chunk at p as fp32 (elements past n: 0, never used)
template <typename T, bool VEC>
__device__ __forceinline__ void load_chunk(const T *p, int n, float *v) {
    constexpr int N = 16 / sizeof(T);
    if constexpr (VEC) {
        const uint4 raw = *reinterpret_cast<const uint4 *>(p);
        const T *e = reinterpret_cast<const T *>(&raw);
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = vtm::to_f32(e[k]);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = k < n ? vtm::to_f32(p[k]) : 0.0f;
    }
}

template <typename T, bool VEC>
__device__ __forceinline__ void store_chunk(T *p, int n, const float *v) {
    constexpr int N = 16 / sizeof(T);
    if constexpr (VEC) {
        uint4 raw;
        T *e = reinterpret_cast<T *>(&raw);
#pragma unroll
        for (int k = 0; k < N; ++k) e[k] = from_f32<T>(v[k]);
        *reinterpret_cast<uint4 *>(p) = raw;
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < n) p[k] = from_f32<T>(v[k]);
    }
}

// Where a keyed step's noise comes from (philox.h) instead of a chunk-local tensor.  frame0: the whole-video row of row 0 of
// the launch's whole-video operands (a caller that steps an ascending run of frames offsets those pointers and sends no ids).
struct KeyedNoise {
    NoiseKey key;
    uint32_t frame0;
};

// the chunk at element e of row `row` of keyed noise as fp32, each normal rounded ONCE to T first: the values load_chunk reads
// from a stored noise tensor of the model dtype.  (Elements past the frame's end are never used.)
template <typename T>
__device__ __forceinline__ void normal_chunk(const KeyedNoise &kn, int64_t row, int64_t e, float *v) {
    constexpr int N = 16 / sizeof(T);
#pragma unroll
    for (int q = 0; q < N / 4; ++q) normal_quad(kn.key, (uint32_t)(e >> 2) + q, kn.frame0 + (uint32_t)row, v + 4 * q);
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = vtm::to_f32(from_f32<T>(v[k]));
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the predicted clean sample x0 and the predicted noise eps from the noisy sample xv and the model output m, for the three
// prediction types.  A caller that uses one of the two gets that one's operations alone.
__device__ __forceinline__ void predict(int pred, float sqrt_alpha, float sqrt_beta, float xv, float m, float &x0, float &eps) {
    if (pred == VTM_PRED_EPSILON) {
        eps = m;
        x0 = (xv - sqrt_beta * m) / sqrt_alpha;
    } else if (pred == VTM_PRED_V) {
        x0 = sqrt_alpha * xv - sqrt_beta * m;
        eps = sqrt_alpha * m + sqrt_beta * xv;
    } else {
        x0 = m;
        eps = (xv - sqrt_alpha * m) / sqrt_beta;
    }
}

// the workgroup's sums of a and b in every thread: 64-lane butterfly, then a binary tree over the wave sums
template <int WAVES>
__device__ __forceinline__ void block_sum2(float &a, float &b, float (*scratch)[WAVES]) {
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
    float wa[WAVES], wb[WAVES];
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        wa[w] = scratch[0][w];
        wb[w] = scratch[1][w];
    }
#pragma unroll
    for (int h = WAVES / 2; h > 0; h >>= 1)
#pragma unroll
        for (int w = 0; w < h; ++w) {
            wa[w] += wa[w + h];
            wb[w] += wb[w + h];
        }
    a = wa[0];
    b = wb[0];
}

template <typename T, bool VEC, typename P>
__device__ __forceinline__ void step_elementwise(const P &p, int64_t F, int64_t E, const int32_t *__restrict__ frame_ids) {
    constexpr int N = 16 / sizeof(T);
    const int64_t chunks = (E + N - 1) / N, total = F * chunks;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * EW_THREADS) {
        const int64_t f = i / chunks, e = (i - f * chunks) * N;
        const int n = (int)std::min<int64_t>(N, E - e);
        const int64_t row = frame_ids ? (int64_t)frame_ids[f] : f;
        p.template update<VEC, false>(1.0f, f * E + e, row * E + e, n, row, e);
    }
}

template <typename T, bool VEC, typename P>
__device__ __forceinline__ void step_rescale(const P &p, int64_t E, const int32_t *__restrict__ frame_ids) {
    constexpr int N = 16 / sizeof(T);
    __shared__ float scratch[2][2][STEP_WAVES];   // one pair of rows per pass: no barrier between a read and the next write
    const int64_t f = blockIdx.x, chunks = (E + N - 1) / N;
    float r[N], m[N];

    float sum_r = 0.0f, sum_m = 0.0f;
    for (int64_t i = threadIdx.x; i < chunks; i += STEP_THREADS) {
        const int n = (int)std::min<int64_t>(N, E - i * N);
        p.template ref<VEC>(f * E + i * N, n, r);
        p.template m<VEC>(f * E + i * N, n, m);
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < n) {
                sum_r += r[k];
                sum_m += m[k];
            }
    }
    block_sum2<STEP_WAVES>(sum_r, sum_m, scratch[0]);
    const float mean_r = sum_r / (float)E, mean_m = sum_m / (float)E;

    float dev_r = 0.0f, dev_m = 0.0f;
    for (int64_t i = threadIdx.x; i < chunks; i += STEP_THREADS) {
        const int n = (int)std::min<int64_t>(N, E - i * N);
        p.template ref<VEC>(f * E + i * N, n, r);
        p.template m<VEC>(f * E + i * N, n, m);
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < n) {
                const float dr = r[k] - mean_r, dm = m[k] - mean_m;
                dev_r += dr * dr;
                dev_m += dm * dm;
            }
    }
    block_sum2<STEP_WAVES>(dev_r, dev_m, scratch[1]);
    // torch.std: unbiased.  std(m) == 0 divides by zero as IEEE says (no special case)
    const float std_r = sqrtf(dev_r / (float)(E - 1)), std_m = sqrtf(dev_m / (float)(E - 1));
    const float factor = p.s.rescale * (std_r / std_m) + (1.0f - p.s.rescale);

    const int64_t row = frame_ids ? (int64_t)frame_ids[f] : f;
    for (int64_t i = threadIdx.x; i < chunks; i += STEP_THREADS) {
        const int64_t e = i * N;
        p.template update<VEC, true>(factor, f * E + e, row * E + e, (int)std::min<int64_t>(N, E - e), row, e);
    }
}

// One launch of a step on stream st with the kernels' arguments args.  elementwise / rescaled: the {element, 16-byte}
// instantiations of the step's two kernels; per_frame (rescale > 0) picks the second pair, one STEP_THREADS workgroup per
// frame, otherwise the grid-stride launch is capped at EW_GRID_CAP blocks.  A chunk is moved with one 16-byte access when E
// is a multiple of the chunk and every pointer in use (null: not in use) is 16-byte aligned.
template <typename T, typename K, typename... A>
void launch_step(bool per_frame, K *const (&elementwise)[2], K *const (&rescaled)[2], int64_t F, int64_t E,
                 std::initializer_list<const void *> pointers, hipStream_t st, A... args) {
    constexpr int N = 16 / sizeof(T);
    const bool vec = E % N == 0 && std::all_of(pointers.begin(), pointers.end(), aligned16);
    K *const kernel = (per_frame ? rescaled : elementwise)[vec];
    const dim3 grid((unsigned)(per_frame ? F : std::min<int64_t>(cdiv(F * cdiv(E, N), EW_THREADS), EW_GRID_CAP)));
    hipLaunchKernelGGL(kernel, grid, dim3(per_frame ? STEP_THREADS : EW_THREADS), 0, st, args...);
}

// the two requirements every export that takes a prediction type starts with
inline int check_dtype_pred(const char *who, int dtype, int pred_type) {
    VTM_REQUIRE(dtype == VTM_F32 || dtype == VTM_F16 || dtype == VTM_BF16, "%s: unsupported dtype %d", who, dtype);
    VTM_REQUIRE(pred_type == VTM_PRED_EPSILON || pred_type == VTM_PRED_V || pred_type == VTM_PRED_SAMPLE,
                "%s: unknown pred_type %d", who, pred_type);
    return VTM_OK;
}

// what a keyed export requires beyond its tensor form: the counter's words are 32 bits (quad e >> 2, frame)
inline int check_keyed(const char *who, int64_t frame0, int64_t E) {
    VTM_REQUIRE(frame0 >= 0 && frame0 <= INT32_MAX, "%s: frame0 = %lld outside [0, 2^31)", who, (long long)frame0);
    VTM_REQUIRE(E <= (int64_t(1) << 34), "%s: E = %lld: a frame's quad index must fit 32 bits", who, (long long)E);
    return VTM_OK;
}

}  // namespace vtm
