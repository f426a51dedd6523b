// The 16-byte chunk accesses of the step kernels (guided_step.hip, solver_step.hip): a chunk is 4 fp32 / 8 16-bit elements of
// a frame, moved with one 16-byte access (VEC) or element by element; which of the two changes no bit of what is computed.
#pragma once
#include "common.h"

namespace vtm {

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

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace vtm
