// What the LayerNorm kernels (layernorm.hip) and the kernels that fuse a LayerNorm behind another row operation
// (broadcast.hip's vtm_residual_replay_layernorm) share: a lane's 16-byte pieces of a token row as fp32 and the wave /
// lane-group sums of the row statistics.
#pragma once
#include "common.h"

namespace vtm {
namespace ln {

constexpr int MAX_CHUNKS = 4;       // 8-channel chunks per lane: C <= 64 * 8 * 4 = 2048

template <typename T, bool NT = false>
__device__ __forceinline__ void load8(const T *p, float (&f)[8]) {
    if constexpr (sizeof(T) == 4) {
        const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
        f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    } else {
        const uint4 v = vtm::ld16<NT>(p);
        const T *e = reinterpret_cast<const T *>(&v);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = vtm::to_f32(e[j]);
    }
}

template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ __half from_f32<__half>(float v) { return __float2half_rn(v); }
template <> __device__ __forceinline__ vtm_bf16 from_f32<vtm_bf16>(float v) { return __float2bfloat16(v); }

template <typename T, bool NT = false>
__device__ __forceinline__ void store8(T *p, const float (&f)[8]) {
    if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4 *>(p) = make_float4(f[0], f[1], f[2], f[3]);
        *reinterpret_cast<float4 *>(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
    } else {
        uint4 v;
        T *e = reinterpret_cast<T *>(&v);
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = from_f32<T>(f[j]);
        vtm::st16<NT>(p, v);
    }
}

// all-lanes sum of a wave: butterfly over DPP row operations (no LDS round trip like ds_bpermute-based shuffles)
__device__ __forceinline__ float wave_sum(float v) {
    // within rows of 16 lanes: quad_perm swaps (xor 1, xor 2), then row_half_mirror / row_mirror reversals
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));  // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));  // row_mirror
    // across the four rows: every lane of a row now holds the row's sum
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// sum over aligned groups of LPR lanes (8, 16 or 32): the first log2(LPR) steps of wave_sum's butterfly
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));  // row_half_mirror
    if constexpr (LPR >= 16)
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));  // row_mirror
    if constexpr (LPR >= 32) v += __shfl_xor(v, 16, 64);
    return v;
}

}  // namespace ln
}  // namespace vtm
