// vtm_lora_fold: the effective weight of a LoRA-adapted projection, W_eff = W + sum_a s_a B_a A_a (Diffusers' PEFT backend
// wraps every projection of a BasicTransformerBlock once `pipe.load_lora_weights(...)` ran -- the reference's `use_lora` /
// `lora:` option, generate.py:93-94, configs/default.yaml:63-69).  The host concatenates the active adapters along k and
// passes up = [s_1 B_1 | s_2 B_2 | ...] (c_out, r) and down = [A_1; A_2; ...] (r, c_in), both fp32 row-major; the folded
// weight then feeds the projection kernels that exist.  It runs once per adapter state, not per step: plain fp32 FMA tiles,
// one 64 x 64 output tile per workgroup, the up / down slices of a k-step staged in LDS, each lane a 4 x 4 patch.
// out[o, i] = round_dtype(w[o, i] + (k-ascending fmaf chain of up[o, k] * down[k, i] from +0)).
#include "common.h"

namespace {

constexpr int TILE = 64;        // output tile edge
constexpr int KT = 32;          // k-step staged in LDS
constexpr int THREADS = 256;    // 16 x 16 lanes, 4 x 4 outputs each

template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ __half from_f32<__half>(float v) { return __float2half_rn(v); }
template <> __device__ __forceinline__ vtm_bf16 from_f32<vtm_bf16>(float v) { return __float2bfloat16(v); }

template <typename T>
__global__ __launch_bounds__(THREADS) void lora_fold_kernel(const T *__restrict__ w, const float *__restrict__ up,
                                                            const float *__restrict__ down, int64_t c_out, int64_t c_in,
                                                            int64_t r, T *__restrict__ out) {
    // us[k][o]: the up slice transposed (a lane reads its 4 rows as one 16-byte word; rows padded by 4 floats so that the
    // k-major stores spread over 8 banks instead of one); ds[k][i]: the down slice
    __shared__ __attribute__((aligned(16))) float us[KT][TILE + 4];
    __shared__ __attribute__((aligned(16))) float ds[KT][TILE];
    const int t = threadIdx.x, tx = t % 16, ty = t / 16;
    const int64_t o0 = (int64_t)blockIdx.y * TILE, i0 = (int64_t)blockIdx.x * TILE;
    float acc[4][4] = {};
    for (int64_t k0 = 0; k0 < r; k0 += KT) {
        // up tile: 64 rows x 32 k, read along k (coalesced), 8 per lane
#pragma unroll
        for (int j = 0; j < TILE * KT / THREADS; ++j) {
            const int e = t + j * THREADS, kk = e % KT, oo = e / KT;
            const int64_t o = o0 + oo, k = k0 + kk;
            us[kk][oo] = (o < c_out && k < r) ? up[o * r + k] : 0.0f;
        }
        // down tile: 32 k x 64 columns, read along the columns
#pragma unroll
        for (int j = 0; j < TILE * KT / THREADS; ++j) {
            const int e = t + j * THREADS, ii = e % TILE, kk = e / TILE;
            const int64_t i = i0 + ii, k = k0 + kk;
            ds[kk][ii] = (i < c_in && k < r) ? down[k * c_in + i] : 0.0f;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < KT; ++kk) {
            const float4 a = *reinterpret_cast<const float4 *>(&us[kk][4 * ty]);
            const float4 b = *reinterpret_cast<const float4 *>(&ds[kk][4 * tx]);
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = fmaf(av[p], bv[q], acc[p][q]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int64_t o = o0 + 4 * ty + p;
        if (o >= c_out) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = i0 + 4 * tx + q;
            if (i < c_in) out[o * c_in + i] = from_f32<T>(vtm::to_f32(w[o * c_in + i]) + acc[p][q]);
        }
    }
}

template <typename T>
int launch(const void *w, const float *up, const float *down, int64_t c_out, int64_t c_in, int64_t r, void *out,
           hipStream_t s) {
    const dim3 grid((unsigned)vtm::cdiv(c_in, TILE), (unsigned)vtm::cdiv(c_out, TILE)), block(THREADS);
    hipLaunchKernelGGL(lora_fold_kernel<T>, grid, block, 0, s, (const T *)w, up, down, c_out, c_in, r, (T *)out);
    return vtm::launch_status("vtm_lora_fold");
}

}  // namespace

VTM_EXPORT int vtm_lora_fold(const void *w, int dtype, const float *up, const float *down, int64_t c_out, int64_t c_in,
                             int64_t r, void *out, vtm_stream_t stream) {
    VTM_REQUIRE(w && up && down && out, "vtm_lora_fold: null pointer");
    VTM_REQUIRE(c_out > 0 && c_in > 0 && r > 0, "vtm_lora_fold: bad sizes (c_out %lld, c_in %lld, r %lld)", (long long)c_out,
                (long long)c_in, (long long)r);
    VTM_REQUIRE(vtm::cdiv(c_out, TILE) <= 65535 && vtm::cdiv(c_in, TILE) <= (1ll << 31) - 1,
                "vtm_lora_fold: c_out %lld / c_in %lld too large", (long long)c_out, (long long)c_in);
    hipStream_t s = vtm::as_stream(stream);
    switch (dtype) {
        case VTM_F32: return launch<float>(w, up, down, c_out, c_in, r, out, s);
        case VTM_F16: return launch<__half>(w, up, down, c_out, c_in, r, out, s);
        case VTM_BF16: return launch<vtm_bf16>(w, up, down, c_out, c_in, r, out, s);
        default: return vtm::fail(VTM_EINVAL, "vtm_lora_fold: unsupported dtype %d", dtype);
    }
}
