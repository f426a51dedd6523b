// vtm_cross_edit_values: the value operand of a Prompt-to-Prompt edited cross-attention call (vidtome_amd/p2p.py).  The edit
//     P_edit[i, n] = a[n] * sum_w P_src[i, w] M[w, n] + b[n] * P_own[i, n]
// is linear in the probabilities, so it moves onto V:  P_edit V = P_src (M diag(a) V) + P_own (diag(b) V).  This kernel
// writes the two operands, channel-major like every V^T of the library, into two key ranges of one buffer:
//     vt_out[b, c, start_src + w] = round( sum_{n < K} (M[w, n] * a[n]) * V[b, n, c] )   fp32, n ascending, fmaf from +0
//     vt_out[b, c, start_own + n] = round( b[n] * V[b, n, c] )                           one fp32 product
// with V[b, n, c] = vt[b, c, v_start + n].  It runs once per edited attn2 call on 77-odd keys: nothing here is tuned.
//   * workgroup = 256 threads = one output key each (K <= 256), for CG channels of one sample; the channels' V rows sit in
//     LDS (every thread reads the same element: a broadcast), M diag(a) comes through LDS in tiles of TN columns, stored
//     column-major so that thread w reads consecutive words;
//   * one launch, no atomics, no workspace: the same operands give the same bits.
#include "common.h"

namespace {

constexpr int CE_NT = 256;        // threads = the key limit
constexpr int CE_CG = 8;          // channels per workgroup
constexpr int CE_TN = 16;         // columns of M per LDS tile

template <typename T> __device__ __forceinline__ T ce_from_f32(float v);
template <> __device__ __forceinline__ __half ce_from_f32<__half>(float v) { return __float2half_rn(v); }
template <> __device__ __forceinline__ vtm_bf16 ce_from_f32<vtm_bf16>(float v) { return __float2bfloat16(v); }

template <typename T>
__global__ __launch_bounds__(CE_NT) void cross_edit_values_kernel(
    const T *__restrict__ vt, int64_t ldvt, int64_t v_start, int64_t C, int K, const float *__restrict__ mapper,
    const float *__restrict__ src_w, const float *__restrict__ own_w, T *__restrict__ vt_out, int64_t ldvt_out,
    int64_t start_src, int64_t start_own, int64_t ngroups) {
    __shared__ float sV[CE_CG][CE_NT];          // V[n, c] of the workgroup's channels
    __shared__ float sM[CE_TN][CE_NT + 1];      // (M[w, n] * a[n]) of the tile, [n - n0][w]
    __shared__ float sA[CE_NT];                 // a[n]

    const int tid = threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x / ngroups;
    const int64_t c0 = ((int64_t)blockIdx.x % ngroups) * CE_CG;

    sA[tid] = tid < K ? src_w[tid] : 0.0f;
#pragma unroll
    for (int c = 0; c < CE_CG; ++c) {
        float v = 0.0f;
        if (tid < K && c0 + c < C) v = vtm::to_f32(vt[(b * C + c0 + c) * ldvt + v_start + tid]);
        sV[c][tid] = v;
    }
    __syncthreads();

    if (tid < K) {   // the own range: one product
        const float bw = own_w[tid];
#pragma unroll
        for (int c = 0; c < CE_CG; ++c) {
            // (the product must exist as an fp32 value: without the barrier the compiler selects v_fma_mixlo_f16, which
            // rounds b * V to fp16 ONCE -- not the fp32 product the contract states, and another result on a tie)
            float p = bw * sV[c][tid];
            asm volatile("" : "+v"(p));
            if (c0 + c < C) vt_out[(b * C + c0 + c) * ldvt_out + start_own + tid] = ce_from_f32<T>(p);
        }
    }

    float acc[CE_CG];
#pragma unroll
    for (int c = 0; c < CE_CG; ++c) acc[c] = 0.0f;
    for (int n0 = 0; n0 < K; n0 += CE_TN) {
        // the tile M[0 .. K) x [n0, n0 + TN): 16 threads read 16 consecutive columns of one row
        const int tn = tid % CE_TN, n = n0 + tn;
        for (int w = tid / CE_TN; w < K; w += CE_NT / CE_TN)
            sM[tn][w] = n < K ? mapper[(int64_t)w * K + n] * sA[n] : 0.0f;
        __syncthreads();
        if (tid < K) {
            const int lim = K - n0 < CE_TN ? K - n0 : CE_TN;
            for (int j = 0; j < lim; ++j) {
                const float m = sM[j][tid];
#pragma unroll
                for (int c = 0; c < CE_CG; ++c) acc[c] = __builtin_fmaf(m, sV[c][n0 + j], acc[c]);
            }
        }
        __syncthreads();   // every thread has read the tile
    }
    if (tid < K) {
#pragma unroll
        for (int c = 0; c < CE_CG; ++c) {
            asm volatile("" : "+v"(acc[c]));   // (likewise: the chain's last fmaf stays an fp32 result)
            if (c0 + c < C) vt_out[(b * C + c0 + c) * ldvt_out + start_src + tid] = ce_from_f32<T>(acc[c]);
        }
    }
}

}  // namespace

VTM_EXPORT int vtm_cross_edit_values(const void *vt, int64_t ldvt, int64_t v_start, int dtype, int64_t B, int64_t C, int64_t K,
                                     const float *mapper, const float *src_w, const float *own_w, void *vt_out,
                                     int64_t ldvt_out, int64_t start_src, int64_t start_own, vtm_stream_t stream) {
    const char *who = "vtm_cross_edit_values";
    VTM_REQUIRE(vt && mapper && src_w && own_w && vt_out, "%s: null pointer", who);
    VTM_REQUIRE(B > 0 && C > 0, "%s: bad sizes", who);
    VTM_REQUIRE(K >= 1 && K <= CE_NT, "%s: K = %lld, 1 .. %d keys are taken", who, (long long)K, CE_NT);
    if (dtype != VTM_F16 && dtype != VTM_BF16) return vtm::fail(VTM_EINVAL, "%s: dtype must be VTM_F16 or VTM_BF16", who);
    VTM_REQUIRE(v_start >= 0 && v_start + K <= ldvt, "%s: keys [%lld, %lld) do not lie inside ldvt = %lld", who,
                (long long)v_start, (long long)(v_start + K), (long long)ldvt);
    VTM_REQUIRE(start_src >= 0 && start_own >= 0 && start_src % 8 == 0 && start_own % 8 == 0,
                "%s: start_src = %lld and start_own = %lld must be multiples of 8", who, (long long)start_src,
                (long long)start_own);
    VTM_REQUIRE(start_src + K <= ldvt_out && start_own + K <= ldvt_out, "%s: an output range does not lie inside ldvt_out = %lld",
                who, (long long)ldvt_out);
    VTM_REQUIRE(start_src + K <= start_own || start_own + K <= start_src, "%s: the two output ranges overlap", who);
    {   // vt_out may not alias vt: every workgroup reads rows of vt that others write
        const char *a0 = static_cast<const char *>(vt), *a1 = a0 + B * C * ldvt * 2;
        const char *o0 = static_cast<const char *>(vt_out), *o1 = o0 + B * C * ldvt_out * 2;
        VTM_REQUIRE(a1 <= o0 || o1 <= a0, "%s: vt_out overlaps vt", who);
    }
    const int64_t ngroups = vtm::cdiv(C, (int64_t)CE_CG);
    VTM_REQUIRE(B * ngroups < (1ll << 31), "%s: grid too large", who);
    hipStream_t s = vtm::as_stream(stream);
    const dim3 grid((unsigned)(B * ngroups)), block(CE_NT);
    if (dtype == VTM_F16)
        hipLaunchKernelGGL(cross_edit_values_kernel<__half>, grid, block, 0, s, (const __half *)vt, ldvt, v_start, C, (int)K,
                           mapper, src_w, own_w, (__half *)vt_out, ldvt_out, start_src, start_own, ngroups);
    else
        hipLaunchKernelGGL(cross_edit_values_kernel<vtm_bf16>, grid, block, 0, s, (const vtm_bf16 *)vt, ldvt, v_start, C, (int)K,
                           mapper, src_w, own_w, (vtm_bf16 *)vt_out, ldvt_out, start_src, start_own, ngroups);
    return vtm::launch_status(who);
}
