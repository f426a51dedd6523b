// vtm_linear_f32: y = gather(pool, rows) @ W^T (+ bias) in fp32 on the f32 MFMA -- every projection of an fp32 model's
// patched block (attn1's q | k, V^T and output projection fed by the composed merge map, patch.py:157-162 /
// pnp_utils.py:47-95; attn2's projections, patch.py:171-185; the GEGLU feed-forward, patch.py:187-199).
//
// The A operand has vtm_linear_rows' contract (linear.hip): pool = x0 | x1, row i of sample b = pool[rows[b, rows2[b, i]]]
// (either map may be NULL), so the merged tensor is never written.  Epilogues:
//   NONE   out = x W^T + b
//   RESID  out = (x W^T + b) + resid           (torch's order: the Linear's result, then the residual add)
//   GEGLU  W holds 2D rows [value; gate]: out (n, D) = value * gelu_erf(gate); the 2D-wide product is never written.
// fp32 operands, products and accumulation: v_mfma_f32_32x32x2_f32 computes c + a0 b0 + a1 b1 as two fmaf steps, so
// every output is ONE fmaf chain over k in ascending order from +0 (the exact matcher's convention, match.hip), then the
// bias, then the epilogue; a VTM_F16 output is that fp32 value rounded once at the store.
//
// Operand layout.  Both operands are k-contiguous rows (tokens, and nn.Linear's (out, in) weight rows).  A workgroup
// stages a 32-wide k-slice of its token rows and of its weight rows through LDS in the k-PANEL layout of
// vtm_normalize_gather ([g = k/8][kh = k%2][row][e = (k%8)/2], include/vidtome_hip.h): the lane that fetched 8
// consecutive channels of a row from global memory (two 16-byte loads) writes them as the two 16-byte panel entries
// {k0, k2, k4, k6} and {k1, k3, k5, k7}; a compute lane (row, kh) then reads one 16-byte entry per operand and it feeds
// four consecutive 32x32x2 k-steps in ascending k order.  A lane computes its row pointers once (the gather costs
// nothing in the loop).
//
// Tile.  gfx950 has no xf32: this MFMA issues one instruction per 64 cycles per SIMD with a 64-cycle dependent latency,
// so 4 independent 32 x 32 accumulators per wave (a 64 x 64 wave tile) keep the matrix pipe busy and 64 accumulator
// VGPRs leave room for two workgroups per CU.  The workgroup tile is 4 waves: 128 tokens x 128 weight rows, or 256 x 64
// when N is not a multiple of 128 (N = 320: a 128-wide tile would compute 384 columns).  What bounds it: the
// double-buffered LDS ring is 64 KB (80 KB for 256 x 64; two workgroups per CU fit gfx950's 160 KB), and the k-slice is
// one 32-channel step per barrier -- 64 MFMAs (4096 cycles) per wave between barriers, against ~1 us of L2 latency per
// refill, which the other workgroup on the SIMD covers.  Operand intensity is 64 flop per byte fetched from L2.
// The GEGLU tile orders its 128 weight rows as [value 0..31 | gate 0..31 | value 32..63 | gate 32..63]: a wave's two
// weight fragments are the value and gate rows of the same 32 output channels, in the same accumulator positions.
//
// No workspace, no scratch, no atomics; one launch on the caller's stream.
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NT = 256, TK = 32, NG = TK / 8;   // threads, k per LDS slice, 8-channel groups per slice

__device__ __forceinline__ float gelu_erf(float g) { return 0.5f * g * (1.0f + erff(g * 0.70710678118654752440f)); }

template <typename TO> struct Out;
template <> struct Out<float> {
    __device__ static void store4(float *p, f32x4 v, bool vec) {
        if (vec) *reinterpret_cast<f32x4 *>(p) = v;
        else for (int e = 0; e < 4; ++e) p[e] = v[e];
    }
    __device__ static void store1(float *p, float v) { *p = v; }
};
// The fp16 store rounds the finished fp32 value: the empty asm pins it in a register first, or the compiler folds the
// epilogue's last multiply into the conversion (v_fma_mixlo_f16: one rounding of the exact product, not of the fp32 value).
__device__ __forceinline__ __half round_f16(float v) {
    asm volatile("" : "+v"(v));
    return __float2half_rn(v);
}
template <> struct Out<__half> {
    __device__ static void store4(__half *p, f32x4 v, bool vec) {
        __half h[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = round_f16(v[e]);
        if (vec) *reinterpret_cast<uint2 *>(p) = *reinterpret_cast<const uint2 *>(h);
        else for (int e = 0; e < 4; ++e) p[e] = h[e];
    }
    __device__ static void store1(__half *p, float v) { *p = round_f16(v); }
};

// TMW: waves along the token axis (2: 128 x 128 tile, 4: 256 x 64).  TRANS = false: out[b][token][channel];
// TRANS = true: out[b][channel][token].  Nout = output channels (N, or D = N / 2 for GEGLU).  resid: same layout as out.
template <int TMW, bool TRANS, int EPI, typename TO>
__global__ __launch_bounds__(NT, 2) void linear_f32_kernel(
    const float *__restrict__ x0, int64_t P0, const float *__restrict__ x1, int64_t P1, int64_t K,
    const int32_t *__restrict__ rows, int64_t rows_ld, const int32_t *__restrict__ rows2, int64_t n,
    const float *__restrict__ W, const float *__restrict__ bias, int64_t Nout, const float *__restrict__ resid,
    TO *__restrict__ out, int64_t ldo, int64_t obs) {
    constexpr int TNW = 4 / TMW, TM = 64 * TMW, TN = 64 * TNW;   // token rows / weight rows of the workgroup tile
    constexpr int PA = TM / 64, PW = TN / 64;                      // (row, group) pieces per thread
    __shared__ __attribute__((aligned(16))) f32x4 sA[2][NG][2][TM];
    __shared__ __attribute__((aligned(16))) f32x4 sW[2][NG][2][TN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int wm = wave % TMW, wn = wave / TMW;
    const int64_t m0 = (int64_t)blockIdx.x * TM, b = blockIdx.z;
    // GEGLU: a workgroup covers TN / 2 output channels (value and gate rows); otherwise TN weight rows = channels
    const int64_t c0 = (int64_t)blockIdx.y * (EPI == VTM_LINEAR_GEGLU ? TN / 2 : TN);

    // staging: piece p = tid + 256 i covers row p / 4, channels 8 (p % 4) .. + 7 of the slice
    const int g_ld = tid & 3;
    const float *aptr[PA];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        int64_t t = m0 + (tid >> 2) + 64 * i;
        if (t >= n) t = n - 1;                            // surplus rows recompute the last one; never stored
        int64_t p = rows2 ? rows2[b * n + t] : t;         // live-query rows: position in the merged sequence ...
        if (rows) p = rows[b * rows_ld + p];              // ... -> pool row id
        aptr[i] = (p < P0 ? x0 + (b * P0 + p) * K : x1 + (b * P1 + (p - P0)) * K) + 8 * g_ld;
    }
    const float *wptr[PW];
#pragma unroll
    for (int i = 0; i < PW; ++i) {
        const int r = (tid >> 2) + 64 * i;
        int64_t row;
        if constexpr (EPI == VTM_LINEAR_GEGLU) {
            int64_t c = c0 + 32 * (r >> 6) + (r & 31);
            if (c >= Nout) c = Nout - 1;
            row = c + ((r >> 5) & 1) * Nout;              // value row c, or gate row D + c
        } else {
            row = c0 + r;
            if (row >= Nout) row = Nout - 1;
        }
        wptr[i] = W + row * K + 8 * g_ld;
    }

    f32x4 ra[PA][2], rw[PW][2];
    auto fetch = [&](int64_t k0) {
        const bool ok = k0 + 8 * g_ld < K;                // K % 8 == 0: a group is wholly inside or outside
#pragma unroll
        for (int i = 0; i < PA; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h)
                ra[i][h] = ok ? *reinterpret_cast<const f32x4 *>(aptr[i] + k0 + 4 * h) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < PW; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h)
                rw[i][h] = ok ? *reinterpret_cast<const f32x4 *>(wptr[i] + k0 + 4 * h) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    auto stage = [&](int buf) {                           // 8 channels -> panels kh = 0 {k0,k2,k4,k6}, kh = 1 {k1,k3,k5,k7}
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const f32x4 u = ra[i][0], v = ra[i][1];
            sA[buf][g_ld][0][(tid >> 2) + 64 * i] = f32x4{u[0], u[2], v[0], v[2]};
            sA[buf][g_ld][1][(tid >> 2) + 64 * i] = f32x4{u[1], u[3], v[1], v[3]};
        }
#pragma unroll
        for (int i = 0; i < PW; ++i) {
            const f32x4 u = rw[i][0], v = rw[i][1];
            sW[buf][g_ld][0][(tid >> 2) + 64 * i] = f32x4{u[0], u[2], v[0], v[2]};
            sW[buf][g_ld][1][(tid >> 2) + 64 * i] = f32x4{u[1], u[3], v[1], v[3]};
        }
    };

    f32x16 acc[2][2];                                     // [token fragment i][weight fragment j]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int64_t ntiles = (K + TK - 1) / TK;
    fetch(0);
    stage(0);
    __syncthreads();
    for (int64_t t = 0; t < ntiles; ++t) {
        const int buf = (int)(t & 1);
        // the next slice's loads go out first (the last slice re-fetches itself: a fixed issue sequence keeps the
        // compiler's waits counted) and land while this slice's 64 MFMAs run
        fetch((t + 1 < ntiles ? t + 1 : t) * TK);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            f32x4 fa[2], fw[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = sA[buf][g][hi][64 * wm + 32 * i + l31];
#pragma unroll
            for (int j = 0; j < 2; ++j) fw[j] = sW[buf][g][hi][64 * wn + 32 * j + l31];
#pragma unroll
            for (int e = 0; e < 4; ++e)                   // k = 8 g + 2 e + kh: ascending
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        // MFMA result rows = first operand's rows
                        if constexpr (TRANS) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fw[j][e], acc[i][j], 0, 0, 0);
                        else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fw[j][e], fa[i][e], acc[i][j], 0, 0, 0);
                    }
        }
        stage(buf ^ 1);                                   // (the other buffer's readers passed the last barrier)
        __syncthreads();
    }

    // epilogue.  Accumulator register r = result row (r & 3) + 8 (r >> 2) + 4 hi, column l31: a lane owns 4 consecutive
    // result rows -- 4 consecutive channels of one token (token-major) or 4 consecutive tokens of one channel (channel-major),
    // one 16-byte (fp32) or 8-byte (fp16) store either way.
    TO *ob = out + b * obs;
    const float *rb = resid ? resid + b * obs : nullptr;
    const bool aligned = (ldo & 3) == 0 && (obs & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & (4 * sizeof(TO) - 1)) == 0 &&
                         (!resid || (reinterpret_cast<uintptr_t>(resid) & 15) == 0);
    constexpr int NJ = EPI == VTM_LINEAR_GEGLU ? 1 : 2;       // GEGLU: fragment 0 = value, 1 = gate
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int rr = 8 * q + 4 * hi;            // first of the 4 consecutive result rows of this group
                int64_t tok, ch;                          // first token / channel of the lane's 4 values
                if constexpr (TRANS) {
                    tok = m0 + 64 * wm + 32 * i + rr;
                    ch = EPI == VTM_LINEAR_GEGLU ? c0 + 32 * wn + l31 : c0 + 64 * wn + 32 * j + l31;
                } else {
                    tok = m0 + 64 * wm + 32 * i + l31;
                    ch = EPI == VTM_LINEAR_GEGLU ? c0 + 32 * wn + rr : c0 + 64 * wn + 32 * j + rr;
                }
                if (tok >= n || ch >= Nout) continue;
                // element offset of value 0 (the 4 values are consecutive) and how many of them lie inside the output
                const int64_t idx = TRANS ? ch * ldo + tok : tok * ldo + ch;
                const int64_t left = TRANS ? n - tok : Nout - ch;
                const int cnt = left < 4 ? (int)left : 4;
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int64_t che = TRANS ? ch : ch + e;  // channel of value e
                    const bool in = TRANS || che < Nout;
                    float y = acc[i][j][4 * q + e] + ((bias && in) ? bias[che] : 0.0f);
                    if constexpr (EPI == VTM_LINEAR_GEGLU) {
                        const float gt = acc[i][1][4 * q + e] + ((bias && in) ? bias[Nout + che] : 0.0f);
                        y = y * gelu_erf(gt);
                    }
                    v[e] = y;
                }
                const bool vec = cnt == 4 && aligned;
                if constexpr (EPI == VTM_LINEAR_RESID) {
                    if (vec) {
                        v += *reinterpret_cast<const f32x4 *>(rb + idx);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (e < cnt) v[e] += rb[idx + e];
                    }
                }
                if (vec) {
                    Out<TO>::store4(ob + idx, v, true);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (e < cnt) Out<TO>::store1(ob + idx + e, v[e]);
                }
            }
}

template <int TMW, bool TRANS, typename TO>
void launch_epi(int epi, dim3 grid, hipStream_t s, const float *x0, int64_t P0, const float *x1, int64_t P1, int64_t K,
                const int32_t *rows, int64_t rows_ld, const int32_t *rows2, int64_t n, const float *W, const float *bias,
                int64_t Nout, const float *resid, void *out, int64_t ldo, int64_t obs) {
#define VTM_LF32(E)                                                                                                    \
    hipLaunchKernelGGL((linear_f32_kernel<TMW, TRANS, E, TO>), grid, dim3(NT), 0, s, x0, P0, x1, P1, K, rows, rows_ld, \
                       rows2, n, W, bias, Nout, resid, (TO *)out, ldo, obs)
    if (epi == VTM_LINEAR_NONE) VTM_LF32(VTM_LINEAR_NONE);
    else if (epi == VTM_LINEAR_RESID) VTM_LF32(VTM_LINEAR_RESID);
    else VTM_LF32(VTM_LINEAR_GEGLU);
#undef VTM_LF32
}

template <int TMW, typename TO>
void launch_tr(int transposed, int epi, dim3 grid, hipStream_t s, const float *x0, int64_t P0, const float *x1, int64_t P1,
               int64_t K, const int32_t *rows, int64_t rows_ld, const int32_t *rows2, int64_t n, const float *W,
               const float *bias, int64_t Nout, const float *resid, void *out, int64_t ldo, int64_t obs) {
    if (transposed) launch_epi<TMW, true, TO>(epi, grid, s, x0, P0, x1, P1, K, rows, rows_ld, rows2, n, W, bias, Nout, resid, out, ldo, obs);
    else launch_epi<TMW, false, TO>(epi, grid, s, x0, P0, x1, P1, K, rows, rows_ld, rows2, n, W, bias, Nout, resid, out, ldo, obs);
}

}  // namespace

VTM_EXPORT int vtm_linear_f32(const float *x0, int64_t P0, const float *x1, int64_t P1, int64_t B, int64_t K,
                              const int32_t *rows, int64_t rows_ld, const int32_t *rows2, int64_t n, const float *W,
                              const float *bias, int64_t N, int epilogue, const float *resid, void *out, int out_dtype,
                              int64_t ldo, int64_t out_batch_stride, int transposed, vtm_stream_t stream) {
    VTM_REQUIRE(x0 && W && out, "vtm_linear_f32: null pointer");
    VTM_REQUIRE(P1 == 0 || x1, "vtm_linear_f32: x1 is null but P1 > 0");
    VTM_REQUIRE(B > 0 && B < 65536 && K > 0 && N > 0 && n >= 0 && P0 >= 0 && P1 >= 0, "vtm_linear_f32: bad sizes");
    VTM_REQUIRE(K % 8 == 0, "vtm_linear_f32: K=%lld must be a multiple of 8", (long long)K);
    VTM_REQUIRE(N % 8 == 0, "vtm_linear_f32: N=%lld must be a multiple of 8", (long long)N);
    VTM_REQUIRE(epilogue == VTM_LINEAR_NONE || epilogue == VTM_LINEAR_RESID || epilogue == VTM_LINEAR_GEGLU,
                "vtm_linear_f32: unknown epilogue %d", epilogue);
    VTM_REQUIRE(epilogue != VTM_LINEAR_RESID || resid, "vtm_linear_f32: RESID needs resid");
    VTM_REQUIRE(epilogue != VTM_LINEAR_GEGLU || N % 16 == 0, "vtm_linear_f32: GEGLU needs N = 2 D with D % 8 == 0");
    VTM_REQUIRE(out_dtype == VTM_F32 || out_dtype == VTM_F16, "vtm_linear_f32: out_dtype must be VTM_F32 or VTM_F16");
    VTM_REQUIRE(((reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(x1) | reinterpret_cast<uintptr_t>(W)) & 15) == 0,
                "vtm_linear_f32: x0, x1 and W must be 16-byte aligned");
    VTM_REQUIRE(rows || rows2 || n <= P0 + P1, "vtm_linear_f32: identity rows must lie inside the pool");
    VTM_REQUIRE(!rows || rows_ld > 0, "vtm_linear_f32: rows_ld");
    const int64_t Nout = epilogue == VTM_LINEAR_GEGLU ? N / 2 : N;
    VTM_REQUIRE(ldo >= (transposed ? n : Nout), "vtm_linear_f32: ldo too small");
    if (n == 0) return VTM_OK;
    const int tmw = (epilogue == VTM_LINEAR_GEGLU || N % 128 == 0) ? 2 : 4;
    const int64_t tn = tmw == 2 ? 128 : 64;
    const int64_t ytiles = epilogue == VTM_LINEAR_GEGLU ? vtm::cdiv(Nout, tn / 2) : vtm::cdiv(N, tn);
    const int64_t xtiles = vtm::cdiv(n, 64 * tmw);
    VTM_REQUIRE(ytiles < 65536 && xtiles < (1ll << 31), "vtm_linear_f32: N or n too large");
    const dim3 grid((unsigned)xtiles, (unsigned)ytiles, (unsigned)B);
    hipStream_t s = vtm::as_stream(stream);
#define VTM_LF32_ARGS transposed, epilogue, grid, s, x0, P0, x1, P1, K, rows, rows_ld, rows2, n, W, bias, Nout, resid, out, ldo, \
                      out_batch_stride
    if (out_dtype == VTM_F32) {
        if (tmw == 2) launch_tr<2, float>(VTM_LF32_ARGS); else launch_tr<4, float>(VTM_LF32_ARGS);
    } else {
        if (tmw == 2) launch_tr<2, __half>(VTM_LF32_ARGS); else launch_tr<4, __half>(VTM_LF32_ARGS);
    }
#undef VTM_LF32_ARGS
    return vtm::launch_status("vtm_linear_f32");
}
