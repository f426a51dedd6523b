// vtm_lora_fold: the effective weight of a LoRA-adapted projection, W_eff = W + sum_a s_a B_a A_a (Diffusers' PEFT backend
// wraps every projection of a BasicTransformerBlock once `pipe.load_lora_weights(...)` ran -- the reference's `use_lora` /
// `lora:` option, generate.py:93-94, configs/default.yaml:63-69).  The host concatenates the active adapters along k and
// passes up = [s_1 B_1 | s_2 B_2 | ...] (c_out, r) and down = [A_1; A_2; ...] (r, c_in), both fp32 row-major; the folded
// weight then feeds the projection kernels that exist.  It runs once per adapter state, not per step: plain fp32 FMA tiles,
// one 64 x 64 output tile per workgroup, the up / down slices of a k-step staged in LDS, each lane a 4 x 4 patch.
// out[o, i] = round_dtype(w[o, i] + (k-ascending fmaf chain of up[o, k] * down[k, i] from +0)).
//
// vtm_dora_norms / vtm_dora_fold: the same for a layer whose first active adapter is DoRA (PEFT use_dora, weight-decomposed
// LoRA): its forward is diag(m / ||W + s_d B_d A_d||_row) (W + s_d B_d A_d) + the plain adapters after it, so the host passes
// the DoRA adapter as the first k_dora columns of up / rows of down.  The norms take a reduction over all of c_in: one
// workgroup per 64-row band walks the column tiles in order (fixed summation order, the same bits on every call); the fold
// is the tile kernel above with two chains, k < k_dora scaled per row by magnitude / norm, and k >= k_dora added as is.
//
// vtm_loha_delta / vtm_lokr_delta / vtm_delta_fold: the same for LyCORIS layers (PEFT LoHaConfig / LoKrConfig), whose
// forward adds x (s (W1a W1b) * (W2a W2b))^T (LoHa, * elementwise) or x (s kron(W1, W2))^T (LoKr) per active adapter.  The
// two delta kernels write (or add to) an fp32 delta of the projection's size, one adapter per call in PEFT's order; LoHa's
// two low-rank products are the tile chains above, multiplied once; LoKr's is one product per element.  vtm_delta_fold
// adds the summed delta to fp32(W) and rounds once to the model dtype.
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

// acc[p][q] += sum_{kbeg <= k < kend} up[o, k] * down[k, i] for the lane's 4 x 4 patch of the 64 x 64 tile at (o0, i0): the
// k-ascending fmaf chain of lora_fold_kernel (same staging, same order; the padding of a partial k-step is exact zeros, which
// leave the chain unchanged).  Every lane of the workgroup calls it with the same bounds (it holds barriers).
__device__ __forceinline__ void tile_chain(float (&us)[KT][TILE + 4], float (&ds)[KT][TILE], float (&acc)[4][4],
                                           const float *__restrict__ up, const float *__restrict__ down, int64_t o0,
                                           int64_t i0, int64_t c_out, int64_t c_in, int64_t r, int64_t kbeg, int64_t kend) {
    const int t = threadIdx.x, tx = t % 16, ty = t / 16;
    for (int64_t k0 = kbeg; k0 < kend; k0 += KT) {
#pragma unroll
        for (int j = 0; j < TILE * KT / THREADS; ++j) {
            const int e = t + j * THREADS, kk = e % KT, oo = e / KT;
            const int64_t o = o0 + oo, k = k0 + kk;
            us[kk][oo] = (o < c_out && k < kend) ? up[o * r + k] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < TILE * KT / THREADS; ++j) {
            const int e = t + j * THREADS, ii = e % TILE, kk = e / TILE;
            const int64_t i = i0 + ii, k = k0 + kk;
            ds[kk][ii] = (i < c_in && k < kend) ? down[k * c_in + i] : 0.0f;
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
}

// norms[o] = sqrtf(sum_i v[o, i]^2), v = w + (chain over k < k_dora): one workgroup per 64-row band, column tiles in
// ascending order; a lane squares its 4 columns of a tile into its row sums (fmaf, q ascending), and the 16 lanes of a row
// are added in lane order at the end.
template <typename T>
__global__ __launch_bounds__(THREADS) void dora_norm_kernel(const T *__restrict__ w, const float *__restrict__ up,
                                                            const float *__restrict__ down, int64_t c_out, int64_t c_in,
                                                            int64_t r, int64_t k_dora, float *__restrict__ norms) {
    __shared__ __attribute__((aligned(16))) float us[KT][TILE + 4];
    __shared__ __attribute__((aligned(16))) float ds[KT][TILE];
    __shared__ float part[TILE][16 + 1];
    const int t = threadIdx.x, tx = t % 16, ty = t / 16;
    const int64_t o0 = (int64_t)blockIdx.x * TILE;
    float ss[4] = {};
    for (int64_t i0 = 0; i0 < c_in; i0 += TILE) {
        float acc[4][4] = {};
        tile_chain(us, ds, acc, up, down, o0, i0, c_out, c_in, r, 0, k_dora);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int64_t o = o0 + 4 * ty + p;
            if (o >= c_out) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t i = i0 + 4 * tx + q;
                if (i < c_in) {
                    const float v = vtm::to_f32(w[o * c_in + i]) + acc[p][q];
                    ss[p] = fmaf(v, v, ss[p]);
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) part[4 * ty + p][tx] = ss[p];
    __syncthreads();
    if (t < TILE && o0 + t < c_out) {
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < 16; ++j) s += part[t][j];
        norms[o0 + t] = sqrtf(s);
    }
}

// out[o, i] = round_dtype((m[o] / n[o]) * (w + chain_{k < k_dora}) + chain_{k_dora <= k < r}): each step one fp32 rounding.
template <typename T>
__global__ __launch_bounds__(THREADS) void dora_fold_kernel(const T *__restrict__ w, const float *__restrict__ up,
                                                            const float *__restrict__ down, const float *__restrict__ mag,
                                                            const float *__restrict__ norms, int64_t c_out, int64_t c_in,
                                                            int64_t r, int64_t k_dora, T *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float us[KT][TILE + 4];
    __shared__ __attribute__((aligned(16))) float ds[KT][TILE];
    const int t = threadIdx.x, tx = t % 16, ty = t / 16;
    const int64_t o0 = (int64_t)blockIdx.y * TILE, i0 = (int64_t)blockIdx.x * TILE;
    float ad[4][4] = {}, ap[4][4] = {};
    tile_chain(us, ds, ad, up, down, o0, i0, c_out, c_in, r, 0, k_dora);
    tile_chain(us, ds, ap, up, down, o0, i0, c_out, c_in, r, k_dora, r);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int64_t o = o0 + 4 * ty + p;
        if (o >= c_out) continue;
        const float scale = mag[o] / norms[o];          // IEEE: a zero norm gives +-inf or NaN, as PEFT's division does
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = i0 + 4 * tx + q;
            if (i < c_in) out[o * c_in + i] = from_f32<T>(scale * (vtm::to_f32(w[o * c_in + i]) + ad[p][q]) + ap[p][q]);
        }
    }
}

template <typename T>
int launch_norms(const void *w, const float *up, const float *down, int64_t c_out, int64_t c_in, int64_t r, int64_t k_dora,
                 float *norms, hipStream_t s) {
    hipLaunchKernelGGL(dora_norm_kernel<T>, dim3((unsigned)vtm::cdiv(c_out, TILE)), dim3(THREADS), 0, s, (const T *)w, up,
                       down, c_out, c_in, r, k_dora, norms);
    return vtm::launch_status("vtm_dora_norms");
}

template <typename T>
int launch_dora(const void *w, const float *up, const float *down, const float *mag, const float *norms, int64_t c_out,
                int64_t c_in, int64_t r, int64_t k_dora, void *out, hipStream_t s) {
    const dim3 grid((unsigned)vtm::cdiv(c_in, TILE), (unsigned)vtm::cdiv(c_out, TILE)), block(THREADS);
    hipLaunchKernelGGL(dora_fold_kernel<T>, grid, block, 0, s, (const T *)w, up, down, mag, norms, c_out, c_in, r, k_dora,
                       (T *)out);
    return vtm::launch_status("vtm_dora_fold");
}

// delta[o, i] (+)= chain(w1a, w1b)[o, i] * chain(w2a, w2b)[o, i]: the two k-ascending fmaf chains of tile_chain through the
// same staging, one after the other, then one fp32 product (and, accumulating, one fp32 addition to what delta holds).
__global__ __launch_bounds__(THREADS) void loha_delta_kernel(const float *__restrict__ w1a, const float *__restrict__ w1b,
                                                             const float *__restrict__ w2a, const float *__restrict__ w2b,
                                                             int64_t c_out, int64_t c_in, int64_t r, int accumulate,
                                                             float *__restrict__ delta) {
    __shared__ __attribute__((aligned(16))) float us[KT][TILE + 4];
    __shared__ __attribute__((aligned(16))) float ds[KT][TILE];
    const int t = threadIdx.x, tx = t % 16, ty = t / 16;
    const int64_t o0 = (int64_t)blockIdx.y * TILE, i0 = (int64_t)blockIdx.x * TILE;
    float a1[4][4] = {}, a2[4][4] = {};
    tile_chain(us, ds, a1, w1a, w1b, o0, i0, c_out, c_in, r, 0, r);
    tile_chain(us, ds, a2, w2a, w2b, o0, i0, c_out, c_in, r, 0, r);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int64_t o = o0 + 4 * ty + p;
        if (o >= c_out) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = i0 + 4 * tx + q;
            if (i >= c_in) continue;
            const float v = a1[p][q] * a2[p][q];
            delta[o * c_in + i] = accumulate ? delta[o * c_in + i] + v : v;
        }
    }
}

// delta[i1 * a2 + i2, j1 * b2 + j2] (+)= w1[i1, j1] * w2[i2, j2]: one workgroup per 256 columns of one output row.
__global__ __launch_bounds__(THREADS) void lokr_delta_kernel(const float *__restrict__ w1, const float *__restrict__ w2,
                                                             int64_t b1, int64_t a2, int64_t b2, int64_t c_in,
                                                             int accumulate, float *__restrict__ delta) {
    const int64_t o = blockIdx.x, i = (int64_t)blockIdx.y * THREADS + threadIdx.x;
    if (i >= c_in) return;
    const int64_t i1 = o / a2, i2 = o % a2, j1 = i / b2, j2 = i % b2;
    const float v = w1[i1 * b1 + j1] * w2[i2 * b2 + j2];
    delta[o * c_in + i] = accumulate ? delta[o * c_in + i] + v : v;
}

// out[e] = round_dtype(fp32(w[e]) + delta[e])
template <typename T>
__global__ __launch_bounds__(THREADS) void delta_fold_kernel(const T *__restrict__ w, const float *__restrict__ delta,
                                                             int64_t n, T *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (e < n) out[e] = from_f32<T>(vtm::to_f32(w[e]) + delta[e]);
}

template <typename T> int launch_delta_fold(const void *w, const float *delta, int64_t n, void *out, hipStream_t s) {
    hipLaunchKernelGGL(delta_fold_kernel<T>, dim3((unsigned)vtm::cdiv(n, THREADS)), dim3(THREADS), 0, s, (const T *)w, delta, n,
                       (T *)out);
    return vtm::launch_status("vtm_delta_fold");
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

// the checks both DoRA entry points share (sizes as vtm_lora_fold, plus 0 < k_dora <= r)
static int dora_args(const char *what, int64_t c_out, int64_t c_in, int64_t r, int64_t k_dora) {
    VTM_REQUIRE(c_out > 0 && c_in > 0 && r > 0, "%s: bad sizes (c_out %lld, c_in %lld, r %lld)", what, (long long)c_out,
                (long long)c_in, (long long)r);
    VTM_REQUIRE(k_dora > 0 && k_dora <= r, "%s: k_dora %lld not in [1, r = %lld]", what, (long long)k_dora, (long long)r);
    VTM_REQUIRE(vtm::cdiv(c_out, TILE) <= 65535 && vtm::cdiv(c_in, TILE) <= (1ll << 31) - 1, "%s: c_out %lld / c_in %lld too large",
                what, (long long)c_out, (long long)c_in);
    return VTM_OK;
}

VTM_EXPORT int vtm_dora_norms(const void *w, int dtype, const float *up, const float *down, int64_t c_out, int64_t c_in,
                              int64_t r, int64_t k_dora, float *norms, vtm_stream_t stream) {
    VTM_REQUIRE(w && up && down && norms, "vtm_dora_norms: null pointer");
    if (const int rc = dora_args("vtm_dora_norms", c_out, c_in, r, k_dora)) return rc;
    hipStream_t s = vtm::as_stream(stream);
    switch (dtype) {
        case VTM_F32: return launch_norms<float>(w, up, down, c_out, c_in, r, k_dora, norms, s);
        case VTM_F16: return launch_norms<__half>(w, up, down, c_out, c_in, r, k_dora, norms, s);
        case VTM_BF16: return launch_norms<vtm_bf16>(w, up, down, c_out, c_in, r, k_dora, norms, s);
        default: return vtm::fail(VTM_EINVAL, "vtm_dora_norms: unsupported dtype %d", dtype);
    }
}

VTM_EXPORT int vtm_dora_fold(const void *w, int dtype, const float *up, const float *down, const float *magnitude,
                             const float *norms, int64_t c_out, int64_t c_in, int64_t r, int64_t k_dora, void *out,
                             vtm_stream_t stream) {
    VTM_REQUIRE(w && up && down && magnitude && norms && out, "vtm_dora_fold: null pointer");
    if (const int rc = dora_args("vtm_dora_fold", c_out, c_in, r, k_dora)) return rc;
    hipStream_t s = vtm::as_stream(stream);
    switch (dtype) {
        case VTM_F32: return launch_dora<float>(w, up, down, magnitude, norms, c_out, c_in, r, k_dora, out, s);
        case VTM_F16: return launch_dora<__half>(w, up, down, magnitude, norms, c_out, c_in, r, k_dora, out, s);
        case VTM_BF16: return launch_dora<vtm_bf16>(w, up, down, magnitude, norms, c_out, c_in, r, k_dora, out, s);
        default: return vtm::fail(VTM_EINVAL, "vtm_dora_fold: unsupported dtype %d", dtype);
    }
}

VTM_EXPORT int vtm_loha_delta(const float *w1a, const float *w1b, const float *w2a, const float *w2b, int64_t c_out,
                              int64_t c_in, int64_t r, int accumulate, float *delta, vtm_stream_t stream) {
    VTM_REQUIRE(w1a && w1b && w2a && w2b && delta, "vtm_loha_delta: null pointer");
    VTM_REQUIRE(c_out > 0 && c_in > 0 && r > 0, "vtm_loha_delta: bad sizes (c_out %lld, c_in %lld, r %lld)", (long long)c_out,
                (long long)c_in, (long long)r);
    VTM_REQUIRE(vtm::cdiv(c_out, TILE) <= 65535 && vtm::cdiv(c_in, TILE) <= (1ll << 31) - 1,
                "vtm_loha_delta: c_out %lld / c_in %lld too large", (long long)c_out, (long long)c_in);
    VTM_REQUIRE(accumulate == 0 || accumulate == 1, "vtm_loha_delta: accumulate %d is not 0 / 1", accumulate);
    const dim3 grid((unsigned)vtm::cdiv(c_in, TILE), (unsigned)vtm::cdiv(c_out, TILE)), block(THREADS);
    hipLaunchKernelGGL(loha_delta_kernel, grid, block, 0, vtm::as_stream(stream), w1a, w1b, w2a, w2b, c_out, c_in, r,
                       accumulate, delta);
    return vtm::launch_status("vtm_loha_delta");
}

VTM_EXPORT int vtm_lokr_delta(const float *w1, const float *w2, int64_t a1, int64_t b1, int64_t a2, int64_t b2, int64_t c_out,
                              int64_t c_in, int accumulate, float *delta, vtm_stream_t stream) {
    constexpr int64_t LIM = (1ll << 31) - 1;
    VTM_REQUIRE(w1 && w2 && delta, "vtm_lokr_delta: null pointer");
    VTM_REQUIRE(a1 > 0 && b1 > 0 && a2 > 0 && b2 > 0 && c_out > 0 && c_in > 0,
                "vtm_lokr_delta: bad sizes (%lld x %lld kron %lld x %lld for %lld x %lld)", (long long)a1, (long long)b1,
                (long long)a2, (long long)b2, (long long)c_out, (long long)c_in);
    VTM_REQUIRE(a1 <= LIM && b1 <= LIM && a2 <= LIM && b2 <= LIM && a1 * a2 == c_out && b1 * b2 == c_in,
                "vtm_lokr_delta: %lld x %lld kron %lld x %lld is not %lld x %lld", (long long)a1, (long long)b1, (long long)a2,
                (long long)b2, (long long)c_out, (long long)c_in);
    VTM_REQUIRE(c_out <= LIM && vtm::cdiv(c_in, THREADS) <= 65535, "vtm_lokr_delta: c_out %lld / c_in %lld too large",
                (long long)c_out, (long long)c_in);
    VTM_REQUIRE(accumulate == 0 || accumulate == 1, "vtm_lokr_delta: accumulate %d is not 0 / 1", accumulate);
    const dim3 grid((unsigned)c_out, (unsigned)vtm::cdiv(c_in, THREADS)), block(THREADS);
    hipLaunchKernelGGL(lokr_delta_kernel, grid, block, 0, vtm::as_stream(stream), w1, w2, b1, a2, b2, c_in, accumulate, delta);
    return vtm::launch_status("vtm_lokr_delta");
}

VTM_EXPORT int vtm_delta_fold(const void *w, int dtype, const float *delta, int64_t c_out, int64_t c_in, void *out,
                              vtm_stream_t stream) {
    constexpr int64_t LIM = (1ll << 31) - 1;
    VTM_REQUIRE(w && delta && out, "vtm_delta_fold: null pointer");
    VTM_REQUIRE(c_out > 0 && c_in > 0, "vtm_delta_fold: bad sizes (c_out %lld, c_in %lld)", (long long)c_out, (long long)c_in);
    VTM_REQUIRE(c_out <= LIM && c_in <= LIM && vtm::cdiv(c_out * c_in, THREADS) <= LIM,
                "vtm_delta_fold: c_out %lld / c_in %lld too large", (long long)c_out, (long long)c_in);
    hipStream_t s = vtm::as_stream(stream);
    const int64_t n = c_out * c_in;
    switch (dtype) {
        case VTM_F32: return launch_delta_fold<float>(w, delta, n, out, s);
        case VTM_F16: return launch_delta_fold<__half>(w, delta, n, out, s);
        case VTM_BF16: return launch_delta_fold<vtm_bf16>(w, delta, n, out, s);
        default: return vtm::fail(VTM_EINVAL, "vtm_delta_fold: unsupported dtype %d", dtype);
    }
}
