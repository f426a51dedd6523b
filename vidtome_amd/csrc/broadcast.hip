// Pyramid attention broadcast (broadcast.py): a patched block's attention segments are computed every k-th step of a window of
// timesteps and REPLAYED in between.  What is kept of a segment is its contribution to the residual stream, per frame:
//   vtm_residual_record            cache[g, id(f)] = T(f32(h_out[g, f]) - f32(h_in[g, f]))
//   vtm_residual_replay            out[g, f] = T(f32(h[g, f]) + f32(cache1[g, id(f)])), then the same with cache2 on the rounded sum
//   vtm_residual_replay_layernorm  the replay to token rows AND the LayerNorm of those rows as k-panels, in one launch: the
//                                  block of a step that replays both attentions is this launch and the feed-forward's two GEMMs
// The batch is group-major, sample b = g * Fg + f; a cache holds the whole video, (G, num_frames, E); id(f) = frame_ids[f] (f
// without ids): distinct, in range, NOT checked here.  Everything is fp32 arithmetic on exactly representable inputs, every
// stored value rounded once; no workspace, no atomics: a frame's bits depend on that frame's operands alone.
//
// The first two are elementwise over step_core.h's 16-byte chunks (a grid-stride launch, capped).  The third keeps the row in
// registers like layernorm.hip's kernels and restates their row arithmetic on layernorm_row.h's pieces -- BOTH families, with
// launch_layernorm's choice between them: the two orders of summation differ in the last bits, and the promise is
// vtm_layernorm_panels' bits on the replayed rows.
#include "common.h"
#include "layernorm_row.h"
#include "step_core.h"

namespace {

// the cache row of sample b of a group-major batch
__device__ __forceinline__ int64_t cache_row(int64_t b, int64_t Fg, int64_t num_frames, const int32_t *__restrict__ frame_ids) {
    const int64_t g = b / Fg, f = b - g * Fg;
    return g * num_frames + (frame_ids ? (int64_t)frame_ids[f] : f);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(vtm::EW_THREADS) void residual_record_kernel(const T *__restrict__ h_in, const T *__restrict__ h_out,
                                                                         T *__restrict__ cache,
                                                                         const int32_t *__restrict__ frame_ids, int64_t B,
                                                                         int64_t Fg, int64_t num_frames, int64_t E) {
    constexpr int N = 16 / sizeof(T);
    const int64_t chunks = (E + N - 1) / N, total = B * chunks;
    for (int64_t i = (int64_t)blockIdx.x * vtm::EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * vtm::EW_THREADS) {
        const int64_t b = i / chunks, e = (i - b * chunks) * N;
        const int n = (int)std::min<int64_t>(N, E - e);
        float a[N], c[N];
        vtm::load_chunk<T, VEC>(h_out + b * E + e, n, a);
        vtm::load_chunk<T, VEC>(h_in + b * E + e, n, c);
#pragma unroll
        for (int k = 0; k < N; ++k) a[k] -= c[k];
        vtm::store_chunk<T, VEC>(cache + cache_row(b, Fg, num_frames, frame_ids) * E + e, n, a);
    }
}

// (h and out may be the same buffer: a thread reads its chunk before it writes it)
template <typename T, bool VEC>
__global__ __launch_bounds__(vtm::EW_THREADS) void residual_replay_kernel(const T *h, const T *__restrict__ cache1,
                                                                         const T *__restrict__ cache2,
                                                                         const int32_t *__restrict__ frame_ids, int64_t B,
                                                                         int64_t Fg, int64_t num_frames, int64_t E, T *out) {
    constexpr int N = 16 / sizeof(T);
    const int64_t chunks = (E + N - 1) / N, total = B * chunks;
    for (int64_t i = (int64_t)blockIdx.x * vtm::EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * vtm::EW_THREADS) {
        const int64_t b = i / chunks, e = (i - b * chunks) * N;
        const int n = (int)std::min<int64_t>(N, E - e);
        const int64_t at = cache_row(b, Fg, num_frames, frame_ids) * E + e;
        float a[N], d[N];
        vtm::load_chunk<T, VEC>(h + b * E + e, n, a);
        vtm::load_chunk<T, VEC>(cache1 + at, n, d);
#pragma unroll
        for (int k = 0; k < N; ++k) a[k] += d[k];
        if (cache2 != nullptr) {
            vtm::load_chunk<T, VEC>(cache2 + at, n, d);
#pragma unroll
            for (int k = 0; k < N; ++k) a[k] = vtm::to_f32(vtm::from_f32<T>(a[k])) + d[k];      // the intermediate rounding
        }
        vtm::store_chunk<T, VEC>(out + b * E + e, n, a);
    }
}

constexpr int LN_WAVES = 4;         // waves per block of the fused kernels

// the 8 channels at p of the replayed row: h + d1 rounded to T, + d2 rounded to T, as fp32
template <typename T>
__device__ __forceinline__ void replay8(const T *h, const T *__restrict__ c1, const T *__restrict__ c2, float (&v)[8]) {
    float d[8];
    vtm::ln::load8(h, v);
    vtm::ln::load8(c1, d);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = vtm::to_f32(vtm::ln::from_f32<T>(v[j] + d[j]));
    if (c2 != nullptr) {
        vtm::ln::load8(c2, d);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = vtm::to_f32(vtm::ln::from_f32<T>(v[j] + d[j]));
    }
}

// y = (x - mean) * rstd * gamma + beta of 8 channels: the epilogue of layernorm.hip's kernels
__device__ __forceinline__ void affine8(const float (&v)[8], float mean, float rstd, bool has_g, bool has_b, const float (&g)[8],
                                        const float (&b)[8], float (&y)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float n = (v[j] - mean) * rstd;
        y[j] = has_g ? (has_b ? __builtin_fmaf(n, g[j], b[j]) : n * g[j]) : (has_b ? n + b[j] : n);
    }
}

struct Replay {
    const int32_t *frame_ids;
    int64_t Fg, num_frames, N;      // N: token rows of a frame
};
// the cache's token row of token row `row` of h
__device__ __forceinline__ int64_t cache_token_row(const Replay &r, int64_t row) {
    const int64_t b = row / r.N;
    return cache_row(b, r.Fg, r.num_frames, r.frame_ids) * r.N + (row - b * r.N);
}

// layernorm_kernel's arithmetic (a wave per row, lane l the 8-channel pieces l, l + 64, ...; NCH pieces per lane)
template <typename T, int NCH>
__global__ __launch_bounds__(LN_WAVES * 64) void replay_layernorm_kernel(const T *h, const T *__restrict__ cache1,
                                                                         const T *__restrict__ cache2, Replay rp,
                                                                         const T *__restrict__ gamma, const T *__restrict__ beta,
                                                                         int64_t rows, int C, float eps, T *out_rows,
                                                                         T *__restrict__ out_panels, int64_t panel_rows) {
    using namespace vtm::ln;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;                        // (whole waves: the sums below are per wave)
    const int chunks = C / 8;
    const int64_t crow = cache_token_row(rp, row);
    float v[NCH][8];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = lane + 64 * i;
        if (c < chunks) {
            replay8<T>(h + row * C + c * 8, cache1 + crow * C + c * 8, cache2 ? cache2 + crow * C + c * 8 : nullptr, v[i]);
            store8<T>(out_rows + row * C + c * 8, v[i]);
        }
    }
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
        if (lane + 64 * i < chunks) {
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[i][j];
        }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
        if (lane + 64 * i < chunks) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = v[i][j] - mean;
                q = __builtin_fmaf(d, d, q);
            }
        }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = lane + 64 * i;
        if (c < chunks) {
            float g[8], b[8], y[8];
            if (gamma) load8(gamma + c * 8, g);
            if (beta) load8(beta + c * 8, b);
            affine8(v[i], mean, rstd, gamma != nullptr, beta != nullptr, g, b, y);
            store8<T>(out_panels + ((int64_t)c * panel_rows + row) * 8, y);
        }
    }
}

// layernorm_rows_kernel's arithmetic (C = 40 LPR: LPR lanes per row, every lane 5 pieces at a stride of LPR pieces)
template <typename T, int LPR>
__global__ __launch_bounds__(LN_WAVES * 64) void replay_layernorm_rows_kernel(const T *h, const T *__restrict__ cache1,
                                                                              const T *__restrict__ cache2, Replay rp,
                                                                              const T *__restrict__ gamma,
                                                                              const T *__restrict__ beta, int64_t rows, float eps,
                                                                              T *out_rows, T *__restrict__ out_panels,
                                                                              int64_t panel_rows) {
    using namespace vtm::ln;
    constexpr int NCH = 5, C = 8 * NCH * LPR, RPW = 64 / LPR;   // pieces per lane, channels, rows per wave
    const int lane = threadIdx.x & 63, g = lane % LPR, sub = lane / LPR;
    const int64_t row = ((int64_t)blockIdx.x * LN_WAVES + (threadIdx.x >> 6)) * RPW + sub;
    const bool live = row < rows;                   // (a surplus lane group computes on zeros and stores nothing)
    float v[NCH][8];
    if (live) {
        const int64_t crow = cache_token_row(rp, row);
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = g + LPR * i;
            replay8<T>(h + row * C + c * 8, cache1 + crow * C + c * 8, cache2 ? cache2 + crow * C + c * 8 : nullptr, v[i]);
            store8<T>(out_rows + row * C + c * 8, v[i]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) v[i][j] = 0.0f;
    }
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[i][j];
    const float mean = group_sum<LPR>(s) / (float)C;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float d = v[i][j] - mean;
            q = __builtin_fmaf(d, d, q);
        }
    const float rstd = 1.0f / sqrtf(group_sum<LPR>(q) / (float)C + eps);
    if (!live) return;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = g + LPR * i;
        float gm[8], bt[8], y[8];
        if (gamma) load8(gamma + c * 8, gm);
        if (beta) load8(beta + c * 8, bt);
        affine8(v[i], mean, rstd, gamma != nullptr, beta != nullptr, gm, bt, y);
        store8<T>(out_panels + ((int64_t)c * panel_rows + row) * 8, y);
    }
}

// the requirements the three exports share; B = G * Fg samples of E elements
int check_batch(const char *who, int dtype, int64_t G, int64_t Fg, int64_t num_frames, int64_t E) {
    VTM_REQUIRE(dtype == VTM_F32 || dtype == VTM_F16 || dtype == VTM_BF16, "%s: unsupported dtype %d", who, dtype);
    VTM_REQUIRE(G >= 1 && G <= (1 << 16) && Fg >= 1 && Fg <= num_frames && num_frames <= (1 << 20) && E >= 1 &&
                    E <= (int64_t(1) << 40) / (G * num_frames),
                "%s: bad sizes G = %lld, Fg = %lld, num_frames = %lld (1 <= Fg <= num_frames), E = %lld", who, (long long)G,
                (long long)Fg, (long long)num_frames, (long long)E);
    return VTM_OK;
}

inline bool bytes_apart(const void *a, int64_t na, const void *b, int64_t nb) {
    const char *a0 = (const char *)a, *b0 = (const char *)b;
    return a0 + na <= b0 || b0 + nb <= a0;
}

template <typename T, typename K, typename... A>
void launch_elementwise(K *const (&kernels)[2], int64_t B, int64_t E, std::initializer_list<const void *> pointers,
                        hipStream_t st, A... args) {
    constexpr int N = 16 / sizeof(T);
    const bool vec = E % N == 0 && std::all_of(pointers.begin(), pointers.end(), vtm::aligned16);    // (null: aligned, unused)
    const dim3 grid((unsigned)std::min<int64_t>(vtm::cdiv(B * vtm::cdiv(E, N), vtm::EW_THREADS), vtm::EW_GRID_CAP));
    hipLaunchKernelGGL(kernels[vec], grid, dim3(vtm::EW_THREADS), 0, st, args...);
}

}  // namespace

VTM_EXPORT int vtm_residual_record(const void *h_in, const void *h_out, void *cache, const int32_t *frame_ids, int dtype,
                                   int64_t G, int64_t Fg, int64_t num_frames, int64_t E, vtm_stream_t stream) {
    const char *who = "vtm_residual_record";
    if (const int rc = check_batch(who, dtype, G, Fg, num_frames, E)) return rc;
    VTM_REQUIRE(h_in && h_out && cache, "%s: h_in, h_out and cache are required", who);
    VTM_REQUIRE(vtm::rows_apart(cache, G * num_frames, h_in, G * Fg, E, dtype) &&
                    vtm::rows_apart(cache, G * num_frames, h_out, G * Fg, E, dtype), "%s: cache overlaps h_in or h_out", who);
    hipStream_t st = vtm::as_stream(stream);
    const int rc = vtm::with_dtype(dtype, who, [&](auto t) {
        using T = decltype(t);
        using K = decltype(residual_record_kernel<T, true>);
        K *const kernels[2] = {residual_record_kernel<T, false>, residual_record_kernel<T, true>};
        launch_elementwise<T>(kernels, G * Fg, E, {h_in, h_out, cache}, st, (const T *)h_in, (const T *)h_out, (T *)cache,
                              frame_ids, G * Fg, Fg, num_frames, E);
        return (int)VTM_OK;
    });
    return rc != VTM_OK ? rc : vtm::launch_status(who);
}

VTM_EXPORT int vtm_residual_replay(const void *h, const void *cache1, const void *cache2, const int32_t *frame_ids, int dtype,
                                   int64_t G, int64_t Fg, int64_t num_frames, int64_t E, void *out, vtm_stream_t stream) {
    const char *who = "vtm_residual_replay";
    if (const int rc = check_batch(who, dtype, G, Fg, num_frames, E)) return rc;
    VTM_REQUIRE(h && cache1 && out, "%s: h, cache1 and out are required", who);
    VTM_REQUIRE(vtm::rows_apart(out, G * Fg, cache1, G * num_frames, E, dtype) &&
                    (!cache2 || vtm::rows_apart(out, G * Fg, cache2, G * num_frames, E, dtype)),
                "%s: out overlaps a cache", who);
    VTM_REQUIRE(out == h || vtm::rows_apart(out, G * Fg, h, G * Fg, E, dtype), "%s: out overlaps h without being h", who);
    hipStream_t st = vtm::as_stream(stream);
    const int rc = vtm::with_dtype(dtype, who, [&](auto t) {
        using T = decltype(t);
        using K = decltype(residual_replay_kernel<T, true>);
        K *const kernels[2] = {residual_replay_kernel<T, false>, residual_replay_kernel<T, true>};
        launch_elementwise<T>(kernels, G * Fg, E, {h, cache1, cache2, out}, st, (const T *)h, (const T *)cache1,
                              (const T *)cache2, frame_ids, G * Fg, Fg, num_frames, E, (T *)out);
        return (int)VTM_OK;
    });
    return rc != VTM_OK ? rc : vtm::launch_status(who);
}

namespace {

template <typename T>
void launch_replay_layernorm(const void *h, const void *c1, const void *c2, const Replay &rp, const void *gamma, const void *beta,
                             float eps, int64_t rows, int64_t C, void *out_rows, void *out_panels, int64_t panel_rows,
                             hipStream_t s) {
    const dim3 block(LN_WAVES * 64);
    // launch_layernorm's choice (layernorm.hip) for a (rows, C) operand, restated: the family is the summation order
    if (C == 320 || C == 640 || (C == 1280 && rows >= 32768)) {
        const int lpr = (int)(C / 40);
        const dim3 grid((unsigned)vtm::cdiv(rows, (int64_t)LN_WAVES * (64 / lpr)));
#define VTM_RLR(LPR)                                                                                                             \
    hipLaunchKernelGGL((replay_layernorm_rows_kernel<T, LPR>), grid, block, 0, s, (const T *)h, (const T *)c1, (const T *)c2, rp, \
                       (const T *)gamma, (const T *)beta, rows, eps, (T *)out_rows, (T *)out_panels, panel_rows)
        if (lpr == 8) VTM_RLR(8);
        else if (lpr == 16) VTM_RLR(16);
        else VTM_RLR(32);
#undef VTM_RLR
        return;
    }
    const dim3 grid((unsigned)vtm::cdiv(rows, LN_WAVES));
#define VTM_RL(NCH)                                                                                                           \
    hipLaunchKernelGGL((replay_layernorm_kernel<T, NCH>), grid, block, 0, s, (const T *)h, (const T *)c1, (const T *)c2, rp,   \
                       (const T *)gamma, (const T *)beta, rows, (int)C, eps, (T *)out_rows, (T *)out_panels, panel_rows)
    switch ((int)vtm::cdiv(C, 512)) {
        case 1: VTM_RL(1); break;
        case 2: VTM_RL(2); break;
        case 3: VTM_RL(3); break;
        default: VTM_RL(4); break;
    }
#undef VTM_RL
}

}  // namespace

VTM_EXPORT int vtm_residual_replay_layernorm(const void *h, const void *cache1, const void *cache2, const int32_t *frame_ids,
                                             const void *gamma, const void *beta, float eps, int dtype, int64_t G, int64_t Fg,
                                             int64_t num_frames, int64_t N, int64_t C, void *out_rows, void *out_panels,
                                             int64_t panel_rows, vtm_stream_t stream) {
    const char *who = "vtm_residual_replay_layernorm";
    VTM_REQUIRE(dtype == VTM_F16 || dtype == VTM_BF16, "%s: dtype must be VTM_F16 or VTM_BF16 (the panel GEMMs are 16-bit)", who);
    VTM_REQUIRE(N >= 1 && N <= (1 << 24) && C >= 64 && C % 64 == 0 && C <= 64 * 8 * vtm::ln::MAX_CHUNKS,
                "%s: N = %lld, C = %lld: C must be a multiple of 64, <= %d", who, (long long)N, (long long)C,
                64 * 8 * vtm::ln::MAX_CHUNKS);
    if (const int rc = check_batch(who, dtype, G, Fg, num_frames, N * C)) return rc;
    VTM_REQUIRE(h && cache1 && out_rows && out_panels, "%s: h, cache1, out_rows and out_panels are required", who);
    const int64_t rows = G * Fg * N, E = N * C;
    VTM_REQUIRE(rows < (int64_t(1) << 31), "%s: G Fg N = %lld token rows exceed one launch", who, (long long)rows);
    VTM_REQUIRE(panel_rows == vtm_panel_rows(rows), "%s: panel_rows = %lld is not vtm_panel_rows(G Fg N) = %lld", who,
                (long long)panel_rows, (long long)vtm_panel_rows(rows));
    for (const void *p : {h, cache1, cache2, gamma, beta, (const void *)out_rows, (const void *)out_panels})
        VTM_REQUIRE(vtm::aligned16(p), "%s: every operand must be 16-byte aligned", who);
    VTM_REQUIRE(vtm::rows_apart(out_rows, G * Fg, cache1, G * num_frames, E, dtype) &&
                    (!cache2 || vtm::rows_apart(out_rows, G * Fg, cache2, G * num_frames, E, dtype)),
                "%s: out_rows overlaps a cache", who);
    VTM_REQUIRE(out_rows == h || vtm::rows_apart(out_rows, G * Fg, h, G * Fg, E, dtype), "%s: out_rows overlaps h without being h",
                who);
    // (the panels: C / 8 planes of panel_rows rows of 8 elements)
    const int64_t panel_bytes = C / 8 * panel_rows * 8 * 2, batch_bytes = G * Fg * E * 2, cache_bytes = G * num_frames * E * 2;
    VTM_REQUIRE(bytes_apart(out_panels, panel_bytes, h, batch_bytes) && bytes_apart(out_panels, panel_bytes, out_rows, batch_bytes) &&
                    bytes_apart(out_panels, panel_bytes, cache1, cache_bytes) &&
                    (!cache2 || bytes_apart(out_panels, panel_bytes, cache2, cache_bytes)),
                "%s: out_panels overlaps another operand", who);
    const Replay rp{frame_ids, Fg, num_frames, N};
    hipStream_t s = vtm::as_stream(stream);
    if (dtype == VTM_F16) launch_replay_layernorm<__half>(h, cache1, cache2, rp, gamma, beta, eps, rows, C, out_rows, out_panels, panel_rows, s);
    else launch_replay_layernorm<vtm_bf16>(h, cache1, cache2, rp, gamma, beta, eps, rows, C, out_rows, out_panels, panel_rows, s);
    return vtm::launch_status(who);
}
