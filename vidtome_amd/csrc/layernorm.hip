// vtm_layernorm: the block's norm1 (vidtome/patch.py:139-146, plain-LayerNorm branch: `self.norm1(hidden_states)`),
// i.e. torch.nn.LayerNorm over the channel axis -- the first operation of the patched segment and the producer of
// the matching metric.  One wave per token row (2-4 rows per wave in flight), the rows live in registers: read once,
// write once (HBM-bound; cfg-2 top site: 84 MB in + 84 MB out).  Statistics in fp32, two passes over the registers (mean, then the
// centred sum of squares), y = (x - mean) * rstd * gamma + beta evaluated in fp32 and rounded once.
#include "common.h"
#include "layernorm_row.h"

namespace {

#ifndef VTM_LN_RG
#define VTM_LN_RG 0         // A/B build switch: rows per wave of the wave-per-row kernel (0 = the shipped 4 / 2 / 2 / 2)
#endif
#ifndef VTM_LN_WAVES
#define VTM_LN_WAVES 4          // (A/B build switch)
#endif
constexpr int WAVES_PER_BLOCK = VTM_LN_WAVES;
using namespace vtm::ln;       // load8 / store8, wave_sum / group_sum, MAX_CHUNKS (layernorm_row.h)

// vtm_layernorm_gather: the rows of sample blockIdx.y are read through its row of the map -- output row i of the sample is the
// LayerNorm of x[b, map[b, i], :].  Only the source ADDRESS of a row changes: a row is still whole 16-byte pieces per lane, what
// is lost is the contiguity BETWEEN rows.  `rows` of the kernels is then the sample's n, and its output rows start at b n.
struct RowMap {
    const int32_t *map;     // (B, n)
    int64_t L;              // rows of x per sample
};
template <bool G>
__device__ __forceinline__ int64_t source_row(const RowMap &m, int64_t rows, int64_t row) {
    if constexpr (G) return (int64_t)blockIdx.y * m.L + m.map[(int64_t)blockIdx.y * rows + row];
    else return row;
}
template <bool G>
__device__ __forceinline__ int64_t first_out_row(int64_t rows) {
    if constexpr (G) return (int64_t)blockIdx.y * rows;
    else return 0;
}

// NCH: 8-channel chunks per lane (C <= 512 NCH); R: rows per wave, all loaded before the first reduction so that
// a wave keeps R rows of HBM traffic in flight (one row per wave leaves the kernel latency-bound: 2.4 TB/s)
template <typename T, int NCH, int R, bool NT, bool G = false>
__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void layernorm_kernel(const T *__restrict__ x, const T *__restrict__ gamma,
                                                                         const T *__restrict__ beta, int64_t rows, int C,
                                                                         float eps, T *__restrict__ out, int64_t panel_rows,
                                                                         RowMap gm) {
    const int lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6)) * R;
    if (row0 >= rows) return;
    const int chunks = C / 8;
    float v[R][NCH][8];
    float s[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t row = row0 + r < rows ? row0 + r : rows - 1;   // surplus rows recompute the last one, unstored
        const T *xr = x + source_row<G>(gm, rows, row) * C;
        s[r] = 0.0f;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = lane + 64 * i;
            if (c < chunks) load8<T, NT>(xr + c * 8, v[r][i]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int i = 0; i < NCH; ++i)
            if (lane + 64 * i < chunks) {
#pragma unroll
                for (int j = 0; j < 8; ++j) s[r] += v[r][i][j];
            }
    const int64_t orow0 = first_out_row<G>(rows) + row0;
    float mean[R], rstd[R];
#pragma unroll
    for (int r = 0; r < R; ++r) mean[r] = wave_sum(s[r]) / (float)C;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float q = 0.0f;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            if (lane + 64 * i < chunks) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float d = v[r][i][j] - mean[r];
                    q = __builtin_fmaf(d, d, q);
                }
            }
        }
        s[r] = q;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) rstd[r] = 1.0f / sqrtf(wave_sum(s[r]) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = lane + 64 * i;
        if (c < chunks) {
            float g[8], b[8];
            if (gamma) load8(gamma + c * 8, g);
            if (beta) load8(beta + c * 8, b);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (row0 + r < rows) {
                    float y[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float n = (v[r][i][j] - mean[r]) * rstd[r];
                        y[j] = gamma ? (beta ? __builtin_fmaf(n, g[j], b[j]) : n * g[j]) : (beta ? n + b[j] : n);
                    }
                    // panel_rows > 0: the k-panel layout [C / 8][panel_rows][8] of the panel GEMMs (ff.hip)
                    store8<T, NT>(panel_rows ? out + ((int64_t)c * panel_rows + (orow0 + r)) * 8 : out + (orow0 + r) * C + c * 8, y);
                }
            }
        }
    }
}

// The SD channel counts (C = 40 LPR, LPR = 8 / 16 / 32 for 320 / 640 / 1280): LPR lanes per row, every lane 5 pieces of
// 16 bytes at a stride of LPR pieces -- all 64 lanes busy (a wave per 320-channel row keeps 24 of them idle), a load
// instruction covers 64 / LPR rows with 16 LPR contiguous bytes each, and a wave keeps R * 64 / LPR rows in flight.
template <typename T, int LPR, int R, bool NT, bool G = false>
__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void layernorm_rows_kernel(const T *__restrict__ x, const T *__restrict__ gamma,
                                                                              const T *__restrict__ beta, int64_t rows, float eps,
                                                                              T *__restrict__ out, int64_t panel_rows, RowMap gm) {
    constexpr int NCH = 5, C = 8 * NCH * LPR, RPW = 64 / LPR;   // pieces per lane, channels, rows per wave and round
    const int lane = threadIdx.x & 63, g = lane % LPR, sub = lane / LPR;
    const int64_t row0 = ((int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6)) * (RPW * R) + sub;
    float v[R][NCH][8];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int64_t row = row0 + (int64_t)r * RPW;
        if (row >= rows) row = rows - 1;                        // surplus rows recompute the last one, unstored
        const T *xr = x + source_row<G>(gm, rows, row) * C;
#pragma unroll
        for (int i = 0; i < NCH; ++i) load8<T, NT>(xr + (g + LPR * i) * 8, v[r][i]);
    }
    float mean[R], rstd[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[r][i][j];
        mean[r] = group_sum<LPR>(s) / (float)C;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float q = 0.0f;
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = v[r][i][j] - mean[r];
                q = __builtin_fmaf(d, d, q);
            }
        rstd[r] = 1.0f / sqrtf(group_sum<LPR>(q) / (float)C + eps);
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = g + LPR * i;
        float gm[8], bt[8];
        if (gamma) load8(gamma + c * 8, gm);
        if (beta) load8(beta + c * 8, bt);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = row0 + (int64_t)r * RPW;
            if (row < rows) {
                const int64_t orow = first_out_row<G>(rows) + row;
                float y[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float n = (v[r][i][j] - mean[r]) * rstd[r];
                    y[j] = gamma ? (beta ? __builtin_fmaf(n, gm[j], bt[j]) : n * gm[j]) : (beta ? n + bt[j] : n);
                }
                store8<T, NT>(panel_rows ? out + ((int64_t)c * panel_rows + orow) * 8 : out + orow * C + c * 8, y);
            }
        }
    }
}

// `rows`: the rows of x.  G (vtm_layernorm_gather): x is (B, L, C), rows = B L, and each of the B samples writes n rows read
// through gm (the grid's y is the sample).  The kernel family and the streaming policy are decided from the rows of x either
// way, so that a gathered row is computed by the kernel -- the summation order -- vtm_layernorm / vtm_layernorm_panels use for
// the same x.
template <typename T, bool G = false>
void launch_layernorm(const void *x, const void *gamma, const void *beta, int64_t rows, int64_t C, float eps, void *out,
                      int64_t panel_rows, hipStream_t s, RowMap gm = RowMap{nullptr, 0}, int64_t B = 1, int64_t n = 0) {
    const int64_t nr = G ? n : rows;        // output rows of one grid-y slice
    // input + output beyond the Infinity Cache: streaming loads / stores (common.h)
    const bool nt = 2 * rows * C * (int64_t)sizeof(T) > vtm::STREAM_BYTES;
#ifndef VTM_OLD_LN   // (A/B build switch)
    // measured (profiles/r02_sweeps.txt): +24 % HBM rate at C = 320 beyond the Infinity Cache
    // round 3 (one round of rows per wave, profiles/r03_hbm_nt.txt): the lanes-per-row kernel also wins at C = 640 (6.0 vs 4.2
    // TB/s beyond the Infinity Cache, +6 % at the cfg-2 mid sites) and at C = 1280 for large row counts; the few-thousand-row
    // C = 1280 sites stay with a wave per row (14.7 vs 16.7 us)
    if (C == 320 || C == 640 || (C == 1280 && rows >= 32768)) {
#ifndef VTM_LN_R
#define VTM_LN_R 1          // rows per lane group in flight (A/B in profiles/r03_hbm_nt.txt: 1 beats 2, 3, 4)
#endif
        constexpr int R = VTM_LN_R;
        const int lpr = (int)(C / 40);
        const dim3 g((unsigned)vtm::cdiv(nr, (int64_t)WAVES_PER_BLOCK * (64 / lpr) * R), (unsigned)B), b(WAVES_PER_BLOCK * 64);
#define VTM_LNR(LPR, NT_)                                                                                              \
    hipLaunchKernelGGL((layernorm_rows_kernel<T, LPR, R, NT_, G>), g, b, 0, s, (const T *)x, (const T *)gamma, (const T *)beta, \
                       nr, eps, (T *)out, panel_rows, gm)
        if (lpr == 8) { if (nt) VTM_LNR(8, true); else VTM_LNR(8, false); }
        else if (lpr == 16) { if (nt) VTM_LNR(16, true); else VTM_LNR(16, false); }
        else { if (nt) VTM_LNR(32, true); else VTM_LNR(32, false); }
#undef VTM_LNR
        return;
    }
#endif
    const int nch = (int)vtm::cdiv(C, 512);
    const int R = VTM_LN_RG ? VTM_LN_RG : (nch == 1 ? 4 : 2);
    const dim3 grid((unsigned)vtm::cdiv(nr, (int64_t)WAVES_PER_BLOCK * R), (unsigned)B), block(WAVES_PER_BLOCK * 64);
#define VTM_LN(NCH, RR)                                                                                               \
    do {                                                                                                              \
        if (nt)                                                                                                       \
            hipLaunchKernelGGL((layernorm_kernel<T, NCH, RR, true, G>), grid, block, 0, s, (const T *)x, (const T *)gamma, \
                               (const T *)beta, nr, (int)C, eps, (T *)out, panel_rows, gm);                          \
        else                                                                                                          \
            hipLaunchKernelGGL((layernorm_kernel<T, NCH, RR, false, G>), grid, block, 0, s, (const T *)x, (const T *)gamma, \
                               (const T *)beta, nr, (int)C, eps, (T *)out, panel_rows, gm);                          \
    } while (0)
    switch (nch) {
        case 1: VTM_LN(1, (VTM_LN_RG ? VTM_LN_RG : 4)); break;
        case 2: VTM_LN(2, (VTM_LN_RG ? VTM_LN_RG : 2)); break;
        case 3: VTM_LN(3, (VTM_LN_RG ? VTM_LN_RG : 2)); break;
        default: VTM_LN(4, (VTM_LN_RG ? VTM_LN_RG : 2)); break;
    }
#undef VTM_LN
}

}  // namespace

VTM_EXPORT int vtm_layernorm(const void *x, const void *gamma, const void *beta, int dtype, int64_t rows, int64_t C,
                             float eps, void *out, vtm_stream_t stream) {
    VTM_REQUIRE(x && out && rows >= 0, "vtm_layernorm: null pointer");
    VTM_REQUIRE(C > 0 && C % 8 == 0 && C <= 64 * 8 * MAX_CHUNKS, "vtm_layernorm: C must be a multiple of 8, <= %d",
                64 * 8 * MAX_CHUNKS);
    if (rows == 0) return VTM_OK;
    hipStream_t s = vtm::as_stream(stream);
    switch (dtype) {
        case VTM_F32: launch_layernorm<float>(x, gamma, beta, rows, C, eps, out, 0, s); break;
        case VTM_F16: launch_layernorm<__half>(x, gamma, beta, rows, C, eps, out, 0, s); break;
        case VTM_BF16: launch_layernorm<vtm_bf16>(x, gamma, beta, rows, C, eps, out, 0, s); break;
        default: return vtm::fail(VTM_EINVAL, "vtm_layernorm: unsupported dtype %d", dtype);
    }
    return vtm::launch_status("vtm_layernorm");
}

// The same LayerNorm with its result written in the k-panel layout [C / 8][panel_rows][8] -- the token operand of the panel
// GEMMs of ff.hip (norm3 -> GEGLU projection, norm2 -> to_q of the cross-attention: patch.py:171-199); rows >= `rows` of
// the panels are not written.
VTM_EXPORT int vtm_layernorm_panels(const void *x, const void *gamma, const void *beta, int dtype, int64_t rows, int64_t C,
                                    float eps, void *out, int64_t panel_rows, vtm_stream_t stream) {
    VTM_REQUIRE(x && out && rows > 0, "vtm_layernorm_panels: null pointer");
    VTM_REQUIRE(C > 0 && C % 8 == 0 && C <= 64 * 8 * MAX_CHUNKS, "vtm_layernorm_panels: C must be a multiple of 8, <= %d",
                64 * 8 * MAX_CHUNKS);
    VTM_REQUIRE(panel_rows >= rows, "vtm_layernorm_panels: panel_rows < rows");
    hipStream_t s = vtm::as_stream(stream);
    switch (dtype) {
        case VTM_F16: launch_layernorm<__half>(x, gamma, beta, rows, C, eps, out, panel_rows, s); break;
        case VTM_BF16: launch_layernorm<vtm_bf16>(x, gamma, beta, rows, C, eps, out, panel_rows, s); break;
        default: return vtm::fail(VTM_EINVAL, "vtm_layernorm_panels: dtype must be VTM_F16 or VTM_BF16");
    }
    return vtm::launch_status("vtm_layernorm_panels");
}

// norm3 on m(x) (vidtome/patch.py:187 behind merge.py:119-133): the LayerNorm of the rows a merge map selects, for the
// feed-forward on merged tokens (patch.py's merge_mlp).  The kernels above with the source row taken through the map.
VTM_EXPORT int vtm_layernorm_gather(const void *x, const void *gamma, const void *beta, int dtype, int64_t B, int64_t L, int64_t C,
                                    const int32_t *rows, int64_t n, float eps, void *out, int64_t panel_rows,
                                    vtm_stream_t stream) {
    const char *who = "vtm_layernorm_gather";
    VTM_REQUIRE(x && out && rows, "%s: null pointer (x, rows and out are required)", who);
    VTM_REQUIRE(dtype == VTM_F32 || dtype == VTM_F16 || dtype == VTM_BF16, "%s: unsupported dtype %d", who, dtype);
    VTM_REQUIRE(C > 0 && C % 8 == 0 && C <= 64 * 8 * MAX_CHUNKS, "%s: C = %lld must be a multiple of 8, <= %d", who, (long long)C,
                64 * 8 * MAX_CHUNKS);
    // (B is the grid's y)
    VTM_REQUIRE(B >= 0 && B <= 65535 && L >= 0 && n >= 0 && L < ((int64_t)1 << 31), "%s: bad sizes B = %lld (<= 65535), L = %lld, "
                "n = %lld", who, (long long)B, (long long)L, (long long)n);
    VTM_REQUIRE(panel_rows == 0 || panel_rows == vtm_panel_rows(B * n), "%s: panel_rows = %lld is neither 0 (token rows) nor "
                "vtm_panel_rows(B n) = %lld", who, (long long)panel_rows, (long long)vtm_panel_rows(B * n));
    VTM_REQUIRE(panel_rows == 0 || dtype != VTM_F32, "%s: panels are fp16 / bf16 (fp32: panel_rows = 0)", who);
    if (B == 0 || n == 0) return VTM_OK;
    VTM_REQUIRE(L > 0, "%s: rows to gather from an empty sample (L = 0)", who);
    hipStream_t s = vtm::as_stream(stream);
    const RowMap gm{rows, L};
    switch (dtype) {
        case VTM_F32: launch_layernorm<float, true>(x, gamma, beta, B * L, C, eps, out, panel_rows, s, gm, B, n); break;
        case VTM_F16: launch_layernorm<__half, true>(x, gamma, beta, B * L, C, eps, out, panel_rows, s, gm, B, n); break;
        default: launch_layernorm<vtm_bf16, true>(x, gamma, beta, B * L, C, eps, out, panel_rows, s, gm, B, n); break;
    }
    return vtm::launch_status(who);
}
