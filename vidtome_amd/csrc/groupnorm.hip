// The two elementwise ends of the PnP feature-injection resnet (utils/pnp_utils.py:108-172, `register_conv_control`;
// host side: vidtome_amd/pnp.py).  Both are HBM-bound.
//
// vtm_groupnorm_silu: act(GroupNorm(x [+ add])) on an NCHW tensor in one launch (pnp_utils.py:113-114 `norm1` +
// `nonlinearity`, :133-142 `+ temb`, `norm2`, `nonlinearity`).  One workgroup per (sample, group): the group is one
// contiguous run of n = (C / groups) * HW elements.  It is read from HBM once, kept in LDS as the rounded x' = x + add
// while the block reduces the mean (summed in fp64, then one fp32 value) and then the centred sum of squares (fp32,
// biased variance, like vtm_layernorm), and written from LDS.  A group larger than the LDS keeps its first part
// resident and re-reads only the rest in the second and third sweep.  Rounding points are those of torch's separate
// ops (as in vtm_geglu): x', y and z are each rounded to the tensor dtype.
//
// vtm_resnet_tail: out[b] = (shortcut[b] + hidden[row(b)]) / scale (pnp_utils.py:146-162: the injection copies, the
// residual and the division), bit-identical to torch's expression: the sum rounded to the dtype, then multiplied by
// the fp32 reciprocal of the scale (how torch divides a GPU tensor by a host scalar) and rounded again.
#include "common.h"

#include <algorithm>

namespace {

template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ __half from_f32<__half>(float v) { return __float2half_rn(v); }
template <> __device__ __forceinline__ vtm_bf16 from_f32<vtm_bf16>(float v) { return __float2bfloat16(v); }

template <typename T> __device__ __forceinline__ float round_to(float v) { return vtm::to_f32(from_f32<T>(v)); }

constexpr int GN_SCRATCH = 256;                   // bytes of reduction scratch in front of the resident group (16 doubles, 16 floats)
constexpr int GN_LDS_MAX = 160 * 1024;            // LDS of a CU
#ifndef VTM_GN_U
#define VTM_GN_U 4          // (A/B build switch)
#endif
#ifndef VTM_GN_THREADS
#define VTM_GN_THREADS 0    // A/B build switch: block size for every group (0 = the shipped rule of launch_groupnorm)
#endif
constexpr int GN_U = VTM_GN_U;                    // 16-byte loads a thread has in flight in the first sweep

template <typename T>
__device__ __forceinline__ float silu(float y) {
    // 16-bit dtypes: the hardware exp2 and reciprocal (v_exp_f32, v_rcp_f32: ~3e-7 relative together, against a rounding
    // step of 2^-9 or 2^-12) -- with the IEEE division and libm's expf the kernel is VALU-bound, not HBM-bound.  exp
    // overflows to inf below y = -88.7 and the result is -0, as torch's x / (1 + exp(-x)) in fp32.
    if constexpr (sizeof(T) == 4) return y / (1.0f + expf(-y));
    else return y * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(y * -1.4426950408889634f));
}

// all threads get the block's sum; the same summation order in every thread and every run
template <typename A>
__device__ __forceinline__ A block_sum(A v, A *scratch) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    const int waves = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    A s = 0;
    for (int w = 0; w < waves; ++w) s += scratch[w];
    return s;
}

// channel (relative to the group's first) and pixel of element i: one reciprocal multiply per 16-byte piece, corrected
__device__ __forceinline__ void channel_of(int i, int HW, float inv_hw, int &c, int &r) {
    c = (int)((float)i * inv_hw);
    r = i - c * HW;
    while (r < 0) { r += HW; --c; }
    while (r >= HW) { r -= HW; ++c; }
}

// per-channel values p[c ...] for the V elements that start at (channel c, pixel r)
template <int V, typename T>
__device__ __forceinline__ void channel_values(const T *__restrict__ p, int c, int r, int HW, float (&o)[V]) {
    if (r + V <= HW) {
        const float v = vtm::to_f32(p[c]);
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = v;
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            while (r >= HW) { r -= HW; ++c; }
            o[j] = vtm::to_f32(p[c]);
            ++r;
        }
    }
}

template <typename T>
struct GnGroup {
    static constexpr int V = 16 / sizeof(T);
    const T *__restrict__ xg;      // the group's first element
    const T *__restrict__ addg;    // add[b, first channel of the group] or null
    T *sx;                         // resident part: element i at sx[i + pad]
    int n, HW, head, pad, nvec, tail0, resident;
    float inv_hw;

    // x' of the 16-byte piece at element i0 (16-byte aligned in x, out and LDS) from a loaded piece
    __device__ __forceinline__ void xprime(const uint4 &raw, int i0, float (&f)[V]) const {
        const T *e = reinterpret_cast<const T *>(&raw);
#pragma unroll
        for (int j = 0; j < V; ++j) f[j] = vtm::to_f32(e[j]);
        if (addg) {
            int c, r;
            channel_of(i0, HW, inv_hw, c, r);
            float a[V];
            channel_values<V>(addg, c, r, HW, a);
#pragma unroll
            for (int j = 0; j < V; ++j) f[j] = round_to<T>(f[j] + a[j]);
        }
    }
    __device__ __forceinline__ float xprime1(int i) const {
        float v = vtm::to_f32(xg[i]);
        if (addg) {
            int c, r;
            channel_of(i, HW, inv_hw, c, r);
            v = round_to<T>(v + vtm::to_f32(addg[c]));
        }
        return v;
    }
    // the second and third sweep: from LDS where resident, else from memory again
    __device__ __forceinline__ void get(int i0, float (&f)[V]) const {
        if (i0 < resident) {
            const uint4 raw = *reinterpret_cast<const uint4 *>(sx + i0 + pad);
            const T *e = reinterpret_cast<const T *>(&raw);
#pragma unroll
            for (int j = 0; j < V; ++j) f[j] = vtm::to_f32(e[j]);
        } else {
            xprime(*reinterpret_cast<const uint4 *>(xg + i0), i0, f);
        }
    }
    __device__ __forceinline__ float get1(int i) const { return i < resident ? vtm::to_f32(sx[i + pad]) : xprime1(i); }
    // the elements in front of the first and behind the last aligned piece (fewer than 2 V), one per thread
    __device__ __forceinline__ int edge(int t) const { return t < head ? t : tail0 + (t - head); }
    __device__ __forceinline__ int edges() const { return head + (n - tail0); }
};

template <typename T>
__global__ __launch_bounds__(1024) void groupnorm_silu_kernel(const T *__restrict__ x, const T *__restrict__ add,
                                                              const T *__restrict__ gamma, const T *__restrict__ beta,
                                                              int C, int HW, int groups, float eps, int act, int lds_elems,
                                                              T *__restrict__ out) {
    constexpr int V = 16 / sizeof(T);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *scratch_mean = reinterpret_cast<double *>(smem);
    float *scratch_var = reinterpret_cast<float *>(smem + 128);
    const int tid = threadIdx.x, NT = blockDim.x;
    const int b = blockIdx.x / groups, g = blockIdx.x - b * groups, cpg = C / groups;
    const int64_t g0 = ((int64_t)b * C + (int64_t)g * cpg) * HW;

    GnGroup<T> G;
    G.n = cpg * HW;
    G.HW = HW;
    G.inv_hw = 1.0f / (float)HW;
    G.xg = x + g0;
    G.addg = add ? add + (int64_t)b * C + g * cpg : nullptr;
    G.sx = reinterpret_cast<T *>(smem + GN_SCRATCH);
    // x and out are 16-byte aligned: element g0 + i is at a 16-byte boundary when (g0 + i) % V == 0
    G.head = std::min<int>(G.n, (int)((V - g0 % V) % V));
    G.pad = (V - G.head) % V;
    G.nvec = (G.n - G.head) / V;
    G.tail0 = G.head + G.nvec * V;
    // resident: everything, or whole pieces up to the LDS size
    G.resident = G.n + G.pad <= lds_elems ? G.n : G.head + std::max(0, (lds_elems - G.pad - G.head) / V) * V;
    T *og = out + g0;

    // ---- sweep 1: HBM -> x' -> LDS, the sum ----
    // The sum of the mean is carried in fp64: an fp32 sum errs by 2^-24 of the partial sums' magnitude, which for a mean
    // near zero is far more than one rounding of the mean itself.  The mean is then one fp32 value like torch's.
    double s = 0.0;
    for (int v0 = tid; v0 < G.nvec; v0 += NT * GN_U) {
        uint4 raw[GN_U];
#pragma unroll
        for (int u = 0; u < GN_U; ++u) {
            const int v = v0 + u * NT;
            if (v < G.nvec) raw[u] = *reinterpret_cast<const uint4 *>(G.xg + G.head + v * V);
        }
#pragma unroll
        for (int u = 0; u < GN_U; ++u) {
            const int v = v0 + u * NT, i0 = G.head + v * V;
            if (v < G.nvec) {
                float f[V];
                G.xprime(raw[u], i0, f);
                if (i0 < G.resident) {
                    uint4 st;
                    T *e = reinterpret_cast<T *>(&st);
#pragma unroll
                    for (int j = 0; j < V; ++j) e[j] = from_f32<T>(f[j]);
                    *reinterpret_cast<uint4 *>(G.sx + i0 + G.pad) = st;
                }
                if constexpr (sizeof(T) == 4) {
#pragma unroll
                    for (int j = 0; j < V; ++j) s += (double)f[j];
                } else {        // eight 16-bit values: their fp32 sum is exact unless their exponents are far apart
                    s += (double)(((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7])));
                }
            }
        }
    }
    if (tid < G.edges()) {
        const int i = G.edge(tid);
        const float v = G.xprime1(i);
        if (i < G.resident) G.sx[i + G.pad] = from_f32<T>(v);
        s += (double)v;
    }
    const float mean = (float)(block_sum(s, scratch_mean) / (double)G.n);      // (its barrier also publishes the LDS image)

    // ---- sweep 2: the centred sum of squares ----
    float q = 0.0f;
    for (int v = tid; v < G.nvec; v += NT) {
        float f[V];
        G.get(G.head + v * V, f);
        float p = 0.0f;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float d = f[j] - mean;
            p = __builtin_fmaf(d, d, p);
        }
        q += p;
    }
    if (tid < G.edges()) {
        const float d = G.get1(G.edge(tid)) - mean;
        q = __builtin_fmaf(d, d, q);
    }
    const float rstd = 1.0f / sqrtf(block_sum(q, scratch_var) / (float)G.n + eps);

    // ---- sweep 3: normalise, affine, activation, write ----
    const T *gg = gamma ? gamma + g * cpg : nullptr, *bg = beta ? beta + g * cpg : nullptr;
    for (int v = tid; v < G.nvec; v += NT) {
        const int i0 = G.head + v * V;
        float f[V], gm[V], bt[V];
        G.get(i0, f);
        if (gg || bg) {
            int c, r;
            channel_of(i0, HW, G.inv_hw, c, r);
            if (gg) channel_values<V>(gg, c, r, HW, gm);
            if (bg) channel_values<V>(bg, c, r, HW, bt);
        }
        uint4 st;
        T *e = reinterpret_cast<T *>(&st);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float nv = (f[j] - mean) * rstd;
            float y = gg ? (bg ? __builtin_fmaf(nv, gm[j], bt[j]) : nv * gm[j]) : (bg ? nv + bt[j] : nv);
            if (act) y = silu<T>(round_to<T>(y));
            e[j] = from_f32<T>(y);
        }
        *reinterpret_cast<uint4 *>(og + i0) = st;
    }
    if (tid < G.edges()) {
        const int i = G.edge(tid);
        int c, r;
        channel_of(i, HW, G.inv_hw, c, r);
        const float nv = (G.get1(i) - mean) * rstd;
        const float gv = gg ? vtm::to_f32(gg[c]) : 1.0f, bv = bg ? vtm::to_f32(bg[c]) : 0.0f;
        float y = gg ? (bg ? __builtin_fmaf(nv, gv, bv) : nv * gv) : (bg ? nv + bv : nv);
        if (act) y = silu<T>(round_to<T>(y));
        og[i] = from_f32<T>(y);
    }
}

// compact row of `hidden` that output row b adds: the injected rows take the source rows, the others keep their own
__device__ __forceinline__ int64_t tail_row(int64_t b, int64_t inject_rows, int64_t period) {
    return b < inject_rows ? b % period : b - inject_rows + period;
}

constexpr int TAIL_THREADS = 256, TAIL_U = 4;

template <typename T>
__global__ __launch_bounds__(TAIL_THREADS) void resnet_tail_vec_kernel(const T *__restrict__ shortcut, const T *__restrict__ hidden,
                                                                       int64_t pieces, int blocks_per_row, int64_t inject_rows,
                                                                       int64_t period, float inv_scale, T *__restrict__ out) {
    constexpr int V = 16 / sizeof(T);
    const int64_t b = blockIdx.x / blocks_per_row;
    const int64_t p0 = (int64_t)(blockIdx.x - b * blocks_per_row) * (TAIL_THREADS * TAIL_U) + threadIdx.x;
    const T *sr = shortcut + b * pieces * V, *hr = hidden + tail_row(b, inject_rows, period) * pieces * V;
    T *orow = out + b * pieces * V;
    uint4 sv[TAIL_U], hv[TAIL_U];
#pragma unroll
    for (int u = 0; u < TAIL_U; ++u) {
        const int64_t p = p0 + u * TAIL_THREADS;
        if (p < pieces) {
            sv[u] = *reinterpret_cast<const uint4 *>(sr + p * V);
            hv[u] = *reinterpret_cast<const uint4 *>(hr + p * V);
        }
    }
#pragma unroll
    for (int u = 0; u < TAIL_U; ++u) {
        const int64_t p = p0 + u * TAIL_THREADS;
        if (p < pieces) {
            const T *se = reinterpret_cast<const T *>(&sv[u]), *he = reinterpret_cast<const T *>(&hv[u]);
            uint4 st;
            T *e = reinterpret_cast<T *>(&st);
#pragma unroll
            for (int j = 0; j < V; ++j) e[j] = from_f32<T>(round_to<T>(vtm::to_f32(se[j]) + vtm::to_f32(he[j])) * inv_scale);
            *reinterpret_cast<uint4 *>(orow + p * V) = st;
        }
    }
}

// rows whose length is no multiple of a 16-byte piece, or unaligned operands: one element per thread and step
template <typename T>
__global__ __launch_bounds__(TAIL_THREADS) void resnet_tail_scalar_kernel(const T *__restrict__ shortcut, const T *__restrict__ hidden,
                                                                          int64_t M, int blocks_per_row, int64_t inject_rows,
                                                                          int64_t period, float inv_scale, T *__restrict__ out) {
    const int64_t b = blockIdx.x / blocks_per_row;
    const T *sr = shortcut + b * M, *hr = hidden + tail_row(b, inject_rows, period) * M;
    T *orow = out + b * M;
    for (int64_t i = (int64_t)(blockIdx.x - b * blocks_per_row) * TAIL_THREADS + threadIdx.x; i < M;
         i += (int64_t)blocks_per_row * TAIL_THREADS)
        orow[i] = from_f32<T>(round_to<T>(vtm::to_f32(sr[i]) + vtm::to_f32(hr[i])) * inv_scale);
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T>
int launch_groupnorm(const void *x, const void *add, const void *gamma, const void *beta, int64_t B, int64_t C, int64_t HW,
                     int64_t groups, float eps, int act, void *out, hipStream_t s) {
    constexpr int V = 16 / sizeof(T);
    const int64_t n = C / groups * HW;
    // resident bytes: the group, plus one piece of slack when group starts can be off a 16-byte boundary
    const int64_t want = vtm::cdiv((n + (n % V ? V : 0)) * (int64_t)sizeof(T), 16) * 16;
    const int64_t data = std::min<int64_t>(want, GN_LDS_MAX - GN_SCRATCH);
    const int lds = (int)data + GN_SCRATCH;
    // enough waves per CU to cover the HBM latency: about 24 where the LDS allows several blocks, else one large block
    const int per_cu = GN_LDS_MAX / lds;
    int threads = per_cu * 256 >= 1536 ? 256 : (per_cu * 512 >= 1536 ? 512 : 1024);
    if (VTM_GN_THREADS) threads = VTM_GN_THREADS;
    threads = (int)std::min<int64_t>(threads, std::max<int64_t>(64, vtm::cdiv(vtm::cdiv(n, V), 64) * 64));
    if (lds > 64 * 1024) {
        const hipError_t e = vtm::opt_in_lds<groupnorm_silu_kernel<T>, GN_LDS_MAX>();
        if (e != hipSuccess) return vtm::fail(VTM_ELAUNCH, "vtm_groupnorm_silu: LDS attribute: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(groupnorm_silu_kernel<T>, dim3((unsigned)(B * groups)), dim3(threads), lds, s, (const T *)x, (const T *)add,
                       (const T *)gamma, (const T *)beta, (int)C, (int)HW, (int)groups, eps, act, (int)(data / sizeof(T)), (T *)out);
    return vtm::launch_status("vtm_groupnorm_silu");
}

}  // namespace

VTM_EXPORT int vtm_groupnorm_silu(const void *x, const void *add, const void *gamma, const void *beta, int dtype, int64_t B,
                                  int64_t C, int64_t HW, int64_t groups, float eps, int act, void *out, vtm_stream_t stream) {
    VTM_REQUIRE(x && out && B >= 0 && C > 0 && HW > 0, "vtm_groupnorm_silu: bad arguments");
    VTM_REQUIRE(groups > 0 && C % groups == 0, "vtm_groupnorm_silu: groups (%lld) must divide C (%lld)", (long long)groups,
                (long long)C);
    VTM_REQUIRE(act == 0 || act == 1, "vtm_groupnorm_silu: act must be 0 (none) or 1 (SiLU)");
    VTM_REQUIRE(dtype == VTM_F32 || dtype == VTM_F16 || dtype == VTM_BF16, "vtm_groupnorm_silu: unsupported dtype %d", dtype);
    VTM_REQUIRE(C <= INT32_MAX && C / groups * HW <= INT32_MAX && B * groups <= INT32_MAX,
                "vtm_groupnorm_silu: a group or the grid exceeds 2^31 - 1");
    VTM_REQUIRE(aligned16(x) && aligned16(out), "vtm_groupnorm_silu: x and out must be 16-byte aligned");
    VTM_REQUIRE(x != out, "vtm_groupnorm_silu: out must not alias x (a group larger than the LDS is read again after the first writes)");
    if (B == 0) return VTM_OK;
    hipStream_t s = vtm::as_stream(stream);
    return vtm::with_dtype(dtype, "vtm_groupnorm_silu", [&](auto t) {
        return launch_groupnorm<decltype(t)>(x, add, gamma, beta, B, C, HW, groups, eps, act, out, s);
    });
}

VTM_EXPORT int vtm_resnet_tail(const void *shortcut, const void *hidden, int dtype, int64_t B, int64_t M, int64_t inject_rows,
                               int64_t period, double scale, void *out, vtm_stream_t stream) {
    VTM_REQUIRE(shortcut && hidden && out && B >= 0 && M > 0, "vtm_resnet_tail: bad arguments");
    VTM_REQUIRE(inject_rows >= 0 && inject_rows <= B && period >= 0, "vtm_resnet_tail: inject_rows must lie in [0, B], period >= 0");
    VTM_REQUIRE(inject_rows == 0 || period > 0, "vtm_resnet_tail: injected rows need a period > 0");
    VTM_REQUIRE(dtype == VTM_F32 || dtype == VTM_F16 || dtype == VTM_BF16, "vtm_resnet_tail: unsupported dtype %d", dtype);
    VTM_REQUIRE(scale != 0.0 && scale == scale, "vtm_resnet_tail: scale must be a nonzero number");
    if (B == 0) return VTM_OK;
    hipStream_t s = vtm::as_stream(stream);
    const float inv_scale = 1.0f / (float)scale;
    return vtm::with_dtype(dtype, "vtm_resnet_tail", [&](auto t) {
        using T = decltype(t);
        constexpr int V = 16 / sizeof(T);
        if (M % V == 0 && aligned16(shortcut) && aligned16(hidden) && aligned16(out)) {
            const int64_t pieces = M / V, bpr = vtm::cdiv(pieces, TAIL_THREADS * TAIL_U);
            VTM_REQUIRE(B * bpr <= INT32_MAX, "vtm_resnet_tail: grid exceeds 2^31 - 1");
            hipLaunchKernelGGL(resnet_tail_vec_kernel<T>, dim3((unsigned)(B * bpr)), dim3(TAIL_THREADS), 0, s, (const T *)shortcut,
                               (const T *)hidden, pieces, (int)bpr, inject_rows, period, inv_scale, (T *)out);
        } else {
            const int64_t bpr = std::min<int64_t>(vtm::cdiv(M, TAIL_THREADS), 1024);
            VTM_REQUIRE(B * bpr <= INT32_MAX, "vtm_resnet_tail: grid exceeds 2^31 - 1");
            hipLaunchKernelGGL(resnet_tail_scalar_kernel<T>, dim3((unsigned)(B * bpr)), dim3(TAIL_THREADS), 0, s,
                               (const T *)shortcut, (const T *)hidden, M, (int)bpr, inject_rows, period, inv_scale, (T *)out);
        }
        return vtm::launch_status("vtm_resnet_tail");
    });
}
