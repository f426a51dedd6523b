// vtm_freeu: FreeU (Si et al.; Diffusers' enable_freeu, threshold 1) in place on the concatenation cat([hidden, skip], 1) an
// up-block resnet is about to read -- the backbone half-range scaled, the skip planes filtered -- with no FFT.
//
// The identity.  With threshold 1 the "low-frequency box" of the shifted spectrum is the four bins ky, kx in {0, -1}, so
//     Re ifftn(ifftshift(mask * fftshift(fftn(v)))) = v + (s - 1) * (projection of v on those four bins)
// and the projection needs seven real sums over the plane (a = 2 pi y / H, b = 2 pi x / W):
//     S = sum v,  A_c / A_s = sum v cos a / sin a,  B_c / B_s = sum v cos b / sin b,  D_c / D_s = sum v cos(a + b) / sin(a + b)
//     out = v + (s - 1) / P * (S + A_c cos a + A_s sin a + B_c cos b + B_s sin b + D_c cos(a + b) + D_s sin(a + b)).
// (bin (0, -1) is the conjugate of no kept bin, so its real part carries the factor 1, as do (-1, 0) and (-1, -1); for
// H = 2 the bins ky = 0 and ky = -1 are all there is and sin a = 0: the formula is the same.)
//
// The forms.  A plane is cut into CHUNKS of 8 consecutive elements.  G lanes own a plane; lane l holds the chunks l, l + G,
// l + 2 G, ... -- at most 4 of them, IN REGISTERS, between the two passes (sum, then apply).  The issue of keeping a 16-bit
// plane in LDS as fp32 or reading it twice does not arise: every form gives a lane at most 32 values, so the plane is read
// from memory once, converted once, and neither LDS traffic nor a second (L2) read is paid.  G is a function of P alone
// (vtm_freeu_lanes; the same for the three dtypes, so the summation order of a plane does not depend on its dtype's width):
//     P <=   256   G = 16    16 planes per 256-thread workgroup  (8 x 8, 12 x 12, 16 x 16: <= 2 chunks per lane)
//     P <=  2048   G = 64    a wave per plane, 4 per workgroup   (24 x 24, 32 x 32:       <= 4 chunks per lane)
//     P <=  8192   G = 256   one workgroup per plane             (64 x 64:                <= 4 chunks per lane)
//     P <= 16384   G = 1024  one workgroup per plane             (128 x 128:              <= 2 chunks per lane)
// A chunk moves with 16-byte accesses where every plane base is 16-byte aligned (x is, and P * sizeof(T) % 16 == 0) and
// element by element otherwise (5 x 7); the chunk-to-lane map is the same in both, so no bit depends on which one ran.
// Nothing is read or written outside the plane: the last chunk is cut to the elements the plane has.
//
// Arithmetic, all fp32 (-ffp-contract=off: only the fmaf written here fuse).  The workgroup builds cos / sin of the H row
// angles and the W column angles once, in LDS, as sincospif(2 y' / H) with y' = y for 2 y <= H and y - H beyond (the
// argument lies in (-1, 1]: its one rounding is the only error in front of an exactly reduced sincospif).  Per element
//     cd = fmaf(ca, cb, -(sa * sb)),  sd = fmaf(sa, cb, ca * sb)                     the angle sum, from the tables
//     S += v;  X = fmaf(v, w, X) for the six weighted sums                            in the lane's element order
// then a butterfly over the lanes of the plane (__shfl_xor, offsets min(G, 64) / 2 ... 1) and, for G > 64, the waves'
// partials added in ascending wave order by every lane from LDS.  No atomics: the order is fixed by (P) alone, so a
// plane's bits depend on that plane's values and nothing else (not on n, c, B, the dtype's neighbours or the run).
//     t = S;  t = fmaf(A_c, ca, t); ... t = fmaf(D_s, sd, t);  out = fmaf(k, t, v),  k = (s - 1) / P rounded once from double
// and out is rounded once more at the store (to fp16 / bf16; not at all for fp32).
//
// K_s -- roundings from an input value to a stored skip-plane value, in units of 2^-24 (freeu_rounding_counts in _lib.py):
//   R = 8 * ceil(ceil(P / 8) / G)     the lane's fmaf chain (its first element passes through every later one)
//     + log2(min(G, 64))              butterfly additions
//     + G / 64 if G > 64 else 0       the waves' partials
//   is the chain of one SUM.  Each rounding is relative to a partial sum of at most sum|v|, so a sum is off by at most
//   (R + W) 2^-24 sum|v|, W the error of its weight: a table entry is off by at most T = 6 (pi / 2 from the argument's
//   rounding, 4 for two ulp of sincospif), so W = 0 for S, 6 for the A and B sums and 2 sqrt(2) T + 2 < 19 for the D sums:
//   the seven W add up to 62.  The store side multiplies the sums by the same weights (62 again), adds seven terms with six
//   fmaf on partial sums of at most 7 sum|v| (42), scales by k (7) and rounds out = v + ... once (1 on |v|, 7 on the sum).
//   Against the tests' form  K_s 2^-24 (|v| + |s - 1| * 4 * sum|v| / P):
//       K_s = ceil((7 R + 180) / 4) + 1                 (180 = 62 + 62 + 42 + 7 + 7; + 1 for the second-order terms)
//   e.g. 8 x 8: R = 12, K_s = 67;  64 x 64: R = 26, K_s = 92;  128 x 128: R = 38, K_s = 113.
//
// The backbone planes c < C_h / 2 are out = v * g, one fp32 product rounded once at the store.  Version 1: g = b.  Version
// 2 (the original repository's current form): two launches in front,
//     freeu_mean_kernel    m[n, p] = mean over c < C_h: 64 pixels x 16 channel lanes per workgroup; lane j adds the channels
//                          j, j + 16, ... in ascending order, the 16 partials are added in ascending order, one division
//     freeu_minmax_kernel  min / max of m per sample (NaN propagates), one workgroup per sample
// into ws (m: B * P floats, then min, max per sample), and the apply launch forms
//     g = fmaf(b - 1, (m - min) / (max - min), 1)         and g = 1 where max == min (the original divides 0 by 0).
// K_m -- roundings from an input value to m: ceil(C_h / 16) - 1 additions in the lane, 15 across lanes, one division:
//     K_m = ceil(C_h / 16) + 15.
// The planes C_h / 2 <= c < C_h get no work item; neither do the skip planes when s == 1 nor the backbone planes of
// version 1 when b == 1: those bytes are never written.
#include "common.h"
#include "step_core.h"


namespace {

constexpr int FREEU_MAX_PLANE = 16384;
constexpr int CHUNK = 8;                        // elements of a chunk
constexpr int WG_MIN = 256;                     // threads of a workgroup of the G <= 256 forms
constexpr int MEAN_PIX = 64, MEAN_LANES = 16;   // freeu_mean_kernel's workgroup: pixels x channel lanes
// H + W is largest for 2 x 8192: the only shape whose tables pass 64 KiB (and need the attribute below)
constexpr int FREEU_LDS_MAX = (FREEU_MAX_PLANE / 2 + 2) * (int)sizeof(float2) + 7 * 16 * (int)sizeof(float);

// lanes that own a plane of P elements (the table in the header)
inline int lanes_of(int64_t P) { return P <= 256 ? 16 : (P <= 2048 ? 64 : (P <= 8192 ? 256 : 1024)); }

struct Apply {
    int64_t C, C_h, n_back, n_skip, items;      // channels of a sample; backbone / skip planes WITH work; B * (n_back + n_skip)
    int H, W, P, version, vec;
    float b, b1, k;                             // b; b - 1 and (s - 1) / P, each rounded once from double
    const float *m, *mm;                        // version 2: the mean map (B, P) and (min, max) per sample
};

template <typename T>
__device__ __forceinline__ void load8(const T *p, int n, bool vec, float *v) {
    constexpr int N = 16 / sizeof(T);           // step_core.h's chunk: 8 16-bit elements or 4 fp32
#pragma unroll
    for (int h = 0; h < CHUNK / N; ++h) {
        const int nh = n - h * N;
        if (vec && nh >= N) vtm::load_chunk<T, true>(p + h * N, N, v + h * N);
        else vtm::load_chunk<T, false>(p + h * N, nh, v + h * N);
    }
}

template <typename T>
__device__ __forceinline__ void store8(T *p, int n, bool vec, const float *v) {
    constexpr int N = 16 / sizeof(T);
#pragma unroll
    for (int h = 0; h < CHUNK / N; ++h) {
        const int nh = n - h * N;
        if (vec && nh >= N) vtm::store_chunk<T, true>(p + h * N, N, v + h * N);
        else vtm::store_chunk<T, false>(p + h * N, nh, v + h * N);
    }
}

__device__ __forceinline__ float nan_min(float a, float b) { return (a != a || a < b) ? a : b; }
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || a > b) ? a : b; }

template <typename T, int G>
__global__ __launch_bounds__(G > WG_MIN ? G : WG_MIN) void freeu_apply_kernel(T *__restrict__ x, Apply a) {
    constexpr int NT = G > WG_MIN ? G : WG_MIN;             // threads of the workgroup
    constexpr int CPL = (G == 16 || G == 1024) ? 2 : 4;     // chunks a lane holds at most
    constexpr int WAVES = G > 64 ? G / 64 : 1;              // waves that share a plane
    extern __shared__ __attribute__((aligned(16))) float2 tab[];
    float2 *tH = tab, *tW = tab + a.H;
    float *part = reinterpret_cast<float *>(tab + a.H + a.W);   // [7][WAVES], G > 64 only
    const int tid = threadIdx.x, lane = tid % G;

    if (a.n_skip > 0) {
        for (int i = tid; i < a.H + a.W; i += NT) {
            const int n = i < a.H ? a.H : a.W, j = i < a.H ? i : i - a.H;
            const float arg = (float)(2 * (2 * j <= n ? j : j - n)) / (float)n;
            float sn, cs;
            sincospif(arg, &sn, &cs);
            tab[i] = make_float2(cs, sn);
        }
    }
    __syncthreads();
    const int64_t item = (int64_t)blockIdx.x * (NT / G) + tid / G;
    if (item >= a.items) return;                            // (whole lane groups of the last workgroup; G > 64: nobody)
    const int64_t per = a.n_back + a.n_skip, n = item / per, r = item - n * per;
    const bool skip = r >= a.n_back;
    const int64_t c = skip ? a.C_h + (r - a.n_back) : r;
    T *px = x + (n * a.C + c) * a.P;
    const int P = a.P;
    const bool vec = a.vec != 0;

    float v[CPL][CHUNK];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int i0 = (lane + j * G) * CHUNK;
        if (i0 < P) load8<T>(px + i0, min(CHUNK, P - i0), vec, v[j]);
    }

    if (!skip) {
        float lo = 0.0f, d = 0.0f;
        const float *mrow = nullptr;
        if (a.version == 2) {
            lo = a.mm[2 * n];
            d = a.mm[2 * n + 1] - lo;
            mrow = a.m + n * P;
        }
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int i0 = (lane + j * G) * CHUNK;
            if (i0 >= P) continue;
            const int nv = min(CHUNK, P - i0);
#pragma unroll
            for (int e = 0; e < CHUNK; ++e) {
                float g = a.b;
                if (a.version == 2) g = (e < nv && d != 0.0f) ? __builtin_fmaf(a.b1, (mrow[i0 + e] - lo) / d, 1.0f) : 1.0f;
                v[j][e] = v[j][e] * g;
            }
            store8<T>(px + i0, nv, vec, v[j]);
        }
        return;
    }

    // pass 1: the seven sums, in the lane's element order
    float acc[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int i0 = (lane + j * G) * CHUNK;
        if (i0 >= P) continue;
        const int nv = min(CHUNK, P - i0);
        int y = i0 / a.W, xx = i0 - y * a.W;
#pragma unroll
        for (int e = 0; e < CHUNK; ++e) {
            if (e < nv) {
                const float2 ta = tH[y], tb = tW[xx];
                const float cd = __builtin_fmaf(ta.x, tb.x, -(ta.y * tb.y)), sd = __builtin_fmaf(ta.y, tb.x, ta.x * tb.y);
                const float val = v[j][e];
                acc[0] = acc[0] + val;
                acc[1] = __builtin_fmaf(val, ta.x, acc[1]);
                acc[2] = __builtin_fmaf(val, ta.y, acc[2]);
                acc[3] = __builtin_fmaf(val, tb.x, acc[3]);
                acc[4] = __builtin_fmaf(val, tb.y, acc[4]);
                acc[5] = __builtin_fmaf(val, cd, acc[5]);
                acc[6] = __builtin_fmaf(val, sd, acc[6]);
                if (++xx == a.W) { xx = 0; ++y; }
            }
        }
    }
    // the lanes of the plane inside a wave (a lane group is never split: every lane of it got here)
#pragma unroll
    for (int off = (G < 64 ? G : 64) / 2; off >= 1; off >>= 1) {
#pragma unroll
        for (int q = 0; q < 7; ++q) acc[q] = acc[q] + __shfl_xor(acc[q], off, G < 64 ? G : 64);
    }
    if constexpr (WAVES > 1) {
        // one plane per workgroup: every thread is here, the barriers are uniform
        if ((tid & 63) == 0) {
#pragma unroll
            for (int q = 0; q < 7; ++q) part[q * WAVES + tid / 64] = acc[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            float t = part[q * WAVES];
            for (int w = 1; w < WAVES; ++w) t = t + part[q * WAVES + w];
            acc[q] = t;
        }
    }

    // pass 2: the projection on the four bins, added with weight k
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int i0 = (lane + j * G) * CHUNK;
        if (i0 >= P) continue;
        const int nv = min(CHUNK, P - i0);
        int y = i0 / a.W, xx = i0 - y * a.W;
#pragma unroll
        for (int e = 0; e < CHUNK; ++e) {
            if (e < nv) {
                const float2 ta = tH[y], tb = tW[xx];
                const float cd = __builtin_fmaf(ta.x, tb.x, -(ta.y * tb.y)), sd = __builtin_fmaf(ta.y, tb.x, ta.x * tb.y);
                float t = acc[0];
                t = __builtin_fmaf(acc[1], ta.x, t);
                t = __builtin_fmaf(acc[2], ta.y, t);
                t = __builtin_fmaf(acc[3], tb.x, t);
                t = __builtin_fmaf(acc[4], tb.y, t);
                t = __builtin_fmaf(acc[5], cd, t);
                t = __builtin_fmaf(acc[6], sd, t);
                v[j][e] = __builtin_fmaf(a.k, t, v[j][e]);
                if (++xx == a.W) { xx = 0; ++y; }
            }
        }
        store8<T>(px + i0, nv, vec, v[j]);
    }
}

// m[n, p] = mean over c < C_h of x[n, c, p]: 64 pixels x 16 channel lanes; grid: B * tiles
template <typename T>
__global__ __launch_bounds__(MEAN_PIX *MEAN_LANES) void freeu_mean_kernel(const T *__restrict__ x, int64_t C, int64_t C_h, int P,
                                                                           int tiles, float *__restrict__ m) {
    __shared__ float part[MEAN_LANES][MEAN_PIX];
    const int pix = threadIdx.x % MEAN_PIX, cl = threadIdx.x / MEAN_PIX;
    const int64_t n = blockIdx.x / tiles;
    const int p = (int)(blockIdx.x % tiles) * MEAN_PIX + pix;
    float acc = 0.0f;
    if (p < P) {
        const T *col = x + n * C * P + p;
        for (int64_t c = cl; c < C_h; c += MEAN_LANES) acc = acc + vtm::to_f32(col[c * P]);
    }
    part[cl][pix] = acc;
    __syncthreads();
    if (cl == 0 && p < P) {
        float t = part[0][pix];
        for (int j = 1; j < MEAN_LANES; ++j) t = t + part[j][pix];
        m[n * P + p] = t / (float)C_h;
    }
}

// (min, max) over the P entries of a sample's map; NaN propagates (torch's amin / amax); grid: B
__global__ __launch_bounds__(256) void freeu_minmax_kernel(const float *__restrict__ m, int P, float *__restrict__ mm) {
    __shared__ float lo_s[4], hi_s[4];
    const float *row = m + (int64_t)blockIdx.x * P;
    float lo = row[0], hi = lo;
    for (int p = threadIdx.x; p < P; p += 256) {
        const float t = row[p];
        lo = nan_min(lo, t);
        hi = nan_max(hi, t);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        lo = nan_min(lo, __shfl_xor(lo, off, 64));
        hi = nan_max(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        lo_s[threadIdx.x / 64] = lo;
        hi_s[threadIdx.x / 64] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            lo = nan_min(lo, lo_s[w]);
            hi = nan_max(hi, hi_s[w]);
        }
        mm[2 * blockIdx.x] = lo;
        mm[2 * blockIdx.x + 1] = hi;
    }
}

template <typename T, int G>
int launch_apply(void *x, const Apply &a, hipStream_t s) {
    constexpr int NT = G > WG_MIN ? G : WG_MIN;
    const int lds = (a.H + a.W) * (int)sizeof(float2) + (G > 64 ? 7 * (G / 64) * (int)sizeof(float) : 0);
    if (lds > 64 * 1024) {
        const hipError_t e = vtm::opt_in_lds<freeu_apply_kernel<T, G>, FREEU_LDS_MAX>();
        if (e != hipSuccess) return vtm::fail(VTM_ELAUNCH, "vtm_freeu: LDS attribute: %s", hipGetErrorString(e));
    }
    const int64_t blocks = vtm::cdiv(a.items, NT / G);
    hipLaunchKernelGGL((freeu_apply_kernel<T, G>), dim3((unsigned)blocks), dim3(NT), lds, s, (T *)x, a);
    return vtm::launch_status("vtm_freeu");
}

inline size_t ws_bytes_of(int64_t B, int64_t P, int version) {
    return version == 2 && B > 0 && P > 0 ? (size_t)(B * P + 2 * B) * sizeof(float) : 0;
}

}  // namespace

VTM_EXPORT int vtm_freeu_lanes(int64_t P) { return P >= 4 && P <= FREEU_MAX_PLANE ? lanes_of(P) : 0; }

VTM_EXPORT size_t vtm_freeu_ws_bytes(int64_t B, int64_t P, int version) {
    return P <= FREEU_MAX_PLANE && B <= (int64_t)1 << 31 ? ws_bytes_of(B, P, version) : 0;
}

VTM_EXPORT int vtm_freeu(void *x, int dtype, int64_t B, int64_t C_h, int64_t C_s, int64_t H, int64_t W, float b, float s,
                         int version, void *ws, size_t ws_bytes, vtm_stream_t stream) {
    const char *who = "vtm_freeu";
    const int64_t LIM = ((int64_t)1 << 31) - 1;
    VTM_REQUIRE(dtype == VTM_F32 || dtype == VTM_F16 || dtype == VTM_BF16, "%s: unsupported dtype %d", who, dtype);
    VTM_REQUIRE(version == 1 || version == 2, "%s: version = %d, 1 (Diffusers) or 2 (the original repository) is taken", who,
                version);
    const int64_t es = dtype == VTM_F32 ? 4 : 2;
    VTM_REQUIRE(x != nullptr && reinterpret_cast<uintptr_t>(x) % es == 0, "%s: x is required, aligned to its element size", who);
    VTM_REQUIRE(B >= 0, "%s: B = %lld", who, (long long)B);
    VTM_REQUIRE(H >= 2 && W >= 2 && H <= FREEU_MAX_PLANE && W <= FREEU_MAX_PLANE && H * W <= FREEU_MAX_PLANE,
                "%s: H = %lld, W = %lld: H, W >= 2 and a plane of at most %d elements are taken", who, (long long)H,
                (long long)W, FREEU_MAX_PLANE);
    VTM_REQUIRE(C_h >= 2 && C_s >= 1, "%s: C_h = %lld, C_s = %lld: C_h >= 2 and C_s >= 1 are taken", who, (long long)C_h,
                (long long)C_s);
    const int64_t P = H * W;
    const int G = lanes_of(P), per_wg = (G > WG_MIN ? G : WG_MIN) / G;
    // the largest grid any (b, s) gives: the launches of a shape do not depend on the factors' values for this check
    VTM_REQUIRE(B <= LIM && C_h <= LIM && C_s <= LIM && (C_h / 2 + C_s) <= LIM * per_wg / (B > 0 ? B : 1)
                    && B * vtm::cdiv(P, MEAN_PIX) <= LIM,
                "%s: B = %lld samples of %lld + %lld planes: the grid would exceed 2^31 - 1 workgroups", who, (long long)B,
                (long long)(C_h / 2), (long long)C_s);
    const size_t need = ws_bytes_of(B, P, version);
    VTM_REQUIRE(need == 0 || (ws != nullptr && ws_bytes >= need && reinterpret_cast<uintptr_t>(ws) % sizeof(float) == 0),
                "%s: version 2 needs a 4-byte aligned workspace of %zu bytes (ws_bytes = %zu)", who, need, ws_bytes);
    if (B == 0) return VTM_OK;

    hipStream_t st = vtm::as_stream(stream);
    Apply a{};
    a.C = C_h + C_s, a.C_h = C_h;
    a.n_back = (version == 1 && b == 1.0f) ? 0 : C_h / 2;       // identities get no work item: their bytes are not written
    a.n_skip = s == 1.0f ? 0 : C_s;
    a.items = B * (a.n_back + a.n_skip);
    a.H = (int)H, a.W = (int)W, a.P = (int)P, a.version = version;
    a.vec = vtm::aligned16(x) && (P * es) % 16 == 0;
    a.b = b, a.b1 = (float)((double)b - 1.0), a.k = (float)(((double)s - 1.0) / (double)P);
    if (a.items == 0) return VTM_OK;
    return vtm::with_dtype(dtype, who, [&](auto t) {
        using T = decltype(t);
        if (version == 2 && a.n_back > 0) {
            float *m = (float *)ws, *mm = m + B * P;
            const int tiles = (int)vtm::cdiv(P, MEAN_PIX);
            hipLaunchKernelGGL(freeu_mean_kernel<T>, dim3((unsigned)(B * tiles)), dim3(MEAN_PIX * MEAN_LANES), 0, st,
                               (const T *)x, a.C, C_h, (int)P, tiles, m);
            hipLaunchKernelGGL(freeu_minmax_kernel, dim3((unsigned)B), dim3(256), 0, st, (const float *)m, (int)P, mm);
            if (int rc = vtm::launch_status(who)) return rc;
            a.m = m, a.mm = mm;
        }
        switch (G) {
            case 16: return launch_apply<T, 16>(x, a, st);
            case 64: return launch_apply<T, 64>(x, a, st);
            case 256: return launch_apply<T, 256>(x, a, st);
            default: return launch_apply<T, 1024>(x, a, st);
        }
    });
}
