// vtm_sag_degrade: the degrade step of self-attention guidance for one chunk in one launch -- threshold the per-key attention
// mass of the mid block (vtm_attention_key_mass), upsample that mask nearest-neighbour to the latent grid, predict the clean
// sample x0 and the noise eps from x_t and one group's model output (step_core.h's predict), blur x0 with a
// (2 r + 1)^2 Gaussian inside the mask, and re-noise: out = sqrt_alpha * (mask ? blur(x0) : x0) + sqrt_beta * eps.
//
// One workgroup owns one (frame, channel) plane, as groupnorm.hip keeps a group: x0 of the plane goes to LDS (plane A), a
// horizontal pass writes plane B, the vertical pass reads plane B and stores.  Everything is fp32; a blurred value is
// fmaf(tap[k], value[k], acc) over k = 0 .. 2 r in ascending order from acc = 0, with torch's "reflect" padding (the edge
// is not repeated); eps is recomputed at the store (it is two operations on values the thread loads anyway) and each stored
// value is rounded once.  The mask SELECTS: where it is off x0 goes through untouched, so a NaN / Inf next to the mask
// reaches exactly the pixels whose blur window holds it.
// One launch, no workspace, no atomics: a plane's bits depend on that plane's operands alone.
#include "common.h"
#include "step_core.h"

namespace {

constexpr int SAG_MAX_R = 4;                    // taps: 2 r + 1 <= 9
constexpr int SAG_MAX_PLANE = 16384;            // H * W: two fp32 planes are 128 KiB of the CU's 160 KiB of LDS
constexpr int SAG_LDS_MAX = 2 * SAG_MAX_PLANE * (int)sizeof(float);

struct Degrade {
    int pred, r, H, W, h_m, w_m;
    float sqrt_alpha, sqrt_beta, threshold;
    float taps[2 * SAG_MAX_R + 1];
};

// torch's "reflect": -1 -> 1, n -> n - 2 (n > r makes one fold enough)
__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// step_core.h's predict(), for the pass that needs the clean sample alone and for the store, which needs the noise alone
__device__ __forceinline__ float predict_x0(const Degrade &g, float xv, float m) {
    float x0, eps;
    vtm::predict(g.pred, g.sqrt_alpha, g.sqrt_beta, xv, m, x0, eps);
    return x0;
}
__device__ __forceinline__ float predict_eps(const Degrade &g, float xv, float m) {
    float x0, eps;
    vtm::predict(g.pred, g.sqrt_alpha, g.sqrt_beta, xv, m, x0, eps);
    return eps;
}

template <typename T>
__global__ __launch_bounds__(1024) void sag_degrade_kernel(const T *__restrict__ x, const T *__restrict__ model_out,
                                                           const float *__restrict__ mass, int64_t ld_mass,
                                                           const int32_t *__restrict__ frame_ids, int C, Degrade g,
                                                           T *__restrict__ out, uint8_t *__restrict__ mask_out) {
    extern __shared__ __attribute__((aligned(16))) float plane[];
    const int HW = g.H * g.W, tid = threadIdx.x, NT = blockDim.x;
    float *sA = plane, *sB = plane + HW;
    const int64_t f = blockIdx.x / C, c = blockIdx.x % C;
    const int64_t row = frame_ids ? (int64_t)frame_ids[f] : f;
    const T *xp = x + (row * C + c) * HW, *mp = model_out + (f * C + c) * HW;
    T *op = out + (f * C + c) * HW;
    const float *mrow = mass + f * ld_mass;

    for (int i = tid; i < HW; i += NT) sA[i] = predict_x0(g, vtm::to_f32(xp[i]), vtm::to_f32(mp[i]));
    __syncthreads();
    for (int i = tid; i < HW; i += NT) {
        const int y = i / g.W, xx = i - y * g.W;
        const float *line = sA + y * g.W;
        float acc = 0.0f;
        for (int t = 0; t <= 2 * g.r; ++t) acc = __builtin_fmaf(g.taps[t], line[reflect(xx + t - g.r, g.W)], acc);
        sB[i] = acc;
    }
    __syncthreads();
    for (int i = tid; i < HW; i += NT) {
        const int y = i / g.W, xx = i - y * g.W;
        float acc = 0.0f;
        for (int t = 0; t <= 2 * g.r; ++t) acc = __builtin_fmaf(g.taps[t], sB[reflect(y + t - g.r, g.H) * g.W + xx], acc);
        // the nearest-neighbour source cell, in integers
        const bool on = mrow[(y * g.h_m / g.H) * g.w_m + xx * g.w_m / g.W] > g.threshold;
        const float ep = predict_eps(g, vtm::to_f32(xp[i]), vtm::to_f32(mp[i]));
        const float deg = on ? acc : sA[i];
        op[i] = vtm::from_f32<T>(g.sqrt_alpha * deg + g.sqrt_beta * ep);
        if (mask_out != nullptr && c == 0) mask_out[f * HW + i] = on ? 1 : 0;
    }
}

template <typename T>
int launch_degrade(const void *x, const void *model_out, const float *mass, int64_t ld_mass, const int32_t *frame_ids,
                   int64_t F, int64_t C, const Degrade &g, void *out, uint8_t *mask_out, hipStream_t s) {
    const int HW = g.H * g.W;
    const int lds = 2 * HW * (int)sizeof(float);
    if (lds > 64 * 1024) {
        const hipError_t e = vtm::opt_in_lds<sag_degrade_kernel<T>, SAG_LDS_MAX>();
        if (e != hipSuccess) return vtm::fail(VTM_ELAUNCH, "vtm_sag_degrade: LDS attribute: %s", hipGetErrorString(e));
    }
    // several planes per CU where the LDS allows: 256 threads up to 32 x 32 planes, else 1024
    const int threads = HW <= 64 ? 64 : (HW <= 4096 ? 256 : 1024);
    hipLaunchKernelGGL(sag_degrade_kernel<T>, dim3((unsigned)(F * C)), dim3(threads), lds, s, (const T *)x,
                       (const T *)model_out, mass, ld_mass, frame_ids, (int)C, g, (T *)out, mask_out);
    return vtm::launch_status("vtm_sag_degrade");
}

}  // namespace

VTM_EXPORT int vtm_sag_degrade(const void *x, int64_t n_rows, const int32_t *frame_ids, const void *model_out,
                               const float *mass, int64_t ld_mass, int64_t h_m, int64_t w_m, int dtype, int64_t F, int64_t C,
                               int64_t H, int64_t W, int pred_type, float sqrt_alpha, float sqrt_beta, const float *taps,
                               int r, float threshold, void *out, uint8_t *mask_out, vtm_stream_t stream) {
    const char *who = "vtm_sag_degrade";
    if (const int rc = vtm::check_dtype_pred(who, dtype, pred_type)) return rc;
    VTM_REQUIRE(x && model_out && mass && taps && out, "%s: x, model_out, mass, taps and out are required", who);
    VTM_REQUIRE(r >= 0 && r <= SAG_MAX_R, "%s: r = %d, a blur radius of 0 .. %d is taken", who, r, SAG_MAX_R);
    VTM_REQUIRE(F >= 0 && F <= (1 << 20) && C >= 1 && C <= (1 << 10) && H >= 1 && W >= 1 && n_rows >= (frame_ids ? 1 : F),
                "%s: bad sizes F = %lld, C = %lld, H = %lld, W = %lld, n_rows = %lld", who, (long long)F, (long long)C,
                (long long)H, (long long)W, (long long)n_rows);
    VTM_REQUIRE(H > r && W > r, "%s: reflect padding of radius %d needs H, W > %d (H = %lld, W = %lld)", who, r, r,
                (long long)H, (long long)W);
    VTM_REQUIRE(H <= SAG_MAX_PLANE && W <= SAG_MAX_PLANE && H * W <= SAG_MAX_PLANE,
                "%s: H * W = %lld, a plane of at most %d elements is taken (two fp32 planes of it live in LDS)", who,
                (long long)(H * W), SAG_MAX_PLANE);
    VTM_REQUIRE(h_m >= 1 && w_m >= 1 && h_m <= H && w_m <= W && ld_mass >= h_m * w_m,
                "%s: the mass grid (%lld, %lld) must lie inside (H, W) and ld_mass = %lld hold it", who, (long long)h_m,
                (long long)w_m, (long long)ld_mass);
    VTM_REQUIRE(sqrt_alpha == sqrt_alpha && sqrt_beta == sqrt_beta && threshold == threshold,
                "%s: sqrt_alpha, sqrt_beta and threshold must not be NaN", who);
    VTM_REQUIRE(vtm::rows_apart(out, F, x, n_rows, C * H * W, dtype), "%s: out overlaps x", who);
    if (F == 0) return VTM_OK;
    Degrade g{pred_type, r, (int)H, (int)W, (int)h_m, (int)w_m, sqrt_alpha, sqrt_beta, threshold, {}};
    for (int t = 0; t <= 2 * r; ++t) g.taps[t] = taps[t];
    hipStream_t st = vtm::as_stream(stream);
    return vtm::with_dtype(dtype, who, [&](auto t) {
        return launch_degrade<decltype(t)>(x, model_out, mass, ld_mass, frame_ids, F, C, g, out, mask_out, st);
    });
}
