// vtm_semantic_guidance: semantic guidance (SEGA, Brack et al.; Diffusers' SemanticStableDiffusionPipeline, and with region
// masks the masked form of LEditsPPPipelineStableDiffusion) for one chunk in one launch -- per edit concept e the term
// g_e = scale[e] * (model_out[group[e]] - u), kept where |g_e| (or its sum over the channels) reaches a quantile of its
// plane, the weighted sum of the kept terms added to the classifier-free combination, and the momentum buffer read, applied
// and updated in place.  The contract is stated in include/vidtome_hip.h; this header says how the kernel keeps it.
//
// Shape.  One workgroup owns one (frame, channel) plane of P = H W values (64 threads up to P = 64, 256 up to 1024, else
// 1024: a launch is F C workgroups, 64 for a chunk of 16 latent frames, on 256 CUs, and each is a chain of barriers, so the
// plane is spread over as many lanes as a workgroup has -- measured at 16 x 4 x 64 x 64, fp16: 41 / 63 us for one / three
// channel concepts with 1024 threads against 54 / 96 us with 256), in two phases:
//   1  per live concept with a quantile: the population a_e goes to LDS as fp32 bit patterns with the sign bit cleared
//      (non-negative floats order as unsigned integers; a NaN's pattern lies above +inf's, so NaNs take the HIGHEST ranks,
//      where np.sort puts them); a most-significant-digit-first radix select, four passes of 8 bits over an LDS histogram,
//      finds the value of rank rank_lo exactly; one more sweep counts the values <= a_lo and takes the minimum above a_lo,
//      which gives the value of rank min(rank_lo + 1, P - 1) without a second selection; thr goes to LDS (6 floats).
//   2  one sweep over the plane: every g_e is recomputed with the same uncontracted operations (so it has the bits phase 1
//      ranked), compared with thr, summed, and out / momentum / mask_out are written -- each element exactly once.
// Recomputing g_e costs a second read of model_out, which the L2 holds (a chunk of 16 frames at 64 x 64 with 8 groups is
// 4 MiB in fp16); the alternative, keeping the two running sums of a plane in LDS between concepts, needs two more planes
// (192 KiB at P = 16384: more than a CU has).  In the SUM modes each of a frame's C workgroups recomputes the frame's channel
// sum and selects on it: C is 4 for latents, and C separate selections of one population give the same bits by construction,
// so no workgroup waits for another and no workspace is needed.
//
// LDS.  hist | sel | thr | population: 8 KiB + 64 B + P fp32, 72.1 KiB at the limit P = 16384 of the CU's 160 KiB (two
// workgroups per CU there; what bounds a launch is its F C workgroups on 256 CUs, not the occupancy).
// Histogram.  An LDS atomic of several lanes on ONE address is serialised, and the first pass (the exponent's high bits)
// sends almost a whole plane to two or three bins.  So every bin has HIST_COPIES = 8 counters, lane l adds to copy l & 7, and
// the copies of a bin are neighbours (hist[bin * 8 + copy]): the 8 counters of a hot bin lie in 8 different banks, a wave's
// worst case is an 8-way serialisation instead of a 64-way one.  More copies were not tried: 8 keep the scan of wave 0 at
// 32 LDS reads per lane.  Integer atomics only: their result does not depend on the order, so a plane's bits depend on its
// own frame's values alone.
// Arithmetic.  Everything that decides the mask -- d_e, g_e, the channel sum, thr -- is written with __fsub_rn / __fmul_rn /
// __fadd_rn / __dmul_rn / __dadd_rn, which no flag can contract; the rest is plain fp32 in the order of the contract
// (the library is built with -ffp-contract=off).
// One launch, no workspace, no global atomics.
#include "common.h"
#include "step_core.h"

#include <cmath>

namespace {

using vtm::from_f32;
using vtm::to_f32;

constexpr int MAX_E = VTM_SEGA_MAX_CONCEPTS;
constexpr int MAX_PLANE = VTM_SEGA_MAX_PLANE;
constexpr int HIST_BINS = 256, HIST_COPIES = 8;
constexpr int HIST_WORDS = HIST_BINS * HIST_COPIES;
constexpr int SEL_WORDS = 8, THR_WORDS = 8;                        // sel: digit, rank, count, minimum; thr: MAX_E floats
constexpr int HEAD_WORDS = HIST_WORDS + SEL_WORDS + THR_WORDS;
constexpr int LDS_MAX = (HEAD_WORDS + MAX_PLANE) * 4;

struct Sega {
    int n;                                    // live concepts (a weight is not 0), ascending in e
    int g_uncond, g_cond, mom_apply;
    float s, mom_scale, mom_beta;
    int orig[MAX_E];                          // the concept's index e: its rows of regions and mask_out
    int group[MAX_E], mode[MAX_E], rank_lo[MAX_E];
    float scale[MAX_E], w_apply[MAX_E], w_acc[MAX_E];
    double rank_frac[MAX_E];
};

__device__ __forceinline__ bool has_quantile(int mode) { return mode != VTM_SEGA_REGION; }
__device__ __forceinline__ bool has_region(int mode) { return mode >= VTM_SEGA_REGION; }
__device__ __forceinline__ bool is_sum(int mode) { return mode == VTM_SEGA_SUM || mode == VTM_SEGA_SUM_REGION; }

// g_e of one element: one subtraction, one product
template <typename T>
__device__ __forceinline__ float edit_term(const T *e, const T *u, int i, float scale) {
    return __fmul_rn(scale, __fsub_rn(to_f32(e[i]), to_f32(u[i])));
}

// a_e of pixel i: |g_e| of the plane's own channel, or the sum of |g_e| over the frame's channels, ascending from 0.
// e0 / u0 point at channel 0 of the frame in the concept's and the unconditional group.
template <typename T>
__device__ __forceinline__ float magnitude(const T *e0, const T *u0, int ch, int C, int P, int i, float scale, bool sum) {
    if (!sum) return fabsf(edit_term(e0 + (int64_t)ch * P, u0 + (int64_t)ch * P, i, scale));
    float a = 0.0f;
    for (int c = 0; c < C; ++c) a = __fadd_rn(a, fabsf(edit_term(e0 + (int64_t)c * P, u0 + (int64_t)c * P, i, scale)));
    return a;
}

// The value of rank `rank` (ascending, 0-based) of pop[0 .. P): four 8-bit digits, most significant first.  Every thread of
// the workgroup calls it and gets the value.  hist: HIST_WORDS words; sel: 2 words.
__device__ __forceinline__ uint32_t radix_select(const uint32_t *pop, int P, int rank, uint32_t *hist, uint32_t *sel) {
    const int tid = threadIdx.x, NT = blockDim.x;
    uint32_t prefix = 0, known = 0;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int k = tid; k < HIST_WORDS; k += NT) hist[k] = 0;
        __syncthreads();
        for (int i = tid; i < P; i += NT) {
            const uint32_t v = pop[i];
            if ((v & known) == prefix) atomicAdd(&hist[((v >> shift) & 255u) * HIST_COPIES + (tid & (HIST_COPIES - 1))], 1u);
        }
        __syncthreads();
        if (tid < 64) {                                            // wave 0: lane l owns bins 4 l .. 4 l + 3
            uint32_t c[4], mine = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c[j] = 0;
#pragma unroll
                for (int k = 0; k < HIST_COPIES; ++k) c[j] += hist[(tid * 4 + j) * HIST_COPIES + k];
                mine += c[j];
            }
            uint32_t incl = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t up = __shfl_up(incl, o, 64);
                if (tid >= o) incl += up;
            }
            uint32_t below = incl - mine;                          // the values in the bins before this lane's
            if (below <= (uint32_t)rank && (uint32_t)rank < incl) {    // exactly one lane: rank < the pass's total
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if ((uint32_t)rank >= below && (uint32_t)rank < below + c[j]) {
                        sel[0] = (uint32_t)(tid * 4 + j);
                        sel[1] = (uint32_t)rank - below;
                    }
                    below += c[j];
                }
            }
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        known |= 255u << shift;
        rank = (int)sel[1];
    }
    return prefix;
}

template <typename T>
__global__ __launch_bounds__(1024) void semantic_kernel(const T *__restrict__ model_out, int64_t F, int C, int P, Sega s,
                                                        const uint8_t *__restrict__ regions, float *momentum,
                                                        const int32_t *__restrict__ frame_ids, T *__restrict__ out,
                                                        uint8_t *__restrict__ mask_out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t *hist = lds, *sel = lds + HIST_WORDS, *pop = lds + HEAD_WORDS;
    float *thr = reinterpret_cast<float *>(lds + HIST_WORDS + SEL_WORDS);
    const int tid = threadIdx.x, NT = blockDim.x;
    const int64_t f = blockIdx.x / C;
    const int ch = (int)(blockIdx.x % C);
    const int64_t frame = (int64_t)C * P;                          // elements of one frame
    const T *u0 = model_out + ((int64_t)s.g_uncond * F + f) * frame;

    // phase 1: thr of every live concept that has a quantile
#pragma unroll 1
    for (int e = 0; e < s.n; ++e) {
        if (!has_quantile(s.mode[e])) continue;
        const T *e0 = model_out + ((int64_t)s.group[e] * F + f) * frame;
        const float scale = s.scale[e];
        const bool sum = is_sum(s.mode[e]);
        for (int i = tid; i < P; i += NT) pop[i] = __float_as_uint(magnitude(e0, u0, ch, C, P, i, scale, sum)) & 0x7fffffffu;
        if (tid == 0) {
            sel[2] = 0;                                            // the count of values <= a_lo
            sel[3] = 0xffffffffu;                                  // the minimum above a_lo
        }
        const int rank = s.rank_lo[e];
        const uint32_t lo = radix_select(pop, P, rank, hist, sel);     // (its first barrier orders the writes above)
        uint32_t count = 0, above = 0xffffffffu;
        for (int i = tid; i < P; i += NT) {
            const uint32_t v = pop[i];
            count += v <= lo ? 1u : 0u;
            above = v > lo && v < above ? v : above;
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            count += __shfl_xor(count, o, 64);
            const uint32_t other = __shfl_xor(above, o, 64);
            above = other < above ? other : above;
        }
        if ((tid & 63) == 0) {
            atomicAdd(&sel[2], count);
            atomicMin(&sel[3], above);
        }
        __syncthreads();
        const int rank_hi = rank + 1 < P - 1 ? rank + 1 : P - 1;
        const uint32_t hi = (uint32_t)rank_hi < sel[2] ? lo : sel[3];
        if (tid == 0) {
            const double a_lo = (double)__uint_as_float(lo), a_hi = (double)__uint_as_float(hi);
            thr[e] = (float)__dadd_rn(a_lo, __dmul_rn(s.rank_frac[e], __dsub_rn(a_hi, a_lo)));
        }
        __syncthreads();                                           // thr[e] is written; pop and sel are free again
    }

    // phase 2: the plane, each element once
    const int64_t row = frame_ids ? (int64_t)frame_ids[f] : f;
    const T *up = u0 + (int64_t)ch * P;
    const T *cp = s.g_cond >= 0 ? model_out + (((int64_t)s.g_cond * F + f) * C + ch) * P : nullptr;
    float *nup = momentum ? momentum + (row * C + ch) * P : nullptr;
    T *op = out + (f * C + ch) * P;
    const float keep = 1.0f - s.mom_beta;
    for (int i = tid; i < P; i += NT) {
        const float u = to_f32(up[i]);
        float app = 0.0f, acc = 0.0f;
#pragma unroll 1
        for (int e = 0; e < s.n; ++e) {
            const int mode = s.mode[e];
            const float scale = s.scale[e];
            const T *e0 = model_out + ((int64_t)s.group[e] * F + f) * frame;
            const float g = edit_term(e0 + (int64_t)ch * P, up, i, scale);
            bool on = true;
            if (has_quantile(mode)) {
                const float a = is_sum(mode) ? magnitude(e0, u0, ch, C, P, i, scale, true) : fabsf(g);
                on = a >= thr[e];                                  // false for a NaN on either side
            }
            if (has_region(mode)) on = on && regions[((int64_t)s.orig[e] * F + f) * P + i] != 0;
            if (on) {
                if (s.w_apply[e] != 0.0f) app = app + s.w_apply[e] * g;
                if (s.w_acc[e] != 0.0f) acc = acc + s.w_acc[e] * g;
            }
            if (mask_out) mask_out[(((int64_t)s.orig[e] * F + f) * C + ch) * P + i] = on ? 1 : 0;
        }
        float m = u;
        if (cp) m = u + s.s * (to_f32(cp[i]) - u);
        m = m + app;
        if (nup) {
            const float nu = nup[i];
            if (s.mom_apply) m = m + s.mom_scale * nu;
            nup[i] = s.mom_beta * nu + keep * acc;
        }
        op[i] = from_f32<T>(m);
    }
}

template <typename T>
int launch_semantic(const void *model_out, int64_t F, int64_t C, int P, const Sega &s, const uint8_t *regions, float *momentum,
                    const int32_t *frame_ids, void *out, uint8_t *mask_out, hipStream_t st) {
    const int lds = (HEAD_WORDS + P) * 4;
    if (lds > 64 * 1024) {
        const hipError_t e = vtm::opt_in_lds<semantic_kernel<T>, LDS_MAX>();
        if (e != hipSuccess) return vtm::fail(VTM_ELAUNCH, "vtm_semantic_guidance: LDS attribute: %s", hipGetErrorString(e));
    }
    const int threads = P <= 64 ? 64 : (P <= 1024 ? 256 : 1024);
    hipLaunchKernelGGL(semantic_kernel<T>, dim3((unsigned)(F * C)), dim3(threads), lds, st, (const T *)model_out, F, (int)C, P, s,
                       regions, momentum, frame_ids, (T *)out, mask_out);
    return vtm::launch_status("vtm_semantic_guidance");
}

}  // namespace

VTM_EXPORT int vtm_semantic_guidance(const void *model_out, int dtype, int64_t F, int64_t C, int64_t H, int64_t W,
                                     int64_t groups, int64_t g_uncond, int64_t g_cond, float guidance_scale,
                                     int64_t n_concepts, const int32_t *group, const float *scale, const int32_t *rank_lo,
                                     const double *rank_frac, const float *w_apply, const float *w_acc, const int32_t *mode,
                                     const uint8_t *regions, float *momentum, int64_t n_rows, const int32_t *frame_ids,
                                     float mom_scale, float mom_beta, int mom_apply, void *out, uint8_t *mask_out,
                                     vtm_stream_t stream) {
    const char *who = "vtm_semantic_guidance";
    VTM_REQUIRE(dtype == VTM_F32 || dtype == VTM_F16 || dtype == VTM_BF16, "%s: unsupported dtype %d", who, dtype);
    VTM_REQUIRE(model_out && out, "%s: model_out and out are required", who);
    VTM_REQUIRE(F >= 0 && F <= (1 << 20) && C >= 1 && C <= (1 << 10) && H >= 1 && W >= 1,
                "%s: bad sizes F = %lld, C = %lld, H = %lld, W = %lld", who, (long long)F, (long long)C, (long long)H,
                (long long)W);
    VTM_REQUIRE(H <= MAX_PLANE && W <= MAX_PLANE && H * W <= MAX_PLANE,
                "%s: H * W = %lld, a plane of at most %d elements is taken (it lives in LDS as the ranked population)", who,
                (long long)(H * W), MAX_PLANE);
    VTM_REQUIRE(n_concepts >= 0 && n_concepts <= MAX_E, "%s: n_concepts = %lld (0 .. %d)", who, (long long)n_concepts, MAX_E);
    VTM_REQUIRE(groups >= 1 && groups <= VTM_SOLVER_MAX_GROUPS && g_uncond >= 0 && g_uncond < groups && g_cond >= -1 &&
                    g_cond < groups,
                "%s: groups = %lld (1 .. %d), g_uncond = %lld, g_cond = %lld (-1: none) must lie inside", who,
                (long long)groups, VTM_SOLVER_MAX_GROUPS, (long long)g_uncond, (long long)g_cond);
    VTM_REQUIRE(n_concepts == 0 || (group && scale && rank_lo && rank_frac && w_apply && w_acc && mode),
                "%s: the per-concept arrays are required", who);
    VTM_REQUIRE(std::isfinite(guidance_scale) && std::isfinite(mom_scale) && std::isfinite(mom_beta),
                "%s: guidance_scale, mom_scale and mom_beta must be finite", who);
    VTM_REQUIRE(mom_apply == 0 || mom_apply == 1, "%s: mom_apply = %d (0 / 1)", who, mom_apply);
    VTM_REQUIRE(!momentum || n_rows >= (frame_ids ? 1 : F), "%s: momentum has n_rows = %lld rows for F = %lld frames", who,
                (long long)n_rows, (long long)F);
    const int P = (int)(H * W);
    Sega s{};
    s.g_uncond = (int)g_uncond, s.g_cond = (int)g_cond, s.mom_apply = momentum ? mom_apply : 0;
    s.s = guidance_scale, s.mom_scale = mom_scale, s.mom_beta = mom_beta;
    for (int e = 0; e < n_concepts; ++e) {
        VTM_REQUIRE(group[e] >= 0 && group[e] < groups, "%s: group[%d] = %d outside [0, %lld)", who, e, group[e],
                    (long long)groups);
        VTM_REQUIRE(mode[e] >= VTM_SEGA_CHANNEL && mode[e] <= VTM_SEGA_SUM_REGION, "%s: mode[%d] = %d is unknown", who, e, mode[e]);
        VTM_REQUIRE(std::isfinite(w_apply[e]) && std::isfinite(w_acc[e]), "%s: the weights of concept %d must be finite", who, e);
        if (mode[e] != VTM_SEGA_REGION)
            VTM_REQUIRE(rank_lo[e] >= 0 && rank_lo[e] < P && rank_frac[e] >= 0.0 && rank_frac[e] < 1.0,
                        "%s: rank_lo[%d] = %d, rank_frac = %g: a rank inside [0, %d) and a fraction inside [0, 1) are taken", who,
                        e, rank_lo[e], rank_frac[e], P);
        if (w_apply[e] == 0.0f && w_acc[e] == 0.0f) continue;       // never read, never written
        VTM_REQUIRE(mode[e] < VTM_SEGA_REGION || regions, "%s: mode[%d] names a region and regions is NULL", who, e);
        const int k = s.n++;
        s.orig[k] = e, s.group[k] = group[e], s.mode[k] = mode[e], s.rank_lo[k] = rank_lo[e];
        s.scale[k] = scale[e], s.w_apply[k] = w_apply[e], s.w_acc[k] = w_acc[e], s.rank_frac[k] = rank_frac[e];
    }
    VTM_REQUIRE(vtm::rows_apart(out, F, model_out, groups * F, C * H * W, dtype), "%s: out overlaps model_out", who);
    if (F == 0) return VTM_OK;
    hipStream_t st = vtm::as_stream(stream);
    return vtm::with_dtype(dtype, who, [&](auto t) {
        return launch_semantic<decltype(t)>(model_out, F, C, P, s, regions, momentum, frame_ids, out, mask_out, st);
    });
}
