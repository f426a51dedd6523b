// vtm_attention_kv_bias: the cross-attention core with one additive fp32 term PER KEY on the scores,
//     out[b, i, head] = softmax_j(q[b, i, head] . k[b, j, head] * scale + bias[b, j]) v[b, j, head],   j < Mk
// This is what an `encoder_attention_mask` turns the `self.attn2(...)` call of vidtome/patch.py:178-183 into: Diffusers' UNet
// hands the (B, K) mask of a padded prompt on as an additive (B, 1, K) row of 0 / -10000, shared by the heads and the queries.
//
// Structure: attention_sets_kernel (attention_sets.hip) reduced to one set -- no second accumulator, no per-set fold:
//   * workgroup = waves of 32 query rows; the K / V^T tiles of 64 keys are staged through one LDS buffer and shared by the
//     waves, the next tile's global loads in flight in registers while the current one is computed;
//   * beside the K tile lives the tile's bias, one 4-byte slot per key, pre-multiplied by log2(e); the slots of a tile's keys
//     >= Mk hold -inf, which is all the bounds logic the scores need;
//   * S^T = K Q^T on v_mfma_f32_32x32x16 (one query per lane); score = S^T * scale * log2(e) + slot, and only THEN the
//     running maximum: online softmax in registers, base 2, deferred rescale.  P is rounded to the operand type for the PV
//     contraction (bf16: as a hi + lo pair, two MFMAs) and the denominator is summed from the same rounded P;
//   * a key whose bias is -inf has score -inf and p = exp2(-inf) = 0 exactly, whatever its k and v rows hold (finite values);
//     as long as no finite score has been seen the exponent is taken against 0 instead of the running maximum -inf, so
//     leading masked tiles give 0, not NaN.  A sample whose keys are ALL -inf ends as 0 / 0 = NaN, as torch's SDPA does;
//   * no key split, no workspace, no combine kernel: the key axis is a few hundred keys, the launch streams q and out.
#include "attention_checks.h"
#include "attention_stage.h"

namespace vtm_att {
// the bias rows of one vtm_attention_kv_bias call (Call::key_bias): sample b reads bias[b * batch_stride + key]
struct KeyBias {
    const float *bias;
    int64_t ld, batch_stride;
};
}  // namespace vtm_att

namespace {

// the geometry of attention_sets_kernel: 8 waves up to d = 96, 4 above.  One accumulator set instead of two saves 13 - 69
// VGPRs from d = 40 on, not a whole occupancy step: one resident workgroup per CU from d = 32 on (bf16 d = 32 spills two registers at 128),
// two below (profiles/attention_bias_resources.txt)
constexpr int bias_waves(int D) { return D <= 96 ? 8 : 4; }
constexpr int bias_wg_per_cu(int D) { return D <= 16 ? 2 : 1; }
constexpr int bias_qb(int D) { return bias_waves(D) * QW; }   // query rows per workgroup

template <typename T, int D>
__global__ __launch_bounds__(bias_waves(D) * 64, bias_wg_per_cu(D) * bias_waves(D) / 4) void attention_bias_kernel(
    const T *__restrict__ q, int64_t ldq, const T *__restrict__ k, int64_t ldk, const T *__restrict__ vt, int64_t ldvt,
    T *__restrict__ out, int64_t ldo, int64_t H, int64_t M, int64_t Mp, int Mk, int64_t Mkp, float scale_log2e, int64_t nqb,
    int xcd_groups, const float *__restrict__ bias, int64_t bias_batch_stride) {
    using F = Frag<T>;
    using vec = typename F::vec;
    using elem = typename F::elem;
    constexpr int WAVES = bias_waves(D), NT = WAVES * 64;
    using Stage = KvStage<T, D, NT>;
    constexpr int DK = Stage::DK;          // k-steps of the QK^T contraction
    constexpr int DV = (D + 31) / 32;      // 32-row blocks of O^T
    constexpr int VROWS = DV * 32;
    constexpr int K_STRIDE = Stage::K_STRIDE;
    constexpr float LOG2E = 1.4426950408889634f;

    __shared__ __attribute__((aligned(16))) elem sK[KV * K_STRIDE];
    __shared__ __attribute__((aligned(16))) elem sV[VROWS * VT_STRIDE];
    __shared__ __attribute__((aligned(16))) float sB[KV];   // the tile's bias * log2(e); -inf behind the last key

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const WorkItem w = item_coords<bias_qb(D)>(item_of((int64_t)blockIdx.x, nqb, xcd_groups), nqb, H);   // (never key-split)
    const int64_t b = w.b, h = w.h, q0 = w.q0 + wave * QW;
    const int64_t C = H * D;

    zero_kv_pads<T, D, NT>(sK, sV, tid);

    vec qf[DK];
    {
        const int64_t qi = q0 + l31;
        load_q_frags<T, D>(qf, q + (b * Mp + (qi < M ? qi : 0)) * ldq + h * D, qi < M, hi);
    }

    Stage stage;
    stage.init(tid, ldk, ldvt);
    const auto rsrc_k = kv_rsrc(k + b * Mkp * ldk + h * D), rsrc_v = kv_rsrc(vt + (b * C + h * D) * ldvt);
    const float *brow = bias + b * bias_batch_stride;   // this sample's row: one value per key, for every head and query

    float rb = -INFINITY;   // threads 0 .. 63: the bias of key key0 + tid of the tile in flight
    auto issue = [&](int key0) {   // the tile of keys [key0, key0 + 64): rows / keys >= Mk read as zero, their bias as -inf
        stage.issue_masked(rsrc_k, rsrc_v, (uint32_t)key0 * (uint32_t)ldk * 2u, (uint32_t)key0 * 2u, key0, Mk);
        rb = -INFINITY;
        if (tid < KV && key0 + tid < Mk) rb = brow[key0 + tid];
    };
    auto write_lds = [&]() {
        stage.write(sK, sV);
        if (tid < KV) sB[tid] = rb * LOG2E;   // (-inf stays -inf)
    };

    // o: unnormalised O^T in the 32-row layout: [dv][r] = row 32 dv + (r & 3) + 8 (r >> 2) + 4 hi of query l31
    f32x16 o[DV];
#pragma unroll
    for (int dv = 0; dv < DV; ++dv)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dv][r] = 0.0f;
    float m_run = -INFINITY;   // running max, scaled (log2) units
    float l_run = 0.0f;        // this lane's share of the denominator

    auto tile = [&]() {
        f32x16 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kb][r] = 0.0f;
            const elem *kp = sK + (kb * 32 + l31) * K_STRIDE + hi * 8;
#pragma unroll
            for (int ks = 0; ks < DK; ++ks) s[kb] = F::mfma(*reinterpret_cast<const vec *>(kp + ks * 16), qf[ks], s[kb]);
        }
        // scores in log2 units: lane (l31, hi) holds keys 32 kb + (r & 3) + 8 (r >> 2) + 4 hi -- four consecutive slots per
        // register group, the same address for all lanes of a half (a broadcast read).  Keys behind Mk: 0 * scale - inf.
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 bv = *reinterpret_cast<const f32x4 *>(sB + kb * 32 + 8 * g + 4 * hi);
#pragma unroll
                for (int e = 0; e < 4; ++e) s[kb][4 * g + e] = __builtin_fmaf(s[kb][4 * g + e], scale_log2e, bv[e]);
            }
        // online softmax, base 2, deferred rescale.  A tile whose keys are all masked (-inf) leaves the state alone.
        float mt = fmaxf(s[0][0], s[1][0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) mt = fmaxf(fmaxf(mt, s[0][r]), s[1][r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        if (!__all(mt <= m_run + DEFER_THR)) {
            const float m_new = fmaxf(m_run, mt);
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // nothing finite seen before: exp2(-inf) = 0
            m_run = m_new;
            l_run *= alpha;
#pragma unroll
            for (int dv = 0; dv < DV; ++dv)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[dv][r] *= alpha;
        }
        // (only masked keys so far: -inf - (-inf) would be NaN; against 0 every p of such a query is exp2(-inf) = 0)
        const float m_use = m_run == -INFINITY ? 0.0f : m_run;
        // per 16-key step: p of keys 16 st + (e & 3) + 8 (e >> 2) + 4 hi
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            float p[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) p[e] = __builtin_amdgcn_exp2f(s[st >> 1][8 * (st & 1) + e] - m_use);
            pv_step_split<T, D>(o, l_run, p, sV + l31 * VT_STRIDE + 8 * hi + st * 16);
        }
    };

    // the tiles, one after the other; tile ct is in LDS, tile ct + 1 in flight
    const int ntiles = (Mk + KV - 1) / KV;
    issue(0);
    write_lds();
    __syncthreads();
    for (int ct = 0;; ++ct) {
        const bool more = ct + 1 < ntiles;
        if (more) issue((ct + 1) * KV);
        tile();
        if (!more) break;
        __syncthreads();   // every wave has read the tile
        write_lds();
        __syncthreads();
    }

    const float inv_l = 1.0f / (l_run + __shfl_xor(l_run, 32, 64));
    const int64_t qi = q0 + l31;
    if (qi < M) store_rows32<T, D>(o, inv_l, out + (b * Mp + qi) * ldo + h * D, hi);
}

template <typename T, int D>
void launch_bias(const Call &c, const Launch &g) {
    hipLaunchKernelGGL((attention_bias_kernel<T, D>), dim3((unsigned)g.wgs), dim3(bias_waves(D) * 64), 0, c.s, (const T *)c.q,
                       c.ldq, (const T *)c.k, c.ldk, (const T *)c.vt, c.ldvt, (T *)c.out, c.ldo, c.h, c.M, c.Mp, (int)c.Mk, c.Mkp,
                       g.scale_log2e, g.nqb, g.xcd_groups, c.key_bias->bias, c.key_bias->batch_stride);
}

// The family: one workgroup per (query block, head, sample), never key-split (no partial record, no combine kernel) -- the
// planner sizes the grid and pins the (sample, head) pairs to XCDs like every other family's.
template <typename T, int D>
Family bias_family() {
    Family f;
    f.name = "vtm_attention_kv_bias";
    f.qb = bias_qb(D);
    f.wg_per_cu = bias_wg_per_cu(D);
    f.rec_bytes = 0;
    f.xcd_min_nqb = 64;
    f.host_split_all = false;
    f.main = launch_bias<T, D>;
    return f;
}

}  // namespace

VTM_EXPORT int vtm_attention_kv_bias(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt, int64_t ldvt,
                                     void *out, int64_t ldo, int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mqp,
                                     int64_t Mk, int64_t Mkp, int64_t d, float scale, const float *bias, int64_t ld_bias,
                                     int64_t bias_batch_stride, vtm_stream_t stream) {
    const char *who = "vtm_attention_kv_bias";
    VTM_REQUIRE(q && k && vt && out, "%s: null pointer", who);
    VTM_REQUIRE(bias, "%s: null bias", who);
    VTM_REQUIRE(B > 0 && h > 0 && Mq > 0 && Mqp >= Mq && Mk > 0 && Mkp >= Mk && Mkp % 8 == 0 && d > 0, "%s: bad sizes", who);
    if (int rc = check_scale(who, scale)) return rc;
    if (int rc = check_half_dtype(who, dtype)) return rc;
    VTM_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldvt % 8 == 0 && ldo % 4 == 0 && ldvt >= Mk,
                "%s: leading dimensions must keep 16-byte alignment (ldvt >= Mk, %% 8)", who);
    if (int rc = check_kv_slices(who, "sample", Mkp, ldk, d, ldvt)) return rc;
    if (int rc = check_key_rows(who, "bias", "values", ld_bias, bias_batch_stride, Mk)) return rc;
    const KeyBias kb{bias, ld_bias, bias_batch_stride};
    Call c{q, ldq, k, ldk, vt, ldvt, out, ldo, dtype, B, h, Mq, Mqp, Mk, Mkp, scale, 1, nullptr, 0,
           nullptr, vtm::as_stream(stream), false, nullptr, nullptr, 0};
    c.key_bias = &kb;
    return with_half_head_dim(dtype, d, [&](auto t, auto dim) {
        return planned_launch(c, bias_family<decltype(t), decltype(dim)::value>());
    });
}
