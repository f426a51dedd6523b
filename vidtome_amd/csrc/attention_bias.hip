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
#include "attention_plan.h"

#include <cmath>

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
    constexpr bool SPLIT_P = std::is_same_v<T, vtm_bf16>;   // P as hi + lo parts (see tile)
    constexpr int DK = (D + 15) / 16;      // k-steps of the QK^T contraction
    constexpr int DV = (D + 31) / 32;      // 32-row blocks of O^T
    constexpr int VROWS = DV * 32;
    constexpr int K_STRIDE = DK * 16 + 8;  // elements; conflict-free b128 reads (see attention.hip)
    constexpr int DCH = D / 8;             // 16-byte chunks per K row
    constexpr int K_CHUNKS = KV * DCH, V_CHUNKS = D * (KV / 8);
    constexpr int K_PER_T = (K_CHUNKS + NT - 1) / NT, V_PER_T = (V_CHUNKS + NT - 1) / NT;
    constexpr float LOG2E = 1.4426950408889634f;

    __shared__ __attribute__((aligned(16))) elem sK[KV * K_STRIDE];
    __shared__ __attribute__((aligned(16))) elem sV[VROWS * VT_STRIDE];
    __shared__ __attribute__((aligned(16))) float sB[KV];   // the tile's bias * log2(e); -inf behind the last key

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const WorkItem w = item_coords<bias_qb(D)>(item_of((int64_t)blockIdx.x, nqb, xcd_groups), nqb, H);   // (never key-split)
    const int64_t b = w.b, h = w.h, q0 = w.q0 + wave * QW;
    const int64_t C = H * D;

    // one-time LDS init: the K pad columns meet Q's zero padding and the V^T pad rows feed O^T rows nobody stores, but
    // garbage there could be NaN; tile stores never touch them
    for (int i = tid; i < KV * (K_STRIDE - D); i += NT)
        sK[(i / (K_STRIDE - D)) * K_STRIDE + D + i % (K_STRIDE - D)] = (elem)0.0f;
    for (int i = tid; i < (VROWS - D) * VT_STRIDE; i += NT) sV[D * VT_STRIDE + i] = (elem)0.0f;

    // Q fragments (B operand of S^T = K Q^T): lane (query l31, half hi) holds d = 16 ks + 8 hi + 0..7
    vec qf[DK];
    {
        const int64_t qi = q0 + l31;
        const T *qp = q + (b * Mp + (qi < M ? qi : 0)) * ldq + h * D;
#pragma unroll
        for (int ks = 0; ks < DK; ++ks) {
            const int d0 = ks * 16 + hi * 8;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (d0 < D && qi < M) v = *reinterpret_cast<const uint4 *>(qp + d0);
            qf[ks] = *reinterpret_cast<vec *>(&v);
        }
    }

    // staging addresses, as in attention_kernel: chunk c = tid + NT i; K: (row c / DCH, 16-byte piece c % DCH); V^T:
    // (channel row c / 8, key piece c % 8), stored as [k0-3 | k8-11 | k4-7 | k12-15] inside every 16-key group
    uint32_t kgo[K_PER_T], vgo[V_PER_T];
    int koff[K_PER_T], voff[V_PER_T], krow[K_PER_T], vkey[V_PER_T];
    bool kok[K_PER_T], vok[V_PER_T];
#pragma unroll
    for (int i = 0; i < K_PER_T; ++i) {
        const int c = tid + i * NT;
        kok[i] = c < K_CHUNKS;
        krow[i] = c / DCH;
        kgo[i] = kok[i] ? (uint32_t)(krow[i] * (int)ldk + (c % DCH) * 8) * 2u : 0u;
        koff[i] = krow[i] * K_STRIDE + (c % DCH) * 8;
    }
#pragma unroll
    for (int i = 0; i < V_PER_T; ++i) {
        const int c = tid + i * NT;
        vok[i] = c < V_CHUNKS;
        vkey[i] = (c % (KV / 8)) * 8;
        vgo[i] = vok[i] ? (uint32_t)((c / (KV / 8)) * (int)ldvt + vkey[i]) * 2u : 0u;
        voff[i] = (c / (KV / 8)) * VT_STRIDE + (vkey[i] & ~15) + ((vkey[i] >> 3) & 1) * 4;
    }
    // (the descriptors carry no real bound: every fetch is guarded by Mk below)
    const auto rsrc_k = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(k + b * Mkp * ldk + h * D), 0, 0x7fffffff, 0x00020000);
    const auto rsrc_v = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(vt + (b * C + h * D) * ldvt), 0, 0x7fffffff, 0x00020000);
    auto fetch = [](const auto &rsrc, uint32_t voff_, uint32_t soff_) {
        return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff_, soff_, 0));
    };
    const float *brow = bias + b * bias_batch_stride;   // this sample's row: one value per key, for every head and query

    uint4 rk[K_PER_T], rv[V_PER_T];
    float rb = -INFINITY;   // threads 0 .. 63: the bias of key key0 + tid of the tile in flight
    auto issue = [&](int key0) {   // the tile of keys [key0, key0 + 64): rows / keys >= Mk read as zero, their bias as -inf
        const uint32_t so_k = (uint32_t)key0 * (uint32_t)ldk * 2u, so_v = (uint32_t)key0 * 2u;
#pragma unroll
        for (int i = 0; i < K_PER_T; ++i) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (kok[i] && key0 + krow[i] < Mk) v = fetch(rsrc_k, kgo[i], so_k);
            rk[i] = v;
        }
#pragma unroll
        for (int i = 0; i < V_PER_T; ++i) {
            uint4 v = make_uint4(0, 0, 0, 0);
            const int key = key0 + vkey[i];
            if (vok[i] && key < Mk) {   // key % 8 == 0 and ldvt % 8 == 0, ldvt >= Mk: the 16-byte piece is inside the row
                v = fetch(rsrc_v, vgo[i], so_v);
                mask_keys(v, Mk - key);   // p is 0 there, but 0 * garbage may be NaN
            }
            rv[i] = v;
        }
        rb = -INFINITY;
        if (tid < KV && key0 + tid < Mk) rb = brow[key0 + tid];
    };
    auto write_lds = [&]() {
#pragma unroll
        for (int i = 0; i < K_PER_T; ++i)
            if (kok[i]) *reinterpret_cast<uint4 *>(sK + koff[i]) = rk[i];
#pragma unroll
        for (int i = 0; i < V_PER_T; ++i)
            if (vok[i]) {
                uint2 *dst = reinterpret_cast<uint2 *>(sV + voff[i]);
                dst[0] = make_uint2(rv[i].x, rv[i].y);
                dst[2] = make_uint2(rv[i].z, rv[i].w);
            }
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
        // per 16-key step: p of keys 16 st + (e & 3) + 8 (e >> 2) + 4 hi, packed to the operand type, then O^T += V^T P^T with
        // k-slot (hi, e) <-> key 16 st + 8 (e >> 2) + 4 hi + (e & 3).  bf16 keeps 8 bits of P: there P goes in as hi + lo (two
        // MFMAs on the same V^T fragment), so that its rounding stays below the operands' own; the denominator is summed from
        // what the numerator sees.
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            float p[8], plo[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) p[e] = __builtin_amdgcn_exp2f(s[st >> 1][8 * (st & 1) + e] - m_use);
            vec ph, pl;
            F::pack8(ph, p);
            if constexpr (SPLIT_P) {
#pragma unroll
                for (int e = 0; e < 8; ++e) plo[e] = p[e] - (float)ph[e];
                F::pack8(pl, plo);
#pragma unroll
                for (int e = 0; e < 8; ++e) l_run += (float)ph[e] + (float)pl[e];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) l_run += (float)ph[e];
            }
#pragma unroll
            for (int dv = 0; dv < DV; ++dv) {
                const vec vf = *reinterpret_cast<const vec *>(sV + (dv * 32 + l31) * VT_STRIDE + 8 * hi + st * 16);
                o[dv] = F::mfma(vf, ph, o[dv]);
                if constexpr (SPLIT_P) o[dv] = F::mfma(vf, pl, o[dv]);
            }
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
    if (qi < M) {
        T *op = out + (b * Mp + qi) * ldo + h * D;
#pragma unroll
        for (int dv = 0; dv < DV; ++dv)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d0 = dv * 32 + 8 * g + 4 * hi;
                if (d0 < D) {   // D % 8 == 0 and d0 % 4 == 0 -> the 4 channels are all valid
                    elem w4[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) w4[e] = (elem)(o[dv][g * 4 + e] * inv_l);
                    *reinterpret_cast<uint2 *>(op + d0) = *reinterpret_cast<uint2 *>(w4);
                }
            }
    }
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
    VTM_REQUIRE(scale > 0.0f && std::isfinite(scale), "%s: scale must be positive and finite", who);
    if (dtype == VTM_F32)
        return vtm::fail(VTM_EINVAL, "%s: fp32 operands are not taken (dtype must be VTM_F16 or VTM_BF16)", who);
    if (dtype != VTM_F16 && dtype != VTM_BF16) return vtm::fail(VTM_EINVAL, "%s: dtype must be VTM_F16 or VTM_BF16", who);
    VTM_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldvt % 8 == 0 && ldo % 4 == 0 && ldvt >= Mk,
                "%s: leading dimensions must keep 16-byte alignment (ldvt >= Mk, %% 8)", who);
    // K / V^T tiles are addressed with 32-bit byte offsets inside one (sample, head) slice (buffer loads)
    VTM_REQUIRE((Mkp * ldk + d) * 2 < (1ll << 31) && (d * ldvt + Mkp) * 2 < (1ll << 31),
                "%s: a (sample, head) slice of K or V^T must stay below 2 GiB", who);
    VTM_REQUIRE(ld_bias >= Mk, "%s: ld_bias = %lld is shorter than a row of Mk = %lld values", who, (long long)ld_bias,
                (long long)Mk);
    // one row for every sample (stride 0), or per-sample rows that do not overlap
    VTM_REQUIRE(bias_batch_stride == 0 || bias_batch_stride >= ld_bias,
                "%s: bias_batch_stride = %lld must be 0 or at least ld_bias = %lld", who, (long long)bias_batch_stride,
                (long long)ld_bias);
    const KeyBias kb{bias, ld_bias, bias_batch_stride};
    Call c{q, ldq, k, ldk, vt, ldvt, out, ldo, dtype, B, h, Mq, Mqp, Mk, Mkp, scale, 1, nullptr, 0,
           nullptr, vtm::as_stream(stream), false, nullptr, nullptr, 0};
    c.key_bias = &kb;
    return with_head_dim(d, [&](auto dim) {
        constexpr int D = decltype(dim)::value;
        return planned_launch(c, dtype == VTM_F16 ? bias_family<__half, D>() : bias_family<vtm_bf16, D>());
    });
}
