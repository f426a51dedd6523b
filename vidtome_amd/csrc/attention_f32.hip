// attention_f32_kernel: the self-attention core of fp32 models in fp32 -- fp32 operands, fp32 products, fp32 accumulation
// on the f32-input MFMA (v_mfma_f32_16x16x4_f32: bit for bit a k-ordered fmaf chain).  Same arithmetic as attention.hip
// (pnp_utils.py:47-95, PnP sharing of the source sample's q / k included); reached through the same exports with
// dtype VTM_F32 (attention.hip: attention_any).  Opt-in per block on the host (patch.py: `fp32_attention`).
//
// Structure (the conventions of attention_kernel):
//   * workgroup = 4 waves, each wave owns 32 queries as two 16-query halves (NQH = 2; d >= 128: one half, see nqh_for);
//     K / V^T tiles of 32 keys are staged through LDS (register-staged, double-buffered) and shared by the 4 waves;
//   * "swapped" QK^T: S^T = K Q^T; a 16x16x4 MFMA's C/D puts one query per lane & 15 and keys 4 (lane >> 4) + e of the
//     16-key group in register e -> the online softmax is in-register (two cross-group exchanges for the running max);
//   * online softmax in base 2 (one v_fma + one v_exp per score) with the deferred rescale of attention_kernel (P <= 2^8);
//   * P stays in registers as fp32: accumulator register e of lane (l15, g) is the B-operand value of k-step e of the
//     PV MFMA (k = lane >> 4 <-> key 4 g + e), so V^T is read with the matching key order -- 4 consecutive keys, one
//     ds_read_b128 per 16-key group and 16 channels -- and nothing is permuted;
//   * V arrives TRANSPOSED (channel-major) as for the 16-bit kernels; the denominator is an fp32 VALU sum of the same P.
// Tiling choice (16-row O^T blocks): the 32x32x2 form would pad O^T to whole 32-row blocks -- d = 40 -> 64 rows (+60 % PV
// matrix time), d = 80 -> 96 (+20 %) -- where 16-row blocks pad d = 40 to 48 (+20 %) and d = 80 not at all; the QK^T
// contraction steps over 4 channels and pads nothing (a d % 16 == 8 head ends on a 2-step half chunk).  Both forms run
// at the same 64 FLOP / clk / SIMD; 16x16x4 has a 40-cycle dependent latency on a 32-cycle issue, so every chain of MFMAs
// is interleaved with at least one other (2 key groups x 2 query halves for QK^T, O^T blocks x query halves for PV).
// The fp16 / bf16 kernels are not touched by any of this.
#include "attention_plan.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int F_WAVES = 4, F_NT = F_WAVES * 64;
constexpr int KT = 32;                 // keys per tile
constexpr int FVT_STRIDE = KT + 4;     // floats per V^T row in LDS (36 = 4 x odd words: conflict-free b128 reads)
// query halves per wave: 2 (32 queries) while the Q fragments and O^T accumulators of both fit the VGPR budget, 1 for the
// widest heads (d = 160: 2 x (40 + 40) registers for Q and O^T alone)
constexpr int nqh_for(int D) { return D >= 128 ? 1 : 2; }
constexpr int fqb_for(int D) { return F_WAVES * 16 * nqh_for(D); }           // queries per workgroup
constexpr int F_XCD_MIN_NQB = 64;                                             // Family::xcd_min_nqb
constexpr int fwg_per_cu(int D) { return D <= 128 ? 2 : 1; }    // resident workgroups per CU (LDS: d = 160 takes 88 KB)
constexpr int dv16_for(int D) { return (D + 15) / 16; }                       // 16-row blocks of O^T
constexpr int fk_stride(int D) { return D + 4; }                              // floats per K row in LDS (4 x odd words)
// the partial record of a key-split workgroup, per thread: O^T accumulators, then ONE float holding, by lane group g,
// running max of half 0 / half 1, denominator of half 0 / half 1 (they are the same in the four groups of a query)
constexpr int facc_floats(int D) { return dv16_for(D) * 4 * nqh_for(D); }
constexpr int frec_floats(int D) { return facc_floats(D) + 1; }
constexpr int64_t frec_size(int D) { return (int64_t)frec_floats(D) * F_NT; }   // floats of a workgroup's partial record
constexpr size_t flds_bytes(int D) { return (size_t)2 * (KT * fk_stride(D) + dv16_for(D) * 16 * FVT_STRIDE) * sizeof(float); }

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// QK^T contraction step s of lane group g: chunk j = s / 4 of 16 channels, channel 16 j + 4 g + s % 4; a d % 16 == 8 head
// ends on a half chunk of 2 steps, channel 16 j + 2 g + s % 4.  Q and K fragments use the same map (any map does, as long
// as both do), chosen so that a lane's 4 steps of a chunk are 4 consecutive floats.
template <int D> __device__ __forceinline__ void load_chunks(float (&f)[D / 4], const float *p, int g, bool ok) {
#pragma unroll
    for (int j = 0; j < (D + 15) / 16; ++j) {
        if (16 * j + 16 <= D) {
            float4 v = ok ? *reinterpret_cast<const float4 *>(p + 16 * j + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
            f[4 * j] = v.x; f[4 * j + 1] = v.y; f[4 * j + 2] = v.z; f[4 * j + 3] = v.w;
        } else {
            float2 v = ok ? *reinterpret_cast<const float2 *>(p + 16 * j + 2 * g) : make_float2(0.f, 0.f);
            f[4 * j] = v.x; f[4 * j + 1] = v.y;
        }
    }
}

template <int D>
__device__ __forceinline__ void store_row(const f32x4 (&o)[dv16_for(D)], float inv_l, float *__restrict__ op, int g) {
#pragma unroll
    for (int dv = 0; dv < dv16_for(D); ++dv) {
        const int c0 = 16 * dv + 4 * g;
        if (c0 < D)   // D % 8 == 0 and c0 % 4 == 0 -> the 4 channels are all valid
            *reinterpret_cast<float4 *>(op + c0) = make_float4(o[dv][0] * inv_l, o[dv][1] * inv_l, o[dv][2] * inv_l,
                                                               o[dv][3] * inv_l);
    }
}

// merges the `nsplit` partial records of a query block (same thread <-> register mapping as attention_f32_kernel)
template <int D>
__global__ __launch_bounds__(F_NT) void attention_f32_combine_kernel(
    float *__restrict__ out, int64_t ldo, int64_t H, int64_t M, int64_t Mp, PlanArgs plan) {
    constexpr int NQH = nqh_for(D), DV = dv16_for(D), NA = facc_floats(D);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const WorkItem w = decode_combine_item<fqb_for(D), F_XCD_MIN_NQB>(plan, H, blockIdx.x);
    if (w.leave) return;
    const int64_t b = w.b, h = w.h, q0 = w.q0 + wave * 16 * NQH;
    const int nsplit = w.nsplit;
    const float *partial = plan.partial_base + w.rec * frec_size(D);
    f32x4 o[DV][NQH];
    float m[NQH], l[NQH];
#pragma unroll
    for (int qh = 0; qh < NQH; ++qh) {
        m[qh] = -INFINITY;
        l[qh] = 0.0f;
#pragma unroll
        for (int dv = 0; dv < DV; ++dv) o[dv][qh] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int sp = 0; sp < nsplit; ++sp) {
        const float *pp = partial + sp * frec_size(D) + tid;
        const float ml = pp[NA * F_NT];
#pragma unroll
        for (int qh = 0; qh < NQH; ++qh) {
            const float ms = __shfl(ml, l15 + 16 * qh, 64), ls = __shfl(ml, l15 + 32 + 16 * qh, 64);
            const float mn = fmaxf(m[qh], ms);
            const float fa = mn == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(m[qh] - mn);   // (a split that saw no key)
            const float fb = mn == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(ms - mn);
            m[qh] = mn;
            l[qh] = l[qh] * fa + ls * fb;
#pragma unroll
            for (int dv = 0; dv < DV; ++dv)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    o[dv][qh][e] = o[dv][qh][e] * fa + pp[((dv * NQH + qh) * 4 + e) * F_NT] * fb;
        }
    }
#pragma unroll
    for (int qh = 0; qh < NQH; ++qh) {
        const int64_t qi = q0 + 16 * qh + l15;
        f32x4 oq[DV];
#pragma unroll
        for (int dv = 0; dv < DV; ++dv) oq[dv] = o[dv][qh];
        if (qi < M) store_row<D>(oq, 1.0f / l[qh], out + (b * Mp + qi) * ldo + h * D, g);
    }
}

template <int D>
__global__ __launch_bounds__(F_NT, fwg_per_cu(D)) void attention_f32_kernel(
    const float *__restrict__ q, int64_t ldq, const float *__restrict__ k, int64_t ldk, const float *__restrict__ vt,
    int64_t ldvt, float *__restrict__ out, int64_t ldo, int64_t H, int64_t M, int64_t Mp, int64_t Mk, int64_t Mkp,
    float scale_log2e, int64_t src_batch, PlanArgs plan) {
    // Work decomposition as attention_kernel (decode_work_item); a workgroup that takes a key range of a split item leaves a
    // partial record for attention_f32_combine_kernel.
    constexpr int NQH = nqh_for(D), DV = dv16_for(D), DS = D / 4;
    constexpr int KS = fk_stride(D);
    constexpr int CHUNKS = KT * D / 4;                     // 16-byte pieces of a K tile = of a V^T tile
    constexpr int PER_T = (CHUNKS + F_NT - 1) / F_NT;
    constexpr int SK_TILE = KT * KS, SV_TILE = DV * 16 * FVT_STRIDE;
    static_assert(D % 8 == 0, "head dims are multiples of 8");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *sK = reinterpret_cast<float *>(smem);   // [2][KT][KS]
    float *sV = sK + 2 * SK_TILE;                  // [2][DV * 16][FVT_STRIDE]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const WorkItem w = decode_work_item<fqb_for(D), F_XCD_MIN_NQB>(plan, H, blockIdx.x);
    if (w.leave) return;
    const int nsplit = w.nsplit, split = w.split;
    float *partial = w.rec >= 0 ? plan.partial_base + w.rec * frec_size(D) : nullptr;
    const int64_t b = w.b, h = w.h;
    const int64_t bq = b % src_batch;  // PnP injection: q / k of the source sample (pnp_utils.py:57-67)
    const int64_t q0 = w.q0 + wave * 16 * NQH;
    const int64_t C = H * D;

    // V^T rows D .. 16 DV - 1 (d % 16 == 8) meet O^T rows nobody stores: zero them once (tile loads never touch them)
    if constexpr (DV * 16 > D) {
        for (int i = tid; i < 2 * (DV * 16 - D) * FVT_STRIDE; i += F_NT) {
            const int bufi = i / ((DV * 16 - D) * FVT_STRIDE), rem = i % ((DV * 16 - D) * FVT_STRIDE);
            sV[bufi * SV_TILE + D * FVT_STRIDE + rem] = 0.0f;
        }
    }

    // Q fragments (B operand of S^T = K Q^T): lane (query 16 qh + l15, group g), contraction steps as load_chunks
    float qf[NQH][DS];
#pragma unroll
    for (int qh = 0; qh < NQH; ++qh) {
        const int64_t qi = q0 + 16 * qh + l15;
        load_chunks<D>(qf[qh], q + (bq * Mp + (qi < M ? qi : 0)) * ldq + h * D, g, qi < M);
    }

    // staging: chunk c = tid + 256 i; K: (row c / (D/4), piece c % (D/4)); V^T: (channel row c / 8, key piece c % 8).
    // Buffer loads: a wave-uniform descriptor of the (sample, head) slice, per-thread 32-bit byte offsets, a scalar tile
    // offset.  The descriptors carry no real bound (ragged tiles are masked explicitly).
    uint32_t kgo[PER_T], vgo[PER_T];
    int koff[PER_T], voff[PER_T], krow[PER_T], vkey[PER_T];
    bool cok[PER_T];
#pragma unroll
    for (int i = 0; i < PER_T; ++i) {
        const int c = tid + i * F_NT;
        cok[i] = c < CHUNKS;
        krow[i] = c / (D / 4);
        kgo[i] = cok[i] ? (uint32_t)(krow[i] * (int)ldk + (c % (D / 4)) * 4) * 4u : 0u;
        koff[i] = krow[i] * KS + (c % (D / 4)) * 4;
        vkey[i] = (c % (KT / 4)) * 4;
        vgo[i] = cok[i] ? (uint32_t)((c / (KT / 4)) * (int)ldvt + vkey[i]) * 4u : 0u;
        voff[i] = (c / (KT / 4)) * FVT_STRIDE + vkey[i];
    }
    const auto rsrc_k = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(k + bq * Mkp * ldk + h * D), 0, 0x7fffffff, 0x00020000);
    const auto rsrc_v = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(vt + (b * C + h * D) * ldvt), 0, 0x7fffffff, 0x00020000);
    const uint32_t kstep = (uint32_t)(KT * ldk) * 4u, vstep = (uint32_t)KT * 4u;
    uint32_t so_k = 0, so_v = 0;
    auto fetch = [](const auto &rsrc, uint32_t voff_, uint32_t soff_) {
        return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff_, soff_, 0));
    };
    uint4 rk[PER_T], rv[PER_T];
    auto issue_full = [&]() {   // (surplus threads re-read chunk 0 and do not store it: no load behind a branch)
#pragma unroll
        for (int i = 0; i < PER_T; ++i) rk[i] = fetch(rsrc_k, kgo[i], so_k);
#pragma unroll
        for (int i = 0; i < PER_T; ++i) rv[i] = fetch(rsrc_v, vgo[i], so_v);
        so_k += kstep;
        so_v += vstep;
    };
    auto issue_tail = [&](int64_t key0) {   // ragged last tile: keys >= Mk read as zero
#pragma unroll
        for (int i = 0; i < PER_T; ++i) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (cok[i] && key0 + krow[i] < Mk) v = fetch(rsrc_k, kgo[i], so_k);
            rk[i] = v;
        }
#pragma unroll
        for (int i = 0; i < PER_T; ++i) {
            uint4 v = make_uint4(0, 0, 0, 0);
            const int64_t key = key0 + vkey[i];
            if (cok[i] && key < Mk) {   // ldvt >= Mk, % 8: the 4 keys are inside the row; p is 0 past Mk, 0 * garbage is not
                v = fetch(rsrc_v, vgo[i], so_v);
                const int valid = (int)(Mk - key);
                if (valid < 4) v.w = 0u;
                if (valid < 3) v.z = 0u;
                if (valid < 2) v.y = 0u;
            }
            rv[i] = v;
        }
    };
    auto write_lds = [&](int buf) {
        float *dk = sK + buf * SK_TILE, *dv = sV + buf * SV_TILE;
#pragma unroll
        for (int i = 0; i < PER_T; ++i)
            if (cok[i]) {
                *reinterpret_cast<uint4 *>(dk + koff[i]) = rk[i];
                *reinterpret_cast<uint4 *>(dv + voff[i]) = rv[i];
            }
    };

    f32x4 o[DV][NQH];   // o[dv][qh][e] = O^T row 16 dv + 4 g + e of query 16 qh + l15
#pragma unroll
    for (int dv = 0; dv < DV; ++dv)
#pragma unroll
        for (int qh = 0; qh < NQH; ++qh) o[dv][qh] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run[NQH], l_run[NQH];   // running max (scaled, log2 units; the same in the 4 groups), partial denominators
#pragma unroll
    for (int qh = 0; qh < NQH; ++qh) {
        m_run[qh] = -INFINITY;
        l_run[qh] = 0.0f;
    }

    // one tile: S^T = K Q^T -> online softmax -> O^T += V^T P^T.  TAIL = the ragged last tile (keys >= Mk masked).
    auto tile = [&](auto tail_tag, int buf, int64_t key0) {
        constexpr bool TAIL = decltype(tail_tag)::value;
        f32x4 s[2][NQH];   // s[kb][qh][e]: key 16 kb + 4 g + e, query 16 qh + l15
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int qh = 0; qh < NQH; ++qh) s[kb][qh] = f32x4{0.f, 0.f, 0.f, 0.f};
        {
            float kf[2][DS];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) load_chunks<D>(kf[kb], sK + buf * SK_TILE + (16 * kb + l15) * KS, g, true);
#pragma unroll
            for (int st = 0; st < DS; ++st)
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int qh = 0; qh < NQH; ++qh) s[kb][qh] = mfma4(kf[kb][st], qf[qh][st], s[kb][qh]);
        }
        if constexpr (TAIL) {
            const int lim = (int)(Mk - key0);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int qh = 0; qh < NQH; ++qh)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (16 * kb + 4 * g + e >= lim) s[kb][qh][e] = -INFINITY;
        }
        // online softmax, base 2, deferred rescale: the shift is only raised when a score outgrew it by more than 2^8
        float mt[NQH];
        bool keep = true;
#pragma unroll
        for (int qh = 0; qh < NQH; ++qh) {
            float x = fmaxf(fmaxf(s[0][qh][0], s[0][qh][1]), fmaxf(s[0][qh][2], s[0][qh][3]));
            x = fmaxf(x, fmaxf(fmaxf(s[1][qh][0], s[1][qh][1]), fmaxf(s[1][qh][2], s[1][qh][3])));
            x = fmaxf(x, __shfl_xor(x, 16, 64));
            x = fmaxf(x, __shfl_xor(x, 32, 64));
            mt[qh] = x * scale_log2e;
            keep = keep && mt[qh] <= m_run[qh] + DEFER_THR;
        }
        if (!__all(keep)) {
#pragma unroll
            for (int qh = 0; qh < NQH; ++qh) {
                const float m_new = fmaxf(m_run[qh], mt[qh]);
                const float alpha = __builtin_amdgcn_exp2f(m_run[qh] - m_new);   // first tile: exp2(-inf) = 0
                m_run[qh] = m_new;
                l_run[qh] *= alpha;
#pragma unroll
                for (int dv = 0; dv < DV; ++dv)
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[dv][qh][e] *= alpha;
            }
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int qh = 0; qh < NQH; ++qh)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][qh][e], scale_log2e, -m_run[qh]));
                    s[kb][qh][e] = p;
                    l_run[qh] += p;
                }
        // O^T += V^T P^T: k-step e of 16-key group kb <-> key 16 kb + 4 g + e, V^T read with the same assignment
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int dv = 0; dv < DV; ++dv) {
                const float4 a = *reinterpret_cast<const float4 *>(sV + buf * SV_TILE + (16 * dv + l15) * FVT_STRIDE + 16 * kb + 4 * g);
                const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int qh = 0; qh < NQH; ++qh) o[dv][qh] = mfma4(av[e], s[kb][qh][e], o[dv][qh]);
            }
    };
    using std::false_type;
    using std::true_type;

    const int ntiles = (int)((Mk + KT - 1) / KT), nfull = (int)(Mk / KT);
    const int tps = (ntiles + nsplit - 1) / nsplit;
    const int tb = split * tps, te = tb + tps < ntiles ? tb + tps : ntiles;
    const int fe = te < nfull ? te : nfull;
    so_k = (uint32_t)tb * kstep;
    so_v = (uint32_t)tb * vstep;
    if (tb < te) {
        if (tb < fe) issue_full(); else issue_tail((int64_t)tb * KT);
        write_lds(0);
    }
    __syncthreads();
    int t = tb, buf = 0;
    for (; t + 1 < fe; ++t) {
        issue_full();
        tile(false_type{}, buf, (int64_t)t * KT);
        write_lds(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    if (t < fe) {
        const bool ragged_next = te > fe;
        if (ragged_next) issue_tail((int64_t)fe * KT);
        tile(false_type{}, buf, (int64_t)t * KT);
        if (ragged_next) write_lds(buf ^ 1);
        __syncthreads();
        ++t;
        buf ^= 1;
    }
    if (t < te) tile(true_type{}, buf, (int64_t)t * KT);

    float l_tot[NQH];
#pragma unroll
    for (int qh = 0; qh < NQH; ++qh) {
        const float x = l_run[qh] + __shfl_xor(l_run[qh], 16, 64);
        l_tot[qh] = x + __shfl_xor(x, 32, 64);
    }
    if (partial) {   // split workgroup: hand the raw state to attention_f32_combine_kernel
        float *pp = partial + tid;
#pragma unroll
        for (int dv = 0; dv < DV; ++dv)
#pragma unroll
            for (int qh = 0; qh < NQH; ++qh)
#pragma unroll
                for (int e = 0; e < 4; ++e) pp[((dv * NQH + qh) * 4 + e) * F_NT] = o[dv][qh][e];
        float ml = 0.0f;   // group 0 / 1: running max of half 0 / 1, group 2 / 3: denominator of half 0 / 1
#pragma unroll
        for (int qh = 0; qh < NQH; ++qh) {
            if (g == qh) ml = m_run[qh];
            if (g == 2 + qh) ml = l_tot[qh];
        }
        pp[facc_floats(D) * F_NT] = ml;
        return;
    }
#pragma unroll
    for (int qh = 0; qh < NQH; ++qh) {
        const int64_t qi = q0 + 16 * qh + l15;
        f32x4 oq[DV];
#pragma unroll
        for (int dv = 0; dv < DV; ++dv) oq[dv] = o[dv][qh];
        if (qi < M) store_row<D>(oq, 1.0f / l_tot[qh], out + (b * Mp + qi) * ldo + h * D, g);
    }
}

// ---- attention_f32_kernel's family ----
template <int D>
void launch_main(const Call &c, const Launch &g) {
    hipLaunchKernelGGL(attention_f32_kernel<D>, dim3((unsigned)g.wgs), dim3(F_NT), flds_bytes(D), c.s, (const float *)c.q,
                       c.ldq, (const float *)c.k, c.ldk, (const float *)c.vt, c.ldvt, (float *)c.out, c.ldo, c.h, c.M, c.Mp,
                       c.Mk, c.Mkp, g.scale_log2e, g.src_batch, plan_args(c, g));
}

template <int D>
void launch_combine(const Call &c, const Launch &g) {
    hipLaunchKernelGGL(attention_f32_combine_kernel<D>, dim3((unsigned)g.split_items), dim3(F_NT), 0, c.s,
                       (float *)c.out, c.ldo, c.h, c.M, c.Mp, plan_args(c, g));
}

template <int D>
Family make_family() {
    Family f;
    f.name = "vtm_attention (fp32)";
    f.qb = fqb_for(D);
    f.wg_per_cu = fwg_per_cu(D);
    f.rec_bytes = (size_t)frec_size(D) * sizeof(float);
    // a device plan counts this kernel's 32-key tiles; the host plan (plan_tail) counts 64-key tiles in its thresholds and
    // the pieces are cut from 32-key tiles
    f.key_tile = KT;
    f.xcd_min_nqb = F_XCD_MIN_NQB;
    if constexpr (flds_bytes(D) > 64 * 1024) f.lds_opt_in = vtm::opt_in_lds<attention_f32_kernel<D>, flds_bytes(D)>;
    f.main = launch_main<D>;
    f.combine = launch_combine<D>;
    return f;
}

}  // namespace

namespace vtm_att {

int attention_f32(const Call &c, int64_t d) {
    VTM_REQUIRE((c.Mkp * c.ldk + d) * 4 < (1ll << 31) && (d * c.ldvt + c.Mkp) * 4 < (1ll << 31),
                "vtm_attention: a (sample, head) slice of fp32 K or V^T must stay below 2 GiB");
    return with_head_dim(d, [&](auto dim) { return planned_launch(c, make_family<decltype(dim)::value>()); });
}

size_t ws_bytes_f32(int64_t B, int64_t h, int64_t Mq, int64_t Mk, int64_t d, bool bounded) {
    if (B <= 0 || h <= 0 || Mq <= 0 || Mk <= 0) return 0;
    return with_head_dim(d, [&](auto dim) { return ws_bytes(make_family<decltype(dim)::value>(), B, h, Mq, Mk, bounded); });
}

}  // namespace vtm_att
