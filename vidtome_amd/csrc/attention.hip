// vtm_attention: flash-style self-attention over the MERGED token sequence (MFMA, fp16/bf16 in,
// fp32 accumulate).  Reference: the `self.attn1(...)` call at vidtome/patch.py:157-162; the arithmetic
// is the one the reference states itself in utils/pnp_utils.py:47-95 (`sa_forward`):
//     sim = einsum("b i d, b j d -> b i j", q, k) * scale;  attn = sim.softmax(-1);  out = attn @ v
// including its injection branch (probabilities of the source sample reused for every batch group).
//
// Structure:
//   * workgroup = 8 waves, each wave owns 32 query rows; K / V^T tiles of 64 keys are staged through
//     LDS (register-staged, double-buffered) and shared by the 8 waves; all per-thread global pointers
//     and LDS offsets are hoisted, full tiles run without any bounds logic, the ragged last tile has its
//     own masked path (sequence lengths are 34 816, 52 224, 8 704, 64 513 ...);
//   * "swapped" QK^T: S^T = K Q^T with v_mfma_f32_32x32x16 puts one query per lane (j = lane & 31) and
//     its 2 x 16 keys of the tile in that lane's accumulators -> online softmax is in-register, with ONE
//     cross-half exchange per tile for the running max;
//   * per score: one v_fma (scale folded, base 2) + one v_exp; the running max is only raised when it grew
//     by more than 2^8 (deferred rescale: P <= 256 is exact enough in fp16 and the O-rescale, which would
//     drag the accumulators through VALU every tile, becomes rare).  Head dims with a spare k-slot (d = 40)
//     carry the shift INSIDE the contraction (BIAS below): no v_fma, and the maximum is only checked
//     afterwards, on the packed P;
//   * P stays in registers: the PV contraction's k-slot <-> key assignment is chosen to be exactly the
//     one the S^T accumulator layout already has (keys 4*hi + {0..3} and 8 + 4*hi + {0..3} of every
//     16-key group), and V^T is read from LDS with the same assignment -- no permute / LDS round trip;
//   * V arrives TRANSPOSED (channel-major) from the projection GEMM, so V^T needs no transpose; when the
//     head dim leaves a spare row in the last row block of O^T (d = 40, 80), that V^T row is set to
//     ones, so the MFMA itself accumulates the softmax denominator from the SAME fp16-rounded P;
//   * d = 40 builds O^T from 16-row blocks (v_mfma_f32_16x16x32: 48 rows instead of 64, a quarter of the
//     PV matrix work gone); P^T moves from the 32-query accumulator layout to the two 16-query B operands
//     with v_permlane16_swap -- 8 swaps per tile, still no LDS round trip (PV16 below).
#include "attention_plan.h"
#include "attention_stage.h"

#include <algorithm>
#include <type_traits>

namespace {

// ---- the constants of attention_kernel's family, for its kernels and for make_family ----
constexpr int XCD_MIN_NQB = 64;                                                  // Family::xcd_min_nqb
constexpr int qb_for(int D) { return waves_for(D) * QW; }                        // query rows per workgroup
constexpr int64_t rec_size(int D) { return (int64_t)rec_floats(D) * (waves_for(D) * 64); }   // floats of a partial record

// merges the `nsplit` partial states of a query block (same thread <-> register mapping as attention_kernel)
template <typename T, int D>
__global__ __launch_bounds__(waves_for(D) * 64) void attention_combine_kernel(
    T *__restrict__ out, int64_t ldo, int64_t H, int64_t M, int64_t Mp, PlanArgs plan) {
    constexpr int WAVES = waves_for(D), NT = WAVES * 64, DV = (D + 31) / 32;
    constexpr bool PV16 = pv16_for(D);
    constexpr int NA = acc_floats(D), NM = max_floats(D);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const WorkItem w = decode_combine_item<qb_for(D), XCD_MIN_NQB>(plan, H, blockIdx.x);
    if (w.leave) return;
    const int64_t b = w.b, h = w.h, q0 = w.q0 + wave * QW;
    const int nsplit = w.nsplit;
    const float *partial = plan.partial_base + w.rec * rec_size(D);
    float acc[NA], m[NM], l = 0.0f;
#pragma unroll
    for (int r = 0; r < NA; ++r) acc[r] = 0.0f;
#pragma unroll
    for (int j = 0; j < NM; ++j) m[j] = -INFINITY;
    for (int sp = 0; sp < nsplit; ++sp) {
        const float *pp = partial + sp * rec_size(D) + tid;
        float fa[NM], fb[NM];
#pragma unroll
        for (int j = 0; j < NM; ++j) {
            const float ms = pp[(NA + j) * NT];
            const float mn = fmaxf(m[j], ms);
            fa[j] = __builtin_amdgcn_exp2f(m[j] - mn);   // exp2(-inf) = 0
            fb[j] = __builtin_amdgcn_exp2f(ms - mn);
            m[j] = mn;
        }
        l = l * fa[0] + pp[(NA + NM) * NT] * fb[0];
#pragma unroll
        for (int r = 0; r < NA; ++r) {
            const int j = PV16 ? (r >> 2) & 1 : 0;   // PV16: accumulator (dv, qh, e) is register (dv * 2 + qh) * 4 + e
            acc[r] = acc[r] * fa[j] + pp[r * NT] * fb[j];
        }
    }
    if constexpr (PV16) {
        f32x4 o[(D + 16) / 16][2];
#pragma unroll
        for (int r = 0; r < NA; ++r) o[r >> 3][(r >> 2) & 1][r & 3] = acc[r];
        write_output16<T, D>(o, out, ldo, b, h, q0, M, Mp, lane);
    } else {
        f32x16 o[DV];
#pragma unroll
        for (int r = 0; r < NA; ++r) o[r >> 4][r & 15] = acc[r];
        write_output<T, D>(o, l, out, ldo, b, h, q0, M, Mp, l31, hi);
    }
}

// attention_combine_kernel for FEW items (the split tail of a mid block: 16 items x 16 records leave 240 CUs idle and
// every thread walking 16 x 50 floats): blockIdx.y shares an item's accumulator registers out in groups of 8 (= two
// 4-channel groups of one query; 32-row O^T layout only), every part redoing the maxima / denominator bookkeeping.  Two
// passes -- the maxima first, then every record weighted by exp2(its maximum - the overall one) -- so that no load waits
// for arithmetic on an earlier record; the register group is addressed at run time, the 8 accumulators are static.
template <typename T, int D>
__global__ __launch_bounds__(waves_for(D) * 64) void attention_combine_parts_kernel(
    T *__restrict__ out, int64_t ldo, int64_t H, int64_t M, int64_t Mp, PlanArgs plan) {
    using elem = typename Frag<T>::elem;
    static_assert(!pv16_for(D), "32-row O^T layout");
    constexpr int WAVES = waves_for(D), NT = WAVES * 64;
    constexpr int NA = acc_floats(D), REC = rec_floats(D);
    constexpr bool SPARE = (D % 32) != 0;
    constexpr int LREG_ALL = SPARE ? (D / 32) * 16 + ((D % 32) & 3) + 4 * ((D % 32) >> 3) : 0;
    constexpr int LHI = ((D % 32) >> 2) & 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const WorkItem w = decode_combine_item<qb_for(D), XCD_MIN_NQB>(plan, H, blockIdx.x);   // (host plans only)
    if (w.leave) return;
    const int64_t b = w.b, h = w.h, q0 = w.q0 + wave * QW;
    const int nsplit = w.nsplit;
    const int r0 = (int)blockIdx.y * 8;
    const float *p0 = plan.partial_base + w.rec * rec_size(D) + tid;
    float m = -INFINITY;
#pragma unroll 4
    for (int sp = 0; sp < nsplit; ++sp) m = fmaxf(m, p0[((int64_t)sp * REC + NA) * NT]);
    float acc[8], den = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.0f;
#pragma unroll 4
    for (int sp = 0; sp < nsplit; ++sp) {
        const float *pp = p0 + (int64_t)sp * REC * NT;
        const float ms = pp[NA * NT];
        const float w = ms == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(ms - m);   // (a split that saw no key)
        den = __builtin_fmaf(pp[(SPARE ? LREG_ALL : NA + 1) * NT], w, den);       // the O^T denominator row / the fp32 sum
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(pp[(r0 + i) * NT], w, acc[i]);
    }
    const float l_tot = SPARE ? __shfl(den, l31 + 32 * LHI, 64) : den + __shfl_xor(den, 32, 64);
    const float inv_l = 1.0f / l_tot;
    const int64_t qi = q0 + l31;
    if (qi < M) {
        T *op = out + (b * Mp + qi) * ldo + h * D;
        const int dv = r0 >> 4, g0 = (r0 & 15) >> 2;
#pragma unroll
        for (int gi = 0; gi < 2; ++gi) {
            const int d0 = dv * 32 + 8 * (g0 + gi) + 4 * hi;
            if (d0 < D) {
                elem w4[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) w4[e] = (elem)(acc[gi * 4 + e] * inv_l);
                *reinterpret_cast<uint2 *>(op + d0) = *reinterpret_cast<uint2 *>(w4);
            }
        }
    }
}

template <typename T, int D, bool FOLD>
__global__ __launch_bounds__(waves_for(D) * 64, (D <= 48 ? 4 : D <= 96 ? 4 : 1)) void attention_kernel(
    const T *__restrict__ q, int64_t ldq, const T *__restrict__ k, int64_t ldk,
    const T *__restrict__ vt, int64_t ldvt, T *__restrict__ out, int64_t ldo, int64_t H,
    int64_t M, int64_t Mp, int64_t Mk_arg, int64_t Mkp, float scale_log2e, int64_t src_batch,
    const int32_t *__restrict__ k_count, const uint32_t *__restrict__ k_bias, int64_t ldkb, PlanArgs plan) {
    // M / Mp: queries per sample and their row stride; Mk / Mkp: keys per sample and the row stride of k
    // (self-attention passes the same values; cross-attention, patch.py:178-183, has Mk = 77).
    // Work decomposition: work item = (query block, head, sample), query blocks fastest (decode_work_item).  A workgroup
    // that covers the key tiles of one split of its item leaves its unnormalised accumulators, running max and
    // denominator in `partial` for attention_combine_kernel (used for the query blocks that do not fill a whole round of
    // the chip, see planned_launch).
    using F = Frag<T>;
    using vec = typename F::vec;
    using elem = typename F::elem;
    constexpr int WAVES = waves_for(D), NT = WAVES * 64;
    constexpr int DK = (D + 15) / 16;      // k-steps of the QK^T contraction
    constexpr int DV = (D + 31) / 32;      // 32-row blocks of O^T
    constexpr bool PV16 = pv16_for(D);     // ... or 16-row blocks (see pv16_for)
    constexpr int DV16 = (D + 16) / 16, VROWS = vrows_for(D);
    constexpr bool SPARE = (D % 32) != 0;  // O^T row D is free -> softmax denominator through the MFMA
    // BIAS: the QK^T contraction has a spare k-slot (D % 16 != 0, e.g. d = 40 -> 48).  Channel D of every K row is
    // set to 1 and channel D of the (pre-scaled) query to -m, so the MFMA itself delivers s * scale * log2(e) - m
    // and the softmax needs no v_fma per score (with 40-wide heads the kernel is VALU-bound).  The shift m only
    // has to be THE SAME for all keys of a query -- it cancels in the normalisation -- so an fp16-representable
    // running max is as good as the exact one; the scale is folded into the query fragment (one extra fp16
    // rounding of q, the same size as the rounding the projection GEMM already applied).
    constexpr bool BIAS = (D % 16) != 0;
    constexpr int BIAS_HI = (D % 16) / 8, BIAS_E = D % 8;   // lane half / fragment element holding channel D
    // FOLD (vtm_attention_kv_folded): the key list is duplicate-free, key j stands for 2^bias_j identical keys of the merged
    // sequence (vtm_fold_keys); the bias rides in two more spare k-slots (channels D + 2, D + 3 of the K row = hi + lo of
    // log2(multiplicity), against ones in the query), and the number of keys is a DEVICE value (k_count[b] <= Mk_arg).
    static_assert(!FOLD || (BIAS && D % 8 == 0 && D % 16 == 8), "key folding needs the spare k-slots of a d % 16 == 8 head");
    using Stage = KvStage<T, D, NT>;
    constexpr int K_STRIDE = Stage::K_STRIDE;
    constexpr int SK_TILE = KV * K_STRIDE, SV_TILE = VROWS * VT_STRIDE;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    elem *sK = reinterpret_cast<elem *>(smem);   // [2][KV][K_STRIDE]
    elem *sV = sK + 2 * SK_TILE;                 // [2][VROWS][VT_STRIDE]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int l15 = lane & 15, g16 = lane >> 4;   // PV16 operand coordinates
    const WorkItem w = decode_work_item<qb_for(D), XCD_MIN_NQB>(plan, H, blockIdx.x);
    if (w.leave) return;
    const int nsplit = w.nsplit, split = w.split;
    float *partial = w.rec >= 0 ? plan.partial_base + w.rec * rec_size(D) : nullptr;
    const int64_t b = w.b, h = w.h;
    const int64_t bq = b % src_batch;  // PnP injection: q/k of the source sample (pnp_utils.py:57-67)
    const int64_t q0 = w.q0 + wave * QW;
    const int64_t C = H * D;
    int64_t Mk = Mk_arg;
    if constexpr (FOLD) {
        const int64_t kc = k_count[b];
        Mk = kc < Mk_arg ? (kc > 0 ? kc : 1) : Mk_arg;
    }

    // one-time LDS init: K pad columns = 0 (they meet Q's zero padding; garbage could be NaN), V^T pad rows
    // = 0 except row D = 1 (denominator row) -- tile loads never touch these.  FOLD: not the bias pair D + 2, D + 3, which
    // every tile's staging writes (wave 0, write_lds) -- with no barrier in between, a late store here could overwrite the
    // first tile's bias words with 0 and drop the copies of its keys
    for (int i = tid; i < 2 * KV * (K_STRIDE - D); i += NT) {
        const int row = i / (K_STRIDE - D), c = D + i % (K_STRIDE - D);
        if (FOLD && (c == D + 2 || c == D + 3)) continue;
        sK[row * K_STRIDE + c] = (elem)((BIAS && c == D) ? 1.0f : 0.0f);
    }
    if constexpr (VROWS > D) {
        for (int i = tid; i < 2 * (VROWS - D) * VT_STRIDE; i += NT) {
            const int bufi = i / ((VROWS - D) * VT_STRIDE), rem = i % ((VROWS - D) * VT_STRIDE);
            const int row = D + rem / VT_STRIDE, c = rem % VT_STRIDE;
            sV[bufi * SV_TILE + row * VT_STRIDE + c] = (elem)((row == D) ? 1.0f : 0.0f);
        }
    }

    vec qf[DK];
    {
        const int64_t qi = q0 + l31;
        load_q_frags<T, D>(qf, q + (bq * Mp + (qi < M ? qi : 0)) * ldq + h * D, qi < M, hi);
        if constexpr (BIAS) {
#pragma unroll
            for (int ks = 0; ks < DK; ++ks)
#pragma unroll
                for (int e = 0; e < 8; ++e) qf[ks][e] = (elem)((float)qf[ks][e] * scale_log2e);
        }
        if constexpr (FOLD) {   // channels D + 2, D + 3 (lane half BIAS_HI, elements BIAS_E + 2, + 3) meet the key's bias pair
            if (hi == BIAS_HI) {
                qf[DK - 1][BIAS_E + 2] = (elem)1.0f;
                qf[DK - 1][BIAS_E + 3] = (elem)1.0f;
            }
        }
    }

    // the tile stage: the scalar tile offsets advance by 64 rows / 64 keys per tile
    Stage stage;
    stage.init(tid, ldk, ldvt);
    const auto rsrc_k = kv_rsrc(k + bq * Mkp * ldk + h * D), rsrc_v = kv_rsrc(vt + (b * C + h * D) * ldvt);
    const uint32_t kstep = (uint32_t)(KV * ldk) * 2u, vstep = (uint32_t)KV * 2u;   // bytes per tile
    uint32_t so_k = 0, so_v = 0;                                                    // scalar tile offsets (bytes)
    // FOLD: the first wave also stages the tile's 64 bias words (one per key) into the K rows
    const auto rsrc_b = kv_rsrc(FOLD ? k_bias + b * ldkb : nullptr);
    uint32_t so_b = 0, rbias = 0;
    [[maybe_unused]] const uint32_t bgo = (uint32_t)(tid & (KV - 1)) * 4u;

    auto issue_full = [&]() {   // tile completely inside [0, Mk): no bounds logic
        stage.issue_full(rsrc_k, rsrc_v, so_k, so_v);
        if constexpr (FOLD) {   // (every wave fetches the 64 words -- no load behind a branch -- the first one stores them)
            rbias = __builtin_amdgcn_raw_buffer_load_b32(rsrc_b, bgo, so_b, 0);
            so_b += (uint32_t)KV * 4u;
        }
        so_k += kstep;
        so_v += vstep;
    };
    auto issue_tail = [&](int64_t key0) {   // ragged last tile: rows / keys >= Mk read as zero
        stage.issue_masked(rsrc_k, rsrc_v, so_k, so_v, key0, Mk);
        if constexpr (FOLD) {
            rbias = 0u;
            if (key0 + (tid & (KV - 1)) < Mk) rbias = __builtin_amdgcn_raw_buffer_load_b32(rsrc_b, bgo, so_b, 0);
        }
    };
    auto write_lds = [&](int buf) {
        elem *dk = sK + buf * SK_TILE;
        if constexpr (FOLD) {
            if (wave == 0) *reinterpret_cast<uint32_t *>(dk + tid * K_STRIDE + D + 2) = rbias;
        }
        stage.write(dk, sV + buf * SV_TILE);
    };

    f32x16 o[PV16 ? 1 : DV];          // 32-row blocks: o[dv][r] = row 32 dv + (r & 3) + 8 (r >> 2) + 4 hi of query l31
    f32x4 o16[PV16 ? DV16 : 1][2];    // PV16: o16[dv][qh][e] = row 16 dv + 4 g16 + e of query 16 qh + l15
#pragma unroll
    for (int dv = 0; dv < (PV16 ? 1 : DV); ++dv)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dv][r] = 0.0f;
#pragma unroll
    for (int dv = 0; dv < (PV16 ? DV16 : 1); ++dv)
#pragma unroll
        for (int qh = 0; qh < 2; ++qh)
#pragma unroll
            for (int e = 0; e < 4; ++e) o16[dv][qh][e] = 0.0f;
    // O^T *= alpha (alpha is per query, in the S^T layout: lane l31 and l31 + 32 hold the same value)
    auto rescale = [&](float alpha) {
        if constexpr (PV16) {
#pragma unroll
            for (int qh = 0; qh < 2; ++qh) {
                const float a = __shfl(alpha, 16 * qh + l15, 64);
#pragma unroll
                for (int dv = 0; dv < DV16; ++dv)
#pragma unroll
                    for (int e = 0; e < 4; ++e) o16[dv][qh][e] *= a;
            }
        } else {
#pragma unroll
            for (int dv = 0; dv < DV; ++dv)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[dv][r] *= alpha;
        }
    };
    float m_run = -INFINITY;   // running max in scaled (log2) units
    float m_bias = 0.0f;       // BIAS: the fp16-representable shift currently held in channel D of the query
    float l_run = 0.0f;        // only used when there is no spare O^T row

    // one tile: S^T = K Q^T -> online softmax -> O^T += V^T P^T.  TAIL = the ragged last tile (keys >= M masked).
    auto tile = [&](auto tail_tag, int buf, int64_t key0) {
        constexpr bool TAIL = decltype(tail_tag)::value;
        // ---- S^T = K Q^T : 2 blocks of 32 keys
        f32x16 s[2];
        auto compute_s = [&]() {
            if constexpr (PV16) {
                // the two 32-key blocks one after the other: the exps of the first start beside the MFMAs of the second
                vec kf[2][DK];
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    const elem *kp = sK + buf * SK_TILE + (kb * 32 + l31) * K_STRIDE + hi * 8;
#pragma unroll
                    for (int ks = 0; ks < DK; ++ks) kf[kb][ks] = *reinterpret_cast<const vec *>(kp + ks * 16);
                }
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[kb][r] = 0.0f;
#pragma unroll
                    for (int ks = 0; ks < DK; ++ks) s[kb] = F::mfma(kf[kb][ks], qf[ks], s[kb]);
                }
                __builtin_amdgcn_sched_barrier(0);
            } else {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[kb][r] = 0.0f;
                const elem *kp = sK + buf * SK_TILE + (kb * 32 + l31) * K_STRIDE + hi * 8;
#pragma unroll
                for (int ks = 0; ks < DK; ++ks)
                    s[kb] = F::mfma(*reinterpret_cast<const vec *>(kp + ks * 16), qf[ks], s[kb]);
            }
            }
            if constexpr (TAIL) {   // lane (l31, hi) holds keys key0 + 32 kb + (r & 3) + 8 (r >> 2) + 4 hi
                const int lim = (int)(Mk - key0);
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi >= lim) s[kb][r] = -INFINITY;
            }
        };

        // ---- online softmax, base 2, deferred rescale: raises the shift when this tile's maximum outgrew it
        auto raise_shift = [&]() {
            float mt = fmaxf(s[0][0], s[1][0]);
#pragma unroll
            for (int r = 1; r < 16; ++r) mt = fmaxf(fmaxf(mt, s[0][r]), s[1][r]);
            if constexpr (BIAS) {
                // scores arrive as s c - m_bias: mt is the growth over the current shift (m_run = -inf only before
                // the first tile, which therefore always takes the branch and installs its own maximum)
                mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
                if (!__all(m_bias + mt <= m_run + DEFER_THR)) {
                    const float m_new = (float)(elem)(fmaxf(m_run, m_bias + mt));   // fp16-representable
                    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);      // first tile: exp2(-inf) = 0
                    const float delta = m_bias - m_new;                             // exact: both are fp16 values
                    m_run = m_new;
                    m_bias = m_new;
                    l_run *= alpha;
                    rescale(alpha);
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                        for (int r = 0; r < 16; ++r) s[kb][r] += delta;   // this tile was computed with the old shift
                    if (hi == BIAS_HI) qf[DK - 1][BIAS_E] = (elem)(-m_new);
                }
            } else {
                mt = fmaxf(mt, __shfl_xor(mt, 32, 64)) * scale_log2e;
                if (!__all(mt <= m_run + DEFER_THR)) {
                    const float m_new = fmaxf(m_run, mt);
                    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // first tile: exp2(-inf) = 0
                    m_run = m_new;
                    l_run *= alpha;
                    rescale(alpha);
                }
            }
        };
        vec pf[4];
        auto softmax_step = [&](int st) {   // p of keys 16 st + (e & 3) + 8 (e >> 2) + 4 hi
            float p[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float sv = s[st >> 1][8 * (st & 1) + e];
                p[e] = __builtin_amdgcn_exp2f(BIAS ? sv : __builtin_fmaf(sv, scale_log2e, -m_run));
                if constexpr (!SPARE) l_run += p[e];
            }
            F::pack8(pf[st], p);
        };
        compute_s();
        if constexpr (PV16) {
            static_assert(BIAS, "16-row O^T blocks imply a spare k-slot");
            // The shift already rides in the MFMA, so the exps run FIRST and the maximum is taken afterwards, on the
            // packed P (8 packed 3-input maxima instead of 16 fp32 ones, and no cross-half exchange): P <= 2^8 means
            // the shift still holds.  Otherwise -- the first tile, or scores that outgrew the shift by more than
            // 2^8, possibly up to inf in P -- the tile is redone the exact way: scores again, maximum, new shift.
            const elem *vp = sV + buf * SV_TILE + l15 * VT_STRIDE + (g16 & 1) * 16 + (g16 >> 1) * 8;
#pragma unroll
            for (int st = 0; st < 4; ++st) softmax_step(st);
            uint32_t pw[16];
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const u32x4 w = __builtin_bit_cast(u32x4, pf[st]);
#pragma unroll
                for (int j = 0; j < 4; ++j) pw[4 * st + j] = w[j];
            }
#pragma unroll
            for (int j = 0; j < 5; ++j) pw[j] = F::pmax3(pw[3 * j], pw[3 * j + 1], pw[3 * j + 2]);   // 16 -> 5 + 1
            const uint32_t pr = F::pmax3(F::pmax3(pw[0], pw[1], pw[2]), F::pmax3(pw[3], pw[4], pw[15]), pw[15]);
            const uint32_t ptop = max(pr >> 16, pr & 0xffffu);
            if (__any(ptop > F::BITS_256 || m_run == -INFINITY)) {
                compute_s();
                raise_shift();
#pragma unroll
                for (int st = 0; st < 4; ++st) softmax_step(st);
            }
            // ---- O^T += V^T P^T in 16-row blocks: 2 steps of 32 keys.  After the swaps pf[2 ks] / pf[2 ks + 1] are
            // the B operands of queries 0-15 / 16-31: k-slot group g16 holds the keys of 16-key group
            // 2 ks + (g16 & 1), lane half g16 >> 1 -- in the V^T tile that is ONE 16-byte piece (see voff)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                vec a[DV16];
#pragma unroll
                for (int dv = 0; dv < DV16; ++dv)
                    a[dv] = *reinterpret_cast<const vec *>(vp + ks * 32 + dv * 16 * VT_STRIDE);
                u32x4 x = __builtin_bit_cast(u32x4, pf[2 * ks]), y = __builtin_bit_cast(u32x4, pf[2 * ks + 1]);
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const auto r = __builtin_amdgcn_permlane16_swap(x[w], y[w], false, false);
                    x[w] = r[0];
                    y[w] = r[1];
                }
                const vec p0 = __builtin_bit_cast(vec, x), p1 = __builtin_bit_cast(vec, y);
#pragma unroll
                for (int dv = 0; dv < DV16; ++dv) {
                    o16[dv][0] = F::mfma16(a[dv], p0, o16[dv][0]);
                    o16[dv][1] = F::mfma16(a[dv], p1, o16[dv][1]);
                }
            }
        } else {
            raise_shift();
#pragma unroll
            for (int st = 0; st < 4; ++st) softmax_step(st);
            // ---- O^T += V^T P^T : 4 steps of 16 keys; k-slot (hi, e) <-> key 16 st + 8 (e >> 2) + 4 hi + (e & 3)
#pragma unroll
            for (int dv = 0; dv < DV; ++dv) {
                const elem *vp = sV + buf * SV_TILE + (dv * 32 + l31) * VT_STRIDE + 8 * hi;
#pragma unroll
                for (int st = 0; st < 4; ++st)
                    o[dv] = F::mfma(*reinterpret_cast<const vec *>(vp + st * 16), pf[st], o[dv]);
            }
        }
    };
    using std::false_type;
    using std::true_type;

    const int ntiles = (int)((Mk + KV - 1) / KV), nfull = (int)(Mk / KV);
    const int tps = (ntiles + nsplit - 1) / nsplit;                         // key tiles per split
    const int tb = split * tps, te = tb + tps < ntiles ? tb + tps : ntiles;
    const int fe = te < nfull ? te : nfull;                                 // end of the full tiles of this range
    so_k = (uint32_t)tb * kstep;
    so_v = (uint32_t)tb * vstep;
    so_b = (uint32_t)tb * (uint32_t)KV * 4u;
    if (tb < fe) issue_full(); else issue_tail((int64_t)tb * KV);
    write_lds(0);
    __syncthreads();

    // hot loop: full tiles whose successor is full too -- no bounds logic of any kind inside
    int t = tb;
    int buf = 0;
    for (; t + 1 < fe; ++t) {
        issue_full();
        tile(false_type{}, buf, (int64_t)t * KV);
        write_lds(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    if (t < fe) {               // last full tile; prefetches the ragged tile if it belongs to this range
        const bool ragged_next = te > fe;
        if (ragged_next) issue_tail((int64_t)fe * KV);
        tile(false_type{}, buf, (int64_t)t * KV);
        if (ragged_next) write_lds(buf ^ 1);
        __syncthreads();
        ++t;
        buf ^= 1;
    }
    if (t < te) tile(true_type{}, buf, (int64_t)t * KV);

    if (partial) {   // split workgroup: hand the raw state to attention_combine_kernel
        constexpr int NA = acc_floats(D), NM = max_floats(D);
        float *pp = partial + tid;
        if constexpr (PV16) {
#pragma unroll
            for (int r = 0; r < NA; ++r) pp[r * NT] = o16[r >> 3][(r >> 2) & 1][r & 3];
#pragma unroll
            for (int qh = 0; qh < 2; ++qh) pp[(NA + qh) * NT] = __shfl(m_run, 16 * qh + l15, 64);
        } else {
#pragma unroll
            for (int r = 0; r < NA; ++r) pp[r * NT] = o[r >> 4][r & 15];
            pp[NA * NT] = m_run;
        }
        pp[(NA + NM) * NT] = l_run;
        return;
    }
    if constexpr (PV16)
        write_output16<T, D>(o16, out, ldo, b, h, q0, M, Mp, lane);
    else
        write_output<T, D>(o, l_run, out, ldo, b, h, q0, M, Mp, l31, hi);
}

// ---- attention_kernel's family ----
constexpr size_t lds_for(int D) { return (size_t)2 * (KV * ((D + 15) / 16 * 16 + 8) + vrows_for(D) * VT_STRIDE) * 2; }

template <typename T, int D, bool FOLD>
void launch_main(const Call &c, const Launch &g) {
    hipLaunchKernelGGL((attention_kernel<T, D, FOLD>), dim3((unsigned)g.wgs), dim3(waves_for(D) * 64), lds_for(D), c.s,
                       (const T *)c.q, c.ldq, (const T *)c.k, c.ldk, (const T *)c.vt, c.ldvt, (T *)c.out, c.ldo, c.h, c.M, c.Mp,
                       c.Mk, c.Mkp, g.scale_log2e, g.src_batch, c.k_count, c.k_bias, c.ldkb, plan_args(c, g));
}

template <typename T, int D>
void launch_combine(const Call &c, const Launch &g) {
    if constexpr (!pv16_for(D) && acc_floats(D) % 8 == 0) {
        // few items of a host plan: their accumulator groups are shared out (attention_combine_parts_kernel)
        if (g.plan == nullptr && g.split_items * 4 <= vtm::device_cus()) {
            hipLaunchKernelGGL((attention_combine_parts_kernel<T, D>), dim3((unsigned)g.split_items, (unsigned)(acc_floats(D) / 8)),
                               dim3(waves_for(D) * 64), 0, c.s, (T *)c.out, c.ldo, c.h, c.M, c.Mp, plan_args(c, g));
            return;
        }
    }
    hipLaunchKernelGGL((attention_combine_kernel<T, D>), dim3((unsigned)g.split_items), dim3(waves_for(D) * 64), 0, c.s,
                       (T *)c.out, c.ldo, c.h, c.M, c.Mp, plan_args(c, g));
}

template <typename T, int D, bool FOLD = false>
Family make_family() {
    Family f;
    f.qb = qb_for(D);
    f.wg_per_cu = D <= 48 ? 2 : 1;
    f.rec_bytes = (size_t)rec_size(D) * sizeof(float);
    f.xcd_min_nqb = XCD_MIN_NQB;
    f.ws_devplan_min_tiles = 16;
    if constexpr (lds_for(D) > 64 * 1024) f.lds_opt_in = vtm::opt_in_lds<attention_kernel<T, D, FOLD>, lds_for(D)>;
    f.main = launch_main<T, D, FOLD>;
    f.combine = launch_combine<T, D>;
    return f;
}

// Which launches go to the wide-tile d = 40 kernels (round 6): self-attention to attention16s_kernel (attention16.hip, which
// also takes every folded d = 40 launch: vtm_attention_kv_folded), shared probabilities of 2 or 3 groups to attention16g_kernel
// (attention16g.hip).  -> the value groups per wave of the wide kernel, 0 for attention_kernel
int shape16_for(int64_t d, int share_groups, int dtype) {
    if (d != 40 || (dtype != VTM_F16 && dtype != VTM_BF16)) return 0;
    return share_groups <= 3 ? share_groups : 0;
}

// the workspace of the largest plan a 16-bit call of this shape can take (d = 40: the caller does not say how the launch will
// share its probabilities -- attention_kernel, attention16s_kernel or attention16g_kernel); no size depends on the element type
size_t ws_bytes_any(int64_t B, int64_t h, int64_t Mq, int64_t Mk, int64_t d, bool bounded) {
    if (B <= 0 || h <= 0 || Mq <= 0 || Mk <= 0) return 0;
    return with_head_dim(d, [&](auto dim) {
        constexpr int D = decltype(dim)::value;
        size_t n = ws_bytes(make_family<__half, D>(), B, h, Mq, Mk, bounded);
        if constexpr (D == 40) {
            n = std::max(n, ws_bytes(family16s(VTM_F16, false), B, h, Mq, Mk, bounded));
            for (int ng = 2; ng <= 3; ++ng)
                if (B % ng == 0) n = std::max(n, ws_bytes(family16g(VTM_F16, ng), B, h, Mq, Mk, bounded));
        }
        return n;
    });
}

// The argument checks of every attention export; `who` names the export in the messages.  Folded keys (c.fold) also need
// their counts and bias rows and a head dim with spare k-slots.
int check_call(const Call &c, int64_t d, const char *who) {
    VTM_REQUIRE(c.q && c.k && c.vt && c.out && (!c.fold || (c.k_count && c.k_bias)), "%s: null pointer", who);
    // (a folded head dim is checked against 8 and 40 below)
    VTM_REQUIRE(c.B > 0 && c.h > 0 && c.M > 0 && c.Mk > 0 && c.Mp >= c.M && c.Mkp >= c.Mk && (c.fold ? c.ldkb >= c.Mk : d > 0),
                "%s: bad sizes", who);
    VTM_REQUIRE(c.share_groups >= 1 && c.B % c.share_groups == 0, "%s: B %% share_groups != 0", who);
    if (c.fold)
        VTM_REQUIRE(d == 40 || d == 8, "%s: head dim %lld has no spare k-slots for the bias (d = 8, 40 do)", who, (long long)d);
    VTM_REQUIRE(c.ldq % 8 == 0 && c.ldk % 8 == 0 && c.ldvt % 8 == 0 && c.ldo % 4 == 0 && c.ldvt >= c.Mk,
                "%s: leading dimensions must keep 16-byte alignment (ldvt >= Mk, %% 8)", who);
    // K / V^T tiles are addressed with 32-bit byte offsets inside one (sample, head) slice (buffer loads)
    VTM_REQUIRE((c.Mkp * c.ldk + d) * 2 < (1ll << 31) && (d * c.ldvt + c.Mkp) * 2 < (1ll << 31) &&
                    (!c.fold || c.Mkp * 4 < (1ll << 31)),
                "%s: a (sample, head) slice of K or V^T must stay below 2 GiB", who);
    return VTM_OK;
}

}  // namespace

VTM_EXPORT size_t vtm_attention_ws_bytes(int64_t B, int64_t h, int64_t Mq, int64_t Mk, int64_t d) {
    return ws_bytes_any(B, h, Mq, Mk, d, false);
}

VTM_EXPORT size_t vtm_attention_kv_bounded_ws_bytes(int64_t B, int64_t h, int64_t Mq, int64_t Mk, int64_t d) {
    return ws_bytes_any(B, h, Mq, Mk, d, true);
}

// ... for a call of element type `dtype`: VTM_F32 launches go to attention_f32_kernel's family, whose plans are its own
VTM_EXPORT size_t vtm_attention_ws_bytes_dtype(int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mk, int64_t d) {
    return dtype == VTM_F32 ? ws_bytes_f32(B, h, Mq, Mk, d, false) : ws_bytes_any(B, h, Mq, Mk, d, false);
}

VTM_EXPORT size_t vtm_attention_kv_bounded_ws_bytes_dtype(int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mk, int64_t d) {
    return dtype == VTM_F32 ? ws_bytes_f32(B, h, Mq, Mk, d, true) : ws_bytes_any(B, h, Mq, Mk, d, true);
}

static int attention_any(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt, int64_t ldvt,
                         void *out, int64_t ldo, int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mqp, int64_t Mk,
                         int64_t Mkp, int64_t d, float scale, int share_groups, void *ws, size_t ws_bytes,
                         const int32_t *q_count, vtm_stream_t stream) {
    const Call c{q, ldq, k, ldk, vt, ldvt, out, ldo, dtype, B, h, Mq, Mqp, Mk, Mkp, scale, share_groups, ws, ws_bytes,
                 q_count, vtm::as_stream(stream), false, nullptr, nullptr, 0};
    if (const int e = check_call(c, d, "vtm_attention")) return e;
    if (dtype == VTM_F32) return attention_f32(c, d);   // (attention_f32.hip: fp32 operands on the f32 MFMA)
    const int ng = shape16_for(d, share_groups, dtype);
    if (ng == 1) return attention16(c);
    // the value groups of one (source sample, head) share a buffer descriptor: the sample stride rides in the offset
    if (ng > 1 && (ng * (B / share_groups) * h * d * ldvt) * 2 < (1ll << 31)) return attention16g(c, ng);
    if (dtype != VTM_F16 && dtype != VTM_BF16)
        return vtm::fail(VTM_EINVAL, "vtm_attention: dtype must be VTM_F16, VTM_BF16 or VTM_F32");
    return with_head_dim(d, [&](auto dim) {
        constexpr int D = decltype(dim)::value;
        return planned_launch(c, dtype == VTM_F16 ? make_family<__half, D>() : make_family<vtm_bf16, D>());
    });
}

VTM_EXPORT int vtm_attention_kv(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt, int64_t ldvt,
                                void *out, int64_t ldo, int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mqp, int64_t Mk,
                                int64_t Mkp, int64_t d, float scale, int share_groups, void *ws, size_t ws_bytes,
                                vtm_stream_t stream) {
    return attention_any(q, ldq, k, ldk, vt, ldvt, out, ldo, dtype, B, h, Mq, Mqp, Mk, Mkp, d, scale, share_groups, ws,
                         ws_bytes, nullptr, stream);
}

VTM_EXPORT int vtm_attention_kv_bounded(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt, int64_t ldvt,
                                        void *out, int64_t ldo, int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mqp,
                                        int64_t Mk, int64_t Mkp, int64_t d, float scale, const int32_t *q_count, void *ws,
                                        size_t ws_bytes, vtm_stream_t stream) {
    VTM_REQUIRE(q_count, "vtm_attention_kv_bounded: null q_count");
    return attention_any(q, ldq, k, ldk, vt, ldvt, out, ldo, dtype, B, h, Mq, Mqp, Mk, Mkp, d, scale, 1, ws, ws_bytes,
                         q_count, stream);
}

VTM_EXPORT int vtm_attention_kv_shared_bounded(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt, int64_t ldvt,
                                               void *out, int64_t ldo, int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mqp,
                                               int64_t Mk, int64_t Mkp, int64_t d, float scale, int share_groups,
                                               const int32_t *q_count, void *ws, size_t ws_bytes, vtm_stream_t stream) {
    VTM_REQUIRE(q_count, "vtm_attention_kv_shared_bounded: null q_count");
    VTM_REQUIRE(share_groups >= 1 && B % share_groups == 0, "vtm_attention_kv_shared_bounded: B %% share_groups != 0");
    // (d = 40, 2 or 3 groups: attention16g computes the probabilities once per group and reads the source sample's count;
    // other shapes: attention_kernel recomputes them per sample and reads every sample's own -- equal -- count)
    return attention_any(q, ldq, k, ldk, vt, ldvt, out, ldo, dtype, B, h, Mq, Mqp, Mk, Mkp, d, scale, share_groups, ws, ws_bytes,
                         q_count, stream);
}

VTM_EXPORT int vtm_attention_kv_folded(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt, int64_t ldvt,
                                       void *out, int64_t ldo, int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mqp,
                                       int64_t Mk, int64_t Mkp, int64_t d, float scale, const int32_t *q_count,
                                       const int32_t *k_count, const uint32_t *k_bias, int64_t ldkb, void *ws, size_t ws_bytes,
                                       vtm_stream_t stream) {
    const Call c{q, ldq, k, ldk, vt, ldvt, out, ldo, dtype, B, h, Mq, Mqp, Mk, Mkp, scale, 1, ws, ws_bytes,
                 q_count, vtm::as_stream(stream), true, k_count, k_bias, ldkb};
    if (const int e = check_call(c, d, "vtm_attention_kv_folded")) return e;
    if (dtype == VTM_F32) return vtm::fail(VTM_EINVAL, "vtm_attention_kv_folded: fp32 keys are never folded (dtype must be VTM_F16 or VTM_BF16)");
    if (dtype != VTM_F16 && dtype != VTM_BF16) return vtm::fail(VTM_EINVAL, "vtm_attention_kv_folded: dtype must be VTM_F16 or VTM_BF16");
    if (d == 40) return attention16(c);   // attention16s_kernel; d = 8: attention_kernel
    return planned_launch(c, dtype == VTM_F16 ? make_family<__half, 8, true>() : make_family<vtm_bf16, 8, true>());
}

VTM_EXPORT int vtm_attention(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt,
                             int64_t ldvt, void *out, int64_t ldo, int dtype, int64_t B, int64_t h, int64_t M,
                             int64_t Mp, int64_t d, float scale, int share_groups, void *ws, size_t ws_bytes,
                             vtm_stream_t stream) {
    return vtm_attention_kv(q, ldq, k, ldk, vt, ldvt, out, ldo, dtype, B, h, M, Mp, M, Mp, d, scale, share_groups, ws,
                            ws_bytes, stream);
}
