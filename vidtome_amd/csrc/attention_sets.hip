// vtm_attention_kv_sets: cross-attention over SEVERAL key sets, one softmax per set, the sets added with weights:
//     out[b, i, head] = sum_s w_s * softmax_{j in set s}(q[b, i, head] . k[b, j, head] * scale) v[b, j, head]
// This is the "decoupled cross-attention" an image-prompt adapter adds to attn2 (vidtome/patch.py:178-183 is the call it
// stands beside): set 0 = the text tokens, one more set per loaded adapter, all with the same q.  Composed from
// vtm_attention_kv it costs 1 + n launches that each read all of q and write all of out, plus the adds; here a workgroup
// keeps its query fragments, walks the sets and writes out once.
// vtm_attention_kv_sets_masked is the same kernel with a weight per QUERY on chosen sets, w_s * mask_s[b, i]: Diffusers'
// IP-Adapter region masks (one image prompt per region of the frame; every masked image is a set of its own).
// vtm_attention_kv_sets_src is the same kernel with a second QUERY operand for chosen sets: Prompt-to-Prompt's edited
// cross-attention, where one softmax of an edited sample is the source sample's (vidtome_amd/p2p.py).
//
// Structure (the building blocks of attention.hip, without what a few hundred keys do not need -- no key split, no
// workspace, no spare-slot tricks):
//   * workgroup = waves of 32 query rows; the K / V^T tiles of 64 keys are staged through LDS and shared by the waves, the
//     next tile's global loads in flight in registers while the current one is computed; a tile never crosses a set;
//   * S^T = K Q^T on v_mfma_f32_32x32x16 (one query per lane), online softmax in registers, base 2, deferred rescale; P
//     is rounded to the operand type for the PV contraction (bf16: as a hi + lo pair, two MFMAs) and the DENOMINATOR is
//     summed from the same rounded P;
//   * every tile is loaded through the masked path (keys outside [start_s, start_s + len_s) are never fetched as keys and
//     are zeroed as values): the key axis is 2 - 10 tiles long, bounds logic is not what this kernel waits for;
//   * per set: running max, denominator and fp32 accumulators of its own; at the end of the set they are folded into a
//     second fp32 accumulator as w_s / l_s; that sum is rounded to the output type once.
#include "attention_checks.h"
#include "attention_stage.h"

#include <cmath>

namespace {

// Two accumulator sets (the running set's and the weighted sum) double the register budget of attention_kernel: 8 waves
// (2 per SIMD, 256 VGPRs) up to d = 96, 4 waves above.
constexpr int sets_waves(int D) { return D <= 96 ? 8 : 4; }
// resident workgroups per CU (the launch bounds' waves per SIMD follow from it): d = 40 and 64 need 168 VGPRs and spill at 128
constexpr int sets_wg_per_cu(int D) { return D <= 32 ? 2 : 1; }
constexpr int sets_qb(int D) { return sets_waves(D) * QW; }   // query rows per workgroup

// With one trailing SetMasks argument (MASKED) set s is weighted per query, w_s * mask_s[query]: the kernel of
// vtm_attention_kv_sets_masked.  Without it the kernel is instruction for instruction what it was before the flag.
__device__ __forceinline__ const SetMasks *masks_of() { return nullptr; }
__device__ __forceinline__ const SetMasks *masks_of(const SetMasks &m) { return &m; }
__device__ __forceinline__ const SetMasks *masks_of(const SetSrc &) { return nullptr; }
// With one trailing SetSrc argument (SRC) chosen sets take their query rows from a second operand: the kernel of
// vtm_attention_kv_sets_src.  The workgroup keeps ONE set of query fragments and reloads it where the running set's
// operand differs from the one before it (a workgroup meets each set once; 168 VGPRs at d = 40 / 64 leave no room for
// a second set of fragments at 2 waves per SIMD).
__device__ __forceinline__ const SetSrc *src_of() { return nullptr; }
__device__ __forceinline__ const SetSrc *src_of(const SetMasks &) { return nullptr; }
__device__ __forceinline__ const SetSrc *src_of(const SetSrc &s) { return &s; }
// The reload does not fit the 128 VGPRs of two resident workgroups at d <= 32 (fp16 d = 8 spills 6 registers): the SRC
// kernels keep one workgroup per CU at every head dim.  Stable Diffusion's head dims (40, 64, 80, 160) run at one anyway.
template <typename... Masks>
constexpr int sets_wg_per_cu_of(int D) {
    return (std::is_same_v<Masks, SetSrc> || ...) ? 1 : sets_wg_per_cu(D);
}

template <typename T, int D, typename... Masks>
__global__ __launch_bounds__(sets_waves(D) * 64, sets_wg_per_cu_of<Masks...>(D) * sets_waves(D) / 4) void attention_sets_kernel(
    const T *__restrict__ q, int64_t ldq, const T *__restrict__ k, int64_t ldk, const T *__restrict__ vt, int64_t ldvt,
    T *__restrict__ out, int64_t ldo, int64_t H, int64_t M, int64_t Mp, int64_t Mkp, float scale_log2e, int64_t nqb,
    int xcd_groups, KeySets sets, Masks... masks_arg) {
    static_assert(sizeof...(Masks) <= 1, "at most one SetMasks or SetSrc");
    constexpr bool MASKED = (std::is_same_v<Masks, SetMasks> || ...);
    constexpr bool SRC = (std::is_same_v<Masks, SetSrc> || ...);
    using F = Frag<T>;
    using vec = typename F::vec;
    using elem = typename F::elem;
    constexpr int WAVES = sets_waves(D), NT = WAVES * 64;
    using Stage = KvStage<T, D, NT>;
    constexpr int DK = Stage::DK;          // k-steps of the QK^T contraction
    constexpr int DV = (D + 31) / 32;      // 32-row blocks of O^T
    constexpr int VROWS = DV * 32;
    constexpr int K_STRIDE = Stage::K_STRIDE;

    __shared__ __attribute__((aligned(16))) elem sK[KV * K_STRIDE];
    __shared__ __attribute__((aligned(16))) elem sV[VROWS * VT_STRIDE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const WorkItem w = item_coords<sets_qb(D)>(item_of((int64_t)blockIdx.x, nqb, xcd_groups), nqb, H);   // (never key-split)
    const int64_t b = w.b, h = w.h, q0 = w.q0 + wave * QW;
    const int64_t C = H * D;

    zero_kv_pads<T, D, NT>(sK, sV, tid);

    vec qf[DK];
    {
        const int64_t qi = q0 + l31;
        load_q_frags<T, D>(qf, q + (b * Mp + (qi < M ? qi : 0)) * ldq + h * D, qi < M, hi);
    }
    // SRC: whether set s reads the second query operand (uniform), and the fragments of a set that does / does not.  (The
    // load above stays as it is, so that the other instantiations keep their code; a first set on q_src loads again.)
    [[maybe_unused]] auto from_src = [&](int s) { return ((src_of(masks_arg...)->from_src >> s) & 1u) != 0; };
    [[maybe_unused]] auto load_q = [&](int s) {
        const int64_t qi = q0 + l31;
        const SetSrc &src = *src_of(masks_arg...);
        if (from_src(s))
            load_q_frags<T, D>(qf, static_cast<const T *>(src.q) + (b * src.Mp + (qi < M ? qi : 0)) * src.ld + h * D, qi < M,
                               hi);
        else
            load_q_frags<T, D>(qf, q + (b * Mp + (qi < M ? qi : 0)) * ldq + h * D, qi < M, hi);
    };
    if constexpr (SRC)
        if (from_src(0)) load_q(0);

    Stage stage;
    stage.init(tid, ldk, ldvt);
    const auto rsrc_k = kv_rsrc(k + b * Mkp * ldk + h * D), rsrc_v = kv_rsrc(vt + (b * C + h * D) * ldvt);
    // the tile of keys [key0, key0 + 64): rows / keys >= end (the set's end) read as zero
    auto issue = [&](int key0, int end) {
        stage.issue_masked(rsrc_k, rsrc_v, (uint32_t)key0 * (uint32_t)ldk * 2u, (uint32_t)key0 * 2u, key0, end);
    };
    auto write_lds = [&]() { stage.write(sK, sV); };

    // o: the running set's unnormalised O^T; total: the weighted sum over the finished sets.  Both in the 32-row layout:
    // [dv][r] = row 32 dv + (r & 3) + 8 (r >> 2) + 4 hi of query l31
    f32x16 o[DV], total[DV];
#pragma unroll
    for (int dv = 0; dv < DV; ++dv)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            o[dv][r] = 0.0f;
            total[dv][r] = 0.0f;
        }
    float m_run = -INFINITY;   // running max of the set, scaled (log2) units
    float l_run = 0.0f;        // this lane's share of the set's denominator

    auto tile = [&](int lim) {   // lim = keys of the tile that belong to the set (>= 64: all)
        f32x16 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kb][r] = 0.0f;
            const elem *kp = sK + (kb * 32 + l31) * K_STRIDE + hi * 8;
#pragma unroll
            for (int ks = 0; ks < DK; ++ks) s[kb] = F::mfma(*reinterpret_cast<const vec *>(kp + ks * 16), qf[ks], s[kb]);
        }
        if (lim < KV) {   // lane (l31, hi) holds keys 32 kb + (r & 3) + 8 (r >> 2) + 4 hi
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi >= lim) s[kb][r] = -INFINITY;
        }
        // online softmax, base 2, deferred rescale (scale > 0: the maximum commutes with it).  The first tile of a set
        // has at least one key and m_run = -inf, so it always installs its own maximum.
        float mt = fmaxf(s[0][0], s[1][0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) mt = fmaxf(fmaxf(mt, s[0][r]), s[1][r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64)) * scale_log2e;
        if (!__all(mt <= m_run + DEFER_THR)) {
            const float m_new = fmaxf(m_run, mt);
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // first tile: exp2(-inf) = 0
            m_run = m_new;
            l_run *= alpha;
#pragma unroll
            for (int dv = 0; dv < DV; ++dv)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[dv][r] *= alpha;
        }
        // per 16-key step: p of keys 16 st + (e & 3) + 8 (e >> 2) + 4 hi
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            float p[8];
#pragma unroll
            for (int e = 0; e < 8; ++e)
                p[e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[st >> 1][8 * (st & 1) + e], scale_log2e, -m_run));
            pv_step_split<T, D>(o, l_run, p, sV + l31 * VT_STRIDE + 8 * hi + st * 16);
        }
    };
    // MASKED: the weight of this lane's query in the set being computed (mw) and in the set whose first tile is in flight
    // (mw_next) -- one plain global load per set and lane, issued with that first tile and read when the set is finished,
    // at least a whole tile later.  A set without a row, and a query >= M (which stores nothing), weigh 1.
    float mw = 1.0f, mw_next = 1.0f;
    auto issue_weight = [&](int s) {
        if constexpr (MASKED) {
            const SetMasks &masks = *masks_of(masks_arg...);
            const int row = masks.row[s];
            mw_next = 1.0f;
            if (row >= 0 && q0 + l31 < M)
                mw_next = masks.table[b * masks.batch_stride + (int64_t)row * masks.ld + q0 + l31];
        }
    };
    auto finish_set = [&](float w) {   // total += w * o / l; the next set starts from nothing
        float f;
        if constexpr (MASKED)
            f = (w * mw) / (l_run + __shfl_xor(l_run, 32, 64));   // (this association: a weight of 1 gives the unmasked bits)
        else
            f = w / (l_run + __shfl_xor(l_run, 32, 64));
#pragma unroll
        for (int dv = 0; dv < DV; ++dv)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                total[dv][r] = __builtin_fmaf(o[dv][r], f, total[dv][r]);
                o[dv][r] = 0.0f;
            }
        m_run = -INFINITY;
        l_run = 0.0f;
    };

    // the tiles of all sets, one after the other; (cs, ct) is the tile in LDS, (ns, nt) the one in flight
    int cs = 0, ct = 0;
    issue(sets.start[0], sets.start[0] + sets.len[0]);
    if constexpr (MASKED) {
        issue_weight(0);
        mw = mw_next;
    }
    write_lds();
    __syncthreads();
    for (;;) {
        const int len = sets.len[cs];
        int ns = cs, nt = ct + 1;
        if (nt * KV >= len) {
            ns = cs + 1;
            nt = 0;
        }
        const bool more = ns < sets.n;
        if (more) issue(sets.start[ns] + nt * KV, sets.start[ns] + sets.len[ns]);
        if constexpr (MASKED)
            if (more && ns != cs) issue_weight(ns);
        tile(len - ct * KV);
        if (ns != cs) {
            finish_set(sets.w[cs]);
            if constexpr (MASKED) mw = mw_next;
            if constexpr (SRC)   // the fragments of the finished set are dead: the next set's, where its operand is another
                if (more && from_src(ns) != from_src(cs)) load_q(ns);
        }
        if (!more) break;
        __syncthreads();   // every wave has read the tile
        write_lds();
        __syncthreads();
        cs = ns;
        ct = nt;
    }

    const int64_t qi = q0 + l31;
    if (qi < M) store_rows32<T, D>(total, 1.0f, out + (b * Mp + qi) * ldo + h * D, hi);
}

template <typename T, int D>
void launch_sets(const Call &c, const Launch &g) {
    hipLaunchKernelGGL((attention_sets_kernel<T, D>), dim3((unsigned)g.wgs), dim3(sets_waves(D) * 64), 0, c.s, (const T *)c.q,
                       c.ldq, (const T *)c.k, c.ldk, (const T *)c.vt, c.ldvt, (T *)c.out, c.ldo, c.h, c.M, c.Mp, c.Mkp,
                       g.scale_log2e, g.nqb, g.xcd_groups, *c.sets);
}

template <typename T, int D>
void launch_sets_src(const Call &c, const Launch &g) {
    hipLaunchKernelGGL((attention_sets_kernel<T, D, SetSrc>), dim3((unsigned)g.wgs), dim3(sets_waves(D) * 64), 0, c.s,
                       (const T *)c.q, c.ldq, (const T *)c.k, c.ldk, (const T *)c.vt, c.ldvt, (T *)c.out, c.ldo, c.h, c.M, c.Mp,
                       c.Mkp, g.scale_log2e, g.nqb, g.xcd_groups, *c.sets, *c.set_src);
}

template <typename T, int D>
void launch_sets_masked(const Call &c, const Launch &g) {
    hipLaunchKernelGGL((attention_sets_kernel<T, D, SetMasks>), dim3((unsigned)g.wgs), dim3(sets_waves(D) * 64), 0, c.s,
                       (const T *)c.q, c.ldq, (const T *)c.k, c.ldk, (const T *)c.vt, c.ldvt, (T *)c.out, c.ldo, c.h, c.M, c.Mp,
                       c.Mkp, g.scale_log2e, g.nqb, g.xcd_groups, *c.sets, *c.set_masks);
}

// The family: one workgroup per (query block, head, sample), never key-split (no partial record, no combine kernel) -- the
// planner sizes the grid and pins the (sample, head) pairs to XCDs like every other family's.
enum SetsKind { SETS_PLAIN, SETS_MASKED, SETS_SRC };

template <typename T, int D>
Family sets_family(SetsKind kind) {
    Family f;
    f.name = kind == SETS_MASKED ? "vtm_attention_kv_sets_masked"
             : kind == SETS_SRC  ? "vtm_attention_kv_sets_src"
                                 : "vtm_attention_kv_sets";
    f.qb = sets_qb(D);
    f.wg_per_cu = kind == SETS_SRC ? sets_wg_per_cu_of<SetSrc>(D) : sets_wg_per_cu(D);
    f.rec_bytes = 0;
    f.xcd_min_nqb = 64;
    f.host_split_all = false;
    f.main = kind == SETS_MASKED ? launch_sets_masked<T, D> : kind == SETS_SRC ? launch_sets_src<T, D> : launch_sets<T, D>;
    return f;
}

// The checks and the launch of the three exports; `masks` = `src` = nullptr: vtm_attention_kv_sets (at most one is given).
int sets_launch(const char *who, const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt, int64_t ldvt, void *out,
                int64_t ldo, int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mqp, int64_t Mkp, int64_t d, float scale,
                int n_sets, const int64_t *set_start, const int64_t *set_len, const float *set_weight, const SetMasks *masks,
                vtm_stream_t stream, const SetSrc *src = nullptr) {
    VTM_REQUIRE(q && k && vt && out && set_start && set_len && set_weight, "%s: null pointer", who);
    VTM_REQUIRE(n_sets >= 1 && n_sets <= MAX_KEY_SETS, "%s: n_sets must be 1 .. %d, got %d", who, MAX_KEY_SETS, n_sets);
    VTM_REQUIRE(B > 0 && h > 0 && Mq > 0 && Mqp >= Mq && Mkp > 0 && d > 0, "%s: bad sizes", who);
    if (int rc = check_scale(who, scale)) return rc;
    if (int rc = check_half_dtype(who, dtype)) return rc;
    VTM_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldvt % 8 == 0 && ldo % 4 == 0,
                "%s: leading dimensions must keep 16-byte alignment", who);
    if (int rc = check_kv_slices(who, "sample", Mkp, ldk, d, ldvt)) return rc;
    KeySets sets;
    sets.n = n_sets;
    int64_t keys = 0;
    for (int s = 0; s < MAX_KEY_SETS; ++s) {
        sets.start[s] = sets.len[s] = 0;
        sets.w[s] = 0.0f;
        if (s >= n_sets) continue;
        // V^T is fetched in 16-byte pieces of 8 keys: a set starts on one
        VTM_REQUIRE(set_start[s] >= 0 && set_start[s] % 8 == 0, "%s: start of set %d (%lld) must be a multiple of 8", who, s,
                    (long long)set_start[s]);
        VTM_REQUIRE(set_len[s] >= 1 && set_start[s] + set_len[s] <= Mkp && set_start[s] + set_len[s] <= ldvt,
                    "%s: set %d = keys [%lld, %lld) does not lie inside Mkp = %lld, ldvt = %lld", who, s,
                    (long long)set_start[s], (long long)(set_start[s] + set_len[s]), (long long)Mkp, (long long)ldvt);
        VTM_REQUIRE(std::isfinite(set_weight[s]), "%s: weight of set %d is not finite", who, s);
        sets.start[s] = (int)set_start[s];
        sets.len[s] = (int)set_len[s];
        sets.w[s] = set_weight[s];
        keys += set_len[s];
    }
    Call c{q, ldq, k, ldk, vt, ldvt, out, ldo, dtype, B, h, Mq, Mqp, keys, Mkp, scale, 1, nullptr, 0,
           nullptr, vtm::as_stream(stream), false, nullptr, nullptr, 0};
    c.sets = &sets;
    c.set_masks = masks;
    c.set_src = src;
    const SetsKind kind = masks != nullptr ? SETS_MASKED : src != nullptr ? SETS_SRC : SETS_PLAIN;
    return with_half_head_dim(dtype, d, [&](auto t, auto dim) {
        return planned_launch(c, sets_family<decltype(t), decltype(dim)::value>(kind));
    });
}

}  // namespace

VTM_EXPORT int vtm_attention_kv_sets(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt, int64_t ldvt,
                                     void *out, int64_t ldo, int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mqp,
                                     int64_t Mkp, int64_t d, float scale, int n_sets, const int64_t *set_start,
                                     const int64_t *set_len, const float *set_weight, vtm_stream_t stream) {
    return sets_launch("vtm_attention_kv_sets", q, ldq, k, ldk, vt, ldvt, out, ldo, dtype, B, h, Mq, Mqp, Mkp, d, scale, n_sets,
                       set_start, set_len, set_weight, nullptr, stream);
}

VTM_EXPORT int vtm_attention_kv_sets_masked(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt,
                                            int64_t ldvt, void *out, int64_t ldo, int dtype, int64_t B, int64_t h, int64_t Mq,
                                            int64_t Mqp, int64_t Mkp, int64_t d, float scale, int n_sets,
                                            const int64_t *set_start, const int64_t *set_len, const float *set_weight,
                                            const int *set_mask, const float *mask, int64_t ld_mask, int64_t mask_batch_stride,
                                            vtm_stream_t stream) {
    const char *who = "vtm_attention_kv_sets_masked";
    VTM_REQUIRE(set_mask, "%s: null pointer", who);
    VTM_REQUIRE(n_sets >= 1 && n_sets <= MAX_KEY_SETS, "%s: n_sets must be 1 .. %d, got %d", who, MAX_KEY_SETS, n_sets);
    SetMasks masks{mask, ld_mask, mask_batch_stride, {}};
    int rows = 0;   // rows of the table the call names
    for (int s = 0; s < MAX_KEY_SETS; ++s) {
        masks.row[s] = -1;
        if (s >= n_sets) continue;
        // (a table has at most one row per set: that is the range of a row index)
        VTM_REQUIRE(set_mask[s] >= -1 && set_mask[s] < n_sets, "%s: mask row of set %d is %d (-1 = none, or a row 0 .. %d)", who,
                    s, set_mask[s], n_sets - 1);
        masks.row[s] = set_mask[s];
        rows = std::max(rows, set_mask[s] + 1);
    }
    if (rows == 0)   // no set is masked: the unmasked kernel, the table is not looked at
        return sets_launch(who, q, ldq, k, ldk, vt, ldvt, out, ldo, dtype, B, h, Mq, Mqp, Mkp, d, scale, n_sets, set_start,
                           set_len, set_weight, nullptr, stream);
    VTM_REQUIRE(mask, "%s: a set is masked but the table is null", who);
    VTM_REQUIRE(ld_mask >= Mq, "%s: ld_mask = %lld is shorter than a row of Mq = %lld weights", who, (long long)ld_mask,
                (long long)Mq);
    // one table for every sample (stride 0), or per-sample tables that do not overlap: that is also what bounds a row index
    VTM_REQUIRE(mask_batch_stride == 0 || mask_batch_stride >= (int64_t)rows * ld_mask,
                "%s: mask_batch_stride = %lld must be 0 or at least rows * ld_mask = %lld", who, (long long)mask_batch_stride,
                (long long)((int64_t)rows * ld_mask));
    return sets_launch(who, q, ldq, k, ldk, vt, ldvt, out, ldo, dtype, B, h, Mq, Mqp, Mkp, d, scale, n_sets, set_start, set_len,
                       set_weight, &masks, stream);
}

VTM_EXPORT int vtm_attention_kv_sets_src(const void *q, int64_t ldq, const void *q_src, int64_t ldq_src, int64_t Mqp_src,
                                         const void *k, int64_t ldk, const void *vt, int64_t ldvt, void *out, int64_t ldo,
                                         int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mqp, int64_t Mkp, int64_t d,
                                         float scale, int n_sets, const int64_t *set_start, const int64_t *set_len,
                                         const float *set_weight, const int *set_src, vtm_stream_t stream) {
    const char *who = "vtm_attention_kv_sets_src";
    VTM_REQUIRE(set_src, "%s: null pointer", who);
    VTM_REQUIRE(n_sets >= 1 && n_sets <= MAX_KEY_SETS, "%s: n_sets must be 1 .. %d, got %d", who, MAX_KEY_SETS, n_sets);
    SetSrc src{q_src, ldq_src, Mqp_src, 0u};
    for (int s = 0; s < n_sets; ++s) {
        VTM_REQUIRE(set_src[s] == 0 || set_src[s] == 1, "%s: set_src of set %d is %d (0 = q, 1 = q_src)", who, s, set_src[s]);
        src.from_src |= (unsigned)set_src[s] << s;
    }
    if (src.from_src == 0u)   // every set reads q: the plain kernel, q_src is not looked at
        return sets_launch(who, q, ldq, k, ldk, vt, ldvt, out, ldo, dtype, B, h, Mq, Mqp, Mkp, d, scale, n_sets, set_start,
                           set_len, set_weight, nullptr, stream);
    VTM_REQUIRE(q_src, "%s: a set reads q_src but it is null", who);
    VTM_REQUIRE((reinterpret_cast<uintptr_t>(q_src) & 15) == 0 && ldq_src % 8 == 0 && ldq_src >= h * d,
                "%s: q_src must be 16-byte aligned, ldq_src = %lld a multiple of 8 that holds h * d channels", who,
                (long long)ldq_src);
    VTM_REQUIRE(Mqp_src >= Mq, "%s: Mqp_src = %lld is shorter than Mq = %lld query rows", who, (long long)Mqp_src,
                (long long)Mq);
    return sets_launch(who, q, ldq, k, ldk, vt, ldvt, out, ldo, dtype, B, h, Mq, Mqp, Mkp, d, scale, n_sets, set_start, set_len,
                       set_weight, nullptr, stream, &src);
}
