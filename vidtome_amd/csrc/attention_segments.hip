// vtm_attention_kv_segments: the cross-attention core over QUERY SEGMENTS of one row range,
//     out[i, head] = softmax_j(q[i, head] . k[s, j, head] * scale) v[s, j, head],   j < Mk,   seg_off[s] <= i < seg_off[s + 1]
// This is the `self.attn2(...)` call of vidtome/patch.py:171-185 on MERGED tokens (patch.py's `merge_crossattn`): the kept
// rows of a chunk, in frame order (vtm_frame_order), are one (B M_l)-row sequence whose segment s = b F + f holds the rows of
// frame f of sample b, and every row attends to its own frame's conditioning -- key sample s.  How many rows a frame keeps
// depends on the matching, so the segment bounds are DEVICE values; the host knows only an upper bound on a segment's length.
//
// Structure: attention_bias_kernel (attention_bias.hip) with the per-key bias reduced to the key bound and the sample's query
// rows replaced by a segment's:
//   * workgroup = waves of 32 query rows of ONE segment; the K / V^T tiles of 64 keys of the segment's key sample are staged
//     through one LDS buffer and shared by the waves, the next tile's global loads in flight in registers while the current
//     one is computed;
//   * the grid is (query block < ceil(max_seg_rows / rows per workgroup), head, segment), sized on the host through the launch
//     planner; a workgroup reads its segment's two offsets and leaves at once when its block starts behind the segment's
//     length -- with segments of about half the bound, about half of the workgroups;
//   * beside the K tile lives one 4-byte slot per key: 0, or -inf for a key >= Mk -- all the bounds logic the scores need;
//   * S^T = K Q^T on v_mfma_f32_32x32x16 (one query per lane); score = S^T * scale * log2(e) + slot; online softmax in
//     registers, base 2, deferred rescale.  P is rounded ONCE to the operand type for the PV contraction (bf16: as a hi + lo
//     pair, two MFMAs) and the denominator is summed from the same rounded P;
//   * no key split, no workspace, no combine kernel: the key axis is a few hundred keys, the launch streams q and out.
// A segment's rows are clamped to [0, rows_total) before anything is addressed: offsets that break the contract (decreasing,
// negative, beyond rows_total) give rows nobody computes, never an access outside q / out.
#include "attention_checks.h"
#include "attention_stage.h"

namespace vtm_att {
// the segments of one vtm_attention_kv_segments call (Call::B = their number, Call::M = the bound on their length)
struct QuerySegments {
    const int32_t *off;   // DEVICE: n_seg + 1 absolute row offsets
    int64_t rows_total;   // rows of q / out
};
}  // namespace vtm_att

namespace {

// the geometry of attention_bias_kernel: 8 waves up to d = 96, 4 above; one resident workgroup per CU from d = 32 on, two
// below (profiles/attention_segments_resources.txt)
constexpr int seg_waves(int D) { return D <= 96 ? 8 : 4; }
constexpr int seg_wg_per_cu(int D) { return D <= 16 ? 2 : 1; }
constexpr int seg_qb(int D) { return seg_waves(D) * QW; }   // query rows per workgroup

template <typename T, int D>
__global__ __launch_bounds__(seg_waves(D) * 64, seg_wg_per_cu(D) * seg_waves(D) / 4) void attention_segments_kernel(
    const T *__restrict__ q, int64_t ldq, const T *__restrict__ k, int64_t ldk, const T *__restrict__ vt, int64_t ldvt,
    T *__restrict__ out, int64_t ldo, int64_t H, int64_t max_seg_rows, int Mk, int64_t Mkp, float scale_log2e, int64_t nqb,
    int xcd_groups, const int32_t *__restrict__ seg_off, int64_t rows_total) {
    using F = Frag<T>;
    using vec = typename F::vec;
    using elem = typename F::elem;
    constexpr int WAVES = seg_waves(D), NT = WAVES * 64;
    using Stage = KvStage<T, D, NT>;
    constexpr int DK = Stage::DK;          // k-steps of the QK^T contraction
    constexpr int DV = (D + 31) / 32;      // 32-row blocks of O^T
    constexpr int VROWS = DV * 32;
    constexpr int K_STRIDE = Stage::K_STRIDE;

    __shared__ __attribute__((aligned(16))) elem sK[KV * K_STRIDE];
    __shared__ __attribute__((aligned(16))) elem sV[VROWS * VT_STRIDE];
    __shared__ __attribute__((aligned(16))) float sB[KV];   // 0 per key of the tile; -inf behind the last key

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const WorkItem w = item_coords<seg_qb(D)>(item_of((int64_t)blockIdx.x, nqb, xcd_groups), nqb, H);   // (never key-split)
    const int64_t seg = w.b, h = w.h;
    // the segment's rows [row0, row0 + len): inside [0, rows_total), at most max_seg_rows of them (all wave-uniform)
    int64_t row0 = seg_off[seg], row1 = seg_off[seg + 1];
    row0 = row0 < 0 ? 0 : row0;
    row1 = row1 > rows_total ? rows_total : row1;
    int64_t len = row1 - row0;
    len = len > max_seg_rows ? max_seg_rows : len;
    if (w.q0 >= len) return;   // an empty segment, or a block behind its last row (before any barrier: the whole workgroup)
    const int64_t q0 = w.q0 + wave * QW;
    const int64_t C = H * D;

    zero_kv_pads<T, D, NT>(sK, sV, tid);

    vec qf[DK];
    {
        const int64_t qi = q0 + l31;
        load_q_frags<T, D>(qf, q + (row0 + (qi < len ? qi : 0)) * ldq + h * D, qi < len, hi);
    }

    Stage stage;
    stage.init(tid, ldk, ldvt);
    const auto rsrc_k = kv_rsrc(k + seg * Mkp * ldk + h * D), rsrc_v = kv_rsrc(vt + (seg * C + h * D) * ldvt);

    int key_in_flight = 0;
    auto issue = [&](int key0) {   // the tile of keys [key0, key0 + 64): rows / keys >= Mk read as zero
        stage.issue_masked(rsrc_k, rsrc_v, (uint32_t)key0 * (uint32_t)ldk * 2u, (uint32_t)key0 * 2u, key0, Mk);
        key_in_flight = key0;
    };
    auto write_lds = [&]() {
        stage.write(sK, sV);
        if (tid < KV) sB[tid] = key_in_flight + tid < Mk ? 0.0f : -INFINITY;
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
        // online softmax, base 2, deferred rescale (every tile holds at least one key < Mk: the maximum is finite)
        float mt = fmaxf(s[0][0], s[1][0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) mt = fmaxf(fmaxf(mt, s[0][r]), s[1][r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        if (!__all(mt <= m_run + DEFER_THR)) {
            const float m_new = fmaxf(m_run, mt);
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // the first tile: exp2(-inf) = 0
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
            for (int e = 0; e < 8; ++e) p[e] = __builtin_amdgcn_exp2f(s[st >> 1][8 * (st & 1) + e] - m_run);
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
    if (qi < len) store_rows32<T, D>(o, inv_l, out + (row0 + qi) * ldo + h * D, hi);
}

template <typename T, int D>
void launch_segments(const Call &c, const Launch &g) {
    hipLaunchKernelGGL((attention_segments_kernel<T, D>), dim3((unsigned)g.wgs), dim3(seg_waves(D) * 64), 0, c.s,
                       (const T *)c.q, c.ldq, (const T *)c.k, c.ldk, (const T *)c.vt, c.ldvt, (T *)c.out, c.ldo, c.h, c.M,
                       (int)c.Mk, c.Mkp, g.scale_log2e, g.nqb, g.xcd_groups, c.segments->off, c.segments->rows_total);
}

// The family: one workgroup per (query block of the bound, head, segment), never key-split (no partial record, no combine
// kernel) -- the planner sizes the grid and pins the (segment, head) pairs to XCDs like every other family's.
template <typename T, int D>
Family segments_family() {
    Family f;
    f.name = "vtm_attention_kv_segments";
    f.qb = seg_qb(D);
    f.wg_per_cu = seg_wg_per_cu(D);
    f.rec_bytes = 0;
    f.xcd_min_nqb = 64;
    f.host_split_all = false;
    f.main = launch_segments<T, D>;
    return f;
}

}  // namespace

VTM_EXPORT int vtm_attention_kv_segments(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt, int64_t ldvt,
                                         void *out, int64_t ldo, int dtype, int64_t rows_total, const int32_t *seg_off,
                                         int64_t n_seg, int64_t max_seg_rows, int64_t h, int64_t Mk, int64_t Mkp, int64_t d,
                                         float scale, vtm_stream_t stream) {
    const char *who = "vtm_attention_kv_segments";
    VTM_REQUIRE(q && k && vt && out, "%s: null pointer", who);
    VTM_REQUIRE(seg_off, "%s: null seg_off", who);
    VTM_REQUIRE(rows_total > 0 && n_seg > 0 && max_seg_rows > 0 && h > 0 && Mk > 0 && Mkp >= Mk && Mkp % 8 == 0 && d > 0,
                "%s: bad sizes", who);
    VTM_REQUIRE(rows_total < (1ll << 31), "%s: rows_total = %lld does not fit the int32 offsets", who, (long long)rows_total);
    if (int rc = check_scale(who, scale)) return rc;
    if (int rc = check_half_dtype(who, dtype)) return rc;
    VTM_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldvt % 8 == 0 && ldo % 4 == 0 && ldvt >= Mk && ldq >= h * d && ldo >= h * d &&
                    ldk >= h * d,
                "%s: leading dimensions must hold a row and keep 16-byte alignment (ldvt >= Mk, %% 8)", who);
    if (int rc = check_kv_slices(who, "segment", Mkp, ldk, d, ldvt)) return rc;
    const QuerySegments segs{seg_off, rows_total};
    // the planner's "samples" are the segments, its query rows the bound on a segment's length
    Call c{q, ldq, k, ldk, vt, ldvt, out, ldo, dtype, n_seg, h, max_seg_rows, max_seg_rows, Mk, Mkp, scale, 1, nullptr, 0,
           nullptr, vtm::as_stream(stream), false, nullptr, nullptr, 0};
    c.segments = &segs;
    return with_half_head_dim(dtype, d, [&](auto t, auto dim) {
        return planned_launch(c, segments_family<decltype(t), decltype(dim)::value>());
    });
}
