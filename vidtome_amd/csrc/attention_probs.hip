// vtm_attention_probs: the head-averaged probabilities of the cross-attention core, in fp32,
//     out[b, i, j] = (1 / h) * sum_head softmax_j(q[b, i, head] . k[b, j, head] * scale + bias[b, j]),   i < Mq, j < Mk
// -- the "cross-attention map" of the `self.attn2(...)` call of vidtome/patch.py:178-183 that zero-shot video editing reads
// (LocalBlend-style masks, per-word maps), from the q / k rows the fused attn2 segment already holds.  There is no V operand
// and no (B, h, Mq, Mk) intermediate: a storing attention processor writes that tensor in the model's dtype and averages it
// afterwards.
//
// Structure: the QK^T half of attention_bias_kernel, run twice.
//   * workgroup = 4 waves x 32 query rows of ONE sample, looping over the heads; K tiles of 64 keys of one head come through
//     KvStage's K half into one LDS buffer shared by the waves, the next tile's global loads in flight in registers while
//     the current one is computed.  The sample's bias row (<= 256 keys) sits in LDS for the whole launch, pre-multiplied by
//     log2(e); slots >= Mk hold -inf, which is all the bounds logic the scores need;
//   * S^T = K Q^T on v_mfma_f32_32x32x16 (one query per lane); score = fma(S^T, scale * log2(e), slot), base-2 softmax;
//   * sweep 1 (heads outer, tiles inner): the online row maximum and denominator of every head (online_sum,
//     attention_stage.h); at a head's last tile the maximum and 1 / denominator go to LDS, one slot per (head, query row)
//     -- the stats of h heads live there, not in a dynamically indexed register array;
//   * sweep 2 (tiles outer, heads inner): the tile's scores again, exp2(s - m_head) * (1 / l_head) added into the tile's 32
//     fp32 mean accumulators head after head in ascending order, one multiplication by 1 / h, and the tile is written once,
//     turned round through LDS (the K tile's bytes, free between two tiles) so that a half-wave stores 32 consecutive keys
//     of one query row;
//   * as in attention_bias_kernel the exponent is taken against 0 while no finite score has been seen: leading masked tiles
//     give 0, a key with bias -inf gives exactly 0, a sample whose keys are ALL -inf gives 0 * (1 / 0) = NaN for that sample;
//   * one launch, no atomics, no workspace: the same operands give the same bits.
// Cost: K is re-staged from L2 twice per head and q is read once per step of its head (2 ntiles times, from L2 after the
// first).
#include "attention_checks.h"
#include "attention_stage.h"

namespace {

constexpr int PROBS_WAVES = 4, PROBS_NT = PROBS_WAVES * 64;
constexpr int PROBS_QB = PROBS_WAVES * QW;      // query rows per workgroup
constexpr int PROBS_MAX_KEYS = 256;             // the bias row of a sample in LDS; 4 tiles
constexpr int PROBS_MAX_HEADS = 40;             // 2 stats x 4 bytes x PROBS_QB rows = 1 KB of LDS per head

template <typename T, int D>
__global__ __launch_bounds__(PROBS_NT, 2) void attention_probs_kernel(
    const T *__restrict__ q, int64_t ldq, const T *__restrict__ k, int64_t ldk, float *__restrict__ out, int64_t ldo, int H,
    int64_t M, int64_t Mp, int Mk, int64_t Mkp, float scale_log2e, int64_t nqb, const float *__restrict__ bias,
    int64_t bias_batch_stride) {
    using F = Frag<T>;
    using vec = typename F::vec;
    using elem = typename F::elem;
    constexpr int NT = PROBS_NT, QB = PROBS_QB;
    using Stage = KvStage<T, D, NT>;
    constexpr int DK = Stage::DK;
    constexpr int K_STRIDE = Stage::K_STRIDE;
    constexpr float LOG2E = 1.4426950408889634f;

    // The K tile; between two tiles of sweep 2 the same bytes serve the output transposition (sT below), which needs
    // PROBS_WAVES blocks of 32 queries x 32 keys of fp32 in rows of 33
    constexpr int T_STRIDE = 33, T_FLOATS = PROBS_WAVES * QW * T_STRIDE;
    constexpr int K_ELEMS = KV * K_STRIDE > 2 * T_FLOATS ? KV * K_STRIDE : 2 * T_FLOATS;
    __shared__ __attribute__((aligned(16))) elem sK[K_ELEMS];
    __shared__ __attribute__((aligned(16))) float sB[PROBS_MAX_KEYS];   // bias * log2(e); -inf behind the last key
    extern __shared__ float sStat[];   // [head][row]: the row maximum (0 for none), then [H + head][row]: 1 / denominator

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int64_t b = (int64_t)blockIdx.x / nqb;
    const int64_t qi = ((int64_t)blockIdx.x % nqb) * QB + wave * QW + l31;
    const bool q_ok = qi < M;
    const T *qrow = q + (b * Mp + (q_ok ? qi : 0)) * ldq;
    const T *kb0 = k + b * Mkp * ldk;
    const int row = wave * QW + l31;

    auto zero_pads = [&]() { zero_k_pads<T, D, NT>(sK, tid); };   // (again after every flush, which writes over them)
    zero_pads();
    {
        float v = -INFINITY;
        if (tid < Mk) v = bias != nullptr ? bias[b * bias_batch_stride + tid] * LOG2E : 0.0f;   // (-inf stays -inf)
        sB[tid] = v;                                                                             // NT == PROBS_MAX_KEYS
    }
    static_assert(PROBS_NT == PROBS_MAX_KEYS, "one thread per bias slot");

    Stage stage;
    stage.init(tid, ldk, 0);   // (the V^T half is never used)

    // The steps: sweep 1 is step i < n = H * ntiles, (head, tile) = (i / ntiles, i % ntiles); sweep 2 is step n + j,
    // (tile, head) = (j / H, j % H).  One sequence, so that the prefetch runs across the boundary.
    const int ntiles = (Mk + KV - 1) / KV;
    const int n = H * ntiles;
    auto head_of = [&](int i) { return i < n ? i / ntiles : (i - n) % H; };
    auto tile_of = [&](int i) { return i < n ? i % ntiles : (i - n) / H; };
    // the step's Q fragments travel with its K tile (qn: in flight while the step before computes)
    vec qf[DK], qn[DK];
    auto issue = [&](int i) {   // rows >= Mk of a ragged tile read as zero without being fetched
        load_q_frags<T, D>(qn, qrow + head_of(i) * D, q_ok, hi);
        const int key0 = tile_of(i) * KV;
        const auto rsrc = kv_rsrc(kb0 + head_of(i) * D);
        const uint32_t so = (uint32_t)key0 * (uint32_t)ldk * 2u;
        if (key0 + KV <= Mk)
            stage.issue_k(std::true_type{}, rsrc, so);
        else
            stage.issue_k(std::false_type{}, rsrc, so, key0, Mk);
    };

    // scores of tile ct in log2 units: lane (l31, hi) holds keys 64 ct + 32 kb + (r & 3) + 8 (r >> 2) + 4 hi of query l31
    auto scores = [&](int ct, f32x16 (&s)[2]) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kb][r] = 0.0f;
            const elem *kp = sK + (kb * 32 + l31) * K_STRIDE + hi * 8;
#pragma unroll
            for (int ks = 0; ks < DK; ++ks) s[kb] = F::mfma(*reinterpret_cast<const vec *>(kp + ks * 16), qf[ks], s[kb]);
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 bv = *reinterpret_cast<const f32x4 *>(sB + ct * KV + kb * 32 + 8 * g + 4 * hi);
#pragma unroll
                for (int e = 0; e < 4; ++e) s[kb][4 * g + e] = __builtin_fmaf(s[kb][4 * g + e], scale_log2e, bv[e]);
            }
    };

    float m_run = -INFINITY, l_run = 0.0f;   // sweep 1: the head's running max (log2 units) and this lane's share of the sum
    f32x16 acc[2];                           // sweep 2: the tile's mean accumulators, in the layout of the scores
    const float inv_h = 1.0f / (float)H;

    auto step1 = [&](int i) {
        const int head = head_of(i), ct = tile_of(i);
        f32x16 s[2];
        {
            if (ct == 0) {
                m_run = -INFINITY;
                l_run = 0.0f;
            }
            scores(ct, s);
            const float m_use = online_sum(s, m_run, l_run);
            if (ct == ntiles - 1) {
                const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
                if (hi == 0) {
                    sStat[head * QB + row] = m_use;
                    sStat[(H + head) * QB + row] = 1.0f / l_tot;   // every key masked: 1 / 0, and 0 * inf = NaN below
                }
            }
        }
    };
    auto step2 = [&](int i) {
        const int head = head_of(i), ct = tile_of(i);
        f32x16 s[2];
        {
            if (head == 0) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[kb][r] = 0.0f;
            }
            scores(ct, s);
            const float m = sStat[head * QB + row], il = sStat[(H + head) * QB + row];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[kb][r] += __builtin_amdgcn_exp2f(s[kb][r] - m) * il;
            if (head == H - 1) {   // the tile is complete: flush() writes it
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[kb][r] *= inv_h;
            }
        }
    };

    // The finished tile to `out`, once every wave is done with the K tile: a lane holds 32 keys of ONE query row, so a
    // store straight from the accumulators would hit 32 rows per instruction.  Each wave turns its 32 x 32 blocks round
    // through LDS (rows of 33 floats: conflict-free both ways) and stores 32 consecutive keys of a row per half-wave.
    float *sT = reinterpret_cast<float *>(sK) + wave * QW * T_STRIDE;
    const int64_t qw0 = ((int64_t)blockIdx.x % nqb) * QB + wave * QW;   // the wave's first query row
    auto flush = [&](int ct) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sT[l31 * T_STRIDE + (r & 3) + 8 * (r >> 2) + 4 * hi] = acc[kb][r];
            __syncthreads();
            const int key = ct * KV + kb * 32 + l31;
            float *op = out + (b * M + qw0 + hi) * ldo + key;
#pragma unroll 4
            for (int j = 0; j < 16; ++j, op += 2 * ldo) {
                const int rr = 2 * j + hi;
                if (qw0 + rr < M && key < Mk) *op = sT[rr * T_STRIDE + l31];
            }
            __syncthreads();
        }
    };

    // step i is in LDS, step i + 1 in flight.  The barriers between the steps also order sweep 1's stats before sweep 2.
    issue(0);
    stage.write_k(sK);
    __syncthreads();
    for (int i = 0; i < n; ++i) {   // sweep 1 (its last step has the first tile of sweep 2 in flight)
#pragma unroll
        for (int ks = 0; ks < DK; ++ks) qf[ks] = qn[ks];
        issue(i + 1);
        step1(i);
        __syncthreads();   // every wave has read the tile
        stage.write_k(sK);
        __syncthreads();
    }
    for (int i = n;; ++i) {         // sweep 2
        const bool more = i + 1 < 2 * n;
#pragma unroll
        for (int ks = 0; ks < DK; ++ks) qf[ks] = qn[ks];
        if (more) issue(i + 1);
        step2(i);
        const bool tile_done = head_of(i) == H - 1;   // (the last step is one)
        __syncthreads();   // every wave has read the tile
        if (tile_done) {   // (uniform)
            flush(tile_of(i));
            if (!more) break;
            zero_pads();
        }
        stage.write_k(sK);
        __syncthreads();
    }
}

template <typename T, int D>
void launch_probs(const void *q, int64_t ldq, const void *k, int64_t ldk, float *out, int64_t ldo, int64_t B, int64_t h,
                  int64_t Mq, int64_t Mqp, int64_t Mk, int64_t Mkp, float scale, const float *bias, int64_t bias_batch_stride,
                  hipStream_t s) {
    const int64_t nqb = vtm::cdiv(Mq, PROBS_QB);
    hipLaunchKernelGGL((attention_probs_kernel<T, D>), dim3((unsigned)(B * nqb)), dim3(PROBS_NT),
                       (size_t)(2 * h * PROBS_QB) * sizeof(float), s, (const T *)q, ldq, (const T *)k, ldk, out, ldo, (int)h, Mq,
                       Mqp, (int)Mk, Mkp, scale * 1.4426950408889634f, nqb, bias, bias_batch_stride);
}

}  // namespace

VTM_EXPORT int vtm_attention_probs(const void *q, int64_t ldq, const void *k, int64_t ldk, float *out, int64_t ldo, int dtype,
                                   int64_t B, int64_t h, int64_t Mq, int64_t Mqp, int64_t Mk, int64_t Mkp, int64_t d,
                                   float scale, const float *bias, int64_t ld_bias, int64_t bias_batch_stride,
                                   vtm_stream_t stream) {
    const char *who = "vtm_attention_probs";
    VTM_REQUIRE(q && k && out, "%s: null pointer", who);
    if (int rc = check_qk_aligned(who, q, k, (reinterpret_cast<uintptr_t>(out) & 3) == 0)) return rc;
    if (int rc = check_map_sizes(who, B, h, Mq, Mqp, Mk, Mkp, d)) return rc;
    VTM_REQUIRE(Mk <= PROBS_MAX_KEYS, "%s: Mk = %lld, at most %d keys are taken", who, (long long)Mk, PROBS_MAX_KEYS);
    VTM_REQUIRE(h <= PROBS_MAX_HEADS, "%s: h = %lld, at most %d heads are taken", who, (long long)h, PROBS_MAX_HEADS);
    if (int rc = check_scale(who, scale)) return rc;
    if (int rc = check_half_dtype(who, dtype)) return rc;
    if (int rc = check_qk_rows(who, ldq, ldk, h, d, Mk, ldo, Mk, "ldo >= Mk")) return rc;
    VTM_REQUIRE(B * vtm::cdiv(Mq, PROBS_QB) < (1ll << 31), "%s: grid too large", who);
    if (bias != nullptr)
        if (int rc = check_key_rows(who, "bias", "values", ld_bias, bias_batch_stride, Mk)) return rc;
    hipStream_t s = vtm::as_stream(stream);
    return with_half_head_dim(dtype, d, [&](auto t, auto dim) {
        launch_probs<decltype(t), decltype(dim)::value>(q, ldq, k, ldk, out, ldo, B, h, Mq, Mqp, Mk, Mkp, scale, bias,
                                                        bias_batch_stride, s);
        return vtm::launch_status(who);
    });
}
