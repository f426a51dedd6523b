// vtm_attention_word_map: ONE column combination of the head-averaged cross-attention map, added in place,
//     value[b, i] = (1 / h) * sum_head [ sum_j w[b, j] p_head[i, j] ] / [ sum_j p_head[i, j] ]
//     out[r(b) * ldo + i] = (accumulate ? out[...] : 0) + value[b, i],   r(b) = out_rows ? out_rows[b] : b
// -- the `self.attn2(...)` call of vidtome/patch.py:178-183 as a Prompt-to-Prompt LocalBlend reads it: the map of a few
// chosen words, summed over blocks and steps.  It is the attention core with a scalar "value" per key, so nothing of
// attention_probs_kernel's second sweep is needed: no per-head statistics in LDS (and no head limit), no transposition of
// an output tile, half the MFMA work and one float per query row instead of Mk.
//
// Structure: the QK^T half of attention_bias_kernel, run once.
//   * workgroup = 4 waves x 32 query rows of ONE sample, looping over the heads (outer) and the 64-key tiles of a head
//     (inner); K tiles come through KvStage's K half into one LDS buffer shared by the waves, the next tile's global loads
//     in flight in registers while the current one is computed.  The sample's bias row (times log2(e), -inf behind the last
//     key) and its weights row (0 behind the last key) sit in LDS for the whole launch;
//   * no load of a step stands inside a branch (see `issue` below): what a ragged tile, a dead query or a padded
//     contraction must not see is fetched from a place that exists and replaced by zeros when it is used;
//   * scores as in attention_probs_kernel (qk_scores_biased, attention_stage.h), base-2 online softmax whose running
//     maximum (online_max, there too) carries TWO sums, the weighted numerator and the denominator, rescaled together;
//   * at a head's last tile numerator * (1 / denominator) is added to a per-lane fp32 accumulator, heads in ascending
//     order; the accumulator is multiplied by 1 / h once and each query row is stored once (lanes 0-31 of a wave: 32
//     consecutive floats);
//   * as in attention_bias_kernel the exponent is taken against 0 while no finite score has been seen: a key with bias -inf
//     contributes exactly 0 (weights are finite), a sample whose keys are ALL -inf gives 0 * (1 / 0) = NaN for that sample;
//   * one launch, no atomics, no workspace; every output element has one writer: the same operands and the same prior
//     `out` give the same bits.
#include "attention_checks.h"
#include "attention_stage.h"

namespace {

constexpr int WORDS_WAVES = 4, WORDS_NT = WORDS_WAVES * 64;
constexpr int WORDS_QB = WORDS_WAVES * QW;      // query rows per workgroup
constexpr int WORDS_MAX_KEYS = 256;             // the bias and weights rows of a sample in LDS; 4 tiles

template <typename T, int D>
__global__ __launch_bounds__(WORDS_NT, 2) void attention_words_kernel(
    const T *__restrict__ q, int64_t ldq, const T *__restrict__ k, int64_t ldk, float *__restrict__ out, int64_t ldo, int H,
    int64_t M, int64_t Mp, int Mk, int64_t Mkp, float scale_log2e, int64_t nqb, const float *__restrict__ bias,
    int64_t bias_batch_stride, const float *__restrict__ weights, int64_t w_batch_stride,
    const int64_t *__restrict__ out_rows, int accumulate) {
    using F = Frag<T>;
    using vec = typename F::vec;
    using elem = typename F::elem;
    constexpr int NT = WORDS_NT, QB = WORDS_QB;
    using Stage = KvStage<T, D, NT>;
    constexpr int DK = Stage::DK;
    constexpr int K_STRIDE = Stage::K_STRIDE;
    constexpr float LOG2E = 1.4426950408889634f;

    __shared__ __attribute__((aligned(16))) elem sK[KV * K_STRIDE];
    __shared__ __attribute__((aligned(16))) float sB[WORDS_MAX_KEYS];   // bias * log2(e); -inf behind the last key
    __shared__ __attribute__((aligned(16))) float sW[WORDS_MAX_KEYS];   // the weights; 0 behind the last key

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int64_t b = (int64_t)blockIdx.x / nqb;
    const int64_t qi = ((int64_t)blockIdx.x % nqb) * QB + wave * QW + l31;
    const bool q_ok = qi < M;
    const T *qrow = q + (b * Mp + (q_ok ? qi : 0)) * ldq;
    const T *kb0 = k + b * Mkp * ldk;

    zero_k_pads<T, D, NT>(sK, tid);
    {
        float v = -INFINITY, w = 0.0f;
        if (tid < Mk) {
            v = bias != nullptr ? bias[b * bias_batch_stride + tid] * LOG2E : 0.0f;   // (-inf stays -inf)
            w = weights[b * w_batch_stride + tid];
        }
        sB[tid] = v;   // NT == WORDS_MAX_KEYS
        sW[tid] = w;
    }
    static_assert(WORDS_NT == WORDS_MAX_KEYS, "one thread per bias / weights slot");

    Stage stage;
    stage.init(tid, ldk, 0);   // (the V^T half is never used)

    // step i < n = H * ntiles: (head, tile) = (i / ntiles, i % ntiles)
    const int ntiles = (Mk + KV - 1) / KV;
    const int n = H * ntiles;
    // The step's Q fragments travel with its K tile (qn: in flight while the step before computes).  No load of a step
    // stands inside a branch -- the compiler waits for every outstanding load behind one, which puts a memory latency
    // into each of the H * ntiles steps (measured: 1.4 - 2 us a step) -- so what load_q_frags and issue_k guard is selected
    // when the data is used instead: a dead query reads row 0 of its sample, a fragment beyond D its channels 0-7, a key
    // row beyond Mk chunk 0 of its tile (KvStage::issue_k_select), all of which exist, and take_q / write_k_select put
    // zeros in their place.
    vec qf[DK], qn[DK];
    auto issue = [&](int i) {
        const int head = i / ntiles, key0 = (i % ntiles) * KV;
#pragma unroll
        for (int ks = 0; ks < DK; ++ks) {
            const int d0 = ks * 16 + hi * 8;
            qn[ks] = __builtin_bit_cast(vec, *reinterpret_cast<const uint4 *>(qrow + head * D + (d0 < D ? d0 : 0)));
        }
        stage.issue_k_select(kv_rsrc(kb0 + head * D), (uint32_t)key0 * (uint32_t)ldk * 2u, key0, Mk);
    };
    auto take_q = [&]() {
#pragma unroll
        for (int ks = 0; ks < DK; ++ks)
            qf[ks] = q_ok && ks * 16 + hi * 8 < D ? qn[ks] : __builtin_bit_cast(vec, make_uint4(0, 0, 0, 0));
    };

    // the head's running maximum (log2 units) and this lane's share of the two sums; the mean over the heads
    float m_run = -INFINITY, l_run = 0.0f, n_run = 0.0f, acc = 0.0f;

    auto step = [&](int i) {
        const int ct = i % ntiles;
        f32x16 s[2];
        if (ct == 0) {
            m_run = -INFINITY;
            l_run = 0.0f;
            n_run = 0.0f;
        }
        qk_scores_biased<T, D, NT>(s, sK, sB, qf, ct, scale_log2e, l31, hi);
        float m_new;
        const float m_use = online_max(s, m_run, m_new);
        float sum = 0.0f, num = 0.0f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 wv = *reinterpret_cast<const f32x4 *>(sW + ct * KV + kb * 32 + 8 * g + 4 * hi);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float p = __builtin_amdgcn_exp2f(s[kb][4 * g + e] - m_use);
                    sum += p;
                    num = __builtin_fmaf(p, wv[e], num);
                }
            }
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);   // nothing finite seen before: both sums are 0
        l_run = l_run * alpha + sum;
        n_run = n_run * alpha + num;
        m_run = m_new;
        if (ct == ntiles - 1) {
            const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
            const float n_tot = n_run + __shfl_xor(n_run, 32, 64);
            acc += n_tot * (1.0f / l_tot);   // every key masked: 0 * (1 / 0) = NaN
        }
    };

    // step i is in LDS, step i + 1 in flight
    issue(0);
    stage.write_k_select(sK, 0, Mk);
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        take_q();
        const bool more = i + 1 < n;   // (uniform)
        if (more) issue(i + 1);
        step(i);
        if (!more) break;
        __syncthreads();   // every wave has read the tile
        stage.write_k_select(sK, ((i + 1) % ntiles) * KV, Mk);
        __syncthreads();
    }

    if (q_ok && hi == 0) {
        const int64_t r = out_rows != nullptr ? out_rows[b] : b;
        float *op = out + r * ldo + qi;
        const float v = acc * (1.0f / (float)H);
        *op = accumulate ? *op + v : v;
    }
}

template <typename T, int D>
void launch_words(const void *q, int64_t ldq, const void *k, int64_t ldk, float *out, int64_t ldo, int64_t B, int64_t h,
                  int64_t Mq, int64_t Mqp, int64_t Mk, int64_t Mkp, float scale, const float *bias, int64_t bias_batch_stride,
                  const float *weights, int64_t w_batch_stride, const int64_t *out_rows, int accumulate, hipStream_t s) {
    const int64_t nqb = vtm::cdiv(Mq, WORDS_QB);
    hipLaunchKernelGGL((attention_words_kernel<T, D>), dim3((unsigned)(B * nqb)), dim3(WORDS_NT), 0, s, (const T *)q, ldq,
                       (const T *)k, ldk, out, ldo, (int)h, Mq, Mqp, (int)Mk, Mkp, scale * 1.4426950408889634f, nqb, bias,
                       bias_batch_stride, weights, w_batch_stride, out_rows, accumulate);
}

}  // namespace

VTM_EXPORT int vtm_attention_word_map(const void *q, int64_t ldq, const void *k, int64_t ldk, int dtype, int64_t B, int64_t h,
                                      int64_t Mq, int64_t Mqp, int64_t Mk, int64_t Mkp, int64_t d, float scale,
                                      const float *bias, int64_t ld_bias, int64_t bias_batch_stride, const float *weights,
                                      int64_t ld_w, int64_t w_batch_stride, float *out, int64_t ldo, const int64_t *out_rows,
                                      int accumulate, vtm_stream_t stream) {
    const char *who = "vtm_attention_word_map";
    VTM_REQUIRE(q && k && weights && out, "%s: null pointer", who);
    const bool rest_aligned = ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(weights)) & 3) == 0 &&
                              (reinterpret_cast<uintptr_t>(out_rows) & 7) == 0;
    if (int rc = check_qk_aligned(who, q, k, rest_aligned)) return rc;
    if (int rc = check_map_sizes(who, B, h, Mq, Mqp, Mk, Mkp, d)) return rc;
    VTM_REQUIRE(h < (1ll << 20), "%s: h = %lld heads", who, (long long)h);
    VTM_REQUIRE(Mk <= WORDS_MAX_KEYS, "%s: Mk = %lld, at most %d keys are taken", who, (long long)Mk, WORDS_MAX_KEYS);
    if (int rc = check_scale(who, scale)) return rc;
    if (int rc = check_half_dtype(who, dtype)) return rc;
    if (int rc = check_qk_rows(who, ldq, ldk, h, d, Mk, ldo, Mq, "ldo >= Mq")) return rc;
    VTM_REQUIRE(B * vtm::cdiv(Mq, WORDS_QB) < (1ll << 31), "%s: grid too large", who);
    if (bias != nullptr)
        if (int rc = check_key_rows(who, "bias", "values", ld_bias, bias_batch_stride, Mk)) return rc;
    if (int rc = check_key_rows(who, "w", "weights", ld_w, w_batch_stride, Mk)) return rc;
    hipStream_t s = vtm::as_stream(stream);
    return with_half_head_dim(dtype, d, [&](auto t, auto dim) {
        launch_words<decltype(t), decltype(dim)::value>(q, ldq, k, ldk, out, ldo, B, h, Mq, Mqp, Mk, Mkp, scale, bias,
                                                        bias_batch_stride, weights, w_batch_stride, out_rows, accumulate != 0, s);
        return vtm::launch_status(who);
    });
}
