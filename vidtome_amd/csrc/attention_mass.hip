// vtm_attention_key_mass: the per-key attention mass of the self-attention core, in fp32,
//     mass[b, j] = sum_{i < Mq} (1 / h) * sum_head softmax_j(q[b, i, head] . k[b, j, head] * scale)[j],   j < Mk
// -- the column sums of the head-averaged attn1 map that self-attention guidance thresholds (its mean over j is Mq / Mk:
// exactly 1 for self-attention), from the q | k row ranges of the qkv buffer the un-merged attn1 body already holds.  There
// is no V operand, no bias and no (B, h, Mq, Mk) intermediate -- not even a (B, Mq, Mk) one.
//
// Structure: the QK^T half of attention_probs_kernel, run twice PER HEAD.
//   * workgroup = 4 waves x 32 query rows of ONE sample (a query tile of 128 rows), looping over the heads; K tiles of 64
//     keys of one head come through KvStage's K half into one LDS buffer shared by the waves, the next tile's global loads
//     in flight in registers while the current one is computed;
//   * S^T = K Q^T on v_mfma_f32_32x32x16 (one query per lane); score = fma(S^T, scale * log2(e), slot), base-2 softmax; the
//     slot row is 0 for a key that exists and -inf behind the last key, which is all the bounds logic the scores need;
//   * per head, sweep 1 over the key tiles: the online row maximum and denominator (online_sum, attention_stage.h), kept in
//     two REGISTERS of the lane that owns the query -- nothing per head outlives its head, so there is no head limit;
//   * per head, sweep 2 over the key tiles: the tile's scores again, p = exp2(s - m) * (1 / l), SELECTED to 0 for a query
//     row >= Mq (pad rows may hold NaN: they are not read, and what their lanes compute is not used), then summed down the
//     query rows: each wave turns its 32 x 32 blocks round through LDS (rows of 33 floats) and a lane adds the 16 rows of its
//     half in ascending order, the two halves are added, the four waves' sums are added in ascending order and the result
//     is added to the tile's slot of the workgroup's column accumulators in LDS (Mk <= 4096 fp32 = 16 KB).  Heads arrive in
//     ascending order;
//   * one query tile (Mq <= 128): accumulator * (1 / h) goes straight to `out`.  More: the tile's raw accumulators go to
//     the caller's workspace and attention_mass_reduce_kernel adds the tiles in ascending order and multiplies by 1 / h once.
// The form with a grid over (query tile, sample) was chosen over one workgroup per sample: at 768^2 and beyond the mid
// block's few samples would leave all but B of the CUs idle, and the tile order of the second launch is as fixed as a loop.
// No atomics; the order of every addition depends on (h, Mq, Mk) alone, so a sample's bits depend neither on B, nor on the
// other samples, nor on the run.
// Cost: K is re-staged from L2 twice per head and query tile; q is read once per step of its head.
#include "attention_checks.h"
#include "attention_stage.h"

namespace {

constexpr int MASS_WAVES = 4, MASS_NT = MASS_WAVES * 64;
constexpr int MASS_QB = MASS_WAVES * QW;        // query rows per workgroup: the query tile
constexpr int MASS_MAX_KEYS = 4096;             // the column accumulators of a workgroup in LDS: 16 KB
constexpr int64_t MASS_MAX_QUERIES = 65536;     // 512 query tiles

template <typename T, int D>
__global__ __launch_bounds__(MASS_NT, 2) void attention_mass_kernel(const T *__restrict__ q, int64_t ldq,
                                                                    const T *__restrict__ k, int64_t ldk,
                                                                    float *__restrict__ dst, int64_t ld_dst, int H, int64_t M,
                                                                    int64_t Mp, int Mk, int64_t Mkp, float scale_log2e,
                                                                    int64_t nqb, float factor) {
    using F = Frag<T>;
    using vec = typename F::vec;
    using elem = typename F::elem;
    constexpr int NT = MASS_NT;
    using Stage = KvStage<T, D, NT>;
    constexpr int DK = Stage::DK;
    constexpr int K_STRIDE = Stage::K_STRIDE;
    constexpr int T_STRIDE = 33;

    __shared__ __attribute__((aligned(16))) elem sK[KV * K_STRIDE];
    __shared__ __attribute__((aligned(16))) float sSlot[2][KV];          // [0]: a full tile (zeros); [1]: the last tile
    __shared__ float sT[MASS_WAVES][QW * T_STRIDE];                      // a wave's 32 queries x 32 keys, turned round
    __shared__ float sPart[MASS_WAVES][KV];                              // the waves' column sums of one tile
    __shared__ float sCol[MASS_MAX_KEYS];                                // the workgroup's column accumulators

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int64_t b = (int64_t)blockIdx.x / nqb, qt = (int64_t)blockIdx.x % nqb;
    const int64_t qi = qt * MASS_QB + wave * QW + l31;
    const bool q_ok = qi < M;
    const T *qrow = q + (b * Mp + (q_ok ? qi : 0)) * ldq;
    const T *kb0 = k + b * Mkp * ldk;
    const int ntiles = (Mk + KV - 1) / KV;

    zero_k_pads<T, D, NT>(sK, tid);
    if (tid < KV) {
        sSlot[0][tid] = 0.0f;
        sSlot[1][tid] = (ntiles - 1) * KV + tid < Mk ? 0.0f : -INFINITY;
    }
    for (int i = tid; i < ntiles * KV; i += NT) sCol[i] = 0.0f;

    Stage stage;
    stage.init(tid, ldk, 0);   // (the V^T half is never used)

    // The steps: head = i / (2 ntiles); inside a head, sweep 1 over the tiles, then sweep 2 over the tiles.  One sequence,
    // so that the prefetch runs across every boundary.
    const int n = H * 2 * ntiles;
    auto head_of = [&](int i) { return i / (2 * ntiles); };
    auto tile_of = [&](int i) { return i % ntiles; };
    auto second = [&](int i) { return i % (2 * ntiles) >= ntiles; };
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

    float m_run = -INFINITY, l_run = 0.0f;   // sweep 1: the head's running max (log2 units) and this lane's share of the sum
    float m_head = 0.0f, il_head = 0.0f;     // sweep 2: the head's maximum and 1 / denominator of the lane's query

    auto step1 = [&](int ct) {
        f32x16 s[2];
        if (ct == 0) {
            m_run = -INFINITY;
            l_run = 0.0f;
        }
        qk_scores_biased<T, D, NT>(s, sK, sSlot[ct == ntiles - 1 ? 1 : 0], qf, 0, scale_log2e, l31, hi);
        const float m_use = online_sum(s, m_run, l_run);   // (as attention_probs_kernel; every tile has a key)
        if (ct == ntiles - 1) {
            m_head = m_use;
            il_head = 1.0f / (l_run + __shfl_xor(l_run, 32, 64));
        }
    };
    auto step2 = [&](int ct) {   // (barriers inside: every wave takes this step together)
        f32x16 s[2];
        qk_scores_biased<T, D, NT>(s, sK, sSlot[ct == ntiles - 1 ? 1 : 0], qf, 0, scale_log2e, l31, hi);
        float *t = sT[wave];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(s[kb][r] - m_head) * il_head;
                t[l31 * T_STRIDE + (r & 3) + 8 * (r >> 2) + 4 * hi] = q_ok ? p : 0.0f;   // a select, not a product
            }
            __syncthreads();
            float c = 0.0f;   // key 32 kb + l31 of the tile: the query rows 16 hi .. 16 hi + 15 of the wave, ascending
#pragma unroll
            for (int j = 0; j < 16; ++j) c += t[(16 * hi + j) * T_STRIDE + l31];
            c += __shfl_xor(c, 32, 64);
            if (hi == 0) sPart[wave][kb * 32 + l31] = c;
            __syncthreads();
        }
        if (tid < KV) sCol[ct * KV + tid] += ((sPart[0][tid] + sPart[1][tid]) + sPart[2][tid]) + sPart[3][tid];
    };

    // step i is in LDS, step i + 1 in flight.  A column of sCol is only ever touched by thread (column % 64); sPart is
    // rewritten after the barriers that end the step.
    issue(0);
    stage.write_k(sK);
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        const bool more = i + 1 < n;
#pragma unroll
        for (int ks = 0; ks < DK; ++ks) qf[ks] = qn[ks];
        if (more) issue(i + 1);
        if (second(i))   // (uniform)
            step2(tile_of(i));
        else
            step1(tile_of(i));
        __syncthreads();   // every wave has read the tile
        if (more) stage.write_k(sK);
        __syncthreads();
    }
    float *row = dst + (b * nqb + qt) * ld_dst;
    for (int j = tid; j < Mk; j += NT) row[j] = sCol[j] * factor;
}

// out[b, j] = (1 / h) * sum over the query tiles, in ascending order, of the tile's column sums
__global__ __launch_bounds__(256) void attention_mass_reduce_kernel(const float *__restrict__ ws, float *__restrict__ out,
                                                                    int64_t ldo, int Mk, int64_t nqb, float inv_h) {
    const int64_t b = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Mk) return;
    const float *p = ws + b * nqb * Mk + j;
    float acc = 0.0f;
    for (int64_t t = 0; t < nqb; ++t) acc += p[t * Mk];
    out[b * ldo + j] = acc * inv_h;
}

size_t mass_ws_bytes(int64_t B, int64_t Mq, int64_t Mk) {
    const int64_t nqb = vtm::cdiv(Mq, MASS_QB);
    return nqb <= 1 ? 0 : (size_t)(B * nqb * Mk) * sizeof(float);
}

template <typename T, int D>
void launch_mass(const void *q, int64_t ldq, const void *k, int64_t ldk, float *out, int64_t ldo, int64_t B, int64_t h,
                 int64_t Mq, int64_t Mqp, int64_t Mk, int64_t Mkp, float scale, float *ws, hipStream_t s) {
    const int64_t nqb = vtm::cdiv(Mq, MASS_QB);
    const float inv_h = 1.0f / (float)h;
    const bool direct = nqb == 1;
    hipLaunchKernelGGL((attention_mass_kernel<T, D>), dim3((unsigned)(B * nqb)), dim3(MASS_NT), 0, s, (const T *)q, ldq,
                       (const T *)k, ldk, direct ? out : ws, direct ? ldo : Mk, (int)h, Mq, Mqp, (int)Mk, Mkp,
                       scale * 1.4426950408889634f, nqb, direct ? inv_h : 1.0f);
    if (!direct)
        hipLaunchKernelGGL(attention_mass_reduce_kernel, dim3((unsigned)vtm::cdiv(Mk, 256), (unsigned)B), dim3(256), 0, s, ws,
                           out, ldo, (int)Mk, nqb, inv_h);
}

}  // namespace

VTM_EXPORT size_t vtm_attention_key_mass_ws_bytes(int64_t B, int64_t Mq, int64_t Mk) {
    if (B <= 0 || Mq <= 0 || Mq > MASS_MAX_QUERIES || Mk <= 0 || Mk > MASS_MAX_KEYS) return 0;
    return mass_ws_bytes(B, Mq, Mk);
}

VTM_EXPORT int vtm_attention_key_mass(const void *q, int64_t ldq, const void *k, int64_t ldk, float *out, int64_t ldo,
                                      int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mqp, int64_t Mk, int64_t Mkp,
                                      int64_t d, float scale, void *ws, size_t ws_bytes, vtm_stream_t stream) {
    const char *who = "vtm_attention_key_mass";
    VTM_REQUIRE(q && k && out, "%s: null pointer", who);
    if (int rc = check_qk_aligned(who, q, k, (reinterpret_cast<uintptr_t>(out) & 3) == 0)) return rc;
    if (int rc = check_map_sizes(who, B, h, Mq, Mqp, Mk, Mkp, d)) return rc;
    VTM_REQUIRE(Mk <= MASS_MAX_KEYS, "%s: Mk = %lld, at most %d keys are taken", who, (long long)Mk, MASS_MAX_KEYS);
    VTM_REQUIRE(Mq <= MASS_MAX_QUERIES, "%s: Mq = %lld, at most %lld queries are taken", who, (long long)Mq,
                (long long)MASS_MAX_QUERIES);
    VTM_REQUIRE(h < (1ll << 20), "%s: h = %lld is not a head count", who, (long long)h);
    if (int rc = check_scale(who, scale)) return rc;
    if (int rc = check_half_dtype(who, dtype)) return rc;
    if (int rc = check_qk_rows(who, ldq, ldk, h, d, Mk, ldo, Mk, "ldo >= Mk")) return rc;
    VTM_REQUIRE(B * vtm::cdiv(Mq, MASS_QB) < (1ll << 31) && B < 65536, "%s: grid too large", who);
    const size_t need = mass_ws_bytes(B, Mq, Mk);
    VTM_REQUIRE(need == 0 || (ws != nullptr && ws_bytes >= need && (reinterpret_cast<uintptr_t>(ws) & 3) == 0),
                "%s: workspace of %zu bytes needed (vtm_attention_key_mass_ws_bytes), %zu given", who, need,
                ws ? ws_bytes : (size_t)0);
    hipStream_t s = vtm::as_stream(stream);
    return with_half_head_dim(dtype, d, [&](auto t, auto dim) {
        launch_mass<decltype(t), decltype(dim)::value>(q, ldq, k, ldk, out, ldo, B, h, Mq, Mqp, Mk, Mkp, scale, (float *)ws, s);
        return vtm::launch_status(who);
    });
}
