// What the 16-bit attention kernels (attention.hip, attention16.hip, attention16g.hip, attention_sets.hip,
// attention_bias.hip, attention_probs.hip, attention_words.hip, attention_mass.hip) share of their tile handling: the buffer descriptor, the
// K / V^T tile stage global memory -> staging registers -> LDS, the Q-fragment load, the score tile of the map kernels with
// its online-softmax step, the K pad initialisation and, for the two small cross-attention kernels, the V^T pad
// initialisation, the split-P PV step and the 32-row output store.
// Header-only; everything is __forceinline__ and every loop fully unrolled: the
// kernels that use a piece keep the registers they had with its text written out, and where they did not, they do not use it
// (profiles/attention_stage_resources.txt).
#pragma once
#include "attention_common.h"

#include <type_traits>

namespace vtm_att {

// Buffer descriptor of one (sample, head) slice of K, V^T or a bias row.  It carries no real bound (the flags: 2^31 - 1
// bytes, raw dword format): full tiles lie inside the slice by construction, every fetch of a ragged tile is guarded
// explicitly (KvStage::issue_k / issue_v), and the exports check that a slice stays below 2 GiB -- offsets are 32-bit BYTE
// offsets, hence the `* 2u` on every element offset below.
template <typename P>
__device__ __forceinline__ auto kv_rsrc(const P *p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<P *>(p), 0, 0x7fffffff, 0x00020000);
}

// One tile of KV = 64 keys on its way to LDS, for a workgroup of NT threads: K as [key][K_STRIDE], V^T as
// [channel][VT_STRIDE].  A tile is cut into 16-byte chunks, chunk c = tid + NT i: K chunk = (row c / DCH, piece c % DCH),
// V^T chunk = (channel row c / 8, key piece c % 8).  Per thread the global byte offset and the LDS offset of every chunk are
// computed once (init); a tile is then fetched with buffer loads against a wave-uniform descriptor and a SCALAR tile offset
// -- no vector address arithmetic inside the tile loop (the kernels are VALU-bound at d = 40).
// attention16s_kernel and attention16g_kernel carry this stage written out: at 256 VGPRs with spills, either form of the
// shared code moved spills into their tile loops (profiles/attention_stage_resources.txt).  A change here has to be made
// there too.
template <typename T, int D, int NT>
struct KvStage {
    using elem = typename Frag<T>::elem;
    static constexpr int DK = (D + 15) / 16;      // k-steps of the QK^T contraction
    // elements per K row in LDS: (DK * 8 + 4) words = 4 x odd, so the b128 fragment reads of 32 rows are conflict-free
    static constexpr int K_STRIDE = DK * 16 + 8;
    static constexpr int DCH = D / 8;             // 16-byte chunks per K row
    static constexpr int K_CHUNKS = KV * DCH, V_CHUNKS = D * (KV / 8);   // per tile
    static constexpr int K_PER_T = (K_CHUNKS + NT - 1) / NT, V_PER_T = (V_CHUNKS + NT - 1) / NT;

    uint32_t kgo[K_PER_T], vgo[V_PER_T];   // global byte offsets relative to the tile base; 0 for a surplus thread
    int koff[K_PER_T], voff[V_PER_T];      // LDS element offsets inside the tile
    int krow[K_PER_T], vkey[V_PER_T];      // the chunk's key row / first key inside the tile
    bool kok[K_PER_T], vok[V_PER_T];       // the chunk exists (K_CHUNKS, V_CHUNKS need not be multiples of NT)
    uint4 rk[K_PER_T], rv[V_PER_T];        // the tile in flight

    __device__ __forceinline__ void init(int tid, int64_t ldk, int64_t ldvt) {
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
            // The V^T swizzle.  Inside every 16-key group the tile is stored as [k0-3 | k8-11 | k4-7 | k12-15]: the 8 keys
            // one lane feeds to a PV k-step -- 4 hi + {0..3} and 8 + 4 hi + {0..3}, the key order the S^T accumulators
            // already have -- are then ONE contiguous 16-byte read.  This line and the PV fragment reads (32-row blocks:
            // `+ 8 * hi + st * 16`, 16-row blocks: `+ (g16 & 1) * 16 + (g16 >> 1) * 8`) have to agree; write_v splits a
            // chunk accordingly.
            voff[i] = (c / (KV / 8)) * VT_STRIDE + (vkey[i] & ~15) + ((vkey[i] >> 3) & 1) * 4;
        }
    }

    template <typename R>
    __device__ static __forceinline__ uint4 fetch(const R &rsrc, uint32_t voff_, uint32_t soff_) {
        return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff_, soff_, 0));
    }

    // The tile at scalar byte offset `so` into the staging registers, K and V^T halves on their own.
    // FULL (a tile completely inside the keys): no bounds logic, and the loads are UNCONDITIONAL -- surplus threads re-read
    // chunk 0 (their offset is 0) and simply do not store it: a load inside a divergent branch makes the compiler wait for
    // ALL outstanding loads right after it.  A kernel that adds loads of its own to a full tile has to keep to that.
    // Otherwise the tile starts at key `key0` and rows / keys >= `end` read as zero without being fetched.
    template <bool FULL, typename R, typename I = int>
    __device__ __forceinline__ void issue_k(std::bool_constant<FULL>, const R &rsrc, uint32_t so, I key0 = 0, I end = 0) {
#pragma unroll
        for (int i = 0; i < K_PER_T; ++i) {
            if constexpr (FULL) {
                rk[i] = fetch(rsrc, kgo[i], so);
            } else {
                uint4 v = make_uint4(0, 0, 0, 0);
                if (kok[i] && key0 + krow[i] < end) v = fetch(rsrc, kgo[i], so);
                rk[i] = v;
            }
        }
    }
    template <bool FULL, typename R, typename I = int>
    __device__ __forceinline__ void issue_v(std::bool_constant<FULL>, const R &rsrc, uint32_t so, I key0 = 0, I end = 0) {
#pragma unroll
        for (int i = 0; i < V_PER_T; ++i) {
            if constexpr (FULL) {
                rv[i] = fetch(rsrc, vgo[i], so);
            } else {
                uint4 v = make_uint4(0, 0, 0, 0);
                const I key = key0 + vkey[i];
                if (vok[i] && key < end) {   // key % 8 == 0, ldvt % 8 == 0, ldvt >= end: the 16-byte piece is inside the row
                    v = fetch(rsrc, vgo[i], so);
                    // the keys of the piece behind `end` belong to nobody (or to the next set): their p is 0, but 0 * garbage
                    // may be NaN
                    mask_keys(v, (int)(end - key));
                }
                rv[i] = v;
            }
        }
    }
    template <typename R>
    __device__ __forceinline__ void issue_full(const R &rsrc_k, const R &rsrc_v, uint32_t so_k, uint32_t so_v) {
        issue_k(std::true_type{}, rsrc_k, so_k);
        issue_v(std::true_type{}, rsrc_v, so_v);
    }
    template <typename R, typename I>
    __device__ __forceinline__ void issue_masked(const R &rsrc_k, const R &rsrc_v, uint32_t so_k, uint32_t so_v, I key0,
                                                 I end) {
        issue_k(std::false_type{}, rsrc_k, so_k, key0, end);
        issue_v(std::false_type{}, rsrc_v, so_v, key0, end);
    }

    // The K half of ANY tile (full or ragged) without a branch around a load: every thread fetches -- a chunk outside the
    // keys, like a surplus thread's, re-reads chunk 0 of the tile, which exists (key0 < end) -- and write_k_select stores
    // zeros for it.  The selection waits until the write, so the loads stay in flight behind the step that issued them
    // (issue_k's guarded fetches of a ragged tile are waited for on the spot, see above); costs a few VALU operations per
    // chunk on full tiles.  attention_words_kernel uses the pair.
    template <typename R, typename I = int>
    __device__ __forceinline__ void issue_k_select(const R &rsrc, uint32_t so, I key0, I end) {
#pragma unroll
        for (int i = 0; i < K_PER_T; ++i) {
            const bool ok = kok[i] && key0 + krow[i] < end;
            rk[i] = fetch(rsrc, ok ? kgo[i] : 0u, so);
        }
    }
    template <typename I = int>
    __device__ __forceinline__ void write_k_select(elem *sK_tile, I key0, I end) const {
#pragma unroll
        for (int i = 0; i < K_PER_T; ++i)
            if (kok[i])
                *reinterpret_cast<uint4 *>(sK_tile + koff[i]) = key0 + krow[i] < end ? rk[i] : make_uint4(0, 0, 0, 0);
    }

    // staging registers -> the LDS tile (never its pad columns / rows)
    __device__ __forceinline__ void write_k(elem *sK_tile) const {
#pragma unroll
        for (int i = 0; i < K_PER_T; ++i)
            if (kok[i]) *reinterpret_cast<uint4 *>(sK_tile + koff[i]) = rk[i];
    }
    __device__ __forceinline__ void write_v(elem *sV_tile) const {
#pragma unroll
        for (int i = 0; i < V_PER_T; ++i)
            if (vok[i]) {   // keys 0-3 and 4-7 of the chunk go to the two halves of the 16-key group (see voff)
                uint2 *dst = reinterpret_cast<uint2 *>(sV_tile + voff[i]);
                dst[0] = make_uint2(rv[i].x, rv[i].y);
                dst[2] = make_uint2(rv[i].z, rv[i].w);
            }
    }
    __device__ __forceinline__ void write(elem *sK_tile, elem *sV_tile) const {
        write_k(sK_tile);
        write_v(sV_tile);
    }
};

// Q fragments (B operand of S^T = K Q^T) of the query row at `qp`: lane (query l31, half hi) holds d = 16 ks + 8 hi + 0..7,
// zero beyond D and for a dead query (`qi_ok` false; qp then points at row 0 and is not read).
template <typename T, int D>
__device__ __forceinline__ void load_q_frags(typename Frag<T>::vec (&qf)[(D + 15) / 16], const T *qp, bool qi_ok, int hi) {
    using vec = typename Frag<T>::vec;
#pragma unroll
    for (int ks = 0; ks < (D + 15) / 16; ++ks) {
        const int d0 = ks * 16 + hi * 8;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (d0 < D && qi_ok) v = *reinterpret_cast<const uint4 *>(qp + d0);
        qf[ks] = __builtin_bit_cast(vec, v);
    }
}

// ---- the score tile of the map kernels ----
// attention_words_kernel and attention_mass_kernel use it; attention_probs_kernel carries the same text written out in its `scores` lambda: calling
// this helper there kept every instantiation's VGPR / SGPR / LDS numbers but renumbered registers and moved a few
// instructions, and that kernel's code is pinned (profiles/attention_words_resources.txt).  A change here has to be made
// there too.

// Scores of the 64-key tile `ct` in LDS against one query per lane, in log2 units: S^T = K Q^T on v_mfma_f32_32x32x16, then
// fma(S^T, scale * log2(e), slot) with `sB` the sample's bias row times log2(e) (-inf behind the last key: all the bounds
// logic the scores need).  Lane (l31, hi) holds keys 64 ct + 32 kb + (r & 3) + 8 (r >> 2) + 4 hi of query l31 in s[kb][r].
template <typename T, int D, int NT>
__device__ __forceinline__ void qk_scores_biased(f32x16 (&s)[2], const typename Frag<T>::elem *sK, const float *sB,
                                                 const typename Frag<T>::vec (&qf)[(D + 15) / 16], int ct, float scale_log2e,
                                                 int l31, int hi) {
    using F = Frag<T>;
    using vec = typename F::vec;
    using elem = typename F::elem;
    constexpr int DK = KvStage<T, D, NT>::DK, K_STRIDE = KvStage<T, D, NT>::K_STRIDE;
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
}

// The online-softmax step of a score tile `s` (the layout above), per query: the running maximum `m_run` joined with the
// tile's over the lane's 32 scores and both half-waves into `m_new`; returns the base the tile's exponents are taken
// against.  While only masked keys have been seen that base is 0: -inf - (-inf) would be NaN, and against 0 every p of such
// a query is exp2(-inf) = 0.
__device__ __forceinline__ float online_max(const f32x16 (&s)[2], float m_run, float &m_new) {
    float mt = fmaxf(s[0][0], s[1][0]);
#pragma unroll
    for (int r = 1; r < 16; ++r) mt = fmaxf(fmaxf(mt, s[0][r]), s[1][r]);
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    m_new = fmaxf(m_run, mt);
    return m_new == -INFINITY ? 0.0f : m_new;
}

// online_max plus the denominator: `l_run`, this lane's share of the sum, is rescaled to the new base and takes the tile's
// exponentials (nothing finite seen before: l_run is 0); m_run becomes the new maximum.  Returns the base.
__device__ __forceinline__ float online_sum(const f32x16 (&s)[2], float &m_run, float &l_run) {
    float m_new;
    const float m_use = online_max(s, m_run, m_new);
    float sum = 0.0f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += __builtin_amdgcn_exp2f(s[kb][r] - m_use);
    l_run = l_run * __builtin_amdgcn_exp2f(m_run - m_use) + sum;
    m_run = m_new;
    return m_use;
}

// ---- LDS pads ----

// The K pad columns meet Q's zero padding, but garbage there could be NaN; tile stores never touch them.
template <typename T, int D, int NT>
__device__ __forceinline__ void zero_k_pads(typename Frag<T>::elem *sK, int tid) {
    using elem = typename Frag<T>::elem;
    constexpr int K_STRIDE = KvStage<T, D, NT>::K_STRIDE;
    for (int i = tid; i < KV * (K_STRIDE - D); i += NT)
        sK[(i / (K_STRIDE - D)) * K_STRIDE + D + i % (K_STRIDE - D)] = (elem)0.0f;
}

// ---- the single-buffered tile of attention_sets_kernel / attention_bias_kernel: V^T in 32-row blocks, nothing rides in
// the pads ----

// One-time LDS init: the K pad columns as in zero_k_pads, and the V^T pad rows, which feed O^T rows nobody stores but could
// hold NaN just the same.  The K loop stays written out: with a call of zero_k_pads in its place attention_sets_kernel's
// code came out different (profiles/attention_contract_codeobj.txt).  A change there has to be made here too.
template <typename T, int D, int NT>
__device__ __forceinline__ void zero_kv_pads(typename Frag<T>::elem *sK, typename Frag<T>::elem *sV, int tid) {
    using elem = typename Frag<T>::elem;
    constexpr int K_STRIDE = KvStage<T, D, NT>::K_STRIDE, VROWS = (D + 31) / 32 * 32;
    for (int i = tid; i < KV * (K_STRIDE - D); i += NT)
        sK[(i / (K_STRIDE - D)) * K_STRIDE + D + i % (K_STRIDE - D)] = (elem)0.0f;
    for (int i = tid; i < (VROWS - D) * VT_STRIDE; i += NT) sV[D * VT_STRIDE + i] = (elem)0.0f;
}

// One 16-key step of O^T += V^T P^T: p = the lane's 8 probabilities, of keys 16 st + (e & 3) + 8 (e >> 2) + 4 hi, packed to
// the operand type; k-slot (hi, e) <-> that key, so `vp` = sV + l31 * VT_STRIDE + 8 * hi + 16 * st (see voff).  bf16 keeps
// 8 bits of P: there P goes in as hi + lo (two MFMAs on the same V^T fragment, the matrix pipe is idle anyway), so that its
// rounding stays below the operands' own.  The denominator l_run is summed from what the numerator sees.
template <typename T, int D>
__device__ __forceinline__ void pv_step_split(f32x16 (&o)[(D + 31) / 32], float &l_run, const float (&p)[8],
                                              const typename Frag<T>::elem *vp) {
    using F = Frag<T>;
    using vec = typename F::vec;
    constexpr bool SPLIT_P = std::is_same_v<T, vtm_bf16>;
    vec ph, pl;
    F::pack8(ph, p);
    if constexpr (SPLIT_P) {
        float plo[8];
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
    for (int dv = 0; dv < (D + 31) / 32; ++dv) {
        const vec vf = *reinterpret_cast<const vec *>(vp + dv * 32 * VT_STRIDE);
        o[dv] = F::mfma(vf, ph, o[dv]);
        if constexpr (SPLIT_P) o[dv] = F::mfma(vf, pl, o[dv]);
    }
}

// acc * factor, rounded to the output type, to the query row at `op`: acc[dv][r] = channel 32 dv + (r & 3) + 8 (r >> 2) + 4 hi
template <typename T, int D>
__device__ __forceinline__ void store_rows32(const f32x16 (&acc)[(D + 31) / 32], float factor, T *op, int hi) {
    using elem = typename Frag<T>::elem;
#pragma unroll
    for (int dv = 0; dv < (D + 31) / 32; ++dv)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d0 = dv * 32 + 8 * g + 4 * hi;
            if (d0 < D) {   // D % 8 == 0 and d0 % 4 == 0 -> the 4 channels are all valid
                elem w4[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) w4[e] = (elem)(acc[dv][g * 4 + e] * factor);
                *reinterpret_cast<uint2 *>(op + d0) = *reinterpret_cast<uint2 *>(w4);
            }
        }
}

}  // namespace vtm_att
