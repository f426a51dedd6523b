// vtm_match: fused cosine-similarity scoring + row-wise top-1 (the score matrix never exists).
// Reference: vidtome/merge.py:87 `scores = a @ b.transpose(-1, -2)` followed by
//            merge.py:109-113 `node_max, node_idx = scores.max(dim=-1)` (non-aligned) or
//            merge.py:93-97 (aligned: scores of all samples concatenated on the dst axis);
//            same statements at merge.py:392-417 for the global matcher.
// The reference materialises (B, Ns, Nd) fp32 (6.4 GB at the cfg-2 top block) and spends 90 % of the
// matching time in that bmm; here a 128(dst) x 256(src) score tile lives only in MFMA accumulators.
//
// Arithmetic: v_mfma_f32_32x32x2_f32 -- exact fp32, bit-for-bit the k-ascending fmaf chain of the
// oracle (CDNA4 guide section 3), at the fp32 vector peak (157.3 TFLOP/s), so this kernel is bound by
// the fp32 FMA rate, not by HBM (the operands are 12 kFLOP/byte).
//
// Mapping ("swapped" like a flash-attention QK^T): the MFMA A operand is the DST tile and the B operand
// the SRC tile, so D[i = dst][j = src] puts one src row per lane (j = lane & 31) and 16 dst rows per
// accumulator block in that lane's registers: the row-wise max/argmax is a per-lane running
// (value, index) pair with NO cross-lane traffic inside the loop.  Lanes see their dst indices in
// ascending order, so "strictly greater" keeps the first index (torch max semantics); partial results
// of lanes / waves / workgroups / batch samples (aligned mode) are combined with one 64-bit
// atomicMax on the packed key (orderable(value) << 32 | ~index), which is order-independent.
//
// Data movement (v2): operands are stored as k-panels  [C_pad/8][2][rows][4]  (see vidtome_hip.h):
//   * the dst tile of a K-step (128 rows x 32 channels = 8 panels x 2 KiB) goes HBM/L2 -> LDS directly
//     (global_load_lds_dwordx4, no VGPR round trip, no ds_write), lane-linear = conflict-free for the
//     ds_read_b128 fragment reads, double-buffered, one barrier per K-step;
//   * every wave owns 64 src rows and streams its B fragments straight into registers (two fully
//     coalesced 512-byte segments per load), double-buffered in VGPRs -- no LDS, no sharing needed.
// Per wave and K-step: 128 MFMAs (8192 matrix-pipe cycles) against 4 LDS-DMA issues, 8 global loads and
// 16 LDS reads.
//
// vtm_match_masked (the receptive field of merge.py:233-241 / 646-654) is the MASKED instantiation of the same kernel, see
// match_kernel below; vtm_match is the other one and compiles to what it was before the template.
#include <cstdlib>

#include "common.h"

namespace {

constexpr int BD = 128;   // dst rows per tile (MFMA A operand, via LDS)
constexpr int BS = 256;   // src rows per workgroup (MFMA B operand, registers): 64 per wave
constexpr int BK = 32;    // channels per pipeline step = 4 groups of 8
constexpr int THREADS = 256;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void glb_void;

__device__ __forceinline__ uint32_t orderable(float f) {
    // monotone map fp32 -> uint32 (NaN largest, -0 == +0)
    if (f != f) return 0xffffffffu;
    const uint32_t u = __float_as_uint(f + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// What vtm_match_masked adds to the kernel's arguments (an all-zero struct for vtm_match, which never reads it).
struct MaskArgs {
    const float4 *coord;     // coordinate pool (Bc, P, 4)
    int64_t cstride;         // float4s between two samples' coordinates: P, or 0 when Bc == 1
    uint32_t P;
    const int32_t *a_rows;   // (B, Ns) / (B, Nd) rows of the pool
    const int32_t *b_rows;
    float T;                 // a pair is masked when its squared distance is > T
    const float *sbox;       // (B, ns_tiles, 8) / (B, nd_tiles, 8): lo[4] | hi[4] of every tile's valid rows, all NaN when
    const float *dbox;       //   one of them is not finite; only read when `skip`
    int skip;
};

constexpr int LIVE_MAX = 1024;                                        // dst tiles one masked workgroup may be handed
constexpr size_t MASK_LDS = 2 * BD * sizeof(float4) + LIVE_MAX * sizeof(uint16_t) + 16;

// squared distance of two coordinates: fp32, the four components in ascending order, no fma (-ffp-contract=off)
__device__ __forceinline__ float dist2(const float4 &p, const float4 &q) {
    const float d0 = p.x - q.x, d1 = p.y - q.y, d2 = p.z - q.z, d3 = p.w - q.w;
    return ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
}
// ... and of two boxes: per component the gap between them (0 where they overlap), then the same operation sequence.  Rounding
// is monotone, so every pair of the two boxes has dist2 >= this value: a tile whose value is > T holds masked pairs only.
__device__ __forceinline__ float box_dist2(const float4 &alo, const float4 &ahi, const float4 &blo, const float4 &bhi) {
    const float g0 = fmaxf(0.0f, fmaxf(alo.x - bhi.x, blo.x - ahi.x)), g1 = fmaxf(0.0f, fmaxf(alo.y - bhi.y, blo.y - ahi.y));
    const float g2 = fmaxf(0.0f, fmaxf(alo.z - bhi.z, blo.z - ahi.z)), g3 = fmaxf(0.0f, fmaxf(alo.w - bhi.w, blo.w - ahi.w));
    return ((g0 * g0 + g1 * g1) + g2 * g2) + g3 * g3;
}

// One workgroup: src rows [st*256, st*256+256) of sample `bi`, dst tiles [jt0, jt1).
// MASKED (vtm_match_masked): a score whose src and dst coordinates are further apart than the receptive field counts as
// +0.0f in the fold; the workgroup first lists the dst tiles that hold an unmasked pair at all ("live": box test above) and
// runs the pipeline over that list only -- s below then counts K-steps of LIVE tiles, and load_a / load_b / the fold look
// the tile up, so the double-buffered chain is the unmasked kernel's, with no bubble at a gap.  Dead tiles contribute
// (+0.0f, lowest index) to every row, which only the first of them can win: one extra key at publication.
// The 128 dst coordinates of a tile go through LDS (gathered once per tile by 128 threads, a tile ahead, double-buffered):
// every lane of a half-wave needs the same 64 of them, so a ds_read_b128 of one address is a conflict-free broadcast,
// while direct loads would repeat the b_rows indirection (two dependent global loads) in every lane for every score.
// The 2 src coordinates of a lane stay in registers (one float4 per src block).
template <bool MASKED>
__global__ __launch_bounds__(THREADS, 2) void match_kernel(
    const float *__restrict__ a, const float *__restrict__ b, int64_t Ns, int64_t Nd, int64_t Ns_pad,
    int64_t Nd_pad, int64_t C_pad, int align, int ns_tiles, int nd_tiles, int nsplit, int tiles_per_split,
    unsigned long long *__restrict__ best, const MaskArgs m) {
    // dst tile of one K-step as 8 panels [g][kh][128 rows][4 floats], double-buffered (2 x 16 KiB)
    __shared__ __attribute__((aligned(16))) float sA[2][8 * BD * 4];
    // MASKED only (MASK_LDS bytes of dynamic LDS): dst coordinates [2][128] | live tile list | {live tiles, first dead tile}
    extern __shared__ __attribute__((aligned(16))) float4 sD[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kh = lane >> 5;

    int id = blockIdx.x;
    const int split = id % nsplit;
    id /= nsplit;
    const int st = id % ns_tiles;
    const int bi = id / ns_tiles;
    const int jt0 = split * tiles_per_split;
    const int jt1 = min(jt0 + tiles_per_split, nd_tiles);
    if (jt0 >= jt1) return;

    const int KT = (int)(C_pad / BK);
    int ntiles = jt1 - jt0, first_dead = -1;
    [[maybe_unused]] uint16_t *live = reinterpret_cast<uint16_t *>(sD + 2 * BD);
    if constexpr (MASKED) {
        int *meta = reinterpret_cast<int *>(live + LIVE_MAX);
        if (wave == 0) {
            float4 slo = {}, shi = {};
            if (m.skip) {
                const float4 *sb = reinterpret_cast<const float4 *>(m.sbox + ((int64_t)bi * ns_tiles + st) * 8);
                slo = sb[0], shi = sb[1];
            }
            int n = 0, fd = -1;
            for (int base = 0; base < ntiles; base += 64) {
                const int t = base + lane;
                bool dead = false;
                if (m.skip && t < ntiles) {
                    const float4 *db = reinterpret_cast<const float4 *>(m.dbox + ((int64_t)bi * nd_tiles + jt0 + t) * 8);
                    const float4 dlo = db[0], dhi = db[1];
                    dead = slo.x == slo.x && dlo.x == dlo.x && box_dist2(slo, shi, dlo, dhi) > m.T;
                }
                const bool lv = t < ntiles && !dead;
                const unsigned long long lm = __ballot(lv), dm = __ballot(dead);
                if (lv) live[n + __popcll(lm & ((1ull << lane) - 1ull))] = (uint16_t)t;
                if (fd < 0 && dm != 0) fd = base + __ffsll((long long)dm) - 1;
                n += __popcll(lm);
            }
            if (lane == 0) meta[0] = n, meta[1] = fd;
        }
        __syncthreads();
        ntiles = meta[0], first_dead = meta[1];
    }
    auto tile_of = [&](int i) -> int {   // i-th tile of the workgroup's pipeline
        if constexpr (MASKED) return jt0 + live[i];
        else return jt0 + i;
    };
    const int steps = ntiles * KT;
    const float *srcmat = a + (int64_t)bi * C_pad * Ns_pad;   // panels of the src operand
    const float *dstmat = b + (int64_t)bi * C_pad * Nd_pad;   // panels of the dst operand
    const int64_t srow0 = (int64_t)st * BS + wave * 64;

    // B fragments of one 8-channel group: [src block sb] float4 = k-pairs (8g + 2e + kh), e = 0..3;
    // double-buffered in registers at GROUP granularity (32 MFMAs = 2048 matrix-pipe cycles of cover)
    float4 rb[2][2];
    auto load_b = [&](int gi, float4 (&dst)[2]) {
        const int kt = (gi >> 2) % KT, g = gi & 3;
        const float *p = srcmat + (((int64_t)(kt * 4 + g) * 2 + kh) * Ns_pad + srow0 + l31) * 4;
        dst[0] = *reinterpret_cast<const float4 *>(p);
        dst[1] = *reinterpret_cast<const float4 *>(p + 32 * 4);
    };
    // A tile of one K-step: 16 LDS-DMA wave-instructions of 1 KiB (8 panels x 2 halves of 64 rows); wave w
    // issues 4 of them.  LDS image is lane-linear, i.e. exactly [panel][row][4].
    auto load_a = [&](int s, int buf) {
        const int jt = tile_of(s / KT), kt = s % KT;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int q = wave * 4 + t, p = q >> 1, half = q & 1;
            const float *gp = dstmat + (((int64_t)kt * 8 + p) * Nd_pad + (int64_t)jt * BD + half * 64 + lane) * 4;
            float *lp = &sA[buf][(p * BD + half * 64) * 4];
            __builtin_amdgcn_global_load_lds((glb_void *)gp, (lds_void *)lp, 16, 0, 0);
        }
    };

    f32x16 acc[4][2];
#pragma unroll
    for (int ib = 0; ib < 4; ++ib)
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ib][sb][r] = 0.0f;

    float bestv[2] = {-INFINITY, -INFINITY};
    uint32_t besti[2] = {0xffffffffu, 0xffffffffu};
    const uint32_t idx_base = align ? (uint32_t)((int64_t)bi * Nd) : 0u;

    // MASKED: the lane's two src coordinates, and the gather of a dst tile's coordinates (threads 0 .. 127, one row each)
    [[maybe_unused]] float4 sc4[2] = {};
    [[maybe_unused]] auto fetch_dc = [&](int ti) -> float4 {
        const int64_t d = (int64_t)tile_of(ti) * BD + tid;
        float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (d < Nd) v = m.coord[(int64_t)bi * m.cstride + min((uint32_t)m.b_rows[(int64_t)bi * Nd + d], m.P - 1u)];
        return v;
    };
    if constexpr (MASKED) {
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {
            const int64_t srow = srow0 + sb * 32 + l31;
            if (srow < Ns) sc4[sb] = m.coord[(int64_t)bi * m.cstride + min((uint32_t)m.a_rows[(int64_t)bi * Ns + srow], m.P - 1u)];
        }
        if (steps > 0 && tid < BD) sD[tid] = fetch_dc(0);
    }

    if (!MASKED || steps > 0) {   // (a masked workgroup may have no live tile)
        load_a(0, 0);
        load_b(0, rb[0]);
    }
    __syncthreads();   // (drains the LDS-DMA: vmcnt(0) + barrier)

    for (int s = 0; s < steps; ++s) {
        const int buf = s & 1;
        if (s + 1 < steps) load_a(s + 1, buf ^ 1);
        // MASKED: the step that ends a tile gathers the next live tile's dst coordinates; they land behind the MFMAs
        [[maybe_unused]] bool stage = false;
        [[maybe_unused]] float4 next_dc;
        if constexpr (MASKED) {
            stage = s + 1 < steps && (s + 1) % KT == 0 && tid < BD;
            if (stage) next_dc = fetch_dc((s + 1) / KT);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int gi = s * 4 + g;
            if (gi + 1 < steps * 4) load_b(gi + 1, rb[(g + 1) & 1]);
            float4 af[4];
#pragma unroll
            for (int ib = 0; ib < 4; ++ib)
                af[ib] = *reinterpret_cast<const float4 *>(&sA[buf][((g * 2 + kh) * BD + ib * 32 + l31) * 4]);
            const float4 b0 = rb[g & 1][0], b1 = rb[g & 1][1];
            const float bv[2][4] = {{b0.x, b0.y, b0.z, b0.w}, {b1.x, b1.y, b1.z, b1.w}};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int ib = 0; ib < 4; ++ib) {
                    const float av = e == 0 ? af[ib].x : e == 1 ? af[ib].y : e == 2 ? af[ib].z : af[ib].w;
#pragma unroll
                    for (int sb = 0; sb < 2; ++sb)
                        acc[ib][sb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[sb][e], acc[ib][sb], 0, 0, 0);
                }
            }
        }
        if constexpr (MASKED) {
            if (stage) sD[(((s + 1) / KT) & 1) * BD + tid] = next_dc;
        }
        if ((s + 1) % KT == 0) {
            // dst tile finished: fold the wave's 128 x 64 scores into the per-lane running (max, argmax)
            const int jt = tile_of(s / KT);
            const int dst0 = jt * BD + 4 * kh;
            const bool full = (int64_t)(jt + 1) * BD <= Nd;
            if constexpr (MASKED) {
                // same fold, dst-major so that every dst coordinate is read once for both src blocks (per src block the
                // dst indices still come in ascending order); a masked score is +0.0f whatever it was, NaN included
                const float4 *dcs = sD + ((s / KT) & 1) * BD + 4 * kh;
#pragma unroll
                for (int ib = 0; ib < 4; ++ib) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int dl = ib * 32 + (r & 3) + 8 * (r >> 2);
                        const float4 dc = dcs[dl];
                        const int d = dst0 + dl;
                        const bool valid = full || d < Nd;
#pragma unroll
                        for (int sb = 0; sb < 2; ++sb) {
                            const float sc = dist2(sc4[sb], dc) > m.T ? 0.0f : acc[ib][sb][r];
                            const bool upd = !(sc <= bestv[sb]) && (bestv[sb] == bestv[sb]) && valid;
                            bestv[sb] = upd ? sc : bestv[sb];
                            besti[sb] = upd ? (uint32_t)d : besti[sb];
                            acc[ib][sb][r] = 0.0f;
                        }
                    }
                }
            } else {
#pragma unroll
                for (int sb = 0; sb < 2; ++sb) {
                    float bv_ = bestv[sb];
                    uint32_t bi_ = besti[sb];
#pragma unroll
                    for (int ib = 0; ib < 4; ++ib) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int d = dst0 + ib * 32 + (r & 3) + 8 * (r >> 2);
                            const float sc = acc[ib][sb][r];
                            // s > best, or s is NaN while best is not (first NaN sticks: torch max)
                            bool upd = !(sc <= bv_) && (bv_ == bv_);
                            if (!full) upd = upd && (d < Nd);
                            bv_ = upd ? sc : bv_;
                            bi_ = upd ? (uint32_t)d : bi_;
                            acc[ib][sb][r] = 0.0f;
                        }
                    }
                    bestv[sb] = bv_;
                    besti[sb] = bi_;
                }
            }
        }
        __syncthreads();   // next K-step's dst tile has landed (vmcnt(0)) and this one is fully consumed
    }

    // publish: one atomicMax per (lane, src row); combines lane halves, splits and -- in aligned mode --
    // the samples of the batch (merge.py:96-97)
    const int64_t out_row0 = align ? 0 : (int64_t)bi * Ns;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
        const int64_t srow = srow0 + sb * 32 + l31;
        if constexpr (MASKED) {
            // the keys are totally ordered (largest value, then lowest index), so the dead tiles' one candidate -- +0.0f at the
            // lane's lowest dst index of the FIRST dead tile; the later ones tie at higher indices -- joins by a key maximum
            unsigned long long key = 0;
            if (besti[sb] != 0xffffffffu)
                key = ((unsigned long long)orderable(bestv[sb]) << 32) | (uint32_t)(~(besti[sb] + idx_base));
            const int64_t dd = (int64_t)(jt0 + first_dead) * BD + 4 * kh;
            if (first_dead >= 0 && dd < Nd) {
                const unsigned long long kd = ((unsigned long long)orderable(0.0f) << 32) | (uint32_t)(~((uint32_t)dd + idx_base));
                key = kd > key ? kd : key;
            }
            if (srow < Ns && key != 0) atomicMax(&best[out_row0 + srow], key);
        } else if (srow < Ns && besti[sb] != 0xffffffffu) {
            const unsigned long long key =
                ((unsigned long long)orderable(bestv[sb]) << 32) | (uint32_t)(~(besti[sb] + idx_base));
            atomicMax(&best[out_row0 + srow], key);
        }
    }
}

// Pre-pass of vtm_match_masked: block (bi, tile) writes lo[4] | hi[4] over the coordinates of the tile's valid rows -- src
// tiles of 256 rows first, then dst tiles of 128 -- or 8 NaNs when a coordinate is not finite or the tile has no valid row.
__global__ __launch_bounds__(THREADS) void box_kernel(const float4 *__restrict__ coord, int64_t cstride, uint32_t P,
                                                      const int32_t *__restrict__ a_rows, const int32_t *__restrict__ b_rows,
                                                      int64_t Ns, int64_t Nd, int ns_tiles, int nd_tiles,
                                                      float *__restrict__ sbox, float *__restrict__ dbox) {
    __shared__ float red[THREADS / 64][9];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = ns_tiles + nd_tiles;
    const int bi = blockIdx.x / per, t = blockIdx.x % per;
    const bool is_src = t < ns_tiles;
    const int tile = is_src ? t : t - ns_tiles;
    const int64_t n = is_src ? Ns : Nd, row = (int64_t)tile * (is_src ? BS : BD) + tid;
    const int32_t *rows = is_src ? a_rows : b_rows;
    float v[9] = {INFINITY, INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0f};   // lo | hi | bad
    if (row < n && (is_src || tid < BD)) {
        const float4 c = coord[(int64_t)bi * cstride + min((uint32_t)rows[(int64_t)bi * n + row], P - 1u)];
        const float e[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = v[4 + k] = e[k];
            if (!(fabsf(e[k]) < INFINITY)) v[8] = 1.0f;
        }
    }
    auto fold = [&](float (&x)[9], const float (&y)[9]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = fminf(x[k], y[k]), x[4 + k] = fmaxf(x[4 + k], y[4 + k]);
        x[8] = fmaxf(x[8], y[8]);
    };
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        float y[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) y[k] = __shfl_xor(v[k], off);
        fold(v, y);
    }
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 9; ++k) red[wave][k] = v[k];
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < THREADS / 64; ++w) fold(v, red[w]);
        const bool ok = v[8] == 0.0f && v[0] <= v[4];            // finite throughout, and at least one valid row
        float *out = (is_src ? sbox : dbox) + ((int64_t)bi * (is_src ? ns_tiles : nd_tiles) + tile) * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) out[k] = ok ? v[k] : __builtin_nanf("");
    }
}

}  // namespace

// `m` null: vtm_match; else vtm_match_masked (its sbox / dbox / skip are filled in here)
static int launch_match(const float *a, const float *b, int64_t B, int64_t Ns, int64_t Nd, int64_t Ns_pad,
                        int64_t Nd_pad, int64_t C_pad, int align, uint64_t *best, hipStream_t s,
                        MaskArgs *m = nullptr, float *ws = nullptr) {
    const char *what = m ? "vtm_match_masked" : "vtm_match";
    const int64_t out_rows = align ? Ns : B * Ns;
    hipError_t e = hipMemsetAsync(best, 0, (size_t)out_rows * sizeof(uint64_t), s);
    if (e != hipSuccess) return vtm::fail(VTM_ELAUNCH, "%s: memset: %s", what, hipGetErrorString(e));
    const int ns_tiles = (int)(Ns_pad / BS), nd_tiles = (int)(Nd_pad / BD);
    // enough workgroups to fill 256 CUs x 2 resident blocks a few times over, but keep >= 4 dst tiles
    // per block so the running-max epilogue and the atomics stay amortised
    int64_t want = vtm::cdiv(1536, (int64_t)ns_tiles * B);
    int nsplit = (int)(want < 1 ? 1 : want);
    if (nsplit > nd_tiles / 4) nsplit = nd_tiles / 4 > 0 ? nd_tiles / 4 : 1;
    if (m) {
        // masked: the work of a workgroup is its LIVE tiles, which with a small field are a few per src tile, next to each
        // other -- coarse splits leave them to a few workgroups while the rest exit at once (4 frames of 64 x 64, C = 320,
        // rec_field = 2: 286 us with vtm_match's 4 tiles per split, 152 us with 1; profiles/rf_match*.json).  So split down to
        // the fewest tiles that still make 8 K-steps; a workgroup without a live tile costs one box test.
        const int64_t min_tiles = vtm::cdiv(8, C_pad / BK);
        nsplit = (int)vtm::cdiv(nd_tiles, min_tiles);
        if (nsplit < vtm::cdiv(nd_tiles, LIVE_MAX)) nsplit = (int)vtm::cdiv(nd_tiles, LIVE_MAX);   // (the live list's size)
    }
    const int tiles_per_split = (int)vtm::cdiv(nd_tiles, nsplit);
    nsplit = (int)vtm::cdiv(nd_tiles, tiles_per_split);
    const int64_t grid = (int64_t)B * ns_tiles * nsplit;
    if (!m) {
        hipLaunchKernelGGL(match_kernel<false>, dim3((unsigned)grid), dim3(THREADS), 0, s, a, b, Ns, Nd, Ns_pad, Nd_pad,
                           C_pad, align, ns_tiles, nd_tiles, nsplit, tiles_per_split,
                           reinterpret_cast<unsigned long long *>(best), MaskArgs{});
        return vtm::launch_status(what);
    }
    // A/B hook, read once per process: run every tile (same bits; tests/test_gpu_rf.py, tools/rf_match.py)
    static const bool no_skip = [] {
        const char *v = getenv("VTM_DEBUG_NOBOXSKIP");
        return v && v[0] && !(v[0] == '0' && !v[1]);
    }();
    m->skip = !no_skip;
    m->sbox = ws;
    m->dbox = ws + B * ns_tiles * 8;
    if (m->skip) {
        hipLaunchKernelGGL(box_kernel, dim3((unsigned)(B * (ns_tiles + nd_tiles))), dim3(THREADS), 0, s, m->coord, m->cstride,
                           m->P, m->a_rows, m->b_rows, Ns, Nd, ns_tiles, nd_tiles, ws, ws + B * ns_tiles * 8);
        if (int rc = vtm::launch_status("vtm_match_masked: boxes")) return rc;
    }
    hipLaunchKernelGGL(match_kernel<true>, dim3((unsigned)grid), dim3(THREADS), MASK_LDS, s, a, b, Ns, Nd, Ns_pad, Nd_pad,
                       C_pad, align, ns_tiles, nd_tiles, nsplit, tiles_per_split,
                       reinterpret_cast<unsigned long long *>(best), *m);
    return vtm::launch_status(what);
}

VTM_EXPORT int vtm_match(const float *a, const float *b, int64_t B, int64_t Ns, int64_t Nd,
                         int64_t Ns_pad, int64_t Nd_pad, int64_t C_pad, int align, uint64_t *best,
                         vtm_stream_t stream) {
    VTM_REQUIRE(a && b && best, "vtm_match: null pointer");
    VTM_REQUIRE(B > 0 && Ns > 0 && Nd > 0, "vtm_match: bad sizes");
    VTM_REQUIRE(Ns_pad >= Ns && Ns_pad % BS == 0 && Nd_pad >= Nd && Nd_pad % BD == 0,
                "vtm_match: rows must be padded to a multiple of %d", VTM_MATCH_ROW_PAD);
    VTM_REQUIRE(C_pad > 0 && C_pad % BK == 0, "vtm_match: C_pad must be a multiple of %d", BK);
    VTM_REQUIRE(B * Nd < (1ll << 32) - 1, "vtm_match: index space overflow");
    return launch_match(a, b, B, Ns, Nd, Ns_pad, Nd_pad, C_pad, align, best, vtm::as_stream(stream));
}

VTM_EXPORT size_t vtm_match_masked_ws_bytes(int64_t B, int64_t Ns_pad, int64_t Nd_pad) {
    if (B <= 0 || Ns_pad <= 0 || Nd_pad <= 0) return 0;
    return (size_t)(B * (vtm::cdiv(Ns_pad, BS) + vtm::cdiv(Nd_pad, BD))) * 8 * sizeof(float);
}

VTM_EXPORT int vtm_match_masked(const float *a, const float *b, int64_t B, int64_t Ns, int64_t Nd, int64_t Ns_pad,
                                int64_t Nd_pad, int64_t C_pad, int align, const float *coord, int64_t Bc, int64_t P,
                                const int32_t *a_rows, const int32_t *b_rows, float T, void *ws, size_t ws_bytes,
                                uint64_t *best, vtm_stream_t stream) {
    VTM_REQUIRE(a && b && best, "vtm_match_masked: null pointer");
    VTM_REQUIRE(coord && a_rows && b_rows && ws, "vtm_match_masked: null coordinate pool, row list or workspace");
    VTM_REQUIRE(B > 0 && Ns > 0 && Nd > 0, "vtm_match_masked: bad sizes");
    VTM_REQUIRE(Ns_pad >= Ns && Ns_pad % BS == 0 && Nd_pad >= Nd && Nd_pad % BD == 0,
                "vtm_match_masked: rows must be padded to a multiple of %d", VTM_MATCH_ROW_PAD);
    VTM_REQUIRE(C_pad > 0 && C_pad % BK == 0, "vtm_match_masked: C_pad must be a multiple of %d", BK);
    VTM_REQUIRE(B * Nd < (1ll << 32) - 1, "vtm_match_masked: index space overflow");
    VTM_REQUIRE((Bc == B || Bc == 1) && P > 0 && P < (1ll << 31), "vtm_match_masked: the coordinate pool is (B or 1, P, 4)");
    VTM_REQUIRE(T == T, "vtm_match_masked: the threshold is NaN");
    VTM_REQUIRE((reinterpret_cast<uintptr_t>(coord) & 15) == 0 && (reinterpret_cast<uintptr_t>(ws) & 15) == 0,
                "vtm_match_masked: the coordinate pool and the workspace must be 16-byte aligned");
    if (ws_bytes < vtm_match_masked_ws_bytes(B, Ns_pad, Nd_pad))
        return vtm::fail(VTM_EWORKSPACE, "vtm_match_masked: workspace of %zu bytes, %zu needed", ws_bytes,
                         vtm_match_masked_ws_bytes(B, Ns_pad, Nd_pad));
    MaskArgs m{};
    m.coord = reinterpret_cast<const float4 *>(coord);
    m.cstride = Bc == 1 ? 0 : P;
    m.P = (uint32_t)P;
    m.a_rows = a_rows, m.b_rows = b_rows, m.T = T;
    return launch_match(a, b, B, Ns, Nd, Ns_pad, Nd_pad, C_pad, align, best, vtm::as_stream(stream), &m,
                        static_cast<float *>(ws));
}
