// vtm_frame_order: the kept rows of a merge closure in FRAME order, for a cross-attention on the merged tokens (patch.py's
// `merge_crossattn`; vidtome/patch.py:171-185 computes attn2 on every token, tomesd's option on m(x)).
//
// compute_merge's local levels leave `keep` (B, M_l) in MATCHING order -- a level puts its unmerged src rows first, in score
// order, then its dst rows -- while attn2's conditioning is given per frame row: joined row r of the chunk belongs to frame
// r / N.  Sorted ascending, the rows of one frame are one contiguous segment of the merged sequence, and the cross-attention
// core can serve a segment with one key sample (vtm_attention_kv_segments).
//
// The entries of a sample are DISTINCT rows of [0, L), so the sort is a rank over a presence table -- order.hip's counting
// sort with buckets of at most one entry, hence no arrival counters, no atomics and nothing to settle.  Two launches:
//   rank_kernel   one workgroup per (sample, frame).  It reads the sample's M_l entries twice: once to count the rows of the
//                 frames in front of its own -- its segment's offset; every workgroup repeats that count rather than wait for
//                 a launch that scans once -- and once to enter its own frame's rows into a table in LDS, slot r - f N = the
//                 entry's index j (+ 1).  A scan of the table in tiles of 1024 slots then gives every entered row its rank k:
//                 keep_sorted[b, k] = r and pos[b, j] = k.  A frame of more than 8192 tokens takes the table several times.
//   map_kernel    one thread per joined row: inv_sorted[b, i] = pos[b, inv_local[b, i]]
// Every index read from memory is range-checked before it addresses anything: maps that break the contract give wrong
// results inside the buffers, never an access outside them.
#include "common.h"

namespace {

constexpr int FT = 256;       // threads per workgroup of map_kernel
constexpr int RT = 1024;      // threads of a rank workgroup
constexpr int TABLE = 8192;   // rows of a frame per pass: the LDS table (32 KB)

// the sum of v over the workgroup, for every thread (two barriers; `part` is reusable after the next barrier)
__device__ __forceinline__ int block_sum(int v, int *part, int tid) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();
    if ((tid & 63) == 0) part[tid >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < RT / 64; ++w) s += part[w];
    return s;
}

__global__ __launch_bounds__(RT) void rank_kernel(const int32_t *__restrict__ keep, int64_t B, int64_t F, int64_t N, int64_t Ml,
                                                  int32_t *__restrict__ keep_sorted, int32_t *__restrict__ pos,
                                                  int32_t *__restrict__ seg_off) {
    __shared__ int table[TABLE];
    __shared__ int part[RT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x / F, f = blockIdx.x % F;
    const int64_t lo = f * N, hi = lo + N;
    const int32_t *kb = keep + b * Ml;
    int cnt = 0;   // the kept rows of the frames in front
    for (int64_t j = tid; j < Ml; j += RT) {
        const int64_t r = kb[j];
        cnt += r >= 0 && r < lo;
    }
    int run = block_sum(cnt, part, tid);
    run = run < Ml ? run : (int)Ml;
    if (tid == 0) {
        seg_off[b * F + f] = (int32_t)(b * Ml + run);
        if (b == B - 1 && f == F - 1) seg_off[B * F] = (int32_t)(B * Ml);
    }
    for (int64_t t0 = lo; t0 < hi; t0 += TABLE) {
        const int64_t t1 = t0 + TABLE < hi ? t0 + TABLE : hi;
        const int n = (int)(t1 - t0);
        __syncthreads();   // (the table and `part` of the pass before are read)
        for (int i = tid; i < TABLE; i += RT) table[i] = 0;
        __syncthreads();
        // distinct rows: one writer per slot (a repeated row, which the contract excludes, leaves one of its entries)
        for (int64_t j = tid; j < Ml; j += RT) {
            const int64_t r = kb[j];
            if (r >= t0 && r < t1) table[r - t0] = (int)j + 1;
        }
        __syncthreads();
        // the table's slots, 1024 at a time: rank = kept rows in front
        for (int i0 = 0; i0 < n; i0 += RT) {
            const int i = i0 + tid;
            const int v = i < n ? table[i] : 0;
            const int m = v != 0;
            int incl = m;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(incl, d, 64);
                if (lane >= d) incl += t;
            }
            __syncthreads();
            if (lane == 63) part[wave] = incl;
            __syncthreads();
            int before = run, tile = 0;
#pragma unroll
            for (int w = 0; w < RT / 64; ++w) {
                before += w < wave ? part[w] : 0;
                tile += part[w];
            }
            const int k = before + incl - m;
            if (m && k < Ml) {
                keep_sorted[b * Ml + k] = (int32_t)(t0 + i);
                pos[b * Ml + (v - 1)] = k;
            }
            run += tile;
        }
    }
    // (fewer than M_l rows found: `keep` had repeats or rows outside [0, L), which the contract excludes.  The tail is given
    // row 0 so that whoever gathers through keep_sorted stays inside the sample.)
    if (f == F - 1)
        for (int64_t k = run + tid; k < Ml; k += RT) keep_sorted[b * Ml + k] = 0;
}

__global__ __launch_bounds__(FT) void map_kernel(const int32_t *__restrict__ inv_local, int64_t B, int64_t Ml, int64_t L,
                                                 const int32_t *__restrict__ pos, int32_t *__restrict__ inv_sorted) {
    const int64_t g = (int64_t)blockIdx.x * FT + threadIdx.x;
    if (g >= B * L) return;
    const int64_t j = inv_local[g];
    int32_t k = 0;
    if (j >= 0 && j < Ml) k = pos[(g / L) * Ml + j];
    inv_sorted[g] = (k >= 0 && k < Ml) ? k : 0;   // (an entry the rank kernel never placed: see above)
}

}  // namespace

VTM_EXPORT size_t vtm_frame_order_ws_bytes(int64_t B, int64_t F, int64_t N) {
    if (B <= 0 || F <= 0 || N <= 0) return 0;
    return (size_t)(B * F * N) * 4;   // pos (B, M_l) for any M_l <= L
}

VTM_EXPORT int vtm_frame_order(const int32_t *keep, int64_t Ml, const int32_t *inv_local, int64_t B, int64_t F, int64_t N,
                               void *ws, size_t ws_bytes, int32_t *keep_sorted, int32_t *inv_sorted, int32_t *seg_off,
                               vtm_stream_t stream) {
    const char *who = "vtm_frame_order";
    VTM_REQUIRE(keep && inv_local && ws && keep_sorted && inv_sorted && seg_off, "%s: null pointer", who);
    VTM_REQUIRE(B > 0 && F > 0 && N > 0, "%s: bad sizes", who);
    VTM_REQUIRE(F < (1ll << 31) && N < (1ll << 31) && B < (1ll << 31) && B * F * N < (1ll << 31), "%s: too many rows", who);
    VTM_REQUIRE(Ml > 0 && Ml <= F * N, "%s: M_l = %lld is not in [1, L = %lld]", who, (long long)Ml, (long long)(F * N));
    if (ws_bytes < vtm_frame_order_ws_bytes(B, F, N))
        return vtm::fail(VTM_EWORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes, vtm_frame_order_ws_bytes(B, F, N));
    hipStream_t s = vtm::as_stream(stream);
    const int64_t L = F * N;
    int32_t *pos = static_cast<int32_t *>(ws);
    hipLaunchKernelGGL(rank_kernel, dim3((unsigned)(B * F)), dim3(RT), 0, s, keep, B, F, N, Ml, keep_sorted, pos, seg_off);
    hipLaunchKernelGGL(map_kernel, dim3((unsigned)vtm::cdiv(B * L, FT)), dim3(FT), 0, s, inv_local, B, Ml, L,
                       (const int32_t *)pos, inv_sorted);
    return vtm::launch_status(who);
}
