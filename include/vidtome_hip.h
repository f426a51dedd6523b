/*
 * vidtome_hip.h -- C ABI of libvidtome_hip.so: the MI355X (gfx950) implementation of VidToMe's
 * cross-frame token-merging hot path.
 *
 * Every entry point replaces a piece of the reference's Python hot path (the reference has no
 * native code; "binding" = the ctypes stub in vidtome_amd/_lib.py).
 * Citations are file:line under the reference checkout (/root/reference).
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless stated otherwise;
 *   - the caller allocates every input, output and workspace (e.g. through PyTorch's caching
 *     allocator); the library is stateless, never allocates or frees device memory and never
 *     synchronises the device;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - every call returns 0 on success or a negative VTM_E* code; vtm_last_error() returns a
 *     thread-local description of the last failure;
 *   - index arrays are int32 (the reference uses int64 tensors; values are identical);
 *   - token tensors are row-major (B, rows, C) in the model dtype (VTM_F16 / VTM_BF16 / VTM_F32).
 *
 * Canonical arithmetic of the matching path (bitwise equal to oracle/vtm_oracle.c):
 *   tokens upcast to fp32; norm = sqrtf(k-ascending fmaf chain of x*x); xhat = x / norm (IEEE
 *   divide); score = k-ascending fmaf chain from +0 (v_mfma_f32_32x32x2_f32 is exactly that chain);
 *   row max = first index among equals, first NaN wins; sort = descending, NaN first, ties by
 *   ascending index.
 */
#ifndef VIDTOME_HIP_H
#define VIDTOME_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 6): `flags_out` of the vtm_match_filtered* family is 8 int32 (it was 4 in version 1: a host built against the
 * version-1 header would see a 16-byte overrun, hence the bump -- check vtm_version() before calling). */
#define VTM_ABI_VERSION 2

enum vtm_dtype { VTM_F32 = 0, VTM_F16 = 1, VTM_BF16 = 2 };

enum vtm_status {
    VTM_OK = 0,
    VTM_EINVAL = -1,   /* bad argument (null pointer, negative size, unsupported dtype/shape) */
    VTM_ELAUNCH = -2,  /* HIP launch / runtime error (message in vtm_last_error) */
    VTM_EWORKSPACE = -3 /* workspace too small */
};

typedef void *vtm_stream_t; /* hipStream_t */

int vtm_version(void);
const char *vtm_last_error(void);
/* Bit mask of the ablation switches (vidtome_amd/csrc/ablate.h: experiment builds that drop loads / barriers / stores of
 * the hand-scheduled kernels and produce WRONG results) the library was compiled with.  0 for every library that may be
 * shipped; a host should refuse to run on anything else. */
int vtm_build_ablations(void);

/* Tile geometry the operand matrices of vtm_match must be padded to (rows to VTM_MATCH_ROW_PAD,
 * channels to VTM_MATCH_K_PAD). */
#define VTM_MATCH_ROW_PAD 256
#define VTM_MATCH_K_PAD 32
int64_t vtm_pad_rows(int64_t n);
int64_t vtm_pad_k(int64_t C);

/* ------------------------------------------------------------------------------------------------
 * vtm_normalize_gather -- replaces `metric / metric.norm(dim=-1, keepdim=True)` fused with `split`
 * (vidtome/merge.py:76-85 and 383-390).
 * The token pool is two row segments: x0 = the joined chunk (B, P0, C) and x1 = the block's global
 * anchor tokens (B, P1, C) (x1 may be NULL when P1 == 0); pool row id p < P0 addresses x0, else x1.
 * rows (B, n) int32 are pool row ids.  out receives the normalised rows in the k-PANEL operand layout of
 * vtm_match, B * C_pad * n_pad floats indexed [b][g = k/8][kh = k%2][row][e = (k%8)/2]: a panel (g, kh)
 * holds, for every row, the 4 channels 8g + kh + {0,2,4,6} as one 16-byte entry, so that (i) lane
 * (row, kh)'s 16-byte read feeds four consecutive v_mfma_f32_32x32x2_f32 k-steps in ascending k order,
 * (ii) a tile's panel slice is one contiguous run of rows (LDS-DMA friendly, fully coalesced);
 * rows >= n and channels >= C are zero.  norms (B, n) fp32 receives the row norms (it doubles
 * as the scratch between the two kernels of the call).
 * ---------------------------------------------------------------------------------------------- */
int vtm_normalize_gather(const void *x0, int64_t P0, const void *x1, int64_t P1, int dtype, int64_t B,
                         int64_t C, const int32_t *rows, int64_t n, float *norms, float *out,
                         int64_t n_pad, int64_t C_pad, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_match -- replaces `scores = a @ b.transpose(-1,-2)` + `scores.max(dim=-1)`
 * (vidtome/merge.py:87,109-113 and 392,413-417) and, with align != 0, the aligned variant
 * `torch.cat([*scores], dim=-1).max(dim=-1)` (merge.py:93-97 / 397-401).  The (B, Ns, Nd) score
 * matrix is never materialised.
 * a (src, Ns_pad rows), b (dst, Nd_pad rows): k-panel operands written by vtm_normalize_gather.
 * best: (B, Ns) uint64 when align == 0, (Ns) when align != 0.  Each entry is a packed key
 *     (orderable(node_max) << 32) | ~node_idx
 * whose unsigned maximum implements "largest value, first index, first NaN wins"; node_idx is in
 * [0, Nd) (align == 0) or [0, B*Nd) (align != 0, concatenated dst axis).  The call zero-fills
 * `best` itself.  Decode with vtm_decode_best.
 * ---------------------------------------------------------------------------------------------- */
int vtm_match(const float *a, const float *b, int64_t B, int64_t Ns, int64_t Nd, int64_t Ns_pad,
              int64_t Nd_pad, int64_t C_pad, int align, uint64_t *best, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_match_masked -- vtm_match with the receptive field of bipartite_soft_matching_random2d_hier / _2f: replaces
 *     mask = torch.norm(src_coord[:, :, None, :] - dst_coord[:, None, :, :], dim=-1) > rec_field
 *     scores = a @ b.transpose(-1, -2);  scores[mask] = 0
 * (vidtome/merge.py:233-241 and 646-654) in front of the same row maximum (merge.py:249-282 / 662-699).  Neither the
 * scores nor the mask are materialised.
 * a, b, B .. align, best: as vtm_match.  coord: the coordinate pool (Bc, P, 4) fp32, Bc = B or 1 (one set of coordinates
 * for every sample), 16-byte aligned, unused components 0; a_rows (B, Ns) / b_rows (B, Nd) int32: the pool row of every
 * src / dst row (the lists the operands were gathered with).
 * A pair is masked when s = sum_c (sc_c - dc_c)^2 > T, s in fp32 over the four components in ascending order.  T is the
 * host's: the largest fp32 t with fl32(sqrt(t)) <= rec_field (-INFINITY for rec_field < 0: every pair is masked); a
 * correctly rounded sqrt is monotone, so s > T is the reference's `norm > rec_field` without a device sqrt.  A masked
 * score is +0.0f whatever it was (NaN included, as the assignment does); a pair with a NaN coordinate is unmasked
 * (NaN > x is false).  PROMISE: bit parity with the reference for integer-valued coordinates with |value| <= 2048 in at
 * most 4 components, where s is exact; for other coordinates torch's norm may round differently, and a pair EXACTLY at the
 * boundary may then fall on the other side.
 * A 256 x 128 tile whose src and dst coordinate boxes are further apart than the field (same arithmetic on the per-component
 * gaps; exact, no margin; a box holding a non-finite value never qualifies) is all zeros and runs no MFMA: a pre-pass writes
 * the boxes into `ws`.  VTM_DEBUG_NOBOXSKIP=1 in the environment (read once per process) runs every tile: same bits.
 * ws: vtm_match_masked_ws_bytes(B, Ns_pad, Nd_pad) bytes, 16-byte aligned (VTM_EWORKSPACE when ws_bytes is less).
 * ---------------------------------------------------------------------------------------------- */
size_t vtm_match_masked_ws_bytes(int64_t B, int64_t Ns_pad, int64_t Nd_pad);
int vtm_match_masked(const float *a, const float *b, int64_t B, int64_t Ns, int64_t Nd, int64_t Ns_pad,
                     int64_t Nd_pad, int64_t C_pad, int align, const float *coord, int64_t Bc, int64_t P,
                     const int32_t *a_rows, const int32_t *b_rows, float T, void *ws, size_t ws_bytes,
                     uint64_t *best, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_match_filtered -- the same packed result as vtm_normalize_gather x2 + vtm_match, BIT FOR BIT, several
 * times faster: an fp16-MFMA filter pass (operands hi = fp16(1024*xhat), one product hi_dst * hi_src;
 * the residual lo terms are a build-time option) collects for every src row the dst rows whose approximate score lies within a
 * rigorous error window of the row's running maximum -- skipping the rest of a 32 x 32 block once a Cauchy-Schwarz bound on
 * the channels still to come says that none of its pairs can reach that window -- and an fp32 refine pass evaluates the
 * canonical fmaf chain on those candidates only.  Bounded escapes: a row with more than 64 candidates (flat image
 * regions, massively duplicated dst rows), or whose own norm is not a finite positive number in [2^-100, 2^100], is recomputed
 * by exact fp32-MFMA score tiles against all dst rows; a DST row of that kind (zero token -> NaN xhat, merge.py:84 has no eps)
 * makes that kernel recompute every row of the call (device flag, no host round trip).  Four launches per call (operand
 * preparation, filter, refine, escape).  C > 1280 is rejected (the error budget is derived for C <= 1280; use vtm_match).
 * Inputs are the token pool (x0 | x1, as vtm_normalize_gather) and the gathered pool ids a_rows (B, Ns),
 * b_rows (B, Nd); B * Nd < 2^31.  ws: >= vtm_match_filtered_ws_bytes(...) bytes.  flags_out (optional, 8 int32,
 * device): [0] = 1 if every row was recomputed exactly (a dst row without a usable norm), [1] = 1 if any row without a
 * usable norm was seen, [2] = number of rows recomputed by the escape because their candidate list overflowed or their own
 * norm was unusable, [3] = number of (row, dst) pairs the refine pass evaluated, [4] = 32 x 32 score blocks the filter's
 * partial-sum pruning tested, [5] = blocks still alive after the test (the others skipped their remaining MFMAs; both 0
 * when the rows are too short to prune), [6] = internal (the escape launch's work counter while it runs: unspecified), [7] = 0
 * (vtm_match_filtered_plan: blocks inside the spans of the second launch).  The block counters are only collected when flags_out
 * is given.  flags_out may be device memory or host memory (ABI version 2): memory a kernel can store to -- device, pinned /
 * registered host -- is written by the call's last launch itself, pageable host memory by a 32-byte asynchronous copy behind the
 * call; either way the values are there once the stream has passed the call.  Derivation of the window:
 * vidtome_amd/csrc/match_filter.hip.
 *
 * vtm_match_filtered_seeded -- the same result, usually faster on video tokens: before the filter starts every src row gets
 * a starting maximum from ONE guessed pair, the dst row at the same token position (one more small launch).  seed_N =
 * tokens per frame (0 = no seeds = vtm_match_filtered); pool rows < seed_L are tokens of the joined chunk (position =
 * row % seed_N), the rows of x1 have the positions seed_pos1 (B, P1) or, NULL, none; seed_table (B, seed_N) maps a position to
 * a dst index (vtm_partition_global writes it), NULL = identity (a local level: the first dst frame's rows are dst
 * indices 0 .. seed_N-1).  The score of an actual pair is a valid running maximum, so the result cannot change; a useless
 * guess only fails to help.
 * ---------------------------------------------------------------------------------------------- */
size_t vtm_match_filtered_ws_bytes(int64_t B, int64_t C, int64_t Ns, int64_t Nd, int align);
int vtm_match_filtered(const void *x0, int64_t P0, const void *x1, int64_t P1, int dtype, int64_t B,
                       int64_t C, const int32_t *a_rows, int64_t Ns, const int32_t *b_rows, int64_t Nd,
                       int align, void *ws, size_t ws_bytes, uint64_t *best, int32_t *flags_out,
                       vtm_stream_t stream);
int vtm_match_filtered_seeded(const void *x0, int64_t P0, const void *x1, int64_t P1, int dtype, int64_t B,
                              int64_t C, const int32_t *a_rows, int64_t Ns, const int32_t *b_rows, int64_t Nd,
                              int align, void *ws, size_t ws_bytes, uint64_t *best, int32_t *flags_out,
                              int64_t seed_L, int64_t seed_N, const int32_t *seed_pos1, const int32_t *seed_table,
                              vtm_stream_t stream);
/* vtm_match_filtered_plan -- vtm_match_filtered_seeded with the launch plan chosen by the caller; the RESULT is the same bits
 * for every plan.  VTM_MATCH_ONE_LAUNCH = as above.  VTM_MATCH_SCOUT_RANGE (round 5) is for levels whose src AND dst rows are in
 * (frame, position) order (the first local level): a "scout" launch runs the filter loop over the channels in front of the
 * pruning test only and marks the 256 x 128 (src tile, dst tile) pairs in which a block stays alive; the filter launch proper then
 * shrinks every workgroup's dst range -- one dst frame of seed_N tokens per split -- to the span of the marked tiles.  On
 * frames of one clip 94 % of the tile pairs of such a level are dead and a top level-1 call drops from 0.75 to about 0.5 ms;
 * when most tiles stay alive (uncorrelated tokens, noisy clips at this test depth, rows in similarity-rank order) the scout is
 * pure overhead (+ 40 %).  The host steers by the counters of the previous call of the same level: flags_out may be PINNED HOST
 * memory (the 32-byte copy is asynchronous either way); with this plan flags_out[4] / [5] = blocks tested / alive in the scout
 * and flags_out[7] = blocks inside the spans the second launch processed ([7] / [4] = the fraction of the level it had to stream:
 * the plan pays below about 0.09 -- merge.MatchPlanner's HIGH; round 5's first measurement, "below about 0.45", did not survive
 * the per-level runs of profiles/r05_n_scout_range_plan.txt).  Falls back to one launch when there are no seeds, the rows are
 * shorter than 256 channels or seed_N is not a multiple of 128 >= 256. */
#define VTM_MATCH_ONE_LAUNCH 0
#define VTM_MATCH_SCOUT_RANGE 1
/* mode = VTM_MATCH_SCOUT_RANGE | VTM_MATCH_SCOUT_STEPS(k): the scout tests after k 64-channel steps instead of the filter's own
 * test depth (40 % of the channels: 2 steps at C = 320, 4 at C = 640) -- with rest norms of its own, so the certificate is as
 * rigorous; k = 0 or k >= that depth: the filter's depth.  The scout's cost is its steps (1 step: -34 % at C = 320); a low-noise
 * clip's dead tiles are dead after one step already, on noisier data more tiles stay marked and the spans grow. */
#define VTM_MATCH_SCOUT_STEPS(k) (((k) & 0xff) << 8)
int vtm_match_filtered_plan(const void *x0, int64_t P0, const void *x1, int64_t P1, int dtype, int64_t B,
                            int64_t C, const int32_t *a_rows, int64_t Ns, const int32_t *b_rows, int64_t Nd,
                            int align, void *ws, size_t ws_bytes, uint64_t *best, int32_t *flags_out,
                            int64_t seed_L, int64_t seed_N, const int32_t *seed_pos1, const int32_t *seed_table,
                            int mode, vtm_stream_t stream);

/* vtm_position_order + vtm_match_filtered_ordered (round 5) -- the matcher on POSITION-ORDERED rows, result in the caller's
 * indexing.  The reference's sequence order behind the first level is [unmerged tokens by descending score | dst tokens]
 * (merge.py:98-117): a 32 x 32 score block then holds a same-position pair of two frames with probability 0.25-0.4 and a
 * quarter of the blocks survive the filter's pruning test, against 1 % when the rows lie in position order.  The matcher's
 * result -- per src row the maximal canonical score and the LOWEST dst index attaining it -- does not depend on the order in
 * which the rows are met, so:
 *   vtm_position_order sorts both row lists of a call by token position (position of pool row r: r % N for r < L, the
 *   chunk's (frame, position) rows; pos1[b, r - P0] for the rows of x1, pos1 NULL or out of range = none: such rows go behind
 *   the last position) -- a counting sort, stable (ties by original index), 3 small launches for both operands of all B
 *   samples.  Outputs: a_sorted / b_sorted = the lists in position order, a_order / b_order = the original index of every
 *   sorted entry, table (B, N; optional) = position -> first sorted dst entry holding it, -1 = none (the seed table of the
 *   call).  counters: vtm_position_order_counter_ints(B, N) int32 that must be ZERO on entry and are zero again when the call
 *   has run (allocate zeroed once, reuse); ws: vtm_position_order_ws_bytes bytes of scratch.  shared_order != 0 (aligned
 *   matching): sample 0's positions decide ONE order and every sample's lists (and table) are written in it.
 *   vtm_match_filtered_ordered = vtm_match_filtered_plan on the sorted lists (aligned calls: the lists must come from a
 *   shared_order sort -- entry i is the same original index in every sample -- and sample 0's a_order names the rows), with refine / escape reporting
 *   row and column through a_order / b_order and breaking ties by the ORIGINAL dst index: `best` is bit-identical to
 *   vtm_match_filtered(a_rows, b_rows).  With VTM_MATCH_SCOUT_RANGE the dst axis is one position-major run cut
 *   into the one-launch plan's splits (a src tile's span lies in one or two of them).  N <= VTM_POSITION_ORDER_MAX_N. */
#define VTM_POSITION_ORDER_MAX_N 16360   /* tokens per frame: N + 2 offsets in 64 KB of LDS */
size_t vtm_position_order_counter_ints(int64_t B, int64_t N);
size_t vtm_position_order_ws_bytes(int64_t B, int64_t Ns, int64_t Nd, int64_t N);
int vtm_position_order(const int32_t *a_rows, int64_t Ns, const int32_t *b_rows, int64_t Nd, int64_t B, int64_t L,
                       int64_t N, const int32_t *pos1, int64_t P0, int64_t P1, int32_t *counters, void *ws,
                       size_t ws_bytes, int32_t *a_sorted, int32_t *a_order, int32_t *b_sorted, int32_t *b_order,
                       int32_t *table, int shared_order, vtm_stream_t stream);
int vtm_match_filtered_ordered(const void *x0, int64_t P0, const void *x1, int64_t P1, int dtype, int64_t B,
                               int64_t C, const int32_t *a_sorted, int64_t Ns, const int32_t *b_sorted, int64_t Nd,
                               int align, void *ws, size_t ws_bytes, uint64_t *best, int32_t *flags_out, int64_t seed_L,
                               int64_t seed_N, const int32_t *seed_pos1, const int32_t *seed_table, int mode,
                               const int32_t *a_order, const int32_t *b_order, vtm_stream_t stream);

/* node_max (fp32, -0 canonicalised to +0) and node_idx (int32) out of packed keys; either output may
 * be NULL. */
int vtm_decode_best(const uint64_t *best, int64_t n, float *node_max, int32_t *node_idx,
                    vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_sort_desc -- replaces `node_max.argsort(dim=-1, descending=True)` (merge.py:98,113 / 402,417)
 * with the canonical stable order (descending value, NaN first, ties by ascending index).
 * best (rows, n) packed keys from vtm_match -> perm (rows, n) int32.
 * ws: workspace of at least vtm_sort_ws_bytes(rows, n) bytes.
 * ---------------------------------------------------------------------------------------------- */
size_t vtm_sort_ws_bytes(int64_t rows, int64_t n);
int vtm_sort_desc(const uint64_t *best, int64_t rows, int64_t n, int32_t *perm, void *ws,
                  size_t ws_bytes, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Index planning (all tiny, int32, device-resident; no host round trips).
 *
 * vtm_partition_local -- the src/dst partition of bipartite_soft_matching_randframe
 * (merge.py:41-74): tnum = (N_in - unm_pre) / F is passed in; ts = min(target_stride, F);
 * randf is the value of the reference's `torch.randint(0, ts, [1], generator=...)` draw (the host
 * draws it from the same CPU generator).  cur (B, N_in) holds the pool row id of every token of the
 * current sequence (NULL = identity, i.e. the first level).  Outputs: a_pos (Ns) / b_pos (Nd) =
 * a_idx / b_idx of the reference, a_rows (B, Ns) / b_rows (B, Nd) = cur gathered at those positions.
 * Ns / Nd must be the counts vtm_partition_counts returns.
 * ---------------------------------------------------------------------------------------------- */
int vtm_partition_counts(int64_t N_in, int64_t unm_pre, int64_t tnum, int64_t ts, int64_t randf,
                         int64_t *Ns, int64_t *Nd); /* host-only helper */
int vtm_partition_local(const int32_t *cur, int64_t B, int64_t N_in, int64_t unm_pre, int64_t tnum,
                        int64_t ts, int64_t randf, int32_t *a_pos, int32_t *b_pos, int32_t *a_rows,
                        int32_t *b_rows, int64_t Ns, int64_t Nd, vtm_stream_t stream);

/* vtm_partition_global -- bipartite_soft_matching_2s's split (merge.py:374-375) for the sequence
 * `cat([local, global])` (local_is_src != 0, patch.py:63-66) or `cat([global, local])`
 * (patch.py:68-71).  cur_local (B, Ml) pool ids of the local merged tokens; the anchors are pool
 * rows [anchor_base, anchor_base + Mg).  Outputs a_pos/b_pos/a_rows/b_rows as above with
 * Ns = src_len, Nd = Ml + Mg - src_len.
 * seed_table (optional, (B, tokens) int32, tokens = tokens per frame): filled with, for every token position, the index of
 * ONE dst row holding that position (-1: none) -- what vtm_match_filtered_seeded takes; local tokens have position
 * pool id % tokens, anchor j has anchor_pos[b, j] ((B, Mg), optional: without it anchors have no position). */
int vtm_partition_global(const int32_t *cur_local, int64_t B, int64_t Ml, int64_t anchor_base,
                         int64_t Mg, int local_is_src, int32_t *a_pos, int32_t *b_pos,
                         int32_t *a_rows, int32_t *b_rows, int32_t *seed_table, int64_t tokens,
                         const int32_t *anchor_pos, vtm_stream_t stream);

/* vtm_partition_2d -- the per-frame src/dst partition of bipartite_soft_matching_random2d (merge.py:493-528) for one frame
 * of h x w tokens (token (y, x) = y * w + x) and strides sx <= w, sy <= h: of every sy x sx cell (i, j) of the
 * hsy x wsx = (h / sy) x (w / sx) grid, token (i * sy + d / sx, j * sx + d % sx) is dst, d = draws[i * wsx + j] = the
 * reference's `torch.randint(sy * sx, (hsy, wsx, 1))` draw of that cell (the host makes it on the reference's generator and
 * copies it over); draws == NULL = `no_rand` (every d is 0: the cell's top left token).  A draw outside [0, sx * sy) is taken
 * modulo sx * sy (as an unsigned number), so that every cell has exactly one dst token whatever the array holds.  Every other token is src, the rows >= hsy * sy and columns >= wsx * sx of a frame the strides do not
 * divide included.  Outputs: b_idx (hsy * wsx) = the dst tokens, a_idx (h * w - hsy * wsx) = the src tokens (may be NULL
 * when there are none: sx == sy == 1), both in ASCENDING TOKEN ORDER.  The reference gets the two lists from an argsort of a
 * buffer that holds -1 at dst and 0 at src tokens; torch's argsort is not stable by contract, so the order among equal keys
 * is implementation-defined there -- as everywhere in this library the canonical order is the stable one (ties by ascending
 * index).  One launch; h * w < 2^31. */
int vtm_partition_2d(int64_t h, int64_t w, int64_t sx, int64_t sy, const int32_t *draws, int32_t *b_idx, int32_t *a_idx,
                     vtm_stream_t stream);

/* vtm_anchor_pos -- token positions of a new anchor set (the host tracks them next to module.global_tokens so that the
 * next global level can be seeded): anchors_out[b, p] = pool[b, amap[b, p]] (patch.py:80; amap == NULL: the first M pool
 * rows, patch.py:82), pool = [joined chunk: L rows, position = row % tokens | old anchors: old_pos (B, Mg) or NULL].
 * out (B, M) int32, -1 where the position is unknown. */
int vtm_anchor_pos(const int32_t *amap, int64_t B, int64_t M, int64_t L, int64_t tokens, const int32_t *old_pos,
                   int64_t Mg, int32_t *out, vtm_stream_t stream);

/* vtm_anchor_maps -- the maps behind a global level in one launch (they are vtm_compose x 2 + vtm_anchor_pos):
 * loc (B, Ml) = merged position of every local token = inv_g[off + t] (merge.py:459: the local slice of the level's unmerge
 * map inv_g (B, N_in)); amap (B, Ml) = new_cur[loc] = the pool row each token of u(merged) is a copy of (patch.py:80 as one
 * gather from [chunk of L rows | old anchors]); pos (B, Ml), optional = the token position of that row (row % tokens for
 * chunk rows, old_pos (B, Mg) for anchor rows, -1 unknown). */
int vtm_anchor_maps(const int32_t *inv_g, int64_t N_in, int64_t off, const int32_t *new_cur, int64_t M, int64_t B,
                    int64_t Ml, int64_t L, int64_t tokens, const int32_t *old_pos, int64_t Mg, int32_t *loc, int32_t *amap,
                    int32_t *pos, vtm_stream_t stream);

/* vtm_plan_apply -- the index split after the sort (merge.py:100-117 / 404-421) and the bookkeeping
 * of the merge / unmerge closures (merge.py:119-155 / 423-460) as composed maps:
 *   unm_idx = perm[r:], src_idx = perm[:r], dst_idx = node_idx[src_idx] (% Nd when align);
 *   new_cur (B, U + Nd), U = Ns - r: pool ids of `cat([unm, dst])`  (the merge closure);
 *   inv (B, N_in): position in the merged sequence each input position is restored from
 *                  (the unmerge closure: dst -> itself, unm -> itself, src -> its dst).
 * best/perm have one row when align != 0.  unm_idx/src_idx/dst_idx (B, U)/(B, r)/(B, r) are optional
 * (NULL to skip) copies of the reference's index tensors. */
int vtm_plan_apply(const uint64_t *best, const int32_t *perm, const int32_t *a_pos,
                   const int32_t *b_pos, const int32_t *a_rows, const int32_t *b_rows, int64_t B,
                   int64_t N_in, int64_t Ns, int64_t Nd, int64_t r, int align, int32_t *new_cur,
                   int32_t *inv, int32_t *unm_idx, int32_t *src_idx, int32_t *dst_idx,
                   vtm_stream_t stream);

/* vtm_compose -- func_warper composition of unmerge closures (vidtome/utils.py:42-48, patch.py:85):
 * out[b, i] = inv_level[b, offset + inv_acc[b, i]] for i < n (inv_acc NULL = identity).  `offset`
 * selects the part bipartite_soft_matching_2s's unmerge returns (merge.py:459). */
int vtm_compose(const int32_t *inv_acc, const int32_t *inv_level, int64_t B, int64_t n,
                int64_t level_len, int64_t offset, int32_t *out, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_gather_rows -- the composed `merge` closure in replace mode (merge.py:119-133 / 423-437,
 * patch.py:52,76) and the global-token update `u(merged_tokens)` (patch.py:80):
 * out[b, p, :] = pool[b, map[b, p], :], pool = (x0 | x1) as in vtm_normalize_gather.  out is
 * (B, out_rows, C) with out_rows >= M (rows >= M are not written: callers pad merged sequences to a
 * multiple of 8 rows so the projection GEMMs keep 16-byte aligned leading dimensions).
 * ---------------------------------------------------------------------------------------------- */
int vtm_gather_rows(const void *x0, int64_t P0, const void *x1, int64_t P1, int dtype, int64_t B,
                    int64_t C, const int32_t *map, int64_t M, void *out, int64_t out_rows,
                    vtm_stream_t stream);

/* vtm_merge_reduce -- the `merge` closure's OTHER modes (merge.py:127-131 / 431-435; never reached from
 * compute_merge, part of the closure protocol):
 *     dst = dst.scatter_reduce(-2, dst_idx.expand(n, r, c), gather(src, src_idx), reduce=mode, include_self=True)
 * with torch's CPU arithmetic -- the sources of a destination row are folded into it one by one in index order, in fp32;
 * a 16-bit tensor is rounded once at the end; "mean" divides the rounded sum by (1 + number of sources) ROUNDED TO THE
 * TENSOR'S DTYPE (torch holds the count in that dtype: exact up to 2048 in fp16 and 256 in bf16, beyond that the nearest
 * representable count, so 2049 members of an fp16 row divide by 2048) and rounds again; amax / amin propagate NaN and keep
 * the accumulator on a tie (of +0 and -0 the one that came first stays).  x is (B, N, C); src_rows (B, r) / dst_rows (B, Nd) are the rows of x of the merged src tokens
 * (in src_idx order) and of the dst tokens; seg_dst (B, r) lists the destinations of the r pairs in ASCENDING order and
 * seg_order (B, r) the pair each entry is (a STABLE sort by destination, e.g. vtm_sort_desc on keys whose high word is
 * 0xffffffff - dst_idx).  Writes out[b, out_row0 + j, :] for j < Nd; out is (B, out_ld, C) -- the merged sequence
 * [unm | dst] with out_row0 = number of unmerged tokens. */
enum { VTM_REDUCE_SUM = 0, VTM_REDUCE_PROD = 1, VTM_REDUCE_MEAN = 2, VTM_REDUCE_AMAX = 3, VTM_REDUCE_AMIN = 4 };
int vtm_merge_reduce(const void *x, int dtype, int64_t B, int64_t N, int64_t C, const int32_t *src_rows,
                     const int32_t *dst_rows, const int32_t *seg_dst, const int32_t *seg_order, int64_t r, int64_t Nd,
                     int mode, void *out, int64_t out_ld, int64_t out_row0, vtm_stream_t stream);

/* vtm_unmerge_add -- the composed `unmerge` closure + split_frame + residual
 * (merge.py:135-155 / 439-460, vidtome/utils.py:37-40, patch.py:168-169):
 * out[b, i, :] = y[b, inv[b, i], :] (+ resid[b, i, :] when resid != NULL).  y is (B, M, C). */
int vtm_unmerge_add(const void *y, int64_t M, const int32_t *inv, const void *resid, int dtype,
                    int64_t B, int64_t L, int64_t C, void *out, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_attention -- the self-attention core inside `self.attn1(...)` (patch.py:157-162) as stated by
 * the reference's own `sa_forward` (utils/pnp_utils.py:47-95): per head
 *     out = softmax(q k^T * scale) v,      no mask, no dropout.
 * q, k, out: (B, Mp, h*d) buffers of which the first M rows per sample are the sequence (Mp >= M is
 * the per-sample row count of the buffers), with row strides ldq/ldk/ldo elements (heads interleaved on the channel
 * axis = head_to_batch_dim / batch_to_head_dim without the copies); vt: (B, h*d, ldvt) = v
 * TRANSPOSED (channel-major, key-contiguous, ldvt >= M and a multiple of 8) so that the PV operand
 * is read without a transpose.  dtype VTM_F16 or VTM_BF16 (16-bit MFMA, fp32 accumulation) or VTM_F32 (fp32 operands,
 * products and accumulation on the f32 MFMA, csrc/attention_f32.hip: about 16x the matrix time); d in
 * {8,16,32,40,64,80,96,128,160}.  The same dtypes for vtm_attention_kv, _bounded and _shared_bounded; the fp32 path
 * takes its split plans only when the workspace holds them: size it with the *_ws_bytes_dtype functions.
 * share_groups > 1 = the PnP injection branch (pnp_utils.py:57-67,86-90): probabilities of sample
 * b come from q/k of sample b % (B / share_groups), v stays per sample.
 * ---------------------------------------------------------------------------------------------- */
int vtm_attention(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt,
                  int64_t ldvt, void *out, int64_t ldo, int dtype, int64_t B, int64_t h, int64_t M,
                  int64_t Mp, int64_t d, float scale, int share_groups, void *ws, size_t ws_bytes,
                  vtm_stream_t stream);

/* Optional workspace of vtm_attention / vtm_attention_kv (0 = none needed).  All workgroups of an attention launch
 * take the same time; when the last round of workgroups would leave most of the chip idle, those query blocks are
 * split along the key axis into short workgroups (same launch, behind the whole ones) whose partial results (fp32
 * accumulators, running max, denominator) live in this workspace and are merged by a second kernel.  ws may be NULL
 * (no splitting, slower for such shapes). */
size_t vtm_attention_ws_bytes(int64_t B, int64_t h, int64_t Mq, int64_t Mk, int64_t d);
/* The same for a call of element type `dtype`.  VTM_F16 / VTM_BF16: exactly vtm_attention_ws_bytes.  VTM_F32: the size the
 * fp32 kernel's own plans take (other query rows per workgroup, other resident workgroups per CU, another partial record:
 * neither size bounds the other, and an fp32 launch handed the 16-bit size may silently run without its split tail). */
size_t vtm_attention_ws_bytes_dtype(int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mk, int64_t d);

/* The same kernel with separate query / key lengths: the block's cross-attention `self.attn2(...)`
 * (vidtome/patch.py:178-183; SD: Mk = 77 text tokens per frame).  q (B, Mqp, .) / out as above; k (B, Mkp, .),
 * vt (B, h*d, ldvt >= Mk).  vtm_attention is this entry with Mk = Mq, Mkp = Mqp. */
int vtm_attention_kv(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt, int64_t ldvt,
                     void *out, int64_t ldo, int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mqp,
                     int64_t Mk, int64_t Mkp, int64_t d, float scale, int share_groups, void *ws, size_t ws_bytes,
                     vtm_stream_t stream);

/* Row counts of every attention entry: rows are addressed as (b * Mp + i) * ld, so only the LEADING DIMENSIONS must keep the
 * 16-byte alignment (ldq, ldk, ldvt multiples of 8, ldo of 4); Mp / Mqp / Mkp may be any count >= M / Mq / Mk, the sequence
 * length itself included (dense (B, M, .) buffers: a frame of 405 or 1590 tokens needs no padded copy; vtm_attention_kv_bias
 * alone asks Mkp % 8 == 0).  Key rows >= Mk are never read; of vt only ldvt >= Mk rounded up to 8 is asked and the columns
 * >= Mk may hold anything (they are masked before the PV product). */

/* vtm_attention_kv_sets -- cross-attention over SEVERAL key sets, one softmax per set: what an image-prompt adapter
 * (IP-Adapter's "decoupled cross-attention") turns the `self.attn2(...)` call of vidtome/patch.py:178-183 into.  Per head
 *     out[b, i] = sum_{s < n_sets} w_s * softmax_{j in set s}(q[b, i] . k[b, j] * scale) v[b, j]
 * q, out, k, vt exactly as for vtm_attention_kv (heads interleaved on the channel axis, vt channel-major).  All sets live in
 * ONE k buffer (B, Mkp, .) and ONE vt buffer (B, h*d, ldvt); set s is the key range [set_start[s], set_start[s] + set_len[s])
 * inside [0, Mkp) and [0, ldvt).  set_start[s] must be a multiple of 8 (V^T is fetched in 16-byte pieces of 8 keys),
 * set_len[s] >= 1; keys outside every set (padding between sets) are never read as keys.  n_sets (1 .. 8), set_start,
 * set_len and set_weight are HOST values (arrays of n_sets entries, read before the call returns); the weights may be
 * negative or above 1.  Every set keeps a running max, a denominator and fp32 accumulators of its own; the weighted sum
 * is formed in fp32 and rounded to the output type once.  scale > 0.  dtype VTM_F16 or VTM_BF16 (VTM_F32: VTM_EINVAL); d as
 * for vtm_attention.  One launch, no workspace: the key axis is a few hundred keys, the launch streams q and out. */
int vtm_attention_kv_sets(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt, int64_t ldvt,
                          void *out, int64_t ldo, int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mqp,
                          int64_t Mkp, int64_t d, float scale, int n_sets, const int64_t *set_start,
                          const int64_t *set_len, const float *set_weight, vtm_stream_t stream);

/* vtm_attention_kv_sets_masked -- the same sum with a weight PER QUERY on chosen sets: what Diffusers' IP-Adapter region
 * masks (`cross_attention_kwargs={"ip_adapter_masks": [...]}`, one image prompt per region of the frame) turn the
 * `self.attn2(...)` call of vidtome/patch.py:178-183 into.  Per head
 *     out[b, i] = sum_{s < n_sets} w_s * m_s[b, i] * softmax_{j in set s}(q[b, i] . k[b, j] * scale) v[b, j]
 *     m_s[b, i] = set_mask[s] < 0 ? 1 : mask[b * mask_batch_stride + set_mask[s] * ld_mask + i]
 * All arguments of vtm_attention_kv_sets, then: set_mask, n_sets HOST ints, each -1 (the set is not masked) or a row of the
 * table, 0 <= row < n_sets (a table has at most one row per set; sets may share a row); mask, a DEVICE pointer to fp32
 * weights, rows of ld_mask >= Mq elements (may be NULL when no set is masked); mask_batch_stride, in elements: 0 when one
 * table serves every sample (what Diffusers gives), else at least (largest row + 1) * ld_mask.  The weights are shared by the
 * heads and may be fractional, negative or above 1 (a bicubic downsample overshoots).  Set s is folded into the fp32 sum with
 * the factor (w_s * m_s) / l_s: a weight of 1 gives the bits of the unmasked call, and with every set_mask[s] == -1 the call
 * IS vtm_attention_kv_sets (the same kernel).  The masked term is weighted in fp32 and the sum rounded once, where the
 * processor rounds every term, multiplies and adds in the model's dtype.  Rows >= Mq of out are not written. */
int vtm_attention_kv_sets_masked(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt, int64_t ldvt,
                                 void *out, int64_t ldo, int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mqp,
                                 int64_t Mkp, int64_t d, float scale, int n_sets, const int64_t *set_start,
                                 const int64_t *set_len, const float *set_weight, const int *set_mask, const float *mask,
                                 int64_t ld_mask, int64_t mask_batch_stride, vtm_stream_t stream);

/* vtm_attention_kv_sets_src -- the same sum with a second QUERY operand: chosen sets take their probabilities from the
 * queries of ANOTHER sample.  What Prompt-to-Prompt's cross-attention control (word swap, refinement, re-weighting) turns
 * the `self.attn2(...)` call of vidtome/patch.py:178-183 into once the edit is folded into the value operand
 * (vtm_cross_edit_values): one softmax of the edited sample is the source sample's.  Per head
 *     out[b, i] = sum_{s < n_sets} w_s * softmax_{j in set s}(Q_s[b, i] . k[b, j] * scale) v[b, j]
 *     Q_s = set_src[s] ? q_src : q
 * All arguments of vtm_attention_kv_sets (same layouts, alignment rules, n_sets <= 8, scale > 0, VTM_F16 / VTM_BF16 only,
 * every head dim of vtm_attention), then: q_src, a DEVICE pointer to (B, Mqp_src >= Mq, .) query rows of the same dtype
 * and head layout, row (b * Mqp_src + i) * ldq_src, 16-byte aligned, ldq_src a multiple of 8 (it may be another sample
 * range of the buffer q points into); set_src, n_sets HOST ints, each 0 (the set reads q) or 1 (it reads q_src).  k, vt and
 * out are indexed by b alone: the keys a q_src set meets are sample b's.  With every set_src[s] == 0 the call IS
 * vtm_attention_kv_sets (the same kernel; q_src is not looked at), and with q_src == q it gives that call's bits.  One
 * launch, no workspace.  Rows >= Mq of out are not written.  On a bad argument nothing is launched and out is untouched. */
int vtm_attention_kv_sets_src(const void *q, int64_t ldq, const void *q_src, int64_t ldq_src, int64_t Mqp_src,
                              const void *k, int64_t ldk, const void *vt, int64_t ldvt, void *out, int64_t ldo, int dtype,
                              int64_t B, int64_t h, int64_t Mq, int64_t Mqp, int64_t Mkp, int64_t d, float scale,
                              int n_sets, const int64_t *set_start, const int64_t *set_len, const float *set_weight,
                              const int *set_src, vtm_stream_t stream);

/* vtm_cross_edit_values -- the value operand of a Prompt-to-Prompt edited cross-attention call.  The edit replaces the
 * probabilities of query i by  P_edit[i, n] = a[n] * sum_w P_src[i, w] M[w, n] + b[n] * P_own[i, n]  (M = mapper, a = src_w,
 * b = own_w: word swap, refinement, re-weighting and the cross_replace_alpha blend are all of this form); it is linear in
 * the probabilities, so  P_edit V = P_src (M diag(a) V) + P_own (diag(b) V)  and this entry writes the two operands:
 *     vt_out[b, c, start_src + w] = round_dtype( sum_{n < K} (M[w, n] * a[n]) * V[b, n, c] )
 *     vt_out[b, c, start_own + n] = round_dtype( b[n] * V[b, n, c] )
 * with V[b, n, c] = vt[b, c, v_start + n].  vt (B, C, ldvt) and vt_out (B, C, ldvt_out) are channel-major like every V^T of
 * this library; mapper (K, K) row-major, src_w (K) and own_w (K) are DEVICE pointers to fp32.  The sum is an fp32 fmaf
 * chain over n ascending from +0 whose multiplier M[w, n] * a[n] is rounded to fp32 first; the own range is one fp32
 * product; each is rounded to the dtype once.  start_src and start_own are multiples of 8 (a key set of
 * vtm_attention_kv_sets_src starts on one); the ranges [start_src, start_src + K) and [start_own, start_own + K) must not
 * overlap and must lie inside ldvt_out; columns outside them are not written.  vt_out may not overlap vt.  1 <= K <= 256
 * (the limit of vtm_attention_probs), dtype VTM_F16 or VTM_BF16.  One launch, deterministic (no atomics), no workspace.
 * On a bad argument nothing is launched and vt_out is untouched. */
int vtm_cross_edit_values(const void *vt, int64_t ldvt, int64_t v_start, int dtype, int64_t B, int64_t C, int64_t K,
                          const float *mapper, const float *src_w, const float *own_w, void *vt_out, int64_t ldvt_out,
                          int64_t start_src, int64_t start_own, vtm_stream_t stream);

/* vtm_attention_kv_bias -- the cross-attention core with one additive fp32 term PER KEY on the scores: what an
 * `encoder_attention_mask` turns the `self.attn2(...)` call of vidtome/patch.py:178-183 into (Diffusers' UNet hands the
 * (B, K) mask of a padded prompt on as an additive (B, 1, K) row of 0 / -10000).  Per head
 *     out[b, i] = softmax_j(q[b, i] . k[b, j] * scale + bias[b * bias_batch_stride + j]) v[b, j],   j < Mk
 * q, k, vt, out exactly as for vtm_attention_kv (heads interleaved on the channel axis, vt channel-major, ldvt >= Mk), and
 * Mkp % 8 == 0.  bias: a DEVICE pointer to fp32, one value per key, shared by all heads and all queries of a sample; rows of
 * ld_bias >= Mk elements; bias_batch_stride, in elements: 0 when one row serves every sample, else at least ld_bias.  A bias
 * value is finite or -inf; a key whose bias is -inf gets probability exactly 0, whatever (finite) values its k and v rows
 * hold.  A sample whose keys are ALL -inf gives NaN, as torch's scaled_dot_product_attention does.  The bias is added to the
 * scaled scores in fp32 before the running maximum is taken.  scale > 0.  dtype VTM_F16 or VTM_BF16 (VTM_F32: VTM_EINVAL);
 * d as for vtm_attention.  One launch, no workspace, no key split: the key axis is a few hundred keys, the launch streams q
 * and out.  Rows >= Mq of out are not written.  On a bad argument nothing is launched and out is untouched. */
int vtm_attention_kv_bias(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt, int64_t ldvt,
                          void *out, int64_t ldo, int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mqp,
                          int64_t Mk, int64_t Mkp, int64_t d, float scale, const float *bias, int64_t ld_bias,
                          int64_t bias_batch_stride, vtm_stream_t stream);

/* vtm_frame_order -- the kept rows of a "replace"-mode merge closure in FRAME order: what lets the `self.attn2(...)` call of
 * vidtome/patch.py:171-185 run on the merged tokens (tomesd's merge_crossattn, which the reference dropped; patch.py's
 * `merge_crossattn` opt-in here) although its conditioning is given per frame row.  The local levels leave their rows in
 * matching order (unmerged src rows by score, then dst rows: merge.py:98-117); joined row r of a chunk of F frames of N
 * tokens belongs to frame r / N, so in ascending order the rows of one frame are one contiguous segment.
 *   keep        (B, Ml) int32, DEVICE: the joined row of every token of the merged sequence.  The entries of a sample are
 *               DISTINCT and lie in [0, L = F N); any order.
 *   inv_local   (B, L) int32, DEVICE: the merged token every joined row is restored from, entries in [0, Ml); repeats are
 *               the rule.
 *   keep_sorted (B, Ml): keep[b, :] in ascending order.
 *   inv_sorted  (B, L): the position in keep_sorted[b, :] of keep[b, inv_local[b, i]] -- the unmerge map of the sorted
 *               sequence.
 *   seg_off     (B F + 1) int32: ABSOLUTE row offsets into the (B Ml)-row sequence; segment s = b F + f is the rows of sample
 *               b whose kept token lies in frame f.  seg_off[0] = 0, seg_off[B F] = B Ml, never decreasing; a frame that
 *               keeps no row has an empty segment.  This is vtm_attention_kv_segments' seg_off.
 * All integer and deterministic: a rank over a presence table, no atomics.  ws: vtm_frame_order_ws_bytes(B, F, N) bytes of
 * scratch (VTM_EWORKSPACE when smaller).  Two small launches; nothing is read back.  Every index is
 * range-checked on the device before it addresses anything: entries that break the contract (out of range, repeats in keep)
 * give wrong maps whose entries still lie in [0, Ml) / [0, L), never an access outside the buffers.  1 <= Ml <= L,
 * B F N < 2^31.  On a bad argument -- a NULL pointer, a size <= 0, Ml outside [1, L] -- VTM_EINVAL is returned and nothing is
 * launched. */
size_t vtm_frame_order_ws_bytes(int64_t B, int64_t F, int64_t N);
int vtm_frame_order(const int32_t *keep, int64_t Ml, const int32_t *inv_local, int64_t B, int64_t F, int64_t N, void *ws,
                    size_t ws_bytes, int32_t *keep_sorted, int32_t *inv_sorted, int32_t *seg_off, vtm_stream_t stream);

/* vtm_attention_kv_segments -- the cross-attention core over QUERY SEGMENTS of one row range: the `self.attn2(...)` call of
 * vidtome/patch.py:171-185 on merged tokens in frame order (vtm_frame_order), every row attending to the conditioning of
 * the frame its kept token lives in.  Per head
 *     out[i] = softmax_j(q[i] . k[s, j] * scale) v[s, j],   j < Mk,   for seg_off[s] <= i < seg_off[s + 1],   s < n_seg
 * q and out are ONE row range (rows_total, h d): row i at i * ldq / i * ldo, heads interleaved on the channel axis, 16-byte
 * aligned (ldq % 8 == 0, ldo % 4 == 0, both >= h d).  Key sample s has k (n_seg, Mkp, .) and vt (n_seg, h d, ldvt >= Mk)
 * exactly as vtm_attention_kv_bias takes them (Mkp % 8 == 0, vt channel-major).
 *   seg_off       a DEVICE pointer to n_seg + 1 int32 absolute row offsets, never decreasing, inside [0, rows_total].  Empty
 *                 segments are legal.  Rows in front of seg_off[0] and rows >= seg_off[n_seg] are not written.
 *   max_seg_rows  a HOST upper bound on every segment's length (for a chunk's frames: N); it sizes the grid, one query block
 *                 per 256 (d <= 96) or 128 rows of the bound for every (segment, head), and a workgroup whose block starts
 *                 behind its segment's device-side length leaves at once.  A bound far above the lengths costs idle
 *                 workgroups, never a wrong result.
 *   A segment LONGER than max_seg_rows breaks the contract: its first max_seg_rows rows are computed, the rest are not
 *   written.  Offsets outside [0, rows_total] are clamped to it and a decreasing pair is an empty segment: whatever seg_off
 *   holds, nothing outside the rows_total rows of q / out is addressed.
 * scale > 0.  dtype VTM_F16 or VTM_BF16 (VTM_F32: VTM_EINVAL); d as for vtm_attention; rows_total < 2^31.  P is rounded to
 * the operand type once for the PV product (bf16: as a hi + lo pair) and the denominator is summed from the same rounded P,
 * as in vtm_attention_kv_bias.  One launch, no workspace, no key split: the key axis is a few hundred keys, the launch
 * streams q and out.  On a bad argument nothing is launched and out is untouched. */
int vtm_attention_kv_segments(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt, int64_t ldvt,
                              void *out, int64_t ldo, int dtype, int64_t rows_total, const int32_t *seg_off, int64_t n_seg,
                              int64_t max_seg_rows, int64_t h, int64_t Mk, int64_t Mkp, int64_t d, float scale,
                              vtm_stream_t stream);

/* vtm_attention_probs --the head-averaged PROBABILITIES of the `self.attn2(...)` call of vidtome/patch.py:178-183, the
 * "cross-attention map" that zero-shot video editing reads (LocalBlend-style masks, per-word maps), in fp32:
 *     out[b, i, j] = (1 / h) * sum_head softmax_j(q[b, i, head] . k[b, j, head] * scale + bias[b * bias_batch_stride + j])
 * for i < Mq, j < Mk.  q, ldq, k, ldk, dtype, B, h, Mq, Mqp, Mk, Mkp, d, scale exactly as for vtm_attention_kv_bias (heads
 * interleaved on the channel axis, rows addressed as (b * Mp + i) * ld, ld a multiple of 8, key rows >= Mk never read; Mkp
 * may be any count >= Mk); q and k 16-byte aligned.  There is no V operand.  bias: a DEVICE pointer to fp32 as for
 * vtm_attention_kv_bias (ld_bias >= Mk, bias_batch_stride 0 or >= ld_bias), or NULL for none (ld_bias and
 * bias_batch_stride are then not read; the bits are those of a zero bias).  A bias of -inf gives probability exactly 0; a
 * sample whose keys are ALL -inf gives NaN for that sample only.  out: fp32, rows of ldo >= Mk elements, sample b at
 * b * Mq * ldo; rows >= Mq and columns >= Mk are not written.  Limits: dtype VTM_F16 or VTM_BF16, d as for vtm_attention,
 * 1 <= Mk <= 256 (77-token prompts and 154- / 231-token weighted prompts), h <= 40 (the per-head softmax statistics of a
 * workgroup's 128 query rows live in LDS), scale > 0.  Deterministic: one launch, no atomics, no workspace and no
 * (B, h, Mq, Mk) intermediate; the heads are summed in ascending order in fp32 and multiplied by 1 / h once.  On a bad
 * argument nothing is launched and out is untouched. */
int vtm_attention_probs(const void *q, int64_t ldq, const void *k, int64_t ldk, float *out, int64_t ldo, int dtype,
                        int64_t B, int64_t h, int64_t Mq, int64_t Mqp, int64_t Mk, int64_t Mkp, int64_t d, float scale,
                        const float *bias, int64_t ld_bias, int64_t bias_batch_stride, vtm_stream_t stream);

/* vtm_attention_word_map -- ONE weighted column sum of that head-averaged map, added in place: the `self.attn2(...)` call
 * of vidtome/patch.py:178-183 as a Prompt-to-Prompt LocalBlend reads it (the map of a few chosen words, accumulated over
 * blocks and denoising steps), without the (B, Mq, Mk) map:
 *     value[b, i] = (1 / h) * sum_head [ sum_j w[b, j] p_head[i, j] ] / [ sum_j p_head[i, j] ]
 *     p_head[i, j] = exp(q[b, i, head] . k[b, j, head] * scale + bias[b * bias_batch_stride + j] - running max),   j < Mk
 *     out[r(b) * ldo + i] = (accumulate ? out[r(b) * ldo + i] : 0) + value[b, i],   i < Mq,   r(b) = out_rows ? out_rows[b] : b
 * q, ldq, k, ldk, dtype, B, h, Mq, Mqp, Mk, Mkp, d, scale, bias, ld_bias, bias_batch_stride exactly as for
 * vtm_attention_probs (layouts, alignment, VTM_F16 / VTM_BF16 only, every head dim of vtm_attention, 1 <= Mk <= 256, a bias
 * of -inf gives probability exactly 0), but there is NO head-count limit beyond h > 0: nothing per head is kept.  weights: a
 * DEVICE pointer to fp32, w[b, j] = weights[b * w_batch_stride + j]; rows of ld_w >= Mk elements; w_batch_stride, in
 * elements: 0 when one row serves every sample, else at least ld_w.  The weights are finite (not checked).  out: fp32, row
 * r at r * ldo, ldo >= Mq; columns >= Mq and rows no r(b) names are not written.  out_rows: a DEVICE pointer to B int64 row
 * numbers, or NULL; the rows of one call are distinct (the caller's contract: every element then has one writer).
 * accumulate: 0 overwrites, anything else adds to what out holds (one fp32 addition).  One online-softmax sweep, heads
 * outer and key tiles inner: the running maximum carries the weighted numerator and the denominator, rescaled together; at
 * a head's last tile numerator * (1 / denominator) is added to an fp32 accumulator, heads in ascending order, which is
 * multiplied by 1 / h once.  A sample whose keys are ALL -inf gives NaN for that sample only.  Deterministic: one launch,
 * no atomics, no workspace; the same operands and the same prior out give the same bits.  On a bad argument nothing is
 * launched and out is untouched. */
int vtm_attention_word_map(const void *q, int64_t ldq, const void *k, int64_t ldk, int dtype, int64_t B, int64_t h,
                           int64_t Mq, int64_t Mqp, int64_t Mk, int64_t Mkp, int64_t d, float scale, const float *bias,
                           int64_t ld_bias, int64_t bias_batch_stride, const float *weights, int64_t ld_w,
                           int64_t w_batch_stride, float *out, int64_t ldo, const int64_t *out_rows, int accumulate,
                           vtm_stream_t stream);

/* vtm_local_blend -- the tail of Prompt-to-Prompt's LocalBlend on accumulated word maps: pool, threshold against the
 * map's maximum, keep the source latents outside the mask.  acc: DEVICE fp32 (G, F, h, w) contiguous, finite, 1 <= G <= 8
 * groups; x, x_src, out: (F, C, H, W) contiguous NCHW latents of one dtype (VTM_F32, VTM_F16 or VTM_BF16), H % h == 0 and
 * W % w == 0.  Per frame f and latent pixel (y, x)
 *     pooled_g = max of acc[g, f] over the (2 pool + 1)^2 window around (y * h / H, x * w / W), clipped at the border
 *     mask     = OR_g ( pooled_g > threshold * max(acc[g, f]) )            one fp32 multiply, then the comparison
 *     out[f, c, y, x] = mask ? x[f, c, y, x] : x_src[f, c, y, x]           a select: the latents are moved, never computed on
 * pool: the radius, 0 .. 3 (P2P's k = 1 is pool = 1: a 3 x 3 window, stride 1, -inf padding).  Two deliberate differences
 * from P2P: `pooled > threshold * max` stands for `pooled / max > threshold` (no division; a map that is all 0 gives an
 * empty mask for its group, as P2P's 0 / 0 comparison does), and the select stands for x_src + mask * (x - x_src), which
 * rounds in a 16-bit dtype.  out may BE x (no other overlap with x or x_src).  mask_out: DEVICE uint8 (F, H, W) that
 * receives the mask as 0 / 1, or NULL.  One launch, deterministic (no atomics), no workspace.  On a bad argument nothing is
 * launched and out is untouched. */
int vtm_local_blend(const float *acc, int64_t G, int64_t F, int64_t h, int64_t w, const void *x, const void *x_src,
                    void *out, int dtype, int64_t C, int64_t H, int64_t W, int pool, float threshold, uint8_t *mask_out,
                    vtm_stream_t stream);

/* vtm_attention_key_mass -- the per-key attention MASS of a self-attention call, the map self-attention guidance (SAG)
 * thresholds, in fp32:
 *     out[b * ldo + j] = sum_{i < Mq} (1 / h) * sum_head softmax_j(q[b, i, head] . k[b, j, head] * scale)[j],   j < Mk
 * the column sums of the head-averaged probabilities; their mean over j is Mq / Mk (exactly 1 for self-attention).  q, ldq,
 * k, ldk, dtype, B, h, Mq, Mqp, Mk, Mkp, d, scale exactly as for vtm_attention_probs (heads interleaved on the channel
 * axis, rows addressed as (b * Mp + i) * ld, ld a multiple of 8, q and k 16-byte aligned, VTM_F16 / VTM_BF16 only, every
 * head dim of vtm_attention, scale > 0) -- q and k may be row ranges of one (B, N, 3 C) q | k | v buffer (ld = 3 C).  There
 * is no V operand and no bias.  Query rows >= Mq are padding: they are not read and contribute exactly 0 (a select on the
 * row index); key rows >= Mk are never read.  Limits: 1 <= Mk <= 4096 (a workgroup's column accumulators live in LDS),
 * 1 <= Mq <= 65536, any h > 0: nothing per head outlives its head.  out: fp32, sample b at b * ldo, ldo >= Mk; columns
 * >= Mk are not written.  ws: a DEVICE workspace of vtm_attention_key_mass_ws_bytes(B, Mq, Mk) bytes, 0 for Mq <= 128
 * (ws may then be NULL): a grid over (128-row query tile, sample) -- per head a sweep for the row maximum and denominator and
 * a sweep that recomputes the scores and sums p / l down the tile's query rows, heads in ascending order; one tile writes
 * out directly (one launch), more leave their column sums in ws and a second launch adds the tiles in ascending order; 1 / h
 * is applied once.  Deterministic: no atomics, and the order of every addition depends on (h, Mq, Mk) alone -- a sample's
 * bits depend neither on B, nor on the other samples, nor on the run.  On a bad argument nothing is launched and out is
 * untouched. */
size_t vtm_attention_key_mass_ws_bytes(int64_t B, int64_t Mq, int64_t Mk);
int vtm_attention_key_mass(const void *q, int64_t ldq, const void *k, int64_t ldk, float *out, int64_t ldo, int dtype,
                           int64_t B, int64_t h, int64_t Mq, int64_t Mqp, int64_t Mk, int64_t Mkp, int64_t d, float scale,
                           void *ws, size_t ws_bytes, vtm_stream_t stream);

/* vtm_sag_degrade -- the degrade step of self-attention guidance (Hong et al.; Diffusers' StableDiffusionSAGPipeline) for
 * one chunk of frames, in one launch.  x: the whole-video latents, n_rows frames of (C, H, W) from the pointer given;
 * frame_ids: a DEVICE pointer to F int32 rows of x (distinct, inside [0, n_rows): the caller's contract), or NULL for rows
 * 0 .. F - 1; model_out: the chosen group's (F, C, H, W) rows of the UNet output; mass: DEVICE fp32 rows of
 * ld_mass >= h_m * w_m, frame f at f * ld_mass (vtm_attention_key_mass of the mid block's (h_m, w_m) token grid); all
 * latents contiguous NCHW of one dtype (VTM_F32, VTM_F16 or VTM_BF16).  Per frame f, channel c and pixel (y, x), in fp32:
 *     x0, eps      = the pred_type formulas of vtm_guided_step (VTM_PRED_*) on x[row(f)] and m = model_out[f]
 *     mask         = mass[f, (y * h_m / H) * w_m + x * w_m / W] > threshold          integer divisions: nearest-neighbour
 *     blur         = sum_k taps[k] * ( sum_l taps[l] * x0[reflect(y + k - r), reflect(x + l - r)] )
 *     out[f, c, y, x] = sqrt_alpha * (mask ? blur : x0) + sqrt_beta * eps            rounded once, to dtype
 * taps: a HOST pointer to the 2 r + 1 fp32 taps, 0 <= r <= 4 (r = 0: the identity blur for a tap of 1); the horizontal pass
 * runs first, each pass is fmaf(tap, value, acc) in ascending tap order from acc = 0; reflect is torch's "reflect" padding
 * (the edge is not repeated), which needs H, W > r.  Three deliberate differences from the Diffusers pipeline: the mask
 * SELECTS (it does not multiply: equal for finite values, and NaN / Inf do not leak across the mask); the nearest-neighbour
 * source index is the integer floor(y * h_m / H), not a float scale; the blur is fp32 in two separable passes and rounded
 * once at the store (Diffusers blurs in the model dtype).  One workgroup owns a (frame, channel) plane with x0 and the
 * horizontal pass in LDS: H * W <= 16384 (128 x 128 latents; two fp32 planes are 128 KiB of the CU's 160 KiB).  out:
 * chunk-local (F, C, H, W), must not overlap x (checked against the n_rows frames).  mask_out: DEVICE uint8 (F, H, W) that
 * receives the mask as 0 / 1, or NULL.  No workspace, no atomics.  On a bad argument nothing is launched and out is
 * untouched. */
int vtm_sag_degrade(const void *x, int64_t n_rows, const int32_t *frame_ids, const void *model_out, const float *mass,
                    int64_t ld_mass, int64_t h_m, int64_t w_m, int dtype, int64_t F, int64_t C, int64_t H, int64_t W,
                    int pred_type, float sqrt_alpha, float sqrt_beta, const float *taps, int r, float threshold, void *out,
                    uint8_t *mask_out, vtm_stream_t stream);

/* vtm_freeu -- FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net"; Diffusers' enable_freeu with its threshold of 1) in
 * place on x, the contiguous NCHW concatenation cat([hidden_states, res_hidden_states], 1) of B samples of C_h + C_s planes
 * of (H, W) that an up-block resnet is about to read; dtype VTM_F32, VTM_F16 or VTM_BF16.  With P = H * W, in float64 terms:
 *     backbone planes c < C_h / 2 (integer division):   out = v * g
 *         version 1 (Diffusers):                g = b
 *         version 2 (the original repository):  g[n, p] = 1 + (b - 1) (m[n, p] - min_p m[n]) / (max_p m[n] - min_p m[n]),
 *                                               m[n, p] the mean of x[n, c, p] over ALL c < C_h; g = 1 where max == min
 *                                               (the original divides 0 by 0 there: the one stated deviation)
 *     planes C_h / 2 <= c < C_h:                        not touched, their bytes are never written
 *     skip planes c >= C_h, a = 2 pi y / H, b' = 2 pi x / W:
 *         S = sum v,  A_c, A_s = sum v cos a, sum v sin a,  B_c, B_s = sum v cos b', sum v sin b',
 *         D_c, D_s = sum v cos(a + b'), sum v sin(a + b')                        (sums over the plane)
 *         out[y, x] = v[y, x] + (s - 1) / P * (S + A_c cos a + A_s sin a + B_c cos b' + B_s sin b'
 *                                                + D_c cos(a + b') + D_s sin(a + b'))
 * which is Re ifftn(ifftshift(mask * fftshift(fftn(v)))) for mask = s on [H/2 - 1 : H/2 + 1, W/2 - 1 : W/2 + 1] and 1
 * elsewhere: the four bins ky, kx in {0, -1}; it holds for every H, W >= 2, odd sizes and H = 2 included.  Limits:
 * H, W >= 2, P <= 16384, C_h >= 2, C_s >= 1, B >= 0 (B == 0: VTM_OK, nothing is launched).  All arithmetic is fp32 and
 * every stored value is rounded once; csrc/freeu.hip's header counts the roundings.  s == 1 gives the skip planes, and
 * b == 1 with version 1 the backbone planes, no work at all: bit for bit the input.  Non-finite values propagate by IEEE
 * rules through the plane that holds them (version 2: through that sample's map) and reach no other plane.  No atomics:
 * a plane's bits depend on its own values (version 2: and its sample's map) alone, not on its position, B or the run.
 * Version 1 is one launch.  Version 2 is three (the channel mean, min / max per sample, the apply launch) and needs ws, a
 * 4-byte aligned DEVICE workspace of vtm_freeu_ws_bytes(B, P, version) bytes (0 for version 1: ws may be NULL).
 * vtm_freeu_lanes(P): the lanes that own one plane of P elements, 16 / 64 / 256 / 1024 -- the kernel form, a function of
 * P alone (0 for a P outside [4, 16384]).  On a bad argument -- a NULL or misaligned x, B < 0, a size outside the limits,
 * another version or dtype, a missing or short ws, a grid beyond 2^31 - 1 workgroups -- nothing is launched and x is
 * untouched. */
int vtm_freeu_lanes(int64_t P);
size_t vtm_freeu_ws_bytes(int64_t B, int64_t P, int version);
int vtm_freeu(void *x, int dtype, int64_t B, int64_t C_h, int64_t C_s, int64_t H, int64_t W, float b, float s, int version,
              void *ws, size_t ws_bytes, vtm_stream_t stream);

/* vtm_attention_kv with a DEVICE-side query bound: sample b only has q_count[b] <= Mq meaningful query rows (the
 * compacted live queries of vtm_compact_queries); query blocks that start at or beyond the count exit at once, rows
 * beyond it are not meaningful.  The launch is sized for the host-known bound Mq -- no host round trip. */
int vtm_attention_kv_bounded(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt, int64_t ldvt,
                             void *out, int64_t ldo, int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mqp,
                             int64_t Mk, int64_t Mkp, int64_t d, float scale, const int32_t *q_count, void *ws,
                             size_t ws_bytes, vtm_stream_t stream);
/* ... and with shared probabilities (pnp_utils.py:57-67, 75-90) on top: the probabilities of sample b come from q / k of sample
 * b % (B / share_groups), v stays per sample, and every sample of a group has the SAME live rows (align_batch: one index set
 * for the batch, merge.py:73-76), so q_count[b % (B / share_groups)] bounds them all.  q_count has B entries; the first
 * B / share_groups are read.  Workspace: vtm_attention_ws_bytes. */
int vtm_attention_kv_shared_bounded(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt, int64_t ldvt,
                                    void *out, int64_t ldo, int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mqp,
                                    int64_t Mk, int64_t Mkp, int64_t d, float scale, int share_groups,
                                    const int32_t *q_count, void *ws, size_t ws_bytes, vtm_stream_t stream);
/* workspace of a vtm_attention_kv_bounded launch: with a device-side query count the launch cannot plan its rounds, so every
 * work item is split in two along the key axis (one partial record per workgroup, merged by a second kernel); with less
 * workspace than this the launch falls back to the plain plan of vtm_attention_ws_bytes */
size_t vtm_attention_kv_bounded_ws_bytes(int64_t B, int64_t h, int64_t Mq, int64_t Mk, int64_t d);
/* ... for a call of element type `dtype` (see vtm_attention_ws_bytes_dtype) */
size_t vtm_attention_kv_bounded_ws_bytes_dtype(int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mk, int64_t d);

/* vtm_transpose_cols -- V^T of a block that does not merge (patch.py:157-162 at the sites beyond max_downsample: per-frame
 * attention): the q | k | v projection GEMM leaves v as columns of its token-major output, the attention core reads V
 * channel-major.  x (BF, N, ldx) 16-bit, the C columns starting at `x` -> out (BF, C, ldo), tokens N .. ldo zero-filled.
 * C, ldx, ldo multiples of 8, ldo >= N, 16-byte aligned pointers. */
int vtm_transpose_cols(const void *x, int64_t ldx, int dtype, int64_t BF, int64_t N, int64_t C, void *out, int64_t ldo,
                       vtm_stream_t stream);

/* vtm_fold_keys / vtm_attention_kv_folded -- the anchors' exact duplicates as ONE key each.  patch.py:80 stores
 * u(merged_tokens) as the next chunk's global tokens: every local token that merged into an anchor row carries that
 * row's content, so the anchors hold groups of identical rows, and so does the merged sequence they join
 * (patch.py:63-71).  Identical key / value rows weigh in softmax(q k^T) v exactly like one key whose (base-2) score carries
 * + log2(multiplicity).  vtm_fold_keys: cur (B, M) pool row of every merged position (rows >= L are anchor rows cur - L of
 * Ma), cid (B, Ma) a content id in [0, n_ids) per anchor row (equal ids <=> identical rows; vtm_compact_queries' tmap of
 * the block that produced the anchors; an id outside [0, n_ids), e.g. -1, = "no id": the row stands for itself).  Outputs: key_sel (B, M) the surviving merged positions in ascending order (the
 * first copy of every group; entries past the count are 0), k_bias (B, ldkb) per surviving key log2(copies present) as
 * a (hi, lo) pair of the keys' 16-bit type (dtype VTM_F16 / VTM_BF16), k_count (B) the number of surviving keys.
 * vtm_attention_kv_folded is vtm_attention_kv_bounded (q_count may be NULL) over such a key list: k / vt hold the
 * projections of the key_sel rows, only the first k_count[b] (<= Mk, a device value) are keys, and the bias pair rides
 * in the spare k-slots of the contraction -- head dims with d % 16 == 8 only (SD's 40).  Same block output as the
 * unfolded call up to the rounding of log2(m) (2^-21 relative). */
size_t vtm_fold_keys_ws_bytes(int64_t B, int64_t M, int64_t n_ids);
int vtm_fold_keys(const int32_t *cur, int64_t B, int64_t M, int64_t L, const int32_t *cid, int64_t Ma, int64_t n_ids,
                  int dtype, void *ws, size_t ws_bytes, int32_t *key_sel, uint32_t *k_bias, int64_t ldkb,
                  int32_t *k_count, vtm_stream_t stream);
int vtm_attention_kv_folded(const void *q, int64_t ldq, const void *k, int64_t ldk, const void *vt, int64_t ldvt,
                            void *out, int64_t ldo, int dtype, int64_t B, int64_t h, int64_t Mq, int64_t Mqp,
                            int64_t Mk, int64_t Mkp, int64_t d, float scale, const int32_t *q_count,
                            const int32_t *k_count, const uint32_t *k_bias, int64_t ldkb, void *ws, size_t ws_bytes,
                            vtm_stream_t stream);

/* vtm_compact_queries -- which attention outputs a global level with the local chunk on the src side actually needs
 * (bipartite_soft_matching_2s's unmerge, merge.py:439-460, returns for every merged local token the output row of the
 * anchor token it merged into: `src = gather(dst, dst_idx)`; several local tokens may share one).  loc (B, Ml): merged
 * position of every local token (< U: its own row; >= U: anchor row loc - U of Nd).  Outputs: qc (B, Ml) the DISTINCT
 * positions ([0, U) then the matched anchor rows ascending; entries past the count are 0), tmap (B, Ml) the row of
 * that list each local token reads, count (B) the number of distinct positions.  ws: vtm_compact_queries_ws_bytes. */
size_t vtm_compact_queries_ws_bytes(int64_t B, int64_t Nd);
int vtm_compact_queries(const int32_t *loc, int64_t B, int64_t Ml, int64_t U, int64_t Nd, void *ws, size_t ws_bytes,
                        int32_t *qc, int32_t *tmap, int32_t *count, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Panel GEMMs -- the rest of the patched block around the hot path (vidtome/patch.py:171-199): the feed-forward
 * `self.ff(self.norm3(hidden_states)) + hidden_states` (Diffusers FeedForward of SD blocks: GEGLU(Linear C -> 8C), Linear
 * 4C -> C) and the query projection of the cross-attention `self.attn2(self.norm2(hidden_states), ...)`.
 * Operands are k-panels: [K / 8][rows_pad][8 elements], rows_pad = vtm_panel_rows(rows) (a multiple of 256); padding
 * rows may hold anything.  Token operands come from vtm_layernorm_panels (or vtm_to_panels), weights are packed once
 * with vtm_to_panels (`order` = the row permutation below, or NULL).
 *   vtm_layernorm_panels  torch.nn.LayerNorm with its result written as panels (norm3 / norm2; norm1 of the un-merged sites).
 *   vtm_gather_panels     the composed merge closure (merge.py:119-133 / 423-437) writing panels: row b * rows_per_sample + i
 *                         = pool[b, map[b, map2[b, i]]] (either map may be NULL), padding rows zero -- the token operand of
 *                         attn1's projections (patch.py:157-162) at the sites where the panel GEMM is used.
 *   vtm_ff_geglu          out = value * gelu(gate) of  x W1^T + b1  (erf gelu), written as panels [D / 8][n_pad][8] -- the
 *                         2D-wide projection is never written.  W1 is packed in TILE order: 128-row tile t = the value rows of
 *                         output channels 64 t .. 64 t + 63 followed by their gate rows (rows D + 64 t ..); bias (2 D fp32) in
 *                         the same order.  D % 64 == 0, K % 64 == 0.
 *   vtm_linear_panels     out (n, ldo) token rows = x W^T (+ bias fp32 (N)) (+ resid (n, ldo)), rounded like torch's Linear
 *                         followed by the residual add.  N % 8 == 0, K % 64 == 0.  n_pad / w_rows_pad are the ROW STRIDES of the
 *                         two panel operands (either may be a row range of a larger panel tensor, e.g. one sample's rows:
 *                         V^T = W_v X^T is this call with the weight as "token" operand and the sample's tokens as "weight").
 * ---------------------------------------------------------------------------------------------- */
int64_t vtm_panel_rows(int64_t n);
int vtm_to_panels(const void *x, int dtype, int64_t rows, int64_t C, const int32_t *order, void *out, int64_t rows_pad,
                  vtm_stream_t stream);
int vtm_layernorm_panels(const void *x, const void *gamma, const void *beta, int dtype, int64_t rows, int64_t C, float eps,
                         void *out, int64_t panel_rows, vtm_stream_t stream);
int vtm_gather_panels(const void *x0, int64_t P0, const void *x1, int64_t P1, int dtype, int64_t B, int64_t C,
                      const int32_t *map, int64_t map_ld, const int32_t *map2, int64_t n, void *out, int64_t rows_per_sample,
                      vtm_stream_t stream);
int vtm_ff_geglu(const void *x_panels, int64_t n, int64_t n_pad, const void *w1_panels, int64_t D, int64_t w_rows_pad,
                 int64_t K, const float *bias, int dtype, void *out_panels, vtm_stream_t stream);
int vtm_linear_panels(const void *x_panels, int64_t n, int64_t n_pad, const void *w_panels, int64_t N, int64_t w_rows_pad,
                      int64_t K, const float *bias, const void *resid, int dtype, void *out, int64_t ldo,
                      vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_cfg_ddim -- the caller-side elementwise tail of a denoising step:
 * classifier-free guidance `eps = uncond + guidance * (cond - uncond)` (generate.py:276-278) fused with the
 * closed-form DDIM update of `pred_next_x` (generate.py:281-311):
 *     pred_x0 = (x - b*eps) / a ;   x_out = c*pred_x0 + d*eps
 * sampling: (a, b, c, d) = (mu, sigma, mu_prev, sigma_prev); inversion: (mu_prev, sigma_prev, mu, sigma).
 * eps_cond may be NULL (no guidance: eps = eps_uncond); eps_out / x_out are optional outputs.  Every
 * operation rounds to the tensor dtype in the reference's order, so fp16/bf16 results are bit-identical to
 * the torch expression.
 * ---------------------------------------------------------------------------------------------- */
int vtm_cfg_ddim(const void *x, const void *eps_uncond, const void *eps_cond, int dtype, int64_t n,
                 float guidance, float a, float b, float c, float d, void *eps_out, void *x_out,
                 vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_guided_step -- the whole caller-side step of ONE CHUNK in one launch (generate.py:239-311, invert.py:181-211): the
 * group slice `eps.chunk(batch_size)[-2:]` (generate.py:276), classifier-free guidance (generate.py:278), Diffusers'
 * guidance rescale (`rescale_noise_cfg`), the prediction type, the DDIM update of `pred_next_x` (generate.py:281-311) with
 * the stochastic term of eta > 0, and the store of the chunk's frames into the whole-video latents (`noises[chunk] = ...`
 * followed by the whole-video update).  vtm_cfg_ddim above stays the reference's own expression (epsilon, eta = 0, rounded
 * per operation); this call computes in fp32 and rounds every stored value once.
 *   model_out  (groups * F, E) contiguous, group-major: sample g * F + f; E = C * H * W of a latent frame.
 *   g_uncond, g_cond  the two groups (under PnP groups - 2 and groups - 1); g_cond = -1: no guidance, m = model_out[g_uncond]
 *              (inversion: one group).
 *   x, x_out   whole-video latents (n_frames, E); chunk frame f is row frame_ids[f] (DEVICE int32, F entries, distinct,
 *              inside the video -- the caller's business), or row f when frame_ids is NULL.  x_out may BE x.
 *   noise, eps_out, x0_out  chunk-local (F, E), optional; noise is required exactly when sigma != 0 (and not read otherwise).
 *              At least one of x_out, eps_out, x0_out is not NULL.
 * Per frame and element, in fp32:
 *     m  = m_u + guidance * (m_c - m_u)                            (g_cond >= 0)
 *     m  = m * (rescale * std(m_c) / std(m) + 1 - rescale)         (rescale > 0)
 *     VTM_PRED_EPSILON : x0 = (x - sqrt_beta * m) / sqrt_alpha       eps = m
 *     VTM_PRED_V       : x0 = sqrt_alpha * x - sqrt_beta * m         eps = sqrt_alpha * m + sqrt_beta * x
 *     VTM_PRED_SAMPLE  : x0 = m                                      eps = (x - sqrt_alpha * x0) / sqrt_beta
 *     x_out = c_x0 * x0 + c_eps * eps + sigma * noise ;   eps_out = eps ;   x0_out = x0
 * std is torch's default (unbiased) over the frame's E fp32 values, two-pass (mean, then squared deviations); std(m) == 0
 * gives what IEEE arithmetic gives.  Sampling from a_t to a_prev: sqrt_alpha = sqrt(a_t), sqrt_beta = sqrt(1 - a_t),
 * c_x0 = sqrt(a_prev), c_eps = sqrt(1 - a_prev - sigma^2); inversion is the same call with the two levels exchanged.
 * rescale == 0: one elementwise grid-stride launch.  rescale > 0 (needs g_cond >= 0 and E >= 2): one workgroup per frame,
 * fixed reduction order -- a frame's bits depend neither on the other frames of the launch nor on the run, nor on whether
 * 16-byte accesses were possible (E a multiple of 16 bytes and every pointer 16-byte aligned) or not.  Any E >= 1,
 * F <= 2^20; F == 0 is VTM_OK.  One launch, no workspace, no atomics.  On a bad argument (VTM_EINVAL) nothing is launched.
 * ---------------------------------------------------------------------------------------------- */
#define VTM_PRED_EPSILON 0
#define VTM_PRED_V       1
#define VTM_PRED_SAMPLE  2
int vtm_guided_step(const void *x, const void *model_out, const void *noise, int dtype, int64_t F, int64_t E,
                    int64_t groups, int64_t g_uncond, int64_t g_cond, const int32_t *frame_ids, int pred_type,
                    float guidance, float rescale, float sqrt_alpha, float sqrt_beta, float c_x0, float c_eps,
                    float sigma, void *x_out, void *eps_out, void *x0_out, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_solver_step -- the caller-side step of ONE CHUNK in one launch for a MULTISTEP solver (DPM-Solver++ 2M / 3M,
 * sampler.GuidedDPMSolver) and for guidance with more than two terms: a weighted sum over up to VTM_SOLVER_MAX_GROUPS groups
 * of the UNet output (classifier-free guidance is the weights (1 - s, s); InstructPix2Pix and perturbed-attention guidance
 * are three weights), the guidance rescale, the prediction type, and a LINEAR update from the latents, the clean-sample
 * prediction and the clean-sample predictions of the two previous steps, which live per FRAME in whole-video fp32 buffers --
 * so a video can be stepped chunk by chunk, under any chunking, on any stream.  Sizes, dtypes, frame_ids, the prediction
 * types and the launch shapes are vtm_guided_step's.
 *   model_out  (groups * F, E) contiguous, group-major: sample g * F + f.
 *   w          HOST array of `groups` weights, copied into the kernel arguments.  A group of weight 0 is never read (a PnP
 *              source group full of NaN stays out).
 *   g_ref      the group whose per-frame standard deviation the rescale restores (rescale > 0: in range, w[g_ref] != 0,
 *              E >= 2); ignored when rescale == 0.
 *   x, x_out   whole-video latents (n_frames, E) in `dtype`; chunk frame f is row frame_ids[f] (DEVICE int32), or row f when
 *              frame_ids is NULL.  x_out may BE x.
 *   h1, h2, h_out  whole-video FP32 (n_frames, E), rows as x's: the clean-sample predictions of the previous step and of the
 *              one before it, and where this step's goes (16-bit history would compound one rounding per step).  Each may be
 *              NULL; h_out may BE h1 or h2 (every element is read before it is written, by the same thread).
 *   noise, eps_out, x0_out  chunk-local (F, E) in `dtype`, optional.
 * Per frame and element, in fp32, every sum started from 0 and taken in the order written:
 *     m     = sum over g = 0 .. groups - 1 with w[g] != 0 of  w[g] * model_out[g * F + f]
 *     m     = m * (rescale * std(model_out[g_ref * F + f]) / std(m) + 1 - rescale)                  (rescale > 0)
 *     x0, eps from m, x, sqrt_alpha, sqrt_beta by pred_type as in vtm_guided_step
 *     x_out = c_x * x + c_x0 * x0 + c_h1 * h1 + c_h2 * h2 + c_noise * noise
 *     h_out = x0 (fp32, not rounded) ;   eps_out = eps ;   x0_out = x0
 * A term of x_out whose coefficient is exactly 0 is absent: its operand is not read (h1, h2, noise may then be NULL; they are
 * required otherwise) and cannot put a NaN into the sum.  std is vtm_guided_step's: unbiased, two-pass, in the fixed order of
 * a 1024-thread workgroup per frame, so a frame's bits depend neither on the other frames of the launch nor on the run, nor
 * on whether 16-byte accesses were possible (E a multiple of 16 bytes of `dtype` and every pointer 16-byte aligned).
 * At least one of x_out, h_out, eps_out, x0_out is not NULL.  Any E >= 1, F <= 2^20; F == 0 is VTM_OK.  One launch, no
 * workspace, no atomics.  On a bad argument (VTM_EINVAL) nothing is launched.
 * ---------------------------------------------------------------------------------------------- */
#define VTM_SOLVER_MAX_GROUPS 8
int vtm_solver_step(const void *x, const void *model_out, const void *noise, const float *h1, const float *h2, int dtype,
                    int64_t F, int64_t E, int64_t groups, const float *w, int64_t g_ref, const int32_t *frame_ids,
                    int pred_type, float rescale, float sqrt_alpha, float sqrt_beta, float c_x, float c_x0, float c_h1,
                    float c_h2, float c_noise, void *x_out, float *h_out, void *eps_out, void *x0_out, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_invert_step -- edit-friendly DDPM inversion (Huberman-Spiegelglas et al.; LEDITS++, Diffusers'
 * LEditsPPPipelineStableDiffusion.invert; inversion.EditFriendlyInversion): the INVERSE of vtm_solver_step for ONE CHUNK in one
 * launch.  vtm_solver_step computes x_out = mu + c_noise * noise; here x (the current noise level) and `target` (the next
 * level, noised independently by vtm_noise_levels) are given and that line is solved for the noise.  Sizes, dtypes, frame_ids,
 * model_out, w, g_ref, the rescale, the prediction types, the history, the launch shapes and the reduction order are
 * vtm_solver_step's; the arguments are its own plus target and z_out, minus noise and x_out.
 *   x          whole-video (n_frames, E) in `dtype`, rows frame_ids[f]: the level this step starts from.  Read only.
 *   target     whole-video, rows as x's: the level this step lands on.  Read, then CORRECTED IN PLACE.  Required when
 *              c_noise != 0; neither read nor written when c_noise == 0 (the step that lands on alphas_cumprod = 1).
 *   z_out      whole-video, rows as x's, in `dtype`: the step's noise map.  Required.  x, target and z_out are three buffers.
 *   h1, h2, h_out, eps_out, x0_out  as in vtm_solver_step.
 * Per frame and element, in fp32, with the operations of vtm_solver_step in the same order:
 *     m, x0, eps  as in vtm_solver_step
 *     mu      = c_x * x + c_x0 * x0 + c_h1 * h1 + c_h2 * h2            (a term whose coefficient is 0 is absent)
 *     z_out   = (target - mu) / c_noise                                  rounded ONCE to `dtype`;   +0 when c_noise == 0
 *     target  = mu + c_noise * fp32(z_out)                               rounded once
 *     h_out = x0 (fp32, not rounded) ;   eps_out = eps ;   x0_out = x0
 * The last line is vtm_solver_step's own x_out with noise = z_out, operation for operation (one shared helper, no contraction
 * into fma): vtm_solver_step on the same x, model_out and history with noise = z_out returns the corrected target and the same
 * h_out BIT FOR BIT.  Any E >= 1, F <= 2^20; F == 0 is VTM_OK.  One launch, no workspace, no atomics.  On a bad argument
 * (VTM_EINVAL) nothing is launched.
 * ---------------------------------------------------------------------------------------------- */
int vtm_invert_step(const void *x, const void *model_out, const float *h1, const float *h2, int dtype, int64_t F, int64_t E,
                    int64_t groups, const float *w, int64_t g_ref, const int32_t *frame_ids, int pred_type, float rescale,
                    float sqrt_alpha, float sqrt_beta, float c_x, float c_x0, float c_h1, float c_h2, float c_noise,
                    void *target, void *z_out, float *h_out, void *eps_out, void *x0_out, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_noise_levels -- the forward noising of a video to ALL levels of a schedule in one launch, in place on independent
 * N(0, 1) draws:   levels[k, p] = sqrt_alpha[k] * x0[p] + sqrt_beta[k] * levels[k, p]     for k < n, p < P.
 *   x0      (P) contiguous in `dtype`: the clean video.        levels  (n, P) contiguous in `dtype`, not x0.
 *   coef    DEVICE fp32 (n, 2): (sqrt_alpha[k], sqrt_beta[k]).
 * In fp32, every stored value rounded once.  16-byte accesses when P is a multiple of 16 bytes of `dtype` and both pointers
 * are 16-byte aligned, element accesses otherwise; which of the two changes no bit.  n <= 2^20, P >= 1; n == 0 is VTM_OK.
 * On a bad argument (VTM_EINVAL) nothing is launched.
 * ---------------------------------------------------------------------------------------------- */
int vtm_noise_levels(const void *x0, void *levels, const float *coef, int dtype, int64_t n, int64_t P, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Frame-keyed noise -- N(0, 1) noise addressed the way every other caller-side operand is: per frame.  The normal of element
 * e of whole-video frame `frame` at step `step` is a PURE FUNCTION of (seed, tag, step, frame, e) -- a counter-based generator,
 * no state and no stream position -- so a stochastic step's bits depend neither on how the video is cut into chunks, nor on
 * the chunks' order, nor on the rank or the stream that runs a chunk (noise.FrameNoise).  The keying is part of this contract:
 *     generator  Philox4x32-10 (Salmon et al., SC'11; Random123's philox4x32, 10 rounds): multipliers 0xD2511F53, 0xCD9E8D57,
 *                Weyl constants 0x9E3779B9, 0xBB67AE85; per round
 *                c = [hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)], then k0 += W0, k1 += W1.
 *     key        (seed & 0xffffffff, seed >> 32)
 *     counter    (e >> 2, frame, step, tag)   e: the element's offset inside its frame (E = C * H * W elements);
 *                frame: the whole-video row, frame0 + (frame_ids ? frame_ids[f] : f);  tag: names the use (VTM_NOISE_*; a
 *                caller's own tags start at VTM_NOISE_USER).  Element e takes normal number e & 3 of its quad.
 *     normals    from the outputs o0 .. o3, for the pairs (a, b) = (o0, o1) and (o2, o3):
 *                u1 = ((a >> 9) + 0.5f) * 2^-23 (exact in fp32, inside (0, 1));  u2 = (b >> 8) * 2^-24;
 *                r = sqrtf(-2 logf(u1));  the pair's normals are r * cospif(2 u2), r * sinpif(2 u2)
 *                -- the precise fp32 functions, no fast-math.  u1 >= 2^-24, so |z| <= sqrt(48 ln 2) = 5.7682 by construction.
 * In a 16-bit model dtype the fp32 normal is rounded ONCE to the dtype before any use, so a keyed step computes exactly what
 * the tensor-noise step computes from vtm_frame_noise's output.
 *
 * vtm_frame_noise -- out (S, F, E) contiguous in `dtype`: out[s, f, e] = the normal of element e of frame frame0 + row(f) at
 *   step step0 + s (mod 2^32).  frame_ids: DEVICE int32 (F entries) or NULL (row f); frame0 in [0, 2^31).  One thread per quad,
 *   one quad-wide store (16 bytes fp32, 8 bytes 16-bit) when E % 4 == 0 and out is aligned to it, element stores otherwise;
 *   which of the two changes no bit.  E in [1, 2^34], F <= 2^20, S * F * ceil(E / 4) < 2^32 - 256; S == 0 or F == 0 is VTM_OK.
 * vtm_philox_bits -- the integer core alone: out[i] = Philox4x32-10(ctr[i], key of seed) for n counters of four uint32 (both
 *   DEVICE, 16-byte aligned), so the generator can be pinned exactly on the device.
 * vtm_guided_step_keyed / vtm_solver_step_keyed -- vtm_guided_step / vtm_solver_step with (seed, step, tag, frame0) in place
 *   of the noise pointer: the noise of the chunk is drawn where it is used (no randn launch, no (F, E) read), otherwise the
 *   same expression, operation for operation, and the same launch shapes; every other argument is the tensor form's.  frame0:
 *   the whole-video row of row 0 of x / x_out / h1 / h2 / h_out -- a caller that steps an ascending run of frames offsets those
 *   pointers to the run's first row, sends no frame_ids, and names the first row here; 0 otherwise.  With sigma == 0
 *   (c_noise == 0) the term is absent and the key is not used.  One launch, no workspace, no atomics; on a bad argument
 *   (VTM_EINVAL) nothing is launched.
 * ---------------------------------------------------------------------------------------------- */
#define VTM_NOISE_INIT   0   /* the initial latents */
#define VTM_NOISE_STEP   1   /* a sampler's stochastic term; counter.step = the step index i */
#define VTM_NOISE_LEVELS 2   /* edit-friendly inversion's independent levels; counter.step = the level index k */
#define VTM_NOISE_USER   16  /* the first tag that is the caller's */
int vtm_frame_noise(void *out, int dtype, int64_t S, int64_t F, int64_t E, const int32_t *frame_ids, int64_t frame0,
                    uint64_t seed, uint32_t step0, uint32_t tag, vtm_stream_t stream);
int vtm_philox_bits(const uint32_t *ctr, int64_t n, uint64_t seed, uint32_t *out, vtm_stream_t stream);
int vtm_guided_step_keyed(const void *x, const void *model_out, uint64_t seed, uint32_t step, uint32_t tag, int64_t frame0,
                          int dtype, int64_t F, int64_t E, int64_t groups, int64_t g_uncond, int64_t g_cond,
                          const int32_t *frame_ids, int pred_type, float guidance, float rescale, float sqrt_alpha,
                          float sqrt_beta, float c_x0, float c_eps, float sigma, void *x_out, void *eps_out, void *x0_out,
                          vtm_stream_t stream);
int vtm_solver_step_keyed(const void *x, const void *model_out, uint64_t seed, uint32_t step, uint32_t tag, int64_t frame0,
                          const float *h1, const float *h2, int dtype, int64_t F, int64_t E, int64_t groups, const float *w,
                          int64_t g_ref, const int32_t *frame_ids, int pred_type, float rescale, float sqrt_alpha,
                          float sqrt_beta, float c_x, float c_x0, float c_h1, float c_h2, float c_noise, void *x_out,
                          float *h_out, void *eps_out, void *x0_out, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_semantic_guidance -- semantic guidance (SEGA, Brack et al.; Diffusers' SemanticStableDiffusionPipeline, and with
 * `regions` the masked form of LEditsPPPipelineStableDiffusion) for ONE CHUNK in one launch: the combined model output that
 * vtm_guided_step / vtm_solver_step then take as a single group.  Every edit concept has its own group of the UNet output;
 * its term is kept only where its magnitude reaches a quantile of its plane, which no set of group weights can express.
 *   model_out  (groups * F, C, H, W) contiguous NCHW, group-major, dtype VTM_F32 / VTM_F16 / VTM_BF16; groups <=
 *              VTM_SOLVER_MAX_GROUPS.
 *   g_uncond   the group of the unconditional prediction u;  g_cond: the group of the conditional prediction c, or -1 for
 *              no classifier-free term;  guidance_scale: s.
 *   n_concepts E, 0 .. VTM_SEGA_MAX_CONCEPTS, each with HOST arrays copied into the kernel arguments:
 *              group[e]; scale[e] = s_e, signed (a reversed edit is a negative scale); w_apply[e], w_acc[e] finite fp32;
 *              mode[e] one of VTM_SEGA_*; and for the quantile q_e in [0, 1], with P = H W and pos = q_e (P - 1) in double,
 *              rank_lo[e] = floor(pos) in [0, P) and rank_frac[e] = pos - rank_lo[e] in [0, 1) (not read for VTM_SEGA_REGION).
 *   regions    DEVICE uint8 (E, F, H, W) of 0 / 1, or NULL; required when a concept with a non-zero weight names a region.
 *   momentum   whole-video fp32 (n_rows, C, H, W) from the pointer given, or NULL; chunk frame f is row frame_ids[f] (DEVICE
 *              int32, distinct, inside [0, n_rows): the caller's contract), or row f when frame_ids is NULL (vtm_solver_step's
 *              h1).  mom_scale, mom_beta finite; mom_apply 0 / 1.
 *   out        chunk-local (F, C, H, W) in dtype; must not overlap model_out.
 *   mask_out   DEVICE uint8 (E, F, C, H, W), or NULL.
 * Per frame f, channel ch and pixel p, in fp32 (inputs convert to fp32 exactly), every sum started from 0 in the order
 * written:
 *     d_e   = model_out[group[e] * F + f] - u
 *     g_e   = scale[e] * d_e                 one subtraction, one product, each rounded to nearest, not contracted
 *     a_e   = |g_e|                          VTM_SEGA_CHANNEL*: the population is the (f, ch) plane, P values
 *           = sum over ch' = 0 .. C - 1 of |g_e[ch']|, ascending, each addition rounded, not contracted
 *                                            VTM_SEGA_SUM*: one population per frame, the same mask for every channel
 *     a_lo, a_hi = the values of ranks rank_lo and min(rank_lo + 1, P - 1) of the population in ascending order: exact order
 *             statistics; NaNs rank ABOVE +inf (where np.sort puts them)
 *     thr   = (float)((double)a_lo + rank_frac * ((double)a_hi - (double)a_lo))       IEEE double, not contracted
 *     M_e   = a_e >= thr  [ AND regions[e, f, p] != 0 for the *_REGION modes ] ;  = regions[e, f, p] != 0 for VTM_SEGA_REGION,
 *             which takes no quantile at all
 *     gamma_app = sum over e ascending with w_apply[e] != 0 of  w_apply[e] * (M_e ? g_e : 0) ;  gamma_acc: the same with w_acc
 *     m     = u + s * (c - u) + gamma_app + mom_scale * nu      (s term absent for g_cond < 0; nu term absent for a NULL
 *                                                                momentum or mom_apply == 0)
 *     nu'   = mom_beta * nu + (1 - mom_beta) * gamma_acc         in place, by the thread that read nu (1 - mom_beta in fp32)
 *     out   = m rounded once to dtype ;   mask_out[e] = M_e as 0 / 1
 * The mask SELECTS, it does not multiply: a term that is masked off is absent, whatever it holds.  A concept whose two weights
 * are both 0 is never read (a group full of NaN stays out) and its mask_out rows are not written; a term whose weight is
 * exactly 0 is absent from its sum.  A NaN in a_e is never selected, and a population whose chosen ranks hold a NaN (or an
 * infinity: inf - inf and 0 * inf are NaN) has thr = NaN and selects nothing.  A plane's bits depend on its own frame's values alone -- not on F, the
 * other frames, the chunking or the run (integer LDS atomics only, no global atomics, no workspace).  One workgroup owns a
 * (frame, channel) plane with the population in LDS: 1 <= H W <= VTM_SEGA_MAX_PLANE; C >= 1 (<= 1024); F <= 2^20, F == 0 is
 * VTM_OK and launches nothing.  On a bad argument (VTM_EINVAL) nothing is launched, out and momentum are untouched.
 * ---------------------------------------------------------------------------------------------- */
#define VTM_SEGA_MAX_CONCEPTS 6
#define VTM_SEGA_MAX_PLANE 16384
#define VTM_SEGA_CHANNEL 0          /* quantile of |g_e| per (frame, channel) plane */
#define VTM_SEGA_SUM 1              /* quantile of the channel sum of |g_e| per frame */
#define VTM_SEGA_REGION 2           /* the region alone */
#define VTM_SEGA_CHANNEL_REGION 3   /* VTM_SEGA_CHANNEL and the region */
#define VTM_SEGA_SUM_REGION 4       /* VTM_SEGA_SUM and the region */
int vtm_semantic_guidance(const void *model_out, int dtype, int64_t F, int64_t C, int64_t H, int64_t W, int64_t groups,
                          int64_t g_uncond, int64_t g_cond, float guidance_scale, int64_t n_concepts, const int32_t *group,
                          const float *scale, const int32_t *rank_lo, const double *rank_frac, const float *w_apply,
                          const float *w_acc, const int32_t *mode, const uint8_t *regions, float *momentum, int64_t n_rows,
                          const int32_t *frame_ids, float mom_scale, float mom_beta, int mom_apply, void *out,
                          uint8_t *mask_out, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_layernorm -- the block's norm1 (vidtome/patch.py:139-146, the plain torch.nn.LayerNorm branch
 * `norm_hidden_states = self.norm1(hidden_states)`), the first operation of the patched segment and the
 * producer of the matching metric; also usable for norm2 / norm3 (patch.py:173-176, 187).
 * x, out: (rows, C) contiguous in `dtype`; gamma, beta: (C) in the same dtype or NULL (no affine part).
 * fp32 statistics (mean, then centred sum of squares; biased variance like torch), y = (x - mean) *
 * rsqrt(var + eps) * gamma + beta evaluated in fp32, rounded once.  C % 8 == 0, C <= 2048.
 * ---------------------------------------------------------------------------------------------- */
int vtm_layernorm(const void *x, const void *gamma, const void *beta, int dtype, int64_t rows, int64_t C,
                  float eps, void *out, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_layernorm_gather -- norm3 on m(x): `self.norm3(...)` (vidtome/patch.py:187) applied to the rows a "replace"-mode merge
 * closure selects (merge.py:119-133), for a feed-forward that runs on the merged tokens (tomesd's merge_mlp, which the
 * reference dropped; patch.py's `merge_mlp` opt-in here).  It replaces vtm_gather_rows followed by vtm_layernorm /
 * vtm_layernorm_panels: the merged tokens are never written.
 *   x     (B, L, C) contiguous in `dtype`; gamma, beta (C) in the same dtype or NULL.
 *   rows  (B, n) int32: output row b * n + i is the LayerNorm of x[b, rows[b, i], :].  Entries may repeat and come in any
 *         order; n may exceed L.  They are NOT range-checked on the device: every entry must lie in [0, L) -- the caller's
 *         business (the maps of compute_merge's local levels do).
 *   out   panel_rows == 0: (B * n, C) token rows.  panel_rows > 0: k-panels [C / 8][panel_rows][8] as vtm_layernorm_panels
 *         writes them, panel_rows = vtm_panel_rows(B * n) exactly; rows >= B * n of the panels are not written.  fp16 / bf16
 *         only (fp32: token rows).
 * The arithmetic is vtm_layernorm's, kernel for kernel (the kernel family is chosen from C and the B * L rows of x): sums in
 * the same order, the same fused multiply-adds, one rounding.  Output row (b, i) is therefore BIT-EQUAL to row
 * b * L + rows[b, i] of vtm_layernorm / vtm_layernorm_panels over the same x.  C % 8 == 0, C <= 2048, B <= 65535, L < 2^31;
 * B == 0 or n == 0 is VTM_OK.  One launch, no workspace.  On a bad argument -- a NULL x / rows / out, an unsupported C or dtype,
 * a panel_rows that is neither 0 nor vtm_panel_rows(B * n) -- VTM_EINVAL is returned and nothing is launched.
 * ---------------------------------------------------------------------------------------------- */
int vtm_layernorm_gather(const void *x, const void *gamma, const void *beta, int dtype, int64_t B, int64_t L, int64_t C,
                         const int32_t *rows, int64_t n, float eps, void *out, int64_t panel_rows, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_geglu -- the gated activation inside the block's feed-forward `self.ff(...)` (vidtome/patch.py:187-199;
 * SD blocks use the Diffusers GEGLU feed-forward): x (rows, 2 D) = [value | gate] -> out (rows, D) =
 * value * gelu(gate), exact (erf) gelu, the gate rounded to `dtype` before the product like torch's two ops.
 * ---------------------------------------------------------------------------------------------- */
int vtm_geglu(const void *x, int dtype, int64_t rows, int64_t D, void *out, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_linear_rows -- `Linear(gather(tokens))`: the attention projections of the patched block
 * (`self.attn1(...)`, vidtome/patch.py:157-162; to_q / to_k / to_v / to_out[0] as in utils/pnp_utils.py:47-95)
 * fed by the composed merge map instead of a materialised merged tensor (the reference's
 * merge closure `cat([gather(src, unm_idx), dst])`, merge.py:119-133 / 423-437, followed by nn.Linear).
 *   out[b, i, :] = pool[b, p(i), :] @ W^T (+ bias),   p(i) = rows[b, rows2[b, i]]   (either map may be NULL:
 *   rows2 NULL -> p(i) = rows[b, i];  rows NULL -> p(i) = rows2[b, i] or i)
 * pool = x0 (B, P0, K) | x1 (B, P1, K) as in vtm_gather_rows; rows: (B, rows_ld) int32 pool ids (the composed merge
 * map); rows2: (B, n) int32 positions in the merged sequence (the live-query rows of a global level).
 * W: (N, K) row-major like torch.nn.Linear.weight, bias: (N) or NULL; fp16 / bf16, fp32 accumulation.
 * transposed == 0: out is (B, >= n, ldo >= N) token-major; transposed != 0: out is (B, N, ldo >= n) channel-major
 * (V^T for vtm_attention).  out_batch_stride in elements.  K % 32 == 0.  Rows >= n of out are not written.
 * Alignment of out: any ldo >= the row length, any out_batch_stride and any element-aligned base are accepted, and
 * nothing outside the valid (n, N) elements is written.  Vector stores are used where they are aligned, single elements
 * otherwise: 16-byte stores when ldo % 8 == 0 and the sample's base (out + b * out_batch_stride) is 16-byte aligned; for
 * K % 320 != 0, 8-byte stores when ldo % 4 == 0 and that base is 8-byte aligned.  The K = 320 kernel with resident weights
 * needs ldo % 8 == 0, out_batch_stride % 8 == 0 and a 16-byte aligned out; other layouts take the tiled kernel.
 * VTM_F32 is vtm_linear_f32 below with VTM_LINEAR_NONE and a VTM_F32 output (its alignment and shape rules apply).
 * ---------------------------------------------------------------------------------------------- */
int vtm_linear_rows(const void *x0, int64_t P0, const void *x1, int64_t P1, int dtype, int64_t B, int64_t K,
                    const int32_t *rows, int64_t rows_ld, const int32_t *rows2, int64_t n, const void *W,
                    const void *bias, int64_t N, void *out, int64_t ldo, int64_t out_batch_stride,
                    int transposed, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_linear_f32 -- every projection of an fp32 model's patched block in fp32, fed like vtm_linear_rows: attn1's
 * to_q / to_k / to_v / to_out[0] through the composed merge map (vidtome/patch.py:157-162, utils/pnp_utils.py:47-95),
 * attn2's projections (patch.py:171-185) and the GEGLU feed-forward `ff(norm3(h)) + h` (patch.py:187-199).
 *   A rows: pool = x0 (B, P0, K) | x1 (B, P1, K), row i of sample b = pool[b, rows[b, rows2[b, i]]] exactly as
 *   vtm_linear_rows (either map may be NULL).  W: (N, K) fp32 row-major like torch.nn.Linear.weight; bias fp32 (N) or NULL.
 *   epilogue VTM_LINEAR_NONE:  out = x W^T + b
 *            VTM_LINEAR_RESID: out = (x W^T + b) + resid, resid fp32 laid out like out (same ldo / out_batch_stride)
 *            VTM_LINEAR_GEGLU: W holds 2 D rows [value; gate] (N = 2 D; bias likewise): out (n, D) = value * gelu(gate),
 *                              exact (erf) gelu; the 2 D-wide product is never written
 * fp32 operands and products on v_mfma_f32_32x32x2_f32: each output is a k-ascending fp32 fmaf chain from +0, then + bias,
 * then the epilogue.  out_dtype VTM_F32, or VTM_F16 = that value rounded once at the store (q / k / V^T for the fp16
 * attention core).  transposed == 0: out (B, >= n, ldo >= N_out) token-major; transposed != 0: out (B, N_out, ldo >= n)
 * channel-major (V^T); N_out = N, or D for GEGLU; out_batch_stride in elements.  K % 8 == 0, N % 8 (GEGLU: 16) == 0;
 * x0, x1 and W 16-byte aligned.  Rows >= n and columns >= N_out of out are not written.  No workspace; one launch.
 * ---------------------------------------------------------------------------------------------- */
enum { VTM_LINEAR_NONE = 0, VTM_LINEAR_RESID = 1, VTM_LINEAR_GEGLU = 2 };
int vtm_linear_f32(const float *x0, int64_t P0, const float *x1, int64_t P1, int64_t B, int64_t K,
                   const int32_t *rows, int64_t rows_ld, const int32_t *rows2, int64_t n, const float *W,
                   const float *bias, int64_t N, int epilogue, const float *resid, void *out, int out_dtype,
                   int64_t ldo, int64_t out_batch_stride, int transposed, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_lora_fold -- the effective weight of a LoRA-adapted projection of the block (`pipe.load_lora_weights(
 * **gene_config.lora)`, generate.py:93-94 with `use_lora` / `lora:` of configs/default.yaml:63-69; with the PEFT
 * backend Diffusers wraps attn1 / attn2 to_q / to_k / to_v / to_out.0, ff.net.0.proj and ff.net.2 of every
 * BasicTransformerBlock, and its forward is `base(x) + sum_a lora_B_a(lora_A_a(x)) * scaling_a`), so that the
 * projection kernels above run on W_eff = W + sum_a s_a B_a A_a instead of leaving the patched block:
 *   out[o, i] = round_dtype( w[o, i] + sum_{k < r} up[o, k] * down[k, i] )
 * w, out: (c_out, c_in) row-major in `dtype` (VTM_F16 / VTM_BF16 / VTM_F32; out may not alias up / down);
 * up: (c_out, r) fp32 row-major = the adapters' B matrices side by side with each adapter's scale applied;
 * down: (r, c_in) fp32 row-major = their A matrices stacked (r = the sum of the ranks).  The sum is a k-ascending
 * fp32 fmaf chain from +0, added to w in fp32 and rounded once.  Runs once per adapter state, not per step.
 * c_out, c_in, r > 0 (else VTM_EINVAL).
 * ---------------------------------------------------------------------------------------------- */
int vtm_lora_fold(const void *w, int dtype, const float *up, const float *down, int64_t c_out, int64_t c_in,
                  int64_t r, void *out, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_dora_norms / vtm_dora_fold -- the effective weight of a projection whose FIRST active adapter is DoRA (PEFT
 * `use_dora=True`, weight-decomposed LoRA; Diffusers' PEFT backend installs it when the adapter file carries magnitude
 * vectors).  PEFT's forward for it is base + (r - 1) (base - b) + r s_d x (B_d A_d)^T with r = m / ||W + s_d B_d A_d||
 * per output row (m: the adapter's magnitude vector), then the plain adapters after it, i.e. the Linear
 *   W_eff = diag(r) (W + s_d B_d A_d) + sum_{plain a} s_a B_a A_a.
 * up / down as for vtm_lora_fold, the DoRA adapter first: up = [s_d B_d | s_a B_a ...] (c_out, r) and down =
 * [A_d; A_a; ...] (r, c_in), fp32 row-major, the DoRA adapter's rank k_dora (0 < k_dora <= r).
 * vtm_dora_norms: norms[o] = sqrt( sum_i (w[o, i] + sum_{k < k_dora} up[o, k] * down[k, i])^2 ), fp32 (c_out).  The inner
 *   sums are the k-ascending fmaf chains of vtm_lora_fold, added to w in fp32; the squares are summed in a fixed order
 *   (one workgroup per 64-row band, column tiles ascending), so two calls give the same bits.
 * vtm_dora_fold: out[o, i] = round_dtype( (magnitude[o] / norms[o]) * (w[o, i] + sum_{k < k_dora} up[o, k] down[k, i])
 *   + sum_{k_dora <= k < r} up[o, k] down[k, i] ), each chain from +0, each fp32 step rounded once (the division is
 *   IEEE: a zero norm gives +-inf or NaN, as PEFT's does).  magnitude, norms: fp32 (c_out); out may not alias an input.
 * Runs once per adapter state, not per step.  Sizes as vtm_lora_fold (else VTM_EINVAL).
 * ---------------------------------------------------------------------------------------------- */
int vtm_dora_norms(const void *w, int dtype, const float *up, const float *down, int64_t c_out, int64_t c_in,
                   int64_t r, int64_t k_dora, float *norms, vtm_stream_t stream);
int vtm_dora_fold(const void *w, int dtype, const float *up, const float *down, const float *magnitude,
                  const float *norms, int64_t c_out, int64_t c_in, int64_t r, int64_t k_dora, void *out,
                  vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_loha_delta / vtm_lokr_delta / vtm_delta_fold -- the effective weight of a projection wrapped in a LyCORIS layer
 * (PEFT `LoHaConfig` / `LoKrConfig`).  Beyond the reference: it loads adapters through `pipe.load_lora_weights(
 * **gene_config.lora)` (generate.py:93-94), and these are the remaining adapter family Stable Diffusion users load on
 * the same ten projections.  At inference either layer is one Linear,
 *   LoHa: W_eff = W + sum_a s_a (W1a_a W1b_a) * (W2a_a W2b_a)   (* elementwise)
 *   LoKr: W_eff = W + sum_a s_a kron(W1_a, W2_a),
 * built as an fp32 delta (c_out, c_in) row-major, one adapter per call in PEFT's adapter order (accumulate = 0 writes
 * delta, 1 adds to what it holds with one fp32 addition), then folded into W.  All operands fp32 row-major; the host
 * multiplies s_a into one factor (w1a / w1) in fp32.
 * vtm_loha_delta: delta[o, i] (+)= (sum_{k < r} w1a[o, k] w1b[k, i]) * (sum_{k < r} w2a[o, k] w2b[k, i]); w1a, w2a:
 *   (c_out, r), w1b, w2b: (r, c_in).  Each sum is the k-ascending fp32 fmaf chain from +0 of vtm_lora_fold; then one fp32
 *   product.
 * vtm_lokr_delta: delta[i1 * a2 + i2, j1 * b2 + j2] (+)= w1[i1, j1] * w2[i2, j2], one fp32 product; w1: (a1, b1), w2:
 *   (a2, b2), a1 * a2 = c_out and b1 * b2 = c_in (else VTM_EINVAL).  A low-rank factor is multiplied out first by
 *   vtm_lora_fold on a zero fp32 base.
 * vtm_delta_fold: out[o, i] = round_dtype( fp32(w[o, i]) + delta[o, i] ); w, out: (c_out, c_in) in `dtype` (VTM_F16 /
 *   VTM_BF16 / VTM_F32), out may alias w.
 * Run once per adapter state, not per step; two calls give the same bits.  Sizes > 0 (else VTM_EINVAL).
 * ---------------------------------------------------------------------------------------------- */
int vtm_loha_delta(const float *w1a, const float *w1b, const float *w2a, const float *w2b, int64_t c_out, int64_t c_in,
                   int64_t r, int accumulate, float *delta, vtm_stream_t stream);
int vtm_lokr_delta(const float *w1, const float *w2, int64_t a1, int64_t b1, int64_t a2, int64_t b2, int64_t c_out,
                   int64_t c_in, int accumulate, float *delta, vtm_stream_t stream);
int vtm_delta_fold(const void *w, int dtype, const float *delta, int64_t c_out, int64_t c_in, void *out,
                   vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_groupnorm_silu -- the norm + activation pairs of the PnP feature-injection resnet (utils/pnp_utils.py:113-114
 * `norm1` + `nonlinearity`; :133-142 `+ temb`, `norm2`, `nonlinearity`): out = act(GroupNorm(x [+ add])) on an NCHW
 * tensor in one launch.  x, out: (B, C, HW) contiguous in `dtype`, 16-byte aligned, not the same buffer; add: (B, C) in
 * `dtype` or NULL (the projected time embedding); gamma, beta: (C) in `dtype` or NULL; `groups` divides C (else
 * VTM_EINVAL); act: 0 none, 1 SiLU.
 * Rounding points of torch's separate ops: x' = round(x + add[b, c]); fp32 statistics over each (sample, group),
 * the mean first (its sum carried in fp64), then the centred sum of squares (biased variance);
 * y = round((x' - mean) * rstd * gamma + beta); z = round(y / (1 + exp(-y))).  Any group size (C / groups) * HW < 2^31
 * and any HW (group starts need not be 16-byte aligned); a group that fits the LDS is read once, a larger one keeps
 * its first ~160 KiB on chip and re-reads the rest.
 * ---------------------------------------------------------------------------------------------- */
int vtm_groupnorm_silu(const void *x, const void *add, const void *gamma, const void *beta, int dtype, int64_t B,
                       int64_t C, int64_t HW, int64_t groups, float eps, int act, void *out, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * vtm_resnet_tail -- the end of the same resnet (utils/pnp_utils.py:146-162: the injection copies of the source
 * sample's features, the residual and the division by `output_scale_factor`) in one pass:
 *   out[b] = (shortcut[b] + hidden[row(b)]) / scale,   row(b) = b % period for b < inject_rows, else b - inject_rows + period.
 * shortcut, out: (B, M) contiguous in `dtype`; hidden holds only the rows that were computed: (period + B - inject_rows, M),
 * or (B, M) with inject_rows = 0 (row(b) = b, the plain residual).  inject_rows in [0, B]; inject_rows > 0 needs
 * period > 0 (else VTM_EINVAL).  Bit-identical to torch's `(shortcut + hidden_full) / scale` in `dtype`: the sum rounded
 * to `dtype`, then multiplied by the fp32 reciprocal of `scale` and rounded again.
 * ---------------------------------------------------------------------------------------------- */
int vtm_resnet_tail(const void *shortcut, const void *hidden, int dtype, int64_t B, int64_t M, int64_t inject_rows,
                    int64_t period, double scale, void *out, vtm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Attention broadcast -- vtm_residual_record / vtm_residual_replay / vtm_residual_replay_layernorm.  Beyond the reference:
 * Pyramid Attention Broadcast (Zhao et al. 2024) on the patched block.  In a window of timesteps a block's attn1 / attn2
 * segment is computed every k-th step and replayed in between (broadcast.py decides the steps on the host).  What is kept of
 * a segment is its contribution to the residual stream, the residual add included, per frame of the WHOLE video:
 *   d = T(f32(h_after) - f32(h_before)),      replayed as      h' = T(f32(h) + f32(d)),
 * T the model dtype, one rounding each.  The delta is the same whichever route computed the segment (several routes never
 * materialise the attention output before the residual add).
 * The batch is group-major: sample b = g * Fg + f, G groups of the chunk's Fg frames, E = N * C elements per frame.  A cache
 * is (G, num_frames, E) contiguous in `dtype`; frame f of the chunk is cache row (g, id(f)), id(f) = frame_ids[f], or f when
 * frame_ids is NULL.  frame_ids: device int32 (Fg,), the ids distinct and in [0, num_frames): they are NOT checked on the
 * device -- an id outside the range reads or writes outside the cache -- the caller validates them on the host.
 * vtm_residual_record: cache[(g * num_frames + id(f)) * E + e] = T(f32(h_out[b, e]) - f32(h_in[b, e])).  Rows the ids do not
 *   name are not touched.  cache must not overlap h_in / h_out (VTM_EINVAL).
 * vtm_residual_replay: out[b, e] = T(f32(h[b, e]) + f32(cache1[..])); with cache2 (may be NULL) then
 *   out[b, e] = T(f32(that rounded value) + f32(cache2[..])) -- two segments in a row, the intermediate rounding kept.
 *   out may be h itself (any other overlap: VTM_EINVAL).
 * Both: VTM_F32 / VTM_F16 / VTM_BF16; 1 <= Fg <= num_frames, G, E >= 1 (else VTM_EINVAL).  A grid-stride launch over
 * 16-byte chunks, moved with one 16-byte access when E is a multiple of the chunk (4 fp32 / 8 16-bit elements) and every
 * pointer is 16-byte aligned, element by element otherwise; which of the two changes no bit.
 * vtm_residual_replay_layernorm: the replay above to out_rows (G Fg N, C) -- may be h -- AND, in the same launch, the
 *   LayerNorm of those rows over C (gamma, beta: (C) in `dtype` or NULL) to out_panels in the k-panel layout
 *   [C / 8][panel_rows][8] vtm_ff_geglu reads, panel_rows = vtm_panel_rows(G Fg N); panel rows >= G Fg N are not written.
 *   Every written panel row is BIT-EQUAL to vtm_layernorm_panels(out_rows): the row lives in registers, two-pass fp32
 *   statistics, and the summation order is that of the kernel vtm_layernorm_panels launches for the same (G Fg N, C)
 *   (lanes-per-row at C = 320 / 640 and at C = 1280 from 32768 rows, a wave per row otherwise).  VTM_F16 / VTM_BF16 only
 *   (the panel GEMMs are 16-bit); C % 64 == 0, C <= 2048 -- the widths the fused feed-forward takes; every pointer 16-byte
 *   aligned; plain (cached) loads and stores.  Anything else: VTM_EINVAL.
 * No workspace, no atomics: a frame's bits depend on that frame's operands alone, so any chunking of a video gives the same
 * bits per frame.  Cache rows are written on `stream`; launches on two streams must name disjoint frames.
 * ---------------------------------------------------------------------------------------------- */
int vtm_residual_record(const void *h_in, const void *h_out, void *cache, const int32_t *frame_ids, int dtype, int64_t G,
                        int64_t Fg, int64_t num_frames, int64_t E, vtm_stream_t stream);
int vtm_residual_replay(const void *h, const void *cache1, const void *cache2, const int32_t *frame_ids, int dtype, int64_t G,
                        int64_t Fg, int64_t num_frames, int64_t E, void *out, vtm_stream_t stream);
int vtm_residual_replay_layernorm(const void *h, const void *cache1, const void *cache2, const int32_t *frame_ids,
                                  const void *gamma, const void *beta, float eps, int dtype, int64_t G, int64_t Fg,
                                  int64_t num_frames, int64_t N, int64_t C, void *out_rows, void *out_panels,
                                  int64_t panel_rows, vtm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VIDTOME_HIP_H */
