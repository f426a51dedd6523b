"""Cross-frame bipartite soft matching on MI355X -- the host side of vidtome/merge.py.

Public surface mirrors the reference (same names, argument meaning, return protocol and error behaviour):

* ``do_nothing``                           <- vidtome/merge.py:5-6
* ``bipartite_soft_matching_randframe``    <- vidtome/merge.py:20-159   (local merging)
* ``bipartite_soft_matching_2s``           <- vidtome/merge.py:343-463  (global merging)
* ``bipartite_soft_matching_random2d``     <- vidtome/merge.py:467-579  (per-frame 2-D merging: the original ToMe / ToMeSD
  matcher; a ``(merge, unmerge)`` pair, ``merge`` in "mean" mode by default -- not used by ``compute_merge``)
* ``bipartite_soft_matching_random2d_hier`` <- vidtome/merge.py:162-340 (random-frame matching with a receptive field:
  ``coord`` / ``rec_field``, ``adhere_src``, ``b_select`` / ``unm_modi`` on the closures -- not used by ``compute_merge``)
* ``bipartite_soft_matching_2f``           <- vidtome/merge.py:582-767  (the same over a ``[src_len | N - src_len]`` split)

Each matcher returns ``(merge, unmerge, ret_dict)`` closures like the reference, but the closures hold
*composed row maps* on the device instead of index tensors + gather/scatter code: in ``replace`` mode (the
only mode the reference's ``compute_merge`` ever uses, patch.py:45-46,73-75) merged tokens are a pure row
selection, so ``merge`` is one gather and ``unmerge`` is one gather with the inverse map.

The arithmetic lives in libvidtome_hip.so (``_lib``): fused normalise+split, fused score+row-max on the
fp32 MFMA, radix argsort, index planning.  Nothing here touches the CPU except the RNG draws the
reference also makes on its generator (merge.py:57-58, 500-501, patch.py:62).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, replace
from typing import Callable, Optional, Tuple

import torch

from . import _lib

# "filtered" (default) or "exact": both produce bit-identical packed results (tests/test_gpu_parity.py)
MATCH_MODE = os.environ.get("VIDTOME_MATCH", "filtered")


def do_nothing(x: torch.Tensor, mode: str = None, **kwargs):
    """vidtome/merge.py:5-6."""
    return x


@dataclass
class Level:
    """Result of one matching level, everything device-resident (int32)."""
    N_in: int
    Ns: int
    Nd: int
    r: int
    new_cur: torch.Tensor              # (B, U + Nd) pool row id of every merged token  (merge closure)
    inv: torch.Tensor                  # (B, N_in)  merged position each input position is restored from
    a_pos: torch.Tensor                # (Ns,)  = a_idx of the reference
    b_pos: torch.Tensor                # (Nd,)  = b_idx
    best: torch.Tensor                 # packed row maxima (see include/vidtome_hip.h)
    unm_idx: Optional[torch.Tensor] = None
    src_idx: Optional[torch.Tensor] = None
    dst_idx: Optional[torch.Tensor] = None

    @property
    def unm_num(self) -> int:
        return self.Ns - self.r


# Launch plan of the filtered matcher (same bits either way): "auto" = merge.MatchPlanner decides per
# block from the previous call's counters, "one" = always the one-launch filter (rounds 1-4), "range" = always scout + range
MATCH_PLAN = os.environ.get("VIDTOME_MATCH_PLAN", "auto")
# ... and whether the planner may let the scout test after one channel step ("0": always at the filter's own depth)
SHALLOW_SCOUT = os.environ.get("VIDTOME_SHALLOW_SCOUT", "1") != "0"


class MatchPlanner:
    """How the next call of ONE matching level of one block is launched (vtm_match_filtered_plan / _ordered).

    The scout + range plan is ~30 % faster when nearly all 256 x 128 tile pairs die at the scout's test -- frames of one clip
    at low noise -- and ~40 % slower when most stay alive (uncorrelated tokens; a noisy clip, whose matches do not clear the
    rest bound at that depth).  How many stay alive is a property of the data at that block, and consecutive calls (the next
    chunk, the next denoising step) see similar data, so the planner steers by the PREVIOUS call's counters: every
    scout + range call copies its 8 counters asynchronously into this planner's pinned host buffer; the next call reads
    whatever has arrived -- never waiting, never synchronising; a stale or missing reading only delays a switch -- and falls
    back to the one-launch plan for `COOL` calls when the spans the second launch had to stream covered more than `HIGH` of
    the level, then tries again.  Measured per call (profiles/r05_n_scout_range_plan.txt, r05_q_position_order.txt): the plan
    wins up to 0.08 of the level inside the spans (top level 1 on low-noise clips 0.06: -24 %; position-ordered top global level
    0.014: -43 % on top of the ordering; a smooth field's level 2 0.077: -8 %) and loses from 0.11 on (0.25: -11 % ... +50 %;
    ~1.0 on noisy clips and uncorrelated tokens: +40 %).

    Levels behind the first are handed to the matcher in position order (vtm_position_order) -- which the plan needs, and which
    by itself costs a 40 us sort and saves 12-26 % of a top global call (more blocks die) but nothing at level 2.  So
    `order_alone` says what the level does while the plan is off: keep the ordering (global level) or go back to the reference's
    row order (level 2); and a level in which NOTHING died at the scout's test (uncorrelated tokens) drops the ordering too.
    Results never depend on any of this.

    Two pinned buffers, one per KIND of reading (round 6): the scout + range calls copy into `buf`, the one
    one-launch call that is asked for the filter's own counters (the order probe) into `probe_buf` -- the 32-byte copy of
    an earlier scout + range call that lands late can then never be read as the probe's answer.  `__del__` waits for the
    copies still in flight before the pinned memory goes back to torch's host allocator."""

    # COOL (round 6: 32, was 256): how long a level stays on the one-launch plan before the scout is tried again.  It bounds
    # BOTH costs of being wrong (tests/test_gpu_parity.py::test_planner_cost_is_bounded_on_alternating_regimes): on data the plan
    # never pays for, one exploring call (+40 % of ONE call) per COOL + 1 calls = +1.2 % of the level; on a clip that turns
    # plan-friendly again, at most COOL calls at the one-launch price (a shot of 300 calls: < 3 % of the level against a
    # per-call oracle; 256 lost 11 % there).  Fast alternation (every 2 - 8 calls) cannot be followed from the previous call's
    # counters at all; the planner then costs at most the exploring calls against the better FIXED plan.
    HIGH, LOW, COOL = 0.09, 0.07, 32

    def __init__(self, order_alone: bool = False):
        self.mode = _lib.MATCH_SCOUT_RANGE
        self.buf = torch.zeros(8, dtype=torch.int32).pin_memory()
        self.view = self.buf.numpy()
        self.probe_buf = torch.zeros(8, dtype=torch.int32).pin_memory()
        self.probe_view = self.probe_buf.numpy()
        self.cool = 0
        self.switches = 0
        self.order_alone = order_alone
        self.order_off = False
        self.order_probe = False
        # the scout's depth: the filter's own test depth, or ONE 64-channel step (VTM_MATCH_SCOUT_STEPS(1): -20 ... -28 % per
        # call where a tile that is dead at 40 % of the channels is dead at 20 % already -- low-noise clips: same spans;
        # elsewhere more tiles stay marked).  Tried once the deep scout's spans are below LOW, kept while its own are below HIGH
        self.shallow = False
        self.shallow_ban = 0
        self.issued_shallow = False

    def next(self):
        """-> (mode, pinned stats buffer or None, position-order the level?, scout steps) for the call about to be issued."""
        if self.mode == _lib.MATCH_SCOUT_RANGE:
            tested, in_spans = int(self.view[4]), int(self.view[7])        # the last call whose counters have arrived
            if tested > 0:
                self.view[4] = 0                                           # judged once
                wide = in_spans > self.HIGH * tested
                if self.issued_shallow:                                    # (that call scouted after one step)
                    if wide:
                        self.shallow, self.shallow_ban = False, self.COOL
                elif wide:
                    self.mode, self.cool = _lib.MATCH_ONE_LAUNCH, self.COOL
                    self.switches += 1
                    # does the ordering pay without the plan?  Not when nothing dies in the ONE-LAUNCH filter either (its
                    # running maxima grow along the dst axis, the scout only has the seeds: a drifting smooth field leaves
                    # every block alive in the scout and 29 % in the filter) -- asked of the first one-launch call's counters
                    self.order_off, self.order_probe = False, self.order_alone
                    self.probe_view[4] = 0
                elif self.shallow_ban <= 0 and in_spans < self.LOW * tested:      # (some margin: a level at the edge of the
                    self.shallow = True                                           # plan is not the place for a cheaper scout)
            if self.shallow_ban > 0:
                self.shallow_ban -= 1
        else:
            if self.order_probe and int(self.probe_view[4]) > 0:
                self.order_off = int(self.probe_view[5]) > 0.9 * int(self.probe_view[4])
                self.order_probe = False
            self.cool -= 1
            if self.cool <= 0:
                self.mode, self.shallow = _lib.MATCH_SCOUT_RANGE, False
                self.view[4] = 0
        if self.mode == _lib.MATCH_SCOUT_RANGE:
            self.issued_shallow = self.shallow
            return self.mode, self.buf, True, (1 if self.shallow else 0)
        return self.mode, (self.probe_buf if self.order_probe else None), self.order_alone and not self.order_off, 0

    def __del__(self):
        # an asynchronous counter copy may still be in flight towards the pinned buffers: wait for the device
        # before they are released (garbage collection of a block, bench.py dropping a block's planners)
        try:
            if torch.cuda.is_available() and torch.cuda.is_initialized():
                torch.cuda.synchronize()
        except Exception:          # interpreter shutdown: the process' memory goes with it
            pass


# Levels 2 / global meet their rows in position order (vtm_position_order + vtm_match_filtered_ordered: same bits, fewer live
# blocks; "0" = the reference's sequence order as in rounds 1-4) ...
POSITION_ORDER = os.environ.get("VIDTOME_POSITION_ORDER", "1") != "0"
# ... when the level is large enough for the sort (3 launches, ~40 us) to pay: src rows x dst rows per sample
# ... also with align_batch (ONE order for all samples, sample 0's: entry i is the same original index in every sample)
ALIGNED_ORDER = os.environ.get("VIDTOME_ALIGNED_ORDER", "1") != "0"
POSITION_ORDER_MIN_PAIRS = int(os.environ.get("VIDTOME_POSITION_ORDER_MIN_PAIRS", str(1 << 26)))


def order_level(Ns: int, Nd: int, tokens: int, align_batch: bool) -> bool:
    """Does a level of this geometry (not the first local one) meet its rows in position order?"""
    return (POSITION_ORDER and (ALIGNED_ORDER or not align_batch) and Ns * Nd >= POSITION_ORDER_MIN_PAIRS and
            0 < tokens <= _lib.POSITION_ORDER_MAX_N)


def _run_level(x0: torch.Tensor, x1: Optional[torch.Tensor], parts, ratio: float, align_batch: bool,
               want_indices: bool, seed=None, planner: Optional[MatchPlanner] = None, reorder: bool = False,
               r: Optional[int] = None) -> Level:
    """normalise+split -> fused score/top-1 -> argsort -> index split  (merge.py:84-117 / 389-421).  ``reorder``: the level's
    rows are NOT in (frame, position) order (every level but the first local one) -- the matcher is then handed both lists
    sorted by token position and reports in the original indexing; everything behind it sees the reference's order.
    ``r``: the number of src tokens to merge where the caller states it as a count (bipartite_soft_matching_random2d,
    merge.py:542) instead of a ratio."""
    a_pos, b_pos, a_rows, b_rows = parts
    Ns, Nd = a_rows.shape[1], b_rows.shape[1]
    if r is None:
        r = min(Ns, int(Ns * ratio))                   # merge.py:90 (Python float -> int truncation)
    else:
        r = min(Ns, int(r))                            # merge.py:542
    if MATCH_MODE == "exact" or x0.shape[2] > 1280:    # plain fp32-MFMA kernel (filter window holds for C <= 1280)
        a_op, _ = _lib.normalize_gather(x0, x1, a_rows)
        b_op, _ = _lib.normalize_gather(x0, x1, b_rows)
        best = _lib.match(a_op, b_op, Ns, Nd, align_batch)
    else:                                              # fp16 filter + fp32 refine: same bits, ~4x faster
        mode, stats, order, scout = _lib.MATCH_ONE_LAUNCH, None, None, 0
        m_a, m_b = a_rows, b_rows
        seeded = seed is not None and _lib.SEED_MATCHER
        can_order = reorder and seeded and order_level(Ns, Nd, seed[0], align_batch)
        use_order = can_order
        if seeded and (can_order or not reorder) and MATCH_PLAN != "one":     # (rows in similarity-rank order: no plan)
            if MATCH_PLAN == "range":
                mode = _lib.MATCH_SCOUT_RANGE
            elif planner is not None:
                mode, stats, keep, scout = planner.next()
                use_order = can_order and keep
                if not SHALLOW_SCOUT:
                    scout = 0
        if use_order:
            tokens, L, pos1, _ = seed
            m_a, a_order, m_b, b_order, table = _lib.position_order(a_rows, b_rows, L, tokens, pos1, x0.shape[1],
                                                                    shared=align_batch)
            order, seed = (a_order, b_order), (tokens, L, pos1, table)     # the sort's offsets ARE the position -> dst table
        elif can_order and seed[2] is not None and seed[3] is None:
            seed = None        # a global level left in the reference's order without a position -> dst table: unseeded
        best = _lib.match_filtered(x0, x1, m_a, m_b, align_batch, seed=seed, mode=mode, stats_host=stats, order=order,
                                   scout_steps=scout)
    perm = _lib.sort_desc(best)
    new_cur, inv, unm_idx, src_idx, dst_idx = _lib.plan_apply(best, perm, a_pos, b_pos, a_rows, b_rows, r,
                                                              align_batch, want_indices)
    return Level(Ns + Nd, Ns, Nd, r, new_cur, inv, a_pos, b_pos, best, unm_idx, src_idx, dst_idx)


def local_level(x0: torch.Tensor, cur: Optional[torch.Tensor], N_in: int, F: int, ratio: float, unm_pre: int,
                randf: int, target_stride: int, align_batch: bool, want_indices: bool = False,
                tokens: Optional[int] = None, planner: Optional[MatchPlanner] = None) -> Level:
    """One level of local merging on the joined chunk x0 (B, L, C); ``cur`` maps the current sequence to
    rows of x0 (None = identity).  ``tokens`` = tokens per frame of the joined chunk when its rows are (frame, position)
    ordered: the matcher is then seeded with, for every src token, the token at the same position of the first dst frame
    (dst index = position; never changes the result)."""
    B = x0.shape[0]
    tnum = (N_in - unm_pre) // F                       # merge.py:43
    ts = min(target_stride, F)                         # merge.py:56
    parts = _lib.partition_local(cur, B, N_in, unm_pre, tnum, ts, randf, x0.device)
    seed = (tokens, x0.shape[1], None, None) if (tokens and tokens == tnum) else None
    # the scout + range plan is for position-ordered rows on both sides: the first level (cur None) as it comes, the later
    # ones through vtm_position_order.  (Measured with a planner on every level while levels 2 / global still met their rows in
    # similarity-rank order: they switched themselves off on every regime and only paid the exploring calls.)
    return _run_level(x0, None, parts, ratio, align_batch, want_indices, seed, planner, reorder=cur is not None)


def global_level(x0: torch.Tensor, anchors: torch.Tensor, cur_local: Optional[torch.Tensor], Ml: int,
                 local_is_src: bool, ratio: float, align_batch: bool, want_indices: bool = False,
                 tokens: Optional[int] = None, anchor_positions: Optional[torch.Tensor] = None,
                 planner: Optional[MatchPlanner] = None) -> Level:
    """Global merging of the chunk's local tokens against the block's anchor tokens (patch.py:59-82).  ``tokens`` (tokens
    per frame) / ``anchor_positions`` (B, Mg) int32 seed the matcher with the dst token at every src token's position."""
    B, L, _ = x0.shape
    if cur_local is None:
        cur_local = torch.arange(Ml, dtype=torch.int32, device=x0.device).expand(B, Ml).contiguous()
    seed = table = None
    # a seed pairs a src row with the dst row at the same token position: one side of the level is the anchors, so their
    # positions must be known whichever side it is (local-is-src: the position -> dst row table is built from them;
    # local-is-dst: they are the src rows).  Anchors that arrived without positions (an exchange's single-message form, a
    # user-supplied tensor): no table, no seed launch
    if tokens and _lib.SEED_MATCHER and anchor_positions is not None:
        src_len = Ml if local_is_src else anchors.shape[1]
        if not order_level(src_len, Ml + anchors.shape[1] - src_len, tokens, align_batch):   # (position-ordered calls get their table from the sort)
            table = torch.empty((B, tokens), dtype=torch.int32, device=x0.device)
        seed = (tokens, L, anchor_positions, table)
    parts = _lib.partition_global(cur_local, L, anchors.shape[1], local_is_src, table, tokens or 0, anchor_positions)
    return _run_level(x0, anchors, parts, ratio, align_batch, want_indices, seed, planner, reorder=True)


def draw_randf(generator: torch.Generator, ts: int) -> int:
    """merge.py:57-58: ``torch.randint(0, target_stride, [1], generator=generator)`` on the CPU generator."""
    return int(torch.randint(0, ts, torch.Size([1]), generator=generator, device=generator.device))


def _check_metric(metric: torch.Tensor) -> torch.Tensor:
    if metric.dim() != 3:
        raise ValueError("metric must be [B, N, C]")
    if not metric.is_cuda:
        raise RuntimeError("vidtome_amd runs on the GPU only (no CPU path); got a CPU tensor")
    return metric.contiguous()


def _merge_with_mode(level: Level, x: torch.Tensor, mode: str) -> torch.Tensor:
    """merge.py:119-133 / 423-437: ``cat([unm, dst])``; in the modes other than "replace" the matched src rows are first
    folded into their dst rows (``scatter_reduce(..., reduce=mode, include_self=True)``, merge.py:127-131) -- never reached
    from compute_merge, provided for code written against the closure protocol."""
    x = x.contiguous()
    out = _lib.gather_rows(x, None, level.new_cur)                  # [unm | dst]: the replace-mode result
    if mode == "replace":
        return out
    B = x.shape[0]
    src_rows = level.a_pos.long()[level.src_idx.long()].to(torch.int32).contiguous()       # (B, r) rows of x
    dst_rows = level.b_pos.to(torch.int32).expand(B, -1).contiguous()                       # (B, Nd)
    return _lib.merge_reduce(x, src_rows, dst_rows, level.dst_idx.contiguous(), mode, out, level.Ns - level.r)


def _make_closures(level: Level, N: int, out_slice: Optional[Tuple[int, int]] = None, merge_mode="replace"):
    def merge(x: torch.Tensor, mode=None) -> torch.Tensor:
        return _merge_with_mode(level, x, mode if mode is not None else merge_mode)

    def unmerge(x: torch.Tensor, **kwarg) -> torch.Tensor:
        inv = level.inv
        if out_slice is not None:                       # merge.py:459
            inv = inv[:, out_slice[0]:out_slice[1]].contiguous()
        return _lib.unmerge_add(x.contiguous(), inv, None)

    return merge, unmerge


def bipartite_soft_matching_randframe(metric: torch.Tensor, F: int, ratio: float, unm_pre: int,
                                      generator: torch.Generator, target_stride: int = 4,
                                      align_batch: bool = False, merge_mode: str = "replace"
                                      ) -> Tuple[Callable, Callable, dict]:
    """vidtome/merge.py:20-159, same signature.  ``ret_dict`` additionally carries the index tensors the
    reference keeps in closure cells (a_idx, b_idx, unm_idx, src_idx, dst_idx as int32) for parity tests."""
    metric = _check_metric(metric)
    B, N, _ = metric.shape
    tnum = (N - unm_pre) // F
    if ratio <= 0:
        return do_nothing, do_nothing, {"unm_num": tnum}          # merge.py:45-46
    with torch.no_grad():
        randf = draw_randf(generator, min(target_stride, F))
        level = local_level(metric, None, N, F, ratio, unm_pre, randf, target_stride, align_batch, True,
                            tokens=tnum if unm_pre == 0 else None)
    merge, unmerge = _make_closures(level, N, None, merge_mode)
    ret_dict = {"unm_num": level.unm_num, "a_idx": level.a_pos, "b_idx": level.b_pos,
                "unm_idx": level.unm_idx, "src_idx": level.src_idx, "dst_idx": level.dst_idx,
                "level": level}
    return merge, unmerge, ret_dict


def bipartite_soft_matching_2s(metric: torch.Tensor, src_len: int, ratio: float, align_batch: bool,
                               merge_mode: str = "replace", unmerge_chunk: int = 0):
    """vidtome/merge.py:343-463, same signature (including the 2-tuple returned for ratio <= 0,
    merge.py:364-365)."""
    metric = _check_metric(metric)
    B, N, _ = metric.shape
    if ratio <= 0:
        return do_nothing, do_nothing
    with torch.no_grad():
        # [src | dst] = [src_len | N - src_len]: expressed as "local = src part, anchors = dst part"
        x_src = metric[:, :src_len].contiguous()
        x_dst = metric[:, src_len:].contiguous()
        level = global_level(x_src, x_dst, None, src_len, True, ratio, align_batch, True)
    sl = (0, src_len) if unmerge_chunk == 0 else (src_len, N)

    def merge(x: torch.Tensor, mode=None) -> torch.Tensor:
        return _merge_with_mode(level, x, mode if mode is not None else merge_mode)

    def unmerge(x: torch.Tensor, **kwarg) -> torch.Tensor:
        return _lib.unmerge_add(x.contiguous(), level.inv[:, sl[0]:sl[1]].contiguous(), None)

    ret_dict = {"unm_num": level.unm_num, "a_idx": level.a_pos, "b_idx": level.b_pos,
                "unm_idx": level.unm_idx, "src_idx": level.src_idx, "dst_idx": level.dst_idx,
                "level": level}
    return merge, unmerge, ret_dict


def spatial_level(metric: torch.Tensor, w: int, h: int, sx: int, sy: int, r: int,
                  draws: Optional[torch.Tensor]) -> Level:
    """The level of bipartite_soft_matching_random2d (merge.py:493-550) on metric (B, h * w, C): the 2-D partition
    (vtm_partition_2d; ``draws`` = the hsy * wsx cell draws on the device as int32, None = no_rand), then the matcher, the sort
    and the index split of every other level -- never aligned, never seeded (dst tokens are scattered over the frame, one per
    cell: no src token has a dst token at its own position)."""
    B, N, _ = metric.shape
    a_pos, b_pos = _lib.partition_2d(metric.device, h, w, sx, sy, draws)
    a_rows, b_rows = a_pos.expand(B, -1).contiguous(), b_pos.expand(B, -1).contiguous()
    if a_pos.numel() == 0:
        # sx == sy == 1: every token is dst and b_idx = 0 .. N - 1, so "cat([unm, dst])" and its inverse are the identity map;
        # there is no score to take a maximum of (merge.py:542: r = min(0, r) = 0)
        none = torch.empty((B, 0), dtype=torch.int32, device=metric.device)
        return Level(N, 0, N, 0, b_rows, b_rows, a_pos, b_pos, torch.empty((B, 0), dtype=torch.int64, device=metric.device),
                     none, none, none)
    return _run_level(metric, None, (a_pos, b_pos, a_rows, b_rows), 0.0, False, True, r=r)


def bipartite_soft_matching_random2d(metric: torch.Tensor, w: int, h: int, sx: int, sy: int, r: int,
                                     no_rand: bool = False, generator: torch.Generator = None
                                     ) -> Tuple[Callable, Callable]:
    """vidtome/merge.py:467-579, same signature and the same ``(merge, unmerge)`` pair: one random dst token per sy x sx cell
    of the h x w frame, the r most similar src tokens merged into their nearest dst token.  ``merge(x, mode="mean")`` takes
    torch.scatter_reduce's modes (merge.py:558; there is no "replace" here), ``unmerge(x)`` restores the N positions
    (merge.py:562-577).  a_idx / b_idx are in ascending token order (include/vidtome_hip.h, vtm_partition_2d).  The closures
    carry ``.level`` (the index tensors the reference keeps in closure cells) for parity tests."""
    if r <= 0:
        return do_nothing, do_nothing                              # merge.py:487-488: before any draw
    metric = _check_metric(metric)
    B, N, _ = metric.shape
    if N != h * w:
        raise ValueError(f"metric holds {N} tokens per sample, a {w} x {h} frame has {h * w}")
    with torch.no_grad():
        draws = None
        if not no_rand:                                            # merge.py:500-501, on the generator's own device
            hsy, wsx = h // sy, w // sx
            draws = torch.randint(sy * sx, size=(hsy, wsx, 1), device=generator.device, generator=generator)
            draws = draws.reshape(-1).to(device=metric.device, dtype=torch.int32)
        level = spatial_level(metric, w, h, sx, sy, r, draws)
    merge_any, unmerge_any = _make_closures(level, N, None, "mean")

    def merge(x: torch.Tensor, mode="mean") -> torch.Tensor:
        if mode not in _lib.REDUCE_MODES:                          # (the level machinery's "replace" included)
            raise ValueError(f"merge mode {mode!r}: expected one of {sorted(_lib.REDUCE_MODES)}")
        return merge_any(x, mode)

    def unmerge(x: torch.Tensor) -> torch.Tensor:
        return unmerge_any(x)

    merge.level = unmerge.level = level
    return merge, unmerge


# ---- the receptive-field matchers (merge.py:162-340, 582-767) ---------------------------------------------------------------
def _coord_pool(coord: torch.Tensor, metric: torch.Tensor) -> torch.Tensor:
    """coord (B or 1, N, c <= 4) -> the (B or 1, N, 4) fp32 coordinate pool of vtm_match_masked (unused components 0)."""
    B, N, _ = metric.shape
    if coord.dim() != 3 or coord.shape[1] != N or coord.shape[0] not in (1, B):
        raise ValueError(f"coord must be [B, N, c] for a metric of {B} x {N} tokens, got {tuple(coord.shape)}")
    c = coord.shape[2]
    if not 1 <= c <= 4:
        raise ValueError(f"coord has {c} components per token; the masked matcher takes 1 to 4")
    pool = torch.zeros((coord.shape[0], N, 4), dtype=torch.float32, device=metric.device)
    pool[:, :, :c] = coord.to(device=metric.device, dtype=torch.float32)
    return pool


def masked_level(x0: torch.Tensor, parts, ratio: float, align_batch: bool, coord: torch.Tensor, rec_field: float) -> Level:
    """A level whose scores are zeroed outside the receptive field before the row maximum (merge.py:233-241): normalise+split ->
    masked exact matcher (vtm_match_masked) -> argsort -> index split.  The filtered matcher's pruning takes a score for a
    cosine, which a masked 0 is not; so: no filter, no seeds, no planner, no position order."""
    a_pos, b_pos, a_rows, b_rows = parts
    Ns, Nd = a_rows.shape[1], b_rows.shape[1]
    r = min(Ns, int(Ns * ratio))                       # merge.py:244-245
    a_op, _ = _lib.normalize_gather(x0, None, a_rows)
    b_op, _ = _lib.normalize_gather(x0, None, b_rows)
    best = _lib.match_masked(a_op, b_op, Ns, Nd, align_batch, coord, a_rows, b_rows, _lib.mask_threshold(rec_field))
    perm = _lib.sort_desc(best)
    new_cur, inv, unm_idx, src_idx, dst_idx = _lib.plan_apply(best, perm, a_pos, b_pos, a_rows, b_rows, r, align_batch, True)
    return Level(Ns + Nd, Ns, Nd, r, new_cur, inv, a_pos, b_pos, best, unm_idx, src_idx, dst_idx)


def _select(level: Level, b_select) -> Level:
    """The level of the samples ``b_select`` (an int or a list, merge.py:292-295): their maps apply to the rows of x in turn."""
    if b_select is None:
        return level
    sel = torch.as_tensor(b_select if isinstance(b_select, (list, tuple)) else [b_select], dtype=torch.long,
                          device=level.new_cur.device)
    pick = lambda t: t.index_select(0, sel).contiguous()
    return replace(level, new_cur=pick(level.new_cur), inv=pick(level.inv), unm_idx=pick(level.unm_idx),
                   src_idx=pick(level.src_idx), dst_idx=pick(level.dst_idx))


def _rf_closures(level: Level, merge_mode: str, out_slice: Optional[Tuple[int, int]], fold_first_rows: bool):
    """The closures of the two receptive-field matchers: merge(x, mode=None, b_select=None, **kw) and
    unmerge(x, b_select=None, unm_modi=None, **kw) (merge.py:289-337 / 706-764).  ``fold_first_rows``: the non-replace modes
    fold src rows 0 .. r - 1 instead of the matched ones (bipartite_soft_matching_2f)."""
    def merge(x: torch.Tensor, mode=None, b_select=None, **kwarg) -> torch.Tensor:
        lv = _select(level, b_select)
        mode = mode if mode is not None else merge_mode
        if mode == "replace" or not fold_first_rows:
            return _merge_with_mode(lv, x, mode)
        x = x.contiguous()
        out = _lib.gather_rows(x, None, lv.new_cur)
        B = x.shape[0]
        src_rows = lv.a_pos[:lv.r].to(torch.int32).expand(B, -1).contiguous()
        dst_rows = lv.b_pos.to(torch.int32).expand(B, -1).contiguous()
        return _lib.merge_reduce(x, src_rows, dst_rows, lv.dst_idx.contiguous(), mode, out, lv.Ns - lv.r)

    def unmerge(x: torch.Tensor, b_select=None, unm_modi=None, **kwarg) -> torch.Tensor:
        inv = _select(level, b_select).inv
        if out_slice is not None:                       # merge.py:759-762
            inv = inv[:, out_slice[0]:out_slice[1]].contiguous()
        if unm_modi == "zero":                          # merge.py:326-328: the un-merged part restores as zeros
            x = x.clone()
            x[:, :level.unm_num] = 0
        return _lib.unmerge_add(x.contiguous(), inv, None)

    return merge, unmerge


def _rf_dict(level: Level) -> dict:
    return {"unm_num": level.unm_num, "a_idx": level.a_pos, "b_idx": level.b_pos, "unm_idx": level.unm_idx,
            "src_idx": level.src_idx, "dst_idx": level.dst_idx, "level": level}


def bipartite_soft_matching_random2d_hier(metric: torch.Tensor, frame_num: int, ratio: float, unm_pre: int,
                                          generator: torch.Generator, target_stride: int = 4, adhere_src: bool = False,
                                          merge_mode: str = "replace", scores=None, coord: Optional[torch.Tensor] = None,
                                          rec_field: float = 2):
    """vidtome/merge.py:162-340, same signature: bipartite_soft_matching_randframe (``adhere_src`` is its ``align_batch``)
    with a receptive field -- given ``coord`` (B, N, c <= 4), every score whose src and dst coordinates are further apart than
    ``rec_field`` counts as 0 in the row maximum (merge.py:233-241; bit parity for integer-valued coordinates up to 2048 in
    magnitude, include/vidtome_hip.h) -- and with ``b_select`` / ``unm_modi="zero"`` on the closures.  ``scores`` is accepted
    and ignored (the reference overwrites it, merge.py:238).  ``ratio <= 0`` returns the 2-tuple of merge.py:181-182, before
    any draw; c > 4 raises ValueError.  ``ret_dict`` carries the index tensors and the level like randframe's."""
    if ratio <= 0:
        return do_nothing, do_nothing
    metric = _check_metric(metric)
    B, N, _ = metric.shape
    F = frame_num
    tnum = (N - unm_pre) // F
    pool = None if coord is None else _coord_pool(coord, metric)
    with torch.no_grad():
        ts = min(target_stride, F)
        randf = draw_randf(generator, ts)                                   # merge.py:197-198
        if pool is None:
            level = local_level(metric, None, N, F, ratio, unm_pre, randf, target_stride, adhere_src, True,
                                tokens=tnum if unm_pre == 0 else None)
        else:
            parts = _lib.partition_local(None, B, N, unm_pre, tnum, ts, randf, metric.device)
            level = masked_level(metric, parts, ratio, adhere_src, pool, rec_field)
    merge, unmerge = _rf_closures(level, merge_mode, None, False)
    return merge, unmerge, _rf_dict(level)


def bipartite_soft_matching_2f(metric: torch.Tensor, src_len: int, ratio: float, adhere_src: bool,
                               merge_mode: str = "replace", scores=None, coord: Optional[torch.Tensor] = None,
                               rec_field: float = 2, unmerge_chunk: int = 0):
    """vidtome/merge.py:582-767, same signature: bipartite_soft_matching_2s over the ``[src_len | N - src_len]`` split with
    the receptive field and the closure keywords of bipartite_soft_matching_random2d_hier; ``unmerge`` returns the
    ``unmerge_chunk`` part.  The non-replace merge modes reproduce the reference AS WRITTEN: its gather of the matched src
    rows is commented out (merge.py:718), so ``scatter_reduce`` folds the FIRST r src rows -- rows 0 .. r - 1 of x, in that
    order -- into ``dst_idx``; that row list is what vtm_merge_reduce is handed here."""
    if ratio <= 0:
        return do_nothing, do_nothing
    metric = _check_metric(metric)
    B, N, _ = metric.shape
    pool = None if coord is None else _coord_pool(coord, metric)
    with torch.no_grad():
        if pool is None:
            level = global_level(metric[:, :src_len].contiguous(), metric[:, src_len:].contiguous(), None, src_len, True,
                                 ratio, adhere_src, True)
        else:
            cur = torch.arange(src_len, dtype=torch.int32, device=metric.device).expand(B, src_len).contiguous()
            parts = _lib.partition_global(cur, src_len, N - src_len, True)
            level = masked_level(metric, parts, ratio, adhere_src, pool, rec_field)
    sl = (0, src_len) if unmerge_chunk == 0 else (src_len, N)
    merge, unmerge = _rf_closures(level, merge_mode, sl, True)
    return merge, unmerge, _rf_dict(level)
