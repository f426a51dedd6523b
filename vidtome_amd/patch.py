"""apply_patch / remove_patch / update_patch / collect_from_patch -- the hook API of vidtome/patch.py,
with the patched self-attention segment executed by libvidtome_hip.so.

Mirrors (file:line under the reference):
* ``compute_merge``               <- vidtome/patch.py:14-91
* ``make_diffusers_tome_block``   <- vidtome/patch.py:119-203   (class *named* ToMeBlock, ``_parent``)
* ``hook_tome_model`` / ``hook_tome_module`` <- vidtome/patch.py:206-231
* ``apply_patch``                 <- vidtome/patch.py:234-334   (same kwargs and defaults)
* ``remove_patch``                <- vidtome/patch.py:337-355
* ``update_patch``                <- vidtome/patch.py:358-370
* ``collect_from_patch``          <- vidtome/patch.py:373-387

Differences that are design, not omissions:
* the merge chain of a block is ONE composed gather map and the unmerge chain ONE inverse map (all levels
  use merge mode "replace", so merged tokens are a row selection of [chunk tokens | anchor tokens]);
* ``module.global_tokens`` stays on the device (the reference parks it on the CPU and syncs per block,
  patch.py:65,70,80,82);
* the block generator forks the CPU RNG state by default (utils.init_generator; `generator_device="device"` opts into the
  reference's device rule);
* ``attn1`` is evaluated from the module's own weights by the fused path (projection GEMMs fed through the composed
  merge map or as panel GEMMs, attention core = vtm_attention: no library GEMM on the default path), including the
  reference's PnP injection branch when ``utils/pnp_utils.py``-style control is registered on the module;
* with a global level the attention runs only for the DISTINCT merged rows the chunk's local tokens read
  (MergePlan.q_rows / q_count), and the rest of the block (norm2 / attn2, norm3 / GEGLU feed-forward) runs as panel GEMMs
  (csrc/ff.hip) when the modules are the plain arithmetic.
"""
from __future__ import annotations

import math
import os
from typing import Any, Callable, Dict, NamedTuple, Optional, Tuple, Type

import torch
import torch.nn.functional as F

from . import _lib, freeu, ip_adapter, lora, merge, pag
from .utils import init_generator, isinstance_str, join_frame, split_frame

# Attention over the merged sequence computes outputs only for the rows unmerge() reads (see MergePlan.q_rows);
# VIDTOME_LIVE_QUERIES=0 computes every row like the reference does (same block output, more work).
LIVE_QUERIES = os.environ.get("VIDTOME_LIVE_QUERIES", "1") != "0"
# With the local chunk on the src side of the global level several local tokens may have merged into the SAME anchor
# token; its attention output is then computed once and shared (device-side compaction of the live queries, no host
# sync: the attention launch is sized for the upper bound and query blocks past the per-sample count exit).
# VIDTOME_COMPACT_QUERIES=0 computes one query per local token (round 2's behaviour; same block output).
COMPACT_QUERIES = os.environ.get("VIDTOME_COMPACT_QUERIES", "1") != "0"


# ----------------------------------------------------------------------------------------------------
# compute_merge
# ----------------------------------------------------------------------------------------------------
class MergePlan:
    """What ``compute_merge`` produces for one block call: composed maps + the merged tokens."""

    __slots__ = ("fsize", "L", "M", "gather_map", "_inv", "_inv_parts", "_merged", "levels", "global_level", "local_chunk",
                 "x_joined", "anchors_in", "q_rows", "inv_q", "q_count", "pad_to", "fold_args", "_key_fold", "aligned",
                 "keep", "inv_local", "_frame_order")

    def __init__(self):
        self.levels = []
        # The LOCAL levels alone (None when none ran): keep (B, M_l) the joined-chunk row of every token of the locally merged
        # sequence (local levels never reference anchor rows: every entry < L), inv_local (B, L) their composed unmerge map.
        # `gather_map` / `inv` are these too until a global level replaces the first and folds the second into its own; the
        # feed-forward on merged tokens (merge_mlp, ``ff_route``) runs on the local closures whatever follows them.
        self.keep = None
        self.inv_local = None
        self._frame_order = None        # the two in frame order, for attn2 on merged tokens (``frame_order``): on first use
        self.global_level = None
        self.local_chunk = None
        self.gather_map = None
        self._inv = None
        self._inv_parts = None          # (local-levels inverse map, local position -> merged position): composed on demand
        self.anchors_in = None
        # Global level only: the rows of the merged sequence whose attention output unmerge() ever reads
        # (q_rows[b, t] = merged row of local token t) and the local-levels-only inverse map.  The merged
        # sequence also contains the other chunk's tokens; they are keys / values, but nobody reads their
        # attention OUTPUT (merge.py:459 returns the local part only), so the block computes attention for
        # the q_rows queries only -- a third fewer at global_merge_ratio 0.5, same block output.
        # q_count (B,) int32 on the device, or None: with the local chunk on the src side q_rows lists every DISTINCT
        # merged position once (several local tokens may share an anchor row) and only its first q_count[b] entries
        # are queries; inv_q then maps through that compact list.
        self.q_rows = None
        self.inv_q = None
        self.q_count = None
        self.aligned = False            # align_batch: every sample shares the levels' indices (so also q_rows / inv_q)
        # The anchors' exact duplicates (patch.py:80 copies an anchor row to every local token that merged into it) are
        # duplicate KEYS of the next block: (merged-position -> pool row map, L, content id per anchor row, number of ids)
        # when the anchors carry ids, folded on first use by the attention path that can take a per-key multiplicity
        self.fold_args = None
        self._key_fold = None
        self._merged = None
        self.pad_to = 8

    @property
    def inv(self) -> Optional[torch.Tensor]:
        """The composed unmerge map of ALL levels (B, L): merged row every position of the joined chunk is restored from.
        With a global level the patched block unmerges through `inv_q` (the rows its live queries produce) and never needs
        this map, so it is composed on first use (API users, tests, VIDTOME_LIVE_QUERIES=0)."""
        if self._inv is None and self._inv_parts is not None:
            inv_local, loc = self._inv_parts
            self._inv = _lib.compose(inv_local, loc, self.L) if inv_local is not None else loc
        return self._inv

    def key_fold(self, dtype, n: Optional[int] = None) -> Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
        """(key_sel, k_bias, k_count) of _lib.fold_keys, or None when the anchors carried no content ids.  ``n``: fold the
        keys of the first n samples only (the org samples of a perturbed-attention batch: the others have no keys)."""
        if self._key_fold is None and self.fold_args is not None:
            cur, L, cid, n_ids = self.fold_args
            self._key_fold = _lib.fold_keys(cur, L, cid, n_ids, dtype) if n is None else \
                _lib.fold_keys(cur[:n], L, cid[:n], n_ids, dtype)
        return self._key_fold

    def frame_order(self) -> Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
        """(keep_sorted, inv_sorted, seg_off) of _lib.frame_order over the local levels' maps, or None when no local level
        ran: the kept rows in ascending order -- frame by frame --, the unmerge map of that order and the absolute offsets
        of every (sample, frame)'s rows in the (B M_l)-row sequence.  ``keep`` / ``inv_local`` stay as they are."""
        if self._frame_order is None and self.keep is not None and self.inv_local is not None:
            self._frame_order = _lib.frame_order(self.keep, self.inv_local, self.fsize, self.L // self.fsize)
        return self._frame_order

    @property
    def merged(self) -> torch.Tensor:
        """The merged tokens (B, Mp, C) -- what the reference's composed merge closure returns (patch.py:84).  The
        patched block itself does not need them (its projections read the pool through `gather_map`), so they are
        materialised on first use."""
        if self._merged is None:
            self._merged = self.x_joined if self.gather_map is None else \
                _lib.gather_rows(self.x_joined, self.anchors_in, self.gather_map, pad_to=self.pad_to)
        return self._merged


CHECK_CONTENT_IDS = os.environ.get("VIDTOME_CHECK_CID", "0") == "1"


def tag_content_ids(tokens: torch.Tensor, ids: torch.Tensor) -> None:
    """Attach content ids (B, M) int32 -- equal id = byte-identical rows; -1 = none -- to an anchor tensor.  RESULTS depend
    on them (the attention folds rows with equal ids into one key), so the tag also records what the tensor looked like
    when the ids were computed: torch's version counter, the storage address and the shape.  `content_ids` drops the ids
    when any of them changed.  What no tag can see is a write that bypasses torch (`.data`, a raw pointer, another library's
    kernel): `module.global_tokens` must not be edited that way; VIDTOME_CHECK_CID=1 verifies the claim on every use (one
    device sync per block: a debugging aid)."""
    tokens._vtm_cid = (ids, tokens._version, tokens.data_ptr(), tuple(tokens.shape))


def mark_anchors_ready(tokens: Optional[torch.Tensor]) -> None:
    """(round 6) Consecutive chunks may run on DIFFERENT HIP streams (two chunks in flight hide each other's dispatch gaps and
    small launches: bench.py `two_in_flight`, +15 % chunk-steps/s on one GPU).  The anchors are the one thing chunk k + 1 takes
    from chunk k (patch.py:60-82), so the producer leaves an event behind every anchor tensor it stores -- recorded on its
    stream after the last kernel that writes the anchors, their token positions or their content ids."""
    if tokens is not None and tokens.is_cuda:
        s = torch.cuda.current_stream(tokens.device)
        ev = torch.cuda.Event()
        ev.record(s)
        tokens._vtm_ready = (ev, s.cuda_stream)


def await_anchors(tokens: Optional[torch.Tensor]) -> None:
    """... and a consumer on another stream waits for that event ON THE DEVICE (no host synchronisation) and tells torch's
    caching allocator that the tensors are in use on its stream too (`record_stream`: the producer's reference may be dropped
    -- the next anchor update replaces `module.global_tokens` -- while this stream's kernels still read the old rows)."""
    ready = getattr(tokens, "_vtm_ready", None) if tokens is not None else None
    if ready is None or not tokens.is_cuda:
        return
    ev, sid = ready
    cur = torch.cuda.current_stream(tokens.device)
    if cur.cuda_stream == sid:
        return
    cur.wait_event(ev)
    tokens.record_stream(cur)
    pos = getattr(tokens, "_vtm_pos", None)
    if pos is not None and pos.is_cuda:
        pos.record_stream(cur)
    tag = getattr(tokens, "_vtm_cid", None)
    if tag is not None and len(tag) == 4 and tag[0].is_cuda:
        tag[0].record_stream(cur)


def content_ids(tokens: torch.Tensor, device, dtype) -> Optional[torch.Tensor]:
    """The ids `tag_content_ids` attached, or None when the tag is missing or stale."""
    tag = getattr(tokens, "_vtm_cid", None)
    if tag is None or len(tag) != 4:
        return None
    ids, version, ptr, shape = tag
    if (version != tokens._version or ptr != tokens.data_ptr() or shape != tuple(tokens.shape)
            or tuple(ids.shape) != tuple(tokens.shape[:2]) or ids.device != torch.device(device) or tokens.dtype != dtype):
        return None
    if CHECK_CONTENT_IDS:
        # rows with equal ids must be equal: compare every row with the first row of its id
        B, M = ids.shape
        for b in range(B):
            idb = ids[b].long()
            valid = idb >= 0
            if not bool(valid.any()):
                continue
            first = torch.full((int(idb.max()) + 1,), M, dtype=torch.long, device=ids.device)
            first.scatter_reduce_(0, idb[valid], torch.arange(M, device=ids.device)[valid], reduce="amin")
            ref = tokens[b][first[idb.clamp(min=0)].clamp(max=M - 1)]
            same = (tokens[b].view(torch.int16 if tokens.element_size() == 2 else torch.int32)
                    == ref.view(torch.int16 if tokens.element_size() == 2 else torch.int32)).all(dim=1)
            if not bool((same | ~valid).all()):
                raise RuntimeError("vidtome_amd: anchor rows with equal content ids differ -- module.global_tokens was "
                                   "modified behind torch's back (VIDTOME_CHECK_CID=1)")
    return ids


def _planner(module: torch.nn.Module, key, order_alone: bool = False) -> "merge.MatchPlanner":
    """The launch planner of one matching level of the block (merge.MatchPlanner), kept on the module next to its generator
    and its anchors, one per level geometry; `remove_patch` drops them."""
    plans = module.__dict__.get("_vtm_match_plans")
    if plans is None:
        plans = module.__dict__["_vtm_match_plans"] = {}
    p = plans.get(key)
    if p is None:
        p = plans[key] = merge.MatchPlanner(order_alone)
    return p


def _draw_coin(generator: torch.Generator) -> float:
    """patch.py:62: ``torch.rand(1, generator=generator, device=generator.device)``."""
    return float(torch.rand(1, generator=generator, device=generator.device))


def compute_merge(module: torch.nn.Module, x: torch.Tensor, tome_info: Dict[str, Any],
                  pad_to: int = 8, want_indices: bool = False, materialize: bool = True
                  ) -> Tuple[Callable, Callable, torch.Tensor]:
    """vidtome/patch.py:14-91.  Returns ``(m, u, merged_tokens)``; ``u`` accepts ``resid=`` to fuse the
    residual add of patch.py:169 into the unmerge gather.  ``merged_tokens`` is (B, Mp, C) with
    Mp = M rounded up to ``pad_to`` rows (zero rows); ``m.plan`` exposes the MergePlan.  With ``materialize=False``
    (the patched block's own call: its projections gather through the map) the third value is None and
    ``m.plan.merged`` materialises the tokens on demand."""
    original_h, original_w = tome_info["size"]
    original_tokens = original_h * original_w
    downsample = int(math.ceil(math.sqrt(original_tokens // x.shape[1])))        # patch.py:17
    args = tome_info["args"]
    generator = module.generator
    fsize = x.shape[0] // args["batch_size"]                                       # patch.py:23
    tsize = x.shape[1]                                                             # patch.py:24

    if downsample > args["max_downsample"]:                                        # patch.py:27,86-88
        return merge.do_nothing, merge.do_nothing, x

    gmode = args.get("generator_device", None)
    if args["generator"] is None:                                                  # patch.py:29-33
        args["generator"] = init_generator(x.device, mode=gmode)
    elif args["generator"].device != x.device and (gmode or GENERATOR_MODE_DEFAULT()) == "device":
        args["generator"] = init_generator(x.device, fallback=args["generator"], mode=gmode)

    plan = MergePlan()
    plan.fsize = fsize
    plan.aligned = bool(args["align_batch"])
    # chunk-parallel runs (chunk_parallel.py): the exchange replays the draws of the chunks other ranks process
    # and posts the receive of the predecessor's anchor tokens before this block's own first draw
    exchange = getattr(module, "_vtm_exchange", None)
    xkey = getattr(module, "_vtm_key", "")
    with torch.no_grad():
        xj = join_frame(x.contiguous(), fsize)                                     # patch.py:37 (a view)
        B, L, C = xj.shape
        if exchange is not None:
            exchange.begin_block(module, xkey, fsize, tsize, args, xj)
        plan.x_joined, plan.L = xj, L
        cur: Optional[torch.Tensor] = None      # pool row id of every token of the current sequence
        inv: Optional[torch.Tensor] = None      # composed unmerge map so far
        n_cur, unm, curF = L, 0, fsize
        while curF > 1:                                                            # patch.py:44-54
            ratio = args["local_merge_ratio"]
            if ratio <= 0:                                                         # merge.py:45-46
                unm += (n_cur - unm) // curF
            else:
                randf = merge.draw_randf(generator, min(args["target_stride"], curF))
                lv = merge.local_level(xj, cur, n_cur, curF, ratio, unm, randf, args["target_stride"],
                                       args["align_batch"], want_indices, tokens=tsize,
                                       planner=_planner(module, (xj.shape[1], curF, n_cur)))
                plan.levels.append(lv)
                unm += lv.unm_num
                cur = lv.new_cur
                inv = _lib.compose(inv, lv.inv, L) if inv is not None else lv.inv
                n_cur = cur.shape[1]
            curF = (n_cur - unm) // tsize                                          # patch.py:54
        Ml = n_cur
        plan.keep, plan.inv_local = cur, inv       # (before a global level overwrites the one and folds the other away)

        anchors_out = anchors_pos = None
        if args["merge_global"]:                                                   # patch.py:59-82
            if exchange is not None:
                gt = exchange.anchors_for(xkey, lambda: xj if cur is None else _lib.gather_rows(xj, None, cur), xj, cur)
            else:
                gt = getattr(module, "global_tokens", None)
                await_anchors(gt)              # (a predecessor chunk on another stream: device-side wait, see mark_anchors_ready)
            # token positions of the anchors (the matcher's seeds) ride on the tensor THIS function stored (an attribute of the
            # tensor object: they live and die with it); anchors that came from anywhere else (the user, an exchange) have none
            gt_pos = getattr(gt, "_vtm_pos", None) if gt is not None else None
            if gt_pos is not None and (tuple(gt_pos.shape) != tuple(gt.shape[:2]) or gt_pos.device != xj.device):
                gt_pos = None
            # content ids (equal id = identical rows), same lifetime rule -- and, because RESULTS depend on them, only while
            # nobody has written to the tensor since (in-place edits bump torch's version counter)
            gt_cid = content_ids(gt, xj.device, xj.dtype) if gt is not None else None
            if gt is not None:
                gt = gt.to(xj).contiguous()                                        # patch.py:65,70
                coin = _draw_coin(generator)
                local_is_src = coin > args["global_rand"]                          # patch.py:62
                res_ratio = args["global_merge_ratio"]
                if res_ratio <= 0:
                    # merge.py:364-365 returns a 2-tuple which patch.py:73 unpacks into 3 names
                    raise ValueError("not enough values to unpack (expected 3, got 2)")
                gl = merge.global_level(xj, gt, cur, Ml, local_is_src, res_ratio, args["align_batch"],
                                        want_indices, tokens=tsize, anchor_positions=gt_pos,
                                        planner=_planner(module, ("global", xj.shape[1]), order_alone=True))
                plan.global_level, plan.local_chunk = gl, (0 if local_is_src else 1)
                plan.anchors_in = gt
                off = 0 if local_is_src else gt.shape[1]                           # merge.py:459
                # loc: local position -> merged position.  patch.py:80: new anchors = u(merged) = the local tokens with every
                # merged local src row replaced by its matched global row -> one gather (amap) from [chunk | old anchors];
                # their token positions ride along for the next chunk's seeds
                loc, amap, anchors_pos = _lib.anchor_maps(gl.inv, off, gl.new_cur, Ml, L, tsize, gt_pos, _lib.SEED_MATCHER)
                anchors_out = _lib.gather_rows(xj, gt, amap)
                anchors_cid = None
                if gt_cid is not None and _lib.FOLD_KEYS and gl.new_cur.shape[1] <= 131072:
                    plan.fold_args = (gl.new_cur, L, gt_cid, gt.shape[1])
                if local_is_src and COMPACT_QUERIES and gl.Nd <= 131072:      # (vtm_compact_queries' bitmap lives in LDS)
                    qc, tmap, plan.q_count = _lib.compact_queries(loc, gl.Ns - gl.r, gl.Nd)
                    plan.q_rows = qc
                    plan.inv_q = _lib.compose(inv, tmap, L) if inv is not None else tmap
                    # local tokens that share a merged position become identical rows of the new anchors: tmap is an id
                    # per distinct position (old anchor rows that were copies of each other keep distinct ids -- a
                    # missed fold, never a wrong one)
                    anchors_cid = tmap
                else:
                    plan.q_rows, plan.inv_q = loc, inv
                plan._inv_parts, inv = (inv, loc), None      # composed lazily (MergePlan.inv)
                cur = gl.new_cur
                n_cur = cur.shape[1]

        plan.M = n_cur
        plan.gather_map, plan._inv, plan.pad_to = cur, inv, pad_to
        merged = plan.merged if (materialize or cur is None) else None             # cur None: F == 1, a view
        if args["merge_global"]:
            if anchors_out is not None:
                module.global_tokens = anchors_out
                if anchors_pos is not None:
                    anchors_out._vtm_pos = anchors_pos
                if anchors_cid is not None:
                    tag_content_ids(anchors_out, anchors_cid)
            elif plan.global_level is None:
                # patch.py:82: first chunk of a step stores its local tokens (device-resident, shared
                # with `merged`, which nothing mutates)
                if merged is None:
                    merged = plan.merged
                module.global_tokens = merged[:, :Ml] if merged.shape[1] != Ml else merged
                if _lib.SEED_MATCHER:      # (cur None: a single-frame chunk, the local tokens are the chunk's rows themselves)
                    module.global_tokens._vtm_pos = _lib.anchor_pos(cur, B, Ml, L, tsize, None, xj.device)
            mark_anchors_ready(getattr(module, "global_tokens", None))
            if exchange is not None:
                exchange.publish(xkey, module.global_tokens)

    def m(t: torch.Tensor, **kwarg) -> torch.Tensor:                               # patch.py:84
        tj = join_frame(t.contiguous(), fsize)
        if plan.gather_map is None:
            return tj
        if plan.anchors_in is not None:
            raise RuntimeError("the composed merge map of a global level needs the anchor tokens; "
                               "use the merged_tokens compute_merge returned")
        return _lib.gather_rows(tj, None, plan.gather_map)

    def u(t: torch.Tensor, resid: Optional[torch.Tensor] = None, **kwarg) -> torch.Tensor:   # patch.py:85
        if plan.inv is None:
            t = t[:, :plan.L]                                  # drop the 8-row padding of the attention path
            out = t if resid is None else t + join_frame(resid, fsize)
            return split_frame(out, fsize)
        r = None if resid is None else join_frame(resid.contiguous(), fsize)
        return split_frame(_lib.unmerge_add(t.contiguous(), plan.inv, r), fsize)

    m.plan = plan
    u.plan = plan
    return m, u, merged


# ----------------------------------------------------------------------------------------------------
# attn1 on merged tokens
# ----------------------------------------------------------------------------------------------------
def _pnp_num_inputs(attn: torch.nn.Module) -> Optional[int]:
    """If the reference's ``register_attention_control`` (utils/pnp_utils.py:39-106) replaced
    ``attn.forward`` with its ``sa_forward`` closure, recover ``num_inputs`` from that closure; our own
    ``vidtome_amd.pnp.register_attention_control`` stores it as ``attn.vtm_num_inputs``."""
    n = getattr(attn, "vtm_num_inputs", None)
    if n is not None:
        return int(n)
    fwd = attn.__dict__.get("forward")
    clo = getattr(fwd, "__closure__", None)
    if fwd is not None and clo:
        cells = dict(zip(fwd.__code__.co_freevars, clo))
        if "num_inputs" in cells:
            return int(cells["num_inputs"].cell_contents)
    return None


def _pnp_share_groups(attn: torch.nn.Module) -> int:
    """1, or the number of batch groups that share the source group's attention probabilities at this timestep
    (pnp_utils.py:57-67)."""
    sched = getattr(attn, "injection_schedule", None)
    if sched is not None:
        t = getattr(attn, "t", None)
        if t is not None and (t in sched or t == 1000):                 # pnp_utils.py:57-58
            n = _pnp_num_inputs(attn)
            if n is None:
                raise RuntimeError("PnP injection is registered on attn1 but num_inputs is unknown")
            return n
    return 1


def _built_here(device):
    """(event, stream id) behind a cached device tensor that was just built on the current stream: a chunk on ANOTHER stream may
    be the next to use it (scheduler.run_step(streams=...): the first two chunks of a run meet the caches empty) ..."""
    if not torch.cuda.is_available() or torch.device(device).type != "cuda":
        return None
    st = torch.cuda.current_stream(device)
    ev = torch.cuda.Event()
    ev.record(st)
    return ev, st.cuda_stream


def _built_before(mark, device) -> None:
    """... and waits for the build on the device before its own kernels read the tensor (same stream: nothing to do)."""
    if mark is not None:
        cur = torch.cuda.current_stream(device)
        if cur.cuda_stream != mark[1]:
            cur.wait_event(mark[0])


def _linear(m: torch.nn.Module, dtype=None, device=None):
    """(contiguous weight, bias, key) of a projection the caller's predicate accepted (lora.linear_params: its own tensors,
    or the folded ones of a LoRA layer), converted to ``dtype`` / ``device`` when given.  Every weight / bias read of the
    fused path goes through here: a direct `.weight` read of a LoRA wrapper would be its BASE weight and silently drop the
    adapter."""
    p = lora.linear_params(m, dtype, device)
    if p is None:
        raise RuntimeError(f"vidtome_amd: {type(m).__name__} is not a projection the fused path can read")
    w, b, key = p
    return w.contiguous(), b, key


def _apply_linear(m: torch.nn.Module, x: torch.Tensor, dtype=None) -> torch.Tensor:
    """`m(x)` for a projection lora.linear_params reads, as a library GEMM: F.linear with its (effective) weight and bias --
    exactly what a plain Linear's forward computes -- or with both converted to ``dtype`` (the tokens') when given."""
    w, b, _ = _linear(m, dtype)
    return F.linear(x, w, b)


def _scale(attn: torch.nn.Module, C: int) -> float:
    """The softmax scale of an attention module over C channels: its own, or head_dim ** -0.5."""
    return getattr(attn, "scale", None) or (C // attn.heads) ** -0.5


def _plain_layernorm(norm: torch.nn.Module, x: torch.Tensor) -> bool:
    """A plain torch.nn.LayerNorm over the channel axis of ``x`` whose weight and bias, where present, are of the tokens'
    dtype -- what vtm_layernorm / vtm_layernorm_panels compute.  (Each caller adds the widths and dtypes its kernel takes.)"""
    return (type(norm) is torch.nn.LayerNorm and len(norm.normalized_shape) == 1 and norm.normalized_shape[0] == x.shape[-1]
            and (norm.weight is None or norm.weight.dtype == x.dtype) and (norm.bias is None or norm.bias.dtype == x.dtype))


def _fused_weights(attn: torch.nn.Module, dtype, device):
    """[Wq; Wk] stacked once per module (one projection GEMM for q and k), cached on the module."""
    cache = attn.__dict__.get("_vtm_wcache")
    wq, bq, kq = _linear(attn.to_q)
    wk, bk, kk = _linear(attn.to_k)
    key = (kq, kk, dtype, device)
    if cache is None or cache[0] != key:
        wqk = torch.cat([wq, wk], dim=0).to(device=device, dtype=dtype).contiguous()
        bqk = None
        if bq is not None or bk is not None:
            zq = bq if bq is not None else torch.zeros_like(wq[:, 0])
            zk = bk if bk is not None else torch.zeros_like(wk[:, 0])
            bqk = torch.cat([zq, zk]).to(device=device, dtype=dtype)
        cache = (key, wqk, bqk, _built_here(device))
        attn.__dict__["_vtm_wcache"] = cache
    _built_before(cache[3], device)
    return cache[1], cache[2]


_HEAD_DIMS = (8, 16, 32, 40, 64, 80, 96, 128, 160)          # instantiations of attention_kernel (attention.hip)
_PLAIN_PROCESSORS = ("AttnProcessor", "AttnProcessor2_0", "XFormersAttnProcessor")
_ATTN1_PROCESSORS = _PLAIN_PROCESSORS + tuple(pag.PROCESSORS)   # attn1 alone: a PAG processor there is understood (pag.py)
_warned = set()


def _warn_once(key: str, msg: str) -> None:
    if key not in _warned:
        _warned.add(key)
        import warnings
        warnings.warn(msg, stacklevel=3)


def _readable_linear(m) -> bool:
    """A projection the fused path may read through `lora.linear_params`: a plain Linear (or Diffusers' LoRA-compatible
    subclass with no LoRA attached), or a LoRA layer whose adapters fold into one Linear (vidtome_amd/lora.py).  Other
    wrappers compute more than `x W^T + b` and keep the module path."""
    return lora.recognise(m) is not None


def _out_linear(attn: torch.nn.Module):
    to_out = attn.to_out
    return to_out[0] if isinstance(to_out, (torch.nn.ModuleList, torch.nn.Sequential, list, tuple)) else to_out  # pnp_utils.py:41-45


def fused_attention_ok(attn: torch.nn.Module, x: torch.Tensor, self_attn: bool = True,
                       processors=_PLAIN_PROCESSORS) -> bool:
    """True when `attn(x)` is exactly `to_out[0](softmax(to_q(x) to_k(.)^T * scale) to_v(.))` -- the arithmetic of
    utils/pnp_utils.py:47-95 -- so that the fused path (projection GEMMs + vtm_attention) computes what the module
    would.  Anything else (LoRA / PEFT projections, custom processors or a replaced forward, group / cross norms,
    output rescaling or an inner residual, head dims without a kernel instantiation, dropout in training) makes the
    patched block call the module itself on the merged tokens, like the reference does (patch.py:157-162)."""
    if not (x.is_cuda and x.dim() == 3 and x.dtype in (torch.float16, torch.bfloat16, torch.float32)):
        return False
    if not all(hasattr(attn, a) for a in ("to_q", "to_k", "to_v", "to_out", "heads")):
        return False
    if not all(_readable_linear(m) for m in (attn.to_q, attn.to_k, attn.to_v, _out_linear(attn))):
        return False
    C = x.shape[-1]
    if lora.base_linear(attn.to_q).out_features != C or C % attn.heads or (C // attn.heads) not in _HEAD_DIMS:
        return False
    if any(getattr(attn, a, None) is not None for a in ("group_norm", "spatial_norm", "norm_cross", "norm_q", "norm_k")):
        return False
    if getattr(attn, "rescale_output_factor", 1.0) != 1.0 or getattr(attn, "residual_connection", False):
        return False
    proc = getattr(attn, "processor", None)
    if proc is not None and type(proc).__name__ not in processors:
        return False                              # (``processors``: the IP-Adapter path names its own, ip_cross_call)
    if "forward" in attn.__dict__ and not (self_attn and _pnp_num_inputs(attn) is not None):
        return False                              # replaced forward: only the PnP closure is understood
    to_out = attn.to_out
    if attn.training and isinstance(to_out, (torch.nn.ModuleList, torch.nn.Sequential)) and len(to_out) > 1 \
            and getattr(to_out[1], "p", 0.0) != 0.0:
        return False
    return True


# How attn1's projections are computed.  "rows": vtm_linear_rows, GEMMs whose A rows are fetched through the composed
# merge map (no merged tensor, V produced channel-major; the C ABI then covers attn1 end to end).  "blas": library GEMMs
# (torch -> hipBLASLt) over materialised merged tokens.  "auto" (default) picks per site what measures faster on MI355X
# (profiles/r02_*): the gather-fused kernel at C <= 320 (cfg-2 top blocks: k 73 vs 99 us, v^T 65 vs 81 us), the library
# at C >= 640, where its 256 x 256 macro-tiles move half the operand bytes of the 128 x 160 tiles of linear.hip.
PROJ_MODE = os.environ.get("VIDTOME_PROJ", "auto")
FUSED_PROJ = PROJ_MODE != "blas"                      # (tests toggle this to compare the two paths)
# Round 3: at C >= 640 "auto" no longer leaves the C ABI either -- the projections are PANEL GEMMs (csrc/ff.hip: the merged
# rows are gathered straight into the k-panel layout, vtm_gather_panels, and k / v^T / q / out are vtm_linear_panels
# launches; the un-merged C = 1280 sites take their panels from the LayerNorm itself).  VIDTOME_PROJ=panels forces that
# path everywhere, "blas" keeps the library GEMMs of rounds 1-2.


def _proj_dtypes_ok(attn: torch.nn.Module, dtype) -> bool:
    """All four projection weights (and the biases that exist) are of the tokens' dtype: the in-house projection kernels
    read raw 16-bit words and take the dtype from the TOKENS (a mixed-dtype module -- an fp32 to_out next to fp16
    to_q / to_k / to_v, say -- would otherwise be packed and multiplied as garbage instead of leaving the fused path)."""
    for lin in (attn.to_q, attn.to_k, attn.to_v, _out_linear(attn)):
        if not _linear_dtype_ok(lin, dtype):
            return False
    return True


def _linear_dtype_ok(lin: torch.nn.Module, dtype) -> bool:
    """The (effective) weight and bias of a projection are of `dtype` (a LoRA fold is made in its base weight's dtype; the
    adapters themselves may be of any dtype)."""
    base = lora.base_linear(lin)
    return base.weight.dtype == dtype and (base.bias is None or base.bias.dtype == dtype)


def _has_bias(lin: torch.nn.Module) -> bool:
    """The effective Linear has a bias (a PEFT adapter's lora_B bias folds into it)."""
    return lora.linear_params(lin)[1] is not None


def _attn1_kwargs(cross_attention_kwargs) -> dict:
    """What of ``cross_attention_kwargs`` a plain processor on attn1 gets to see.  ``ip_adapter_masks`` is read by the
    IP-Adapter processors on attn2 alone: Diffusers' ``Attention.forward`` drops, without a word, the arguments a processor's
    ``__call__`` does not take, and the plain processors ``fused_attention_ok`` accepts do not take it -- so region masks
    do not send attn1 to its module forward.  (Whenever the module IS called it gets the kwargs untouched.)"""
    return {k: v for k, v in (cross_attention_kwargs or {}).items() if k != "ip_adapter_masks"}


def _fp32_projections(block: torch.nn.Module) -> bool:
    """The block's ``fp32_projections`` opt-in (``update_patch(model, fp32_projections=True)``)."""
    return getattr(block, "fp32_projections", False) is True


def _pag_batch(block: torch.nn.Module, x: torch.Tensor) -> int:
    """The leading batch attn1 sees for block tokens like ``x`` (B F, N, C): ``apply_patch``'s batch_size at a site that merges
    (a sample is a joined chunk), the B F frame rows at one that does not (or before anything is patched)."""
    info = getattr(block, "_tome_info", None)
    if info is None or unmerged_site(block, x):
        return x.shape[0]
    return info["args"]["batch_size"]


def _pag_org(attn: torch.nn.Module, B: int) -> Optional[int]:
    """n_org of a perturbed-attention attn1 call over a leading batch of B (pag.split), None for a plain call.  The processor
    form never gets here with a batch that does not split (``attn1_route``); the registered form raises."""
    groups = pag.groups_of(attn)
    return None if groups is None else pag.split(B, groups)[0]


def _pag_check(block: torch.nn.Module, x: torch.Tensor, route: str) -> None:
    """Before the first launch of a fused segment: a registered perturbed-attention batch that does not split raises."""
    if route != "module":
        _pag_org(block.attn1, _pag_batch(block, x))


def _lead(t: Optional[torch.Tensor], n: Optional[int]) -> Optional[torch.Tensor]:
    """The first n samples of a per-sample operand (a contiguous view), the operand itself for n None."""
    return t if t is None or n is None else t[:n]


def _tail(t: Optional[torch.Tensor], n: int) -> Optional[torch.Tensor]:
    """The samples from n on (a contiguous view)."""
    return None if t is None else t[n:]


def attn1_route(block: torch.nn.Module, x: torch.Tensor, encoder_hidden_states=None, attention_mask=None,
                cross_attention_kwargs=None, gate_msa=None) -> str:
    """How the block computes ``attn1`` on tokens like ``x`` (their device, rank, dtype and width are read).  Launches nothing
    (but the first look at a LoRA-adapted to_v folds its adapters, lora.linear_params).
      "module"  attn1's own forward on the materialised merged tokens, like the reference (patch.py:157-162): a masked call,
                processor kwargs, attn1 as a cross-attention, or a module that is not the plain arithmetic
                (``fused_attention_ok``).  SD never does the first three on attn1
      "rows"    self_attention_rows on vtm_linear_rows: fp16 / bf16 tokens, C % 32 == 0
      "panels"  self_attention_panels (vtm_gather_panels + vtm_linear_panels; the un-merged sites take
                unmerged_self_attention_residual): fp16 / bf16 tokens, C % 64 == 0, no bias on to_v (V^T = W_v X^T is computed
                with the roles of the operands swapped)
      "f32"     self_attention_rows on vtm_linear_f32: fp32 tokens with C % 8 == 0 and the block's ``fp32_projections``
      "blas"    self_attention: library GEMMs over materialised merged tokens
    The three hand-written projection paths ask that all four projection weights are of the tokens' dtype.
    Perturbed attention (pag.groups_of: a PAG processor on attn1, or a registered block) keeps the route of the plain block --
    each body then runs its attention on the org samples only -- except with an AdaLayerNormZero gate (``gate_msa``), under PnP
    sharing, or, in the processor form, with a batch that does not split into the processor's groups: "module"."""
    attn = block.attn1
    if attention_mask is not None or _attn1_kwargs(cross_attention_kwargs) \
            or (encoder_hidden_states is not None and block.only_cross_attention) \
            or not fused_attention_ok(attn, x, processors=_ATTN1_PROCESSORS):
        return "module"
    groups = pag.groups_of(attn)
    if groups is not None and (gate_msa is not None or _pnp_share_groups(attn) != 1
                               or (pag.registered(attn) is None and _pag_batch(block, x) % groups)):
        return "module"
    C = x.shape[-1]
    if x.dtype == torch.float32:
        return "f32" if _fp32_projections(block) and C % 8 == 0 and _proj_dtypes_ok(attn, torch.float32) else "blas"
    if not _proj_dtypes_ok(attn, x.dtype):                 # fp16 / bf16: fused_attention_ok admits no other dtype
        return "blas"
    if FUSED_PROJ and C % 32 == 0 and (PROJ_MODE == "rows" or (PROJ_MODE == "auto" and C <= 320)):
        return "rows"
    if PROJ_MODE in ("auto", "panels") and C % 64 == 0 and not _has_bias(attn.to_v):
        return "panels"
    return "blas"


def _attn1_params(attn: torch.nn.Module, C: int, q_rows: Optional[torch.Tensor], aligned: bool):
    """(heads, scale, share groups) of an attn1 call, before any device work.  Under PnP sharing every group reads the source
    sample's q / k (and its q_count): per-sample query rows are the same rows only when the matching was aligned."""
    share = _pnp_share_groups(attn)
    if share != 1 and q_rows is not None and not aligned:
        raise RuntimeError("vidtome_amd: q_rows with PnP shared probabilities need every sample of a group to have the same "
                           "rows -- align_batch matching (pass aligned=True)")
    return attn.heads, _scale(attn, C), share


def _attn1_core(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, M: int, Mq: Optional[int], scale: float,
                share: int, q_count: Optional[torch.Tensor] = None, k_fold=None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The attention core of attn1 over M keys: every row a query (``Mq`` None, vtm_attention), or Mq query rows of their
    own -- the first q_count[b] of them live -- and / or folded keys (vtm_attention_kv).  ``out``: the leading samples of a
    larger buffer to write into (perturbed attention: the perturbed samples' V follows, ``_pag_out``)."""
    kw = {} if out is None else {"out": out}
    if k_fold is not None:                                 # (folded keys: never under sharing)
        return _lib.attention_kv(q, k, vt, heads, M if Mq is None else Mq, M, scale, q_count=q_count, k_fold=k_fold, **kw)
    if Mq is None:
        return _lib.attention(q, k, vt, heads, M, scale, share, **kw)
    return _lib.attention_kv(q, k, vt, heads, Mq, M, scale, q_count=q_count, share_groups=share, **kw)


def _pag_out(B: int, rows: int, valid: int, C: int, dtype, device) -> torch.Tensor:
    """The (B, rows, C) buffer the output projection of a perturbed-attention batch reads: the cores write the org samples'
    attention output into its head, the perturbed samples' V goes into its tail.  Rows >= ``valid`` are padding nobody
    writes: zero, as the cores' own result has them."""
    o = torch.empty((B, rows, C), dtype=dtype, device=device)
    if rows != valid:
        o[:, valid:].zero_()
    return o


def _panel_weight(lin: torch.nn.Module):
    """(weight as k-panels, fp32 bias or None) of a Linear, cached on the module."""
    w, b, key = _linear(lin)
    return _packed(lin, "rows", key, w.device, lambda: (_lib.to_panels(w.detach().contiguous()),
                                                       None if b is None else b.detach().float().contiguous()))


def self_attention_panels(attn: torch.nn.Module, x0: torch.Tensor, x1: Optional[torch.Tensor], rows: Optional[torch.Tensor],
                          q_rows: Optional[torch.Tensor] = None, q_count: Optional[torch.Tensor] = None,
                          aligned: bool = False, n_org: Optional[int] = None) -> torch.Tensor:
    """``attn1(merged)`` like self_attention_rows, with the projections as panel GEMMs: the merged rows (and the live-query
    rows) are gathered ONCE into the k-panel layout, sample b at rows b * Mpad (Mpad = M rounded up to 256), and
        k    = X W_k^T                     one launch over all samples  -> (B, Mpad, C)
        v^T  = W_v X_b^T                   one launch per sample, the weight as "token" operand -> (B, C, Mpad): no transpose
        q    = X_q W_q^T, out = O W_o^T + b
    Returns (B, Mq rounded up to 256, C); rows >= Mq (or the per-sample q_count) are not meaningful.  ``aligned``: the
    matching was align_batch's (``_attn1_params``).  ``n_org`` (perturbed attention, ``_pag_org``): all of the above for the
    first n_org samples only; the others' rows of O are V = X_q W_v^T, one gather and one GEMM of their own."""
    Ball, _, C = x0.shape
    M = x0.shape[1] if rows is None else rows.shape[1]
    heads, scale, share = _attn1_params(attn, C, q_rows, aligned)
    B = Ball if n_org is None else n_org
    y0, y1, yrows, yq = _lead(x0, n_org), _lead(x1, n_org), _lead(rows, n_org), _lead(q_rows, n_org)
    Mpad = _lib.panel_rows(M)
    xp = _lib.gather_panels(y0, y1, yrows, None, M)                      # (C / 8, B * Mpad, 8)
    wq, bq = _panel_weight(attn.to_q)
    wk, bk = _panel_weight(attn.to_k)
    wv, _ = _panel_weight(attn.to_v)
    k_op = _lib.linear_panels(xp, B * Mpad, wk, C, bk).view(B, Mpad, C)
    vt = torch.empty((B, C, Mpad), dtype=x0.dtype, device=x0.device)
    M8 = (M + 7) // 8 * 8
    for b in range(B):
        _lib.linear_panels(wv, C, xp[:, b * Mpad:(b + 1) * Mpad], M8, None, out=vt[b])
    Mq, Mqpad, qp = None, Mpad, xp
    if q_rows is not None:
        Mq = q_rows.shape[1]
        Mqpad = _lib.panel_rows(Mq)
        qp = _lib.gather_panels(y0, y1, yrows, yq, Mq)
    q_op = _lib.linear_panels(qp, B * Mqpad, wq, C, bq).view(B, Mqpad, C)
    if n_org is None:
        o = _attn1_core(q_op, k_op, vt, heads, M, Mq, scale, share, q_count)
    else:
        o = _pag_out(Ball, Mqpad, M if Mq is None else Mq, C, x0.dtype, x0.device)
        _attn1_core(q_op, k_op, vt, heads, M, Mq, scale, share, _lead(q_count, n_org), out=o[:n_org])
        vp = _lib.gather_panels(_tail(x0, n_org), _tail(x1, n_org), _tail(rows, n_org), _tail(q_rows, n_org),
                                M if Mq is None else Mq)
        _lib.linear_panels(vp, (Ball - n_org) * Mqpad, wv, C, None, out=o[n_org:].view(-1, C))
    wo, bo = _panel_weight(_out_linear(attn))
    op = _lib.to_panels(o.view(Ball * Mqpad, C))
    return _lib.linear_panels(op, Ball * Mqpad, wo, C, bo).view(Ball, Mqpad, C)


def unmerged_site(block: torch.nn.Module, x: torch.Tensor) -> bool:
    """patch.py:15-17,27: the block is too deep in the UNet to merge (downsample > max_downsample)."""
    info = block._tome_info
    if info["size"] is None:
        return False
    downsample = int(math.ceil(math.sqrt((info["size"][0] * info["size"][1]) // x.shape[1])))
    return downsample > info["args"]["max_downsample"]


def sag_registered(block: torch.nn.Module) -> bool:
    """``sag.register_self_attention_guidance`` selected the block: its attn1 leaves ``attn1_key_mass``."""
    return block.__dict__.get("vtm_sag") is True


def _sag_check(block: torch.nn.Module, x: torch.Tensor) -> None:
    """Before the first launch of a registered block's attn1 segment: the key mass is that of the per-frame attention of a
    plain attn1 call, and an edit is never silently dropped -- anything else raises."""
    who = "vidtome_amd: this block is registered for self-attention guidance (register_self_attention_guidance) but "
    if not unmerged_site(block, x):
        raise RuntimeError(who + "its site merges tokens: the key mass would be over merged rows, not the frame's token grid "
                                 "(SAG at merged sites is not supported; register the mid block)")
    if x.shape[1] > _lib.KEY_MASS_MAX_KEYS:
        raise RuntimeError(who + f"its frames have {x.shape[1]} tokens: vtm_attention_key_mass takes at most "
                                 f"{_lib.KEY_MASS_MAX_KEYS} keys (a workgroup's column accumulators live in LDS)")
    if pag.groups_of(block.attn1) is not None:
        raise RuntimeError(who + "its attn1 is under perturbed attention (a PAG processor or register_perturbed_attention): "
                                 "the perturbed samples have no attention map (SAG and PAG on one block are not supported)")
    if _pnp_share_groups(block.attn1) != 1:
        raise RuntimeError(who + "its attn1 shares the source sample's probabilities at this timestep (PnP injection): the "
                                 "groups have no map of their own (SAG and PnP on one block are not supported)")


def _key_mass_torch(q: torch.Tensor, k: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """fp32 torch restatement of vtm_attention_key_mass: sum over the queries of the head-averaged softmax, (B, Mk).  Head by
    head: no (B, heads, N, N) tensor exists."""
    B, _, C = q.shape
    d = C // heads
    acc = torch.zeros((B, k.shape[1]), dtype=torch.float32, device=q.device)
    for h in range(heads):
        s = torch.matmul(q[:, :, h * d:(h + 1) * d].float(), k[:, :, h * d:(h + 1) * d].float().transpose(1, 2)) * scale
        acc += torch.softmax(s, dim=-1).sum(1)
    return acc / heads


def _module_path_key_mass(attn: torch.nn.Module, x: torch.Tensor) -> Optional[torch.Tensor]:
    """The key mass of an attn1 call whose body does not hold 16-bit q | k rows for the kernel ("rows", "f32", "blas",
    "module"): to_q / to_k through lora.linear_params on norm1's output, in fp32, then the torch restatement.  None (one
    warning) when the projections are not readable or something stands between them and the scores; never raises."""
    try:
        ok = (x.dim() == 3 and all(hasattr(attn, a) for a in ("to_q", "to_k", "heads"))
              and _readable_linear(attn.to_q) and _readable_linear(attn.to_k)
              and not any(getattr(attn, a, None) is not None for a in ("group_norm", "spatial_norm", "norm_q", "norm_k"))
              and lora.base_linear(attn.to_q).out_features % attn.heads == 0)
        if ok:
            with torch.no_grad():
                xf = x.float()
                q = _apply_linear(attn.to_q, xf, torch.float32)
                k = _apply_linear(attn.to_k, xf, torch.float32)
                return _key_mass_torch(q, k, attn.heads, _scale(attn, q.shape[-1]))
    except Exception as e:   # (a forward never fails for its map)
        _warn_once("sag-failed", f"vidtome_amd: attn1_key_mass is None: the key mass of an attn1 call failed ({e})")
        return None
    _warn_once("sag-unreadable", "vidtome_amd: attn1_key_mass is None for an attn1 call whose to_q / to_k are not plain "
                                 "projections onto the scores")
    return None


def unmerged_self_attention_ok(block: torch.nn.Module, x: torch.Tensor, route: Optional[str] = None) -> bool:
    """``unmerged_self_attention_residual`` may run: the "panels" route (``route``: what ``attn1_route`` answered for a plain
    attn1 call, when the caller has asked already) behind a plain norm1, without PnP sharing, at a site that does not merge."""
    # (any token count: q and k are row ranges of the dense (BF, N, 3C) projection -- the cores address a row as
    # (sample * N + row) * ld with ld % 8 == 0 -- and only V^T needs a padded row, which vtm_transpose_cols writes)
    return ((route or attn1_route(block, x)) == "panels" and _plain_layernorm(block.norm1, x)
            and _pnp_share_groups(block.attn1) == 1 and unmerged_site(block, x))


def unmerged_self_attention_residual(block: torch.nn.Module, hidden_states: torch.Tensor) -> torch.Tensor:
    """patch.py:139-169 at a site that does not merge (per-frame attention): ``attn1(norm1(h)) + h`` with norm1 writing
    k-panels (its output is only read by the three projections), ONE GEMM for q | k | v over all frames, the attention core
    per frame, and the output projection with bias and residual in its epilogue.  The caller checked
    ``unmerged_self_attention_ok``.
    Perturbed attention (``_pag_org`` over the BF frame rows: the batch is frame-minor per sample, the last sample's frames
    are the perturbed ones): norm1 runs once per part, q | k | v and the core for the org frames only, and the perturbed
    frames' rows of the core's output buffer are V, a GEMM with to_v's panel weight alone."""
    attn, norm = block.attn1, block.norm1
    BF, N, C = hidden_states.shape
    heads, scale = attn.heads, _scale(attn, C)
    hs = hidden_states.contiguous()
    n = BF * N
    sag = sag_registered(block)
    if sag:
        _sag_check(block, hidden_states)                   # (no perturbed attention below: n_org is None)
    n_org = _pag_org(attn, BF)

    qkv_params = [_linear(m) for m in (attn.to_q, attn.to_k, attn.to_v)]

    def pack_qkv():
        w = torch.cat([p[0] for p in qkv_params], dim=0).detach().contiguous()
        bs = [p[1] for p in qkv_params]
        b = None if all(x is None for x in bs) else torch.cat(
            [torch.zeros(C, device=w.device) if x is None else x.detach().float() for x in bs]).contiguous()
        return _lib.to_panels(w), b
    wqkv, bqkv = _packed(attn, "qkv", tuple(p[2] for p in qkv_params), qkv_params[0][0].device, pack_qkv)
    wo, bo = _panel_weight(_out_linear(attn))
    if n_org is not None:
        # (a part of its own each: a panel GEMM fetches whole 256-row tiles from where its operand starts, which a row range
        # that begins in the middle of norm1's panels does not have behind its last rows)
        ho, hp = hs[:n_org], hs[n_org:]
        no = n_org * N
        qkv = _lib.linear_panels(_lib.layernorm_panels(ho, norm.weight, norm.bias, norm.eps), no, wqkv, 3 * C,
                                 bqkv).view(n_org, N, 3 * C)
        vt = _lib.transpose_cols(qkv, 2 * C, C)
        o = torch.empty((BF, N, C), dtype=hs.dtype, device=hs.device)
        _lib.attention(qkv[:, :, :C], qkv[:, :, C:2 * C], vt, heads, N, scale, 1, out=o[:n_org])
        wv, bv = _panel_weight(attn.to_v)
        _lib.linear_panels(_lib.layernorm_panels(hp, norm.weight, norm.bias, norm.eps), n - no, wv, C, bv,
                           out=o[n_org:].view(n - no, C))
        return _lib.linear_panels(_lib.to_panels(o.view(n, C)), n, wo, C, bo, resid=hs.view(n, C)).view(BF, N, C)
    xp = _lib.layernorm_panels(hs, norm.weight, norm.bias, norm.eps)
    qkv = _lib.linear_panels(xp, n, wqkv, 3 * C, bqkv).view(BF, N, 3 * C)
    # (BF, C, N rounded up to 8): V channel-major for the PV contraction, the key columns past N written as zeros
    vt = _lib.transpose_cols(qkv, 2 * C, C)
    if sag:
        # one launch on the q | k row ranges the core reads (N is inside the kernel's key limit: _sag_check)
        with torch.no_grad():
            block.attn1_key_mass = _lib.attention_key_mass(qkv[:, :, :C], qkv[:, :, C:2 * C], heads, N, N, scale)
    o = _lib.attention(qkv[:, :, :C], qkv[:, :, C:2 * C], vt, heads, N, scale, 1)
    op = _lib.to_panels(o.view(n, C))
    return _lib.linear_panels(op, n, wo, C, bo, resid=hs.view(n, C)).view(BF, N, C)


def self_attention_segment(block: torch.nn.Module, hidden_states: torch.Tensor, encoder_hidden_states=None,
                           attention_mask=None, cross_attention_kwargs=None, plan_to: Optional[list] = None) -> torch.Tensor:
    """patch.py:146-169 for the plain-LayerNorm block: norm1 -> compute_merge -> attn1 -> unmerge -> + residual.
    ``plan_to``: a list of the caller's that receives the MergePlan of this call's compute_merge (None where nothing merges)."""
    route = attn1_route(block, hidden_states, encoder_hidden_states, attention_mask, cross_attention_kwargs)
    _pag_check(block, hidden_states, route)
    if unmerged_self_attention_ok(block, hidden_states, route):
        return unmerged_self_attention_residual(block, hidden_states)
    norm_hidden_states = layer_norm(block.norm1, hidden_states)
    # (the route reads the tokens' dtype: a norm1 that changes it is routed on its output)
    return patched_self_attention_segment(block, hidden_states, norm_hidden_states, encoder_hidden_states, attention_mask,
                                          cross_attention_kwargs, None,
                                          route=route if norm_hidden_states.dtype == hidden_states.dtype else None,
                                          plan_to=plan_to)


def cross_attention_segment(block: torch.nn.Module, hidden_states: torch.Tensor, encoder_hidden_states, encoder_attention_mask,
                            cross_attention_kwargs, timestep, plan: Optional["MergePlan"]) -> torch.Tensor:
    """patch.py:171-185: norm2 -> attn2 -> + residual on the body ``attn2_route`` and ``cross_merge_route`` name.  ``plan``:
    the MergePlan of this forward's attn1 segment (None: nothing merged, or nobody asked for it)."""
    cross_attention_kwargs = cross_attention_kwargs if cross_attention_kwargs is not None else {}
    maps = block if getattr(block, "vtm_attention_maps", False) else None      # maps.register_attention_maps
    words = local_blend_of(block)                                              # blend.register_local_blend
    control = cross_control(block)                                             # p2p.register_cross_attention_control
    route = attn2_route(block, hidden_states, encoder_hidden_states, encoder_attention_mask, cross_attention_kwargs, control)
    if cross_merge_route(block, hidden_states, plan, route, encoder_hidden_states,
                         encoder_attention_mask) == "merged-panels":           # attn2 on the merged local tokens
        return merged_cross_attention_residual(block, hidden_states, encoder_hidden_states, plan)
    if route.frame == "panels":
        return norm_cross_attention_residual(block.norm2, block.attn2, hidden_states, encoder_hidden_states, route.ip,
                                             encoder_attention_mask, maps, words, control)
    if route.frame == "f32":
        return norm_cross_attention_f32(block.norm2, block.attn2, hidden_states, encoder_hidden_states, probs_to=maps,
                                        words_to=words)
    # "blas", "module": both read normed tokens
    norm_hidden_states = (block.norm2(hidden_states, timestep) if block.use_ada_layer_norm
                          else layer_norm(block.norm2, hidden_states))
    if control is None and norm_hidden_states.dtype != hidden_states.dtype:
        # (the route reads the tokens' dtype: a norm2 that changes it is routed on its output)
        route = attn2_route(block, norm_hidden_states, encoder_hidden_states, encoder_attention_mask, cross_attention_kwargs,
                            normed=True)
    return cross_attention(block.attn2, norm_hidden_states, encoder_hidden_states, encoder_attention_mask, probs_to=maps,
                           words_to=words, ctl=control, route=route, **cross_attention_kwargs) + hidden_states


def self_attention_rows(attn: torch.nn.Module, x0: torch.Tensor, x1: Optional[torch.Tensor],
                        rows: Optional[torch.Tensor], q_rows: Optional[torch.Tensor] = None,
                        q_count: Optional[torch.Tensor] = None, plan: Optional["MergePlan"] = None,
                        fp32_core: bool = False, aligned: bool = False, n_org: Optional[int] = None) -> torch.Tensor:
    """``attn1(merged)`` (patch.py:157-162; arithmetic of pnp_utils.py:47-95) with ``merged[b, i] = pool[b, rows[b, i]]``
    never materialised: every projection is a GEMM that fetches its A rows through the composed merge map (pool = x0 | x1,
    ``rows`` None = the rows of x0 as they are), k and v for all M rows (v channel-major, what the PV contraction reads),
    q -- and the output projection -- only for the ``q_rows`` positions when given (the rows unmerge() reads).
    Returns (B, Mq rounded up to 8, C); rows >= Mq are not meaningful.  ``aligned``: the matching was align_batch's
    (``_attn1_params``).
    fp16 / bf16 tokens: vtm_linear_rows.  With a ``plan`` whose anchors carried content ids and a head dim that has spare
    contraction slots (40), k and v are projected for the duplicate-free key list only (MergePlan.key_fold) and every key
    carries log2 of its multiplicity.
    fp32 tokens (the block's ``fp32_projections``): vtm_linear_f32, which writes q / k / V^T in fp32 for the fp32 core
    (``fp32_core``, the block's ``fp32_attention``) or rounds them once to fp16 at its store for the fp16 core; the output
    projection reads the core's output as fp32.  fp32 keys are never folded.
    ``n_org`` (perturbed attention, ``_pag_org``): q, k, V^T, the key fold and the core for the first n_org samples only; the
    others' rows of the core's output buffer are V = to_v at the rows the output projection reads (the ``q_rows`` positions,
    or all M), token-major from the same GEMM -- in fp32 for fp32 tokens, whichever core the org samples take."""
    B, _, C = x0.shape
    M = x0.shape[1] if rows is None else rows.shape[1]
    heads, scale, share = _attn1_params(attn, C, q_rows, aligned)
    dt = x0.dtype
    f32 = dt == torch.float32
    gemm, out_kw = _lib.linear_rows, {}
    if f32:
        gemm, out_kw = _lib.linear_f32, {"out_dtype": torch.float32 if fp32_core else torch.float16}
    wqk, bqk = _fused_weights(attn, dt, x0.device)
    wv, bv, _ = _linear(attn.to_v, dt)
    fold = None
    if not f32 and plan is not None and rows is not None and share == 1 and (C // heads) in (8, 40):
        fold = plan.key_fold(dt, n_org)
    key_sel = k_fold = None
    if fold is not None:
        key_sel, k_bias, k_count = fold
        k_fold = (k_count, k_bias)
    y0, y1, yrows, yq = _lead(x0, n_org), _lead(x1, n_org), _lead(rows, n_org), _lead(q_rows, n_org)
    Mq = M if q_rows is None else q_rows.shape[1]
    o = core_out = None
    if n_org is not None:
        Mqp = (Mq + 7) // 8 * 8
        # (fp32 tokens on the fp16 core: the core's fp16 output is widened into the fp32 buffer the output projection reads)
        o = _pag_out(B, Mqp, Mq, C, dt, x0.device)
        if not f32 or fp32_core:
            core_out = o[:n_org]
    vt = gemm(y0, y1, yrows, key_sel, M, wv, bv, transposed=True, **out_kw)                        # (B, C, Mp)
    if q_rows is None and fold is None:
        qk = gemm(y0, y1, yrows, None, M, wqk, bqk, **out_kw)                                      # (B, Mp, 2C): q | k
        oc = _attn1_core(qk[:, :, :C], qk[:, :, C:], vt, heads, M, None, scale, share, out=core_out)
    else:
        k_op = gemm(y0, y1, yrows, key_sel, M, wqk[C:], None if bqk is None else bqk[C:], **out_kw)
        q_op = gemm(y0, y1, yrows, yq, Mq, wqk[:C], None if bqk is None else bqk[:C], **out_kw)
        oc = _attn1_core(q_op, k_op, vt, heads, M, Mq, scale, share, _lead(q_count, n_org), k_fold, out=core_out)
    wo, bo, _ = _linear(_out_linear(attn), dt)
    if n_org is None:
        return gemm(oc.float() if f32 else oc, None, None, None, Mq, wo, bo)
    if core_out is None:
        o[:n_org].copy_(oc)
    gemm(_tail(x0, n_org), _tail(x1, n_org), _tail(rows, n_org), _tail(q_rows, n_org), Mq, wv, bv, out=o[n_org:])
    return gemm(o, None, None, None, Mq, wo, bo)


def self_attention(attn: torch.nn.Module, x: torch.Tensor, M: Optional[int] = None,
                   q_rows: Optional[torch.Tensor] = None, q_count: Optional[torch.Tensor] = None,
                   fp32_core: bool = False, aligned: bool = False, n_org: Optional[int] = None) -> torch.Tensor:
    """``attn1(x)`` for self-attention without mask (patch.py:157-162), arithmetic of pnp_utils.py:47-95:
    q,k,v projections -> softmax(q k^T * scale) v per head -> to_out[0] (+ dropout(0)), on MATERIALISED tokens with
    library GEMMs (torch -> hipBLASLt) for the projections: the path of fp32 models, of channel counts the
    gather-fused GEMM does not take, and of VIDTOME_PROJ=blas (see self_attention_rows for the default).
    x is (B, Mp, C) whose first M rows per sample are the sequence.  With ``q_rows`` (B, Mq) only those rows act
    as queries (every row stays a key / value) and the result is (B, Mq rounded up to 8, C) in q_rows order.
    The caller has checked ``fused_attention_ok(attn, x)``.  ``aligned``: the matching was align_batch's (``_attn1_params``).

    fp16 / bf16 models run everything in their dtype.  fp32 models keep the four projections in fp32 and by default only
    the attention core's operands (q, k, v^T) are rounded to fp16 for the MFMA (fp32 accumulation, fp32 softmax): the
    result is within the 1e-3 class of the fp32 reference, and a warning says so once.  With ``fp32_core`` (the block's
    ``fp32_attention``, set by ``update_patch(model, fp32_attention=True)``) an fp32 model's core runs in fp32 on the f32
    MFMA (csrc/attention_f32.hip), about 16x the matrix time of the fp16 core; the flag means nothing to 16-bit models.
    ``n_org`` (perturbed attention, ``_pag_org``): all of this for the first n_org samples; the others' input of the output
    projection is ``to_v`` of their tokens (of their ``q_rows`` rows), one library GEMM."""
    B, Mp, C = x.shape
    M = Mp if M is None else M
    heads, scale, share = _attn1_params(attn, C, q_rows, aligned)
    if x.shape[1] % 8:
        # keep the transposed V (B, C, Mp) 16-byte aligned per row
        pad = 8 - x.shape[1] % 8
        x = F.pad(x, (0, 0, 0, pad))
        Mp = x.shape[1]
    x_ptb = q_ptb = None
    if n_org is not None:
        x_ptb, q_ptb = x[n_org:], _tail(q_rows, n_org)
        x, q_rows, q_count, B = x[:n_org], _lead(q_rows, n_org), _lead(q_count, n_org), n_org
    core = x.dtype
    if x.dtype != torch.float32 and PROJ_MODE != "blas":
        # an fp16 / bf16 model normally never gets here: say once that (and why) this module's projections are library GEMMs
        _warn_once("lib-proj", f"vidtome_amd: attn1 projections of a {x.dtype} model run as library GEMMs (C = {C}: the "
                               "hand-written projection kernels take C % 32 == 0 with all four projection weights in the "
                               "tokens' dtype and no bias on to_v at C > 320)")
    if x.dtype == torch.float32 and not fp32_core:
        core = torch.float16
        _warn_once("fp32-core", "vidtome_amd: fp32 model -- the self-attention core (QK^T, softmax, PV) runs on the "
                                "fp16 MFMA with fp32 accumulation; projections, matching and merging stay fp32")
    wqk, bqk = _fused_weights(attn, x.dtype, x.device)
    if q_rows is None:
        qk = F.linear(x, wqk, bqk).to(core)                              # (B, Mp, 2C): one GEMM for q and k
        q_op, k_op = qk[:, :, :C], qk[:, :, C:]
    else:
        xq = _lib.gather_rows(x, None, q_rows, pad_to=8)                 # (B, Mqp, C) query tokens
        q_op = F.linear(xq, wqk[:C], None if bqk is None else bqk[:C]).to(core)
        k_op = F.linear(x, wqk[C:], None if bqk is None else bqk[C:]).to(core)
    wv, bv, _ = _linear(attn.to_v, x.dtype)
    if B <= 4:                                                           # merged sites: few long sequences
        vt = torch.empty((B, C, Mp), dtype=x.dtype, device=x.device)     # V^T straight from the GEMM:
        for bi in range(B):                                              # W_v @ x_b^T, transposed operand
            torch.mm(wv, x[bi].t(), out=vt[bi])                          # handled by the BLAS (no copy)
    else:                                                                # un-merged sites: many short ones
        vt = torch.matmul(wv, x.transpose(1, 2))
    if bv is not None:
        vt = vt + bv[None, :, None]
    vt = vt.to(core)
    # (q_count: rows past the count are undefined; the output projection is row-wise, so they stay confined to
    # rows unmerge() never reads)
    o = _attn1_core(q_op, k_op, vt, heads, M, None if q_rows is None else q_rows.shape[1], scale, share, q_count)
    o = o.to(x.dtype)
    if x_ptb is not None:
        xv = x_ptb if q_ptb is None else _lib.gather_rows(x_ptb, None, q_ptb, pad_to=8)
        o = torch.cat([o, F.linear(xv, wv, bv)])
    wo, bo, _ = _linear(_out_linear(attn), o.dtype)
    return F.linear(o, wo, bo)


def _cross_kv(to_k: torch.nn.Module, to_v: torch.nn.Module, enc: torch.Tensor, C: int, mode: str = "panels"):
    """k (B, Mkp, C) and v^T (B, C, Mkp) of conditioning tokens ``enc`` (B, Mkp, D) in the tokens' dtype, Mkp % 8 == 0.
    ``mode`` is the frame's: "panels" -- panel GEMMs when the width allows, else library GEMMs with one warning; "blas" --
    library GEMMs; "f32" -- vtm_linear_f32 on fp32 tokens of any row count (the GEMM pads its output to a multiple of 8)."""
    B, Mkp, D = enc.shape
    dt = enc.dtype
    if mode == "f32":
        return (_lib.linear_f32(enc, None, None, None, Mkp, *_linear(to_k, dt)[:2]),
                _lib.linear_f32(enc, None, None, None, Mkp, *_linear(to_v, dt)[:2], transposed=True))
    panels = mode == "panels"
    if panels and D % 64 == 0 and lora.base_linear(to_k).weight.dtype == dt and lora.base_linear(to_v).weight.dtype == dt:
        ep = _lib.to_panels(enc.reshape(B * Mkp, D))                     # the (few) conditioning tokens: 77 per frame in SD
        wk, bk = _panel_weight(to_k)
        wv, bv = _panel_weight(to_v)
        k = _lib.linear_panels(ep, B * Mkp, wk, C, bk).view(B, Mkp, C)
        vt = _lib.linear_panels(ep, B * Mkp, wv, C, bv).view(B, Mkp, C).transpose(1, 2).contiguous()   # (B, C, Mkp)
    else:
        if panels:
            _warn_once("lib-cross-kv", f"vidtome_amd: attn2's k / v projections run as library GEMMs (conditioning width "
                                       f"{D} is not a multiple of 64, or to_k / to_v are not of the tokens' dtype)")
        k = _apply_linear(to_k, enc, dt)
        vt = _apply_linear(to_v, enc, dt).transpose(1, 2).contiguous()
    return k, vt


def _pad_keys(enc: torch.Tensor, dt) -> torch.Tensor:
    """Conditioning tokens in the tokens' dtype, zero rows appended up to a multiple of 8."""
    enc = enc.to(dt)
    pad = -enc.shape[1] % 8
    return F.pad(enc, (0, 0, 0, pad)) if pad else enc


def _ip_key_sets(attn: torch.nn.Module, ip: "ip_adapter.Call", dt, C: int, mode: str):
    """The operands of the IP-Adapter core: text k / v^T as for the plain block (``mode``: ``_cross_kv``'s), every adapter
    whose scale is not 0 projected the same way with to_k_ip[a] / to_v_ip[a] into its slice of ONE k (B, Mkp, C) and ONE v^T
    (B, C, Mkp) buffer
    -> (k, vt, [(start, length, weight)], mask rows, mask table).  With no adapter taking part k / vt ARE the plain block's
    tensors.  Region masks (``ip.masks``): all m_a * T_a image tokens of a masked adapter are projected in one GEMM like any
    other adapter's, then every image's T_a rows go to a set of their own on a multiple of 8 keys; the mask rows name each
    set's row (-1: none) of the (R, N) fp32 table of per-query weights.  Without a masked set taking part both are None."""
    lens = [im.shape[1] for im in ip.images]
    masks = ip.masks if ip.masks is not None else [None] * len(lens)
    images = [0 if m is None else m.shape[0] for m in masks]
    if any(images):
        sets, active, _, rows = ip_adapter.masked_key_sets(ip.text.shape[1], lens, ip.scales, images)
    else:
        (sets, active, _), rows = ip_adapter.key_sets(ip.text.shape[1], lens, ip.scales), []
    k, vt = _cross_kv(attn.to_k, attn.to_v, _pad_keys(ip.text, dt), C, mode)
    if active:
        parts = [(k, vt)]
        for a in active:
            ka, vta = _cross_kv(ip.k_proj[a], ip.v_proj[a], _pad_keys(ip.images[a], dt), C, mode)
            t = lens[a] // max(images[a], 1)
            if images[a] > 1 and t % 8:                                 # every image's keys onto a multiple of 8
                pad = -t % 8
                ka = torch.cat([F.pad(ka[:, i * t:(i + 1) * t], (0, 0, 0, pad)) for i in range(images[a])], dim=1)
                vta = torch.cat([F.pad(vta[:, :, i * t:(i + 1) * t], (0, pad)) for i in range(images[a])], dim=2)
            parts.append((ka, vta))
        k = torch.cat([p[0] for p in parts], dim=1)
        vt = torch.cat([p[1] for p in parts], dim=2)
    if not any(r >= 0 for r in rows):
        return k, vt, sets, None, None
    table = torch.cat([masks[a] for a in active if masks[a] is not None]).contiguous()
    return k, vt, sets, rows, table


def _key_bias_ok(attention_mask, B: int, Mk: int, device=None) -> bool:
    """The mask form ``key_bias`` takes: Diffusers' UNet turns an ``encoder_attention_mask`` (B, K) into the additive
    (B, 1, K) bias ``(1 - mask) * -10000`` in the sample's dtype -- one value per key, for every head and every query."""
    return (isinstance(attention_mask, torch.Tensor) and attention_mask.is_floating_point() and attention_mask.dim() == 3
            and attention_mask.shape[1] == 1 and attention_mask.shape[0] in (1, B) and attention_mask.shape[2] == Mk
            and (device is None or attention_mask.device == device))


def key_bias(attention_mask, B: int, Mk: int, device=None) -> Optional[torch.Tensor]:
    """The per-key score bias of a masked attn2 call for the biased core (``_attn2_core``): fp32 rows (B or 1, Mk) from an
    additive floating-point ``attention_mask`` of shape (B or 1, 1, Mk) on ``device`` (the tokens'; None: not asked), else None --
    the module path.  Bool / integer masks, 2-D masks, per-query masks (B, N, K) and a key count that is not the
    conditioning's are the module's own business.  One dtype conversion, nothing is read back to the host."""
    if not _key_bias_ok(attention_mask, B, Mk, device):
        return None
    return attention_mask[:, 0].to(torch.float32).contiguous()


def _probs_torch(q: torch.Tensor, k: torch.Tensor, heads: int, scale: float, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """The torch restatement of vtm_attention_probs on q (B, N, C) / k (B, Mk, C) rows of any dtype: fp32 scores, base-e
    softmax, the heads summed in ascending order and divided by their number; bias as ``key_bias`` gives it."""
    B, N, C = q.shape
    d = C // heads
    acc = torch.zeros((B, N, k.shape[1]), dtype=torch.float32, device=q.device)
    for h in range(heads):
        s = torch.matmul(q[:, :, h * d:(h + 1) * d].float(), k[:, :, h * d:(h + 1) * d].float().transpose(1, 2)) * scale
        if bias is not None:
            s = s + bias[:, None, :]
        acc += torch.softmax(s, dim=-1)
    return acc / heads


def _probs_rows(q: torch.Tensor, k: torch.Tensor, heads: int, N: int, Mk: int, scale: float,
                bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The head-averaged probabilities (B, N, Mk) fp32 of a fused attn2 call from the q (B, >= N, C) / k (B, >= Mk, C) rows
    its core reads: one vtm_attention_probs launch for what the kernel takes (16-bit rows, Mk <= 256, at most 40 heads),
    else the torch restatement on the same rows."""
    with torch.no_grad():
        if q.dtype in (torch.float16, torch.bfloat16) and Mk <= _lib.PROBS_MAX_KEYS and heads <= _lib.PROBS_MAX_HEADS:
            return _lib.attention_probs(q, k, heads, N, Mk, scale, bias)
        return _probs_torch(q[:, :N], k[:, :Mk], heads, scale, bias)


def _module_path_probs(attn: torch.nn.Module, x: torch.Tensor, encoder_hidden_states, attention_mask) -> Optional[torch.Tensor]:
    """The map of an attn2 call that ran as the module's own forward (a custom processor, an AdaLayerNorm block, ...): to_q /
    to_k through lora.linear_params on the module's own inputs, in the tokens' dtype as the module computes them, then the
    torch restatement.  An IP-Adapter tuple gives the map of its text set.  None (one warning) when the projections are
    not readable, something stands between them and the scores (norm_cross, norm_q / norm_k, ...) or the mask is not of
    ``key_bias``'s form; never raises."""
    try:
        enc = encoder_hidden_states[0] if isinstance(encoder_hidden_states, tuple) and encoder_hidden_states \
            else encoder_hidden_states
        ok = (isinstance(enc, torch.Tensor) and enc.dim() == 3 and x.dim() == 3 and enc.shape[0] == x.shape[0]
              and all(hasattr(attn, a) for a in ("to_q", "to_k", "heads"))
              and _readable_linear(attn.to_q) and _readable_linear(attn.to_k)
              and not any(getattr(attn, a, None) is not None for a in ("group_norm", "spatial_norm", "norm_cross", "norm_q", "norm_k"))
              and lora.base_linear(attn.to_q).out_features % attn.heads == 0
              and (attention_mask is None or _key_bias_ok(attention_mask, x.shape[0], enc.shape[1], x.device)))
        if ok:
            with torch.no_grad():
                q = _apply_linear(attn.to_q, x, x.dtype)
                k = _apply_linear(attn.to_k, enc.to(x.dtype), x.dtype)
                bias = None if attention_mask is None else key_bias(attention_mask, x.shape[0], enc.shape[1], x.device)
                return _probs_torch(q, k, attn.heads, _scale(attn, q.shape[-1]), bias)
    except Exception as e:   # (a forward never fails for its map)
        _warn_once("maps-failed", f"vidtome_amd: attn2_probs is None: the map of a module-path attn2 call failed ({e})")
        return None
    _warn_once("maps-unreadable", "vidtome_amd: attn2_probs is None for an attn2 call on the module path whose to_q / to_k "
                                  "are not plain projections onto the scores, or whose mask is not an additive (B, 1, K) row")
    return None


def local_blend_of(block: torch.nn.Module):
    """(LocalBlend, block name) when ``blend.register_local_blend`` selected the block, else None."""
    return block.__dict__.get("vtm_local_blend")


def _word_groups(words_to, B: int, N: int, K: int, device):
    """What every route of ``add_word_maps`` starts from: the checks a registered block makes on its call -- the batch is
    ``num_inputs`` groups, K is the weights' length, N the accumulator's token count -- then (lb, Fg, accumulator
    (G, num_frames, N), the chunk's rows in it)."""
    lb, name = words_to
    if B % lb.num_inputs:
        raise RuntimeError(f"vidtome_amd: LocalBlend on block '{name}': the batch of {B} samples is not {lb.num_inputs} "
                           "groups of equal size")
    if K != lb.K:
        raise RuntimeError(f"vidtome_amd: LocalBlend on block '{name}': the conditioning has K = {K} tokens, the word "
                           f"weights are for K = {lb.K}")
    Fg = B // lb.num_inputs
    return lb, Fg, lb.accumulator(N, device, name), lb.frame_rows(Fg, device)


def add_word_maps(words_to, q: torch.Tensor, k: torch.Tensor, heads: int, N: int, Mk: int, scale: float,
                  bias: Optional[torch.Tensor] = None, ctl=None) -> None:
    """A registered block's contribution to its LocalBlend (``words_to`` = ``local_blend_of(block)``) from the q (B F, >= N,
    C) / k (B F, >= Mk, C) rows the attn2 core reads: for every group g in ``words``, sum_j w_g[j] P[i, j] of the group's
    samples added into the chunk's frame rows of the group's accumulator plane -- one vtm_attention_word_map launch on the
    group's sample slice for what the kernel takes (16-bit rows, Mk <= 256), else the torch restatement on the same rows.
    ``ctl`` (an injecting block under cross-attention control): an edited group's map is P_src . (M (a o w)) + P_own . (b o w),
    two launches into the same rows -- (a) q and k of the SOURCE group's slice, (b) the group's own."""
    with torch.no_grad():
        lb, Fg, acc, rows_out = _word_groups(words_to, q.shape[0], N, Mk, q.device)
        fused = q.dtype in (torch.float16, torch.bfloat16) and Mk <= _lib.PROBS_MAX_KEYS
        weights = lb.weights_on(q.device)
        edits = ctl[1] if ctl is not None else {}
        for gi, g in enumerate(lb.groups):
            own = slice(g * Fg, (g + 1) * Fg)
            if g in edits and not edits[g].is_identity:
                w_src, w_own = lb.edited_weights(edits[g], gi, q.device)
                parts = [(slice(0, Fg), w_src), (own, w_own)]
            else:
                parts = [(own, weights[gi:gi + 1])]
            for rows, w in parts:
                b = None if bias is None else (bias[rows] if bias.shape[0] == q.shape[0] and q.shape[0] > 1 else bias)
                if fused:
                    _lib.attention_word_map(q[rows], k[rows], heads, N, Mk, scale, w, acc[gi], rows_out, True, b)
                else:
                    acc[gi].index_add_(0, rows_out, torch.matmul(_probs_torch(q[rows, :N], k[rows, :Mk], heads, scale, b), w[0]))


def add_word_maps_module_path(words_to, attn: torch.nn.Module, x: torch.Tensor, encoder_hidden_states, attention_mask) -> None:
    """The same contribution for an attn2 call that runs as the module's own forward: ``_module_path_probs``, then ``@ w``
    per group.  Where that map is unavailable the call RAISES: a blend built on a silently missing block is wrong."""
    lb, name = words_to
    probs = _module_path_probs(attn, x, encoder_hidden_states, attention_mask)
    if probs is None:
        raise RuntimeError(f"vidtome_amd: LocalBlend on block '{name}': the map of this module-path attn2 call cannot be read "
                           "(to_q / to_k are not plain projections onto the scores, or the mask is not an additive (B, 1, K) "
                           "row)")
    with torch.no_grad():
        lb, Fg, acc, rows_out = _word_groups(words_to, probs.shape[0], probs.shape[1], probs.shape[2], probs.device)
        weights = lb.weights_on(probs.device)
        for gi, g in enumerate(lb.groups):
            acc[gi].index_add_(0, rows_out, torch.matmul(probs[g * Fg:(g + 1) * Fg], weights[gi]))


def _f32_layernorm_ok(norm: torch.nn.Module, x: torch.Tensor) -> bool:
    """A plain LayerNorm over the channel axis of fp32 tokens that vtm_layernorm takes."""
    return x.dtype == torch.float32 and _plain_layernorm(norm, x) and x.shape[-1] % 8 == 0 and x.shape[-1] <= 2048


def f32_cross_ok(block: torch.nn.Module, norm: torch.nn.Module, attn: torch.nn.Module, x: torch.Tensor,
                 encoder_hidden_states, attention_mask, kwargs) -> bool:
    """attn2 of an fp32 block with the ``fp32_projections`` opt-in on the fp32 GEMMs (norm_cross_attention_f32)."""
    return (_fp32_projections(block) and isinstance(encoder_hidden_states, torch.Tensor) and attention_mask is None
            and not kwargs and encoder_hidden_states.dim() == 3 and x.dim() == 3 and x.is_cuda and x.dtype == torch.float32
            and encoder_hidden_states.shape[0] == x.shape[0] and encoder_hidden_states.shape[-1] % 8 == 0
            and _f32_layernorm_ok(norm, x) and _proj_dtypes_ok(attn, torch.float32)
            and fused_attention_ok(attn, x, self_attn=False))


# ----------------------------------------------------------------------------------------------------
# attn2: the control of an injecting step (vidtome_amd/p2p.py), the route, the core dispatch, one body per frame
# ----------------------------------------------------------------------------------------------------
def cross_control(block: torch.nn.Module):
    """(num_inputs, edits, block name) when ``p2p.register_cross_attention_control`` selected the block and this step
    injects -- ``attn2.t in injection_schedule or attn2.t == 1000``, the PnP rule (pnp_utils.py:57-58), ``t`` stamped by
    ``pnp.register_time`` -- else None: the block then launches what it launches without the control."""
    ctl = block.__dict__.get("vtm_cross_control")
    if ctl is None or getattr(block, "attn2", None) is None:
        return None
    schedule, num_inputs, edits, name = ctl
    t = getattr(block.attn2, "t", None)
    if t is None or not (t in schedule or t == 1000):
        return None
    return num_inputs, edits, name


def _edited_probs(probs: torch.Tensor, rows: slice, src: slice, edit) -> None:
    """The head-averaged map of an edited group, in place: head-averaging commutes with the edit."""
    M, a, b = edit.on(probs.device)
    probs[rows] = torch.matmul(probs[src], M) * a + probs[rows] * b


class Attn2Route(NamedTuple):
    """``attn2_route``'s answer: the frame, and the recognised IP-Adapter call when the call is one."""
    frame: str
    ip: Optional["ip_adapter.Call"] = None


def _plain_call_ok(attn: torch.nn.Module, x: torch.Tensor, encoder_hidden_states, attention_mask, kwargs,
                   processors=_PLAIN_PROCESSORS) -> bool:
    """A call the plain or the biased core computes on 16-bit tokens: a (B, K, D) conditioning tensor (an IP-Adapter block
    hands a TUPLE: not this call), no processor kwargs, a module that is the plain arithmetic (``fused_attention_ok``) and no
    mask or one of ``key_bias``'s form."""
    enc = encoder_hidden_states
    return (isinstance(enc, torch.Tensor) and not kwargs and enc.dim() == 3 and x.dtype in (torch.float16, torch.bfloat16)
            and fused_attention_ok(attn, x, self_attn=False, processors=processors)
            and (attention_mask is None or _key_bias_ok(attention_mask, x.shape[0], enc.shape[1], x.device)))


def _panels_ok(norm: torch.nn.Module, attn: torch.nn.Module, x: torch.Tensor, ip: Optional["ip_adapter.Call"] = None) -> bool:
    """What the panels frame asks on top of a call the library-GEMM frame takes: FF_MODE "panels", a plain norm2 on device
    tokens, C % 64 == 0 and the four projection weights in the tokens' dtype.  An IP-Adapter call still asks N % 8 == 0, as
    tests/test_ip_adapter_host.py (test_panel_path_asks_what_fused_cross_ok_asks) pins: other token counts are "blas"."""
    return (FF_MODE == "panels" and x.is_cuda and _plain_layernorm(norm, x) and x.shape[-1] % 64 == 0
            and _proj_dtypes_ok(attn, x.dtype) and (ip is None or x.shape[1] % 8 == 0))


def fused_cross_ok(norm: torch.nn.Module, attn: torch.nn.Module, x: torch.Tensor, encoder_hidden_states,
                   attention_mask, kwargs, processors=_PLAIN_PROCESSORS) -> bool:
    """``attn2_route``'s "panels" for a call without an IP-Adapter and without control, as a predicate."""
    return _plain_call_ok(attn, x, encoder_hidden_states, attention_mask, kwargs, processors) and _panels_ok(norm, attn, x)


def ip_cross_call(attn: torch.nn.Module, x: torch.Tensor, encoder_hidden_states, attention_mask, kwargs,
                  norm: Optional[torch.nn.Module] = None) -> Optional["ip_adapter.Call"]:
    """The IP-Adapter call of attn2 when the fused path may take it, else None (the module path): the processor and the
    call are what `ip_adapter.recognise` understands (never a masked call), and the module is everything
    ``fused_attention_ok`` asks of attn2 apart from the processor's name.  With ``norm`` (norm2): for the panels frame;
    without: for the library GEMMs of ``cross_attention``."""
    ip = ip_adapter.recognise(attn, x, encoder_hidden_states, attention_mask, kwargs)
    if ip is None or not fused_attention_ok(attn, x, self_attn=False, processors=ip_adapter.PROCESSORS):
        return None
    return ip if norm is None or _panels_ok(norm, attn, x, ip) else None


def _attn2_lib_route(attn: torch.nn.Module, x: torch.Tensor, encoder_hidden_states, attention_mask, kwargs) -> Attn2Route:
    """The half of ``attn2_route`` that is attn2's alone, for the tokens ``x`` its core would read: "blas" or "module"."""
    if ip_adapter.is_ip_processor(attn):
        ip = ip_cross_call(attn, x, encoder_hidden_states, attention_mask, kwargs)
        return Attn2Route("module" if ip is None else "blas", ip)
    return Attn2Route("blas" if _plain_call_ok(attn, x, encoder_hidden_states, attention_mask, kwargs) else "module")


def _refuse_control(block: torch.nn.Module, x: torch.Tensor, enc, attention_mask, kwargs, ctl) -> None:
    """What an injecting block does not take RAISES, naming the block and the reason, before anything is launched: there is
    no module path under control, an edit is never silently dropped."""
    num_inputs, edits, name = ctl
    attn = block.attn2

    def refuse(why: str):
        raise RuntimeError(f"vidtome_amd: cross-attention control on block '{name}': {why}")
    if isinstance(enc, tuple) or ip_adapter.is_ip_processor(attn):
        refuse("an IP-Adapter call is not taken (combining the control with image prompts is out of scope)")
    if not (isinstance(enc, torch.Tensor) and enc.dim() == 3 and x.dim() == 3 and enc.shape[0] == x.shape[0]):
        refuse("the conditioning must be a (B F, K, D) tensor with a row set per sample")
    if x.shape[0] % num_inputs:
        refuse(f"the batch of {x.shape[0]} samples is not {num_inputs} groups of equal size")
    K = enc.shape[1]
    if K > _lib.CROSS_EDIT_MAX_KEYS:
        refuse(f"K = {K} conditioning tokens, at most {_lib.CROSS_EDIT_MAX_KEYS} are taken")
    for g, e in sorted(edits.items()):
        if e.K != K:
            refuse(f"the edit of group {g} is for K = {e.K} tokens, the conditioning has {K}")
    if block.use_ada_layer_norm:
        refuse("AdaLayerNorm blocks are not taken")
    if x.dtype not in (torch.float16, torch.bfloat16):
        refuse(f"{x.dtype} blocks are not taken (fp16 / bf16 only)")
    if attention_mask is not None:
        refuse("an attention_mask is not taken (combining the control with masks is out of scope)")
    if kwargs:
        refuse(f"processor kwargs {sorted(kwargs)} are not taken")
    if not fused_attention_ok(attn, x, self_attn=False):
        refuse("attn2 is not the plain arithmetic the fused path computes (fused_attention_ok)")


def attn2_route(block: torch.nn.Module, x: torch.Tensor, encoder_hidden_states, encoder_attention_mask,
                cross_attention_kwargs, control=None, normed: bool = False) -> Attn2Route:
    """How the block computes its ``attn2`` segment on tokens like ``x`` (their device, rank, dtype and width are read), and
    the recognised IP-Adapter call when the call is one.  Launches nothing; `ip_adapter.recognise` runs at most once.
      "panels"  norm_cross_attention_residual: LayerNorm -> panels, q panel GEMM, core, output panel GEMM + residual.  fp16 /
                bf16 device tokens, FF_MODE "panels", a plain norm2, C % 64 == 0, the four projection weights in the tokens'
                dtype (``_panels_ok``), and a call "blas" takes; an IP-Adapter call also asks N % 8 == 0
      "f32"     norm_cross_attention_f32: fp32 tokens with the block's ``fp32_projections``, a plain norm2, C % 8 == 0 and a
                conditioning width % 8 == 0, fp32 projection weights, no mask of any form (``f32_cross_ok``)
      "blas"    cross_attention: library GEMMs around the core.  fp16 / bf16 tokens, a module that is the plain arithmetic
                (``fused_attention_ok``; an IP-Adapter processor when the call is one), and the call: a (B, K, D)
                conditioning tensor without processor kwargs, with no mask or one of ``key_bias``'s form
                (``_plain_call_ok``) -- or what `ip_adapter.recognise` reads (``ip_cross_call``: never with a mask)
      "module"  attn2's own forward, through cross_attention: everything else
    An AdaLayerNorm block never takes "panels" or "f32" (its norm2 needs the timestep), and with any non-None mask, even one
    of ``key_bias``'s form, it is "module".
    ``control`` (``cross_control``: an injecting step) knows "panels" and "blas" alone, by the same rules; every other call
    RAISES (``_refuse_control``).
    Which core runs follows from the call alone: ``_attn2_core``.
    "panels" and "f32" are decided on the tokens in front of norm2, "blas" / "module" for the tokens the core reads: a norm2
    that changes the dtype (a module-path LayerNorm under autocast, an AdaLayerNorm in another dtype) makes them differ, and
    the block then asks again with ``normed`` and the normed tokens -- the question for the two frames that read them."""
    attn, norm = block.attn2, block.norm2
    fused = not (normed or block.use_ada_layer_norm)
    if control is not None:
        _refuse_control(block, x, encoder_hidden_states, encoder_attention_mask, cross_attention_kwargs, control)
        route = Attn2Route("blas")
    elif block.use_ada_layer_norm and encoder_attention_mask is not None:
        return Attn2Route("module")
    elif fused and f32_cross_ok(block, norm, attn, x, encoder_hidden_states, encoder_attention_mask, cross_attention_kwargs):
        return Attn2Route("f32")
    else:
        route = _attn2_lib_route(attn, x, encoder_hidden_states, encoder_attention_mask, cross_attention_kwargs)
    if fused and route.frame == "blas" and _panels_ok(norm, attn, x, route.ip):
        return route._replace(frame="panels")
    return route


def cross_control_route(block: torch.nn.Module, x: torch.Tensor, encoder_hidden_states, attention_mask, kwargs, ctl) -> str:
    """``attn2_route``'s frame for an injecting block: "panels" or "blas"; everything else raises."""
    return attn2_route(block, x, encoder_hidden_states, attention_mask, kwargs, ctl).frame


def _attn2_core(attn: torch.nn.Module, q: torch.Tensor, N: int, encoder_hidden_states, kv: str, attention_mask=None,
                ip: Optional["ip_adapter.Call"] = None, ctl=None, probs_to: Optional[torch.nn.Module] = None,
                words_to=None) -> torch.Tensor:
    """The core of an attn2 call on query rows q (B, Np, C), N <= Np of them meaningful -> o (B, Np, C).  ``kv``: how k / v^T
    are projected, the frame's mode of ``_cross_kv``.  The call alone says which core runs:
      ``ctl`` (an injecting block)          the controlled core, below
      ``ip`` without region masks           vtm_attention_kv_sets: ONE launch over the text keys and every adapter's image keys
      ``ip`` with region masks              vtm_attention_kv_sets_masked, likewise (``_ip_key_sets``); the conditioning is the
                                            call's, ``encoder_hidden_states`` is not read
      an accepted mask (``key_bias``)       vtm_attention_kv_bias
      otherwise                             vtm_attention_kv
    The controlled core: samples are group-major, b = g * Fg + f, and the source of sample b is b % Fg.  k / v^T of EVERY
    sample come from the one projection call the block makes without the control.  Contiguous runs of unedited groups (no
    edit, or the identity) then run the plain core on their slices of q / o -- the bits of an uncontrolled block -- and each
    edited group is
        k   = [k(enc[src]) | k(enc[own])]                      two key sets at 0 and K rounded up to 8
        V^T = [(M diag(a) V_own)^T | (diag(b) V_own)^T]        vtm_cross_edit_values
        o   = softmax(q[src] k_src^T) V' + softmax(q[own] k_own^T) V''     ONE vtm_attention_kv_sets_src launch
    into its slice of o.
    After the cores, from the same q / k rows (an IP-Adapter call: the text set's, with its own softmax): ``probs_to`` (a
    block registered by ``maps.register_attention_maps``) gets ``attn2_probs``, one vtm_attention_probs launch, an edited
    group's rows edited as its probabilities are (``_edited_probs``); then ``words_to`` (``local_blend_of`` a block registered
    by ``blend.register_local_blend``) gets the word maps (``add_word_maps``)."""
    heads, C = attn.heads, q.shape[-1]
    scale = _scale(attn, C)
    bias, edited = None, []
    if ip is not None:
        Mk = ip.text.shape[1]
        k, vt, sets, rows, table = _ip_key_sets(attn, ip, q.dtype, C, kv)
    else:
        Mk = encoder_hidden_states.shape[1]
        enc = encoder_hidden_states.to(q.dtype).contiguous() if kv == "f32" else _pad_keys(encoder_hidden_states, q.dtype)
        k, vt = _cross_kv(attn.to_k, attn.to_v, enc, C, kv)
        bias = None if attention_mask is None else key_bias(attention_mask, q.shape[0], Mk, q.device)
    if ctl is not None:
        num_inputs, edits, _ = ctl
        Fg, K8 = q.shape[0] // num_inputs, (Mk + 7) // 8 * 8
        o = (torch.zeros if q.shape[1] != N else torch.empty)(q.shape, dtype=q.dtype, device=q.device)
        is_edited = [g in edits and not edits[g].is_identity for g in range(num_inputs)]
        src = slice(0, Fg)
        g = 0
        while g < num_inputs:
            g1 = g + 1
            if is_edited[g]:
                own = slice(g * Fg, g1 * Fg)
                M, a, b = edits[g].on(q.device)
                k_sets = torch.cat([k[src], k[own]], dim=1)                # (F, 2 K8, C)
                vt_sets = _lib.cross_edit_values(vt[own], 0, Mk, M, a, b, 0, K8,
                                                 out=torch.empty((Fg, C, 2 * K8), dtype=q.dtype, device=q.device))
                _lib.attention_kv_sets_src(q[own], q[src], k_sets, vt_sets, heads, N, [(0, Mk, 1.0), (K8, Mk, 1.0)], scale,
                                           (1, 0), out=o[own])
                edited.append((own, edits[g]))
            else:
                while g1 < num_inputs and not is_edited[g1]:
                    g1 += 1
                run = slice(g * Fg, g1 * Fg)
                _lib.attention_kv(q[run], k[run], vt[run], heads, N, Mk, scale, out=o[run])
            g = g1
    elif ip is not None:
        o = _lib.attention_kv_sets(q, k, vt, heads, N, sets, scale) if table is None else \
            _lib.attention_kv_sets_masked(q, k, vt, heads, N, sets, scale, rows, table)
    elif bias is not None:
        o = _lib.attention_kv_bias(q, k, vt, heads, N, Mk, scale, bias)
    else:
        o = _lib.attention_kv(q, k, vt, heads, N, Mk, scale)
    if probs_to is not None:
        probs = _probs_rows(q, k, heads, N, Mk, scale, bias)
        for own, edit in edited:
            _edited_probs(probs, own, src, edit)
        probs_to.attn2_probs = probs
    if words_to is not None:
        add_word_maps(words_to, q, k, heads, N, Mk, scale, bias, ctl=ctl)
    return o


def norm_cross_attention_residual(norm: torch.nn.Module, attn: torch.nn.Module, hidden_states: torch.Tensor,
                                  encoder_hidden_states, ip: Optional["ip_adapter.Call"] = None, attention_mask=None,
                                  probs_to: Optional[torch.nn.Module] = None, words_to=None, ctl=None) -> torch.Tensor:
    """patch.py:171-185 on the panels frame: ``attn2(norm2(hidden_states), encoder_hidden_states) + hidden_states`` with the
    query projection as a panel GEMM fed by the LayerNorm (vtm_layernorm_panels -> vtm_linear_panels: the normalised tokens
    are only ever read by to_q, so they are written once, as panels), k / v^T of the (few) conditioning tokens as panel GEMMs
    too, the core (``_attn2_core``: ``ip``, ``attention_mask``, ``ctl``, ``probs_to`` and ``words_to`` are its arguments) and
    the output projection + bias + residual as a panel GEMM.  The caller has asked ``attn2_route`` (or ``fused_cross_ok``;
    ``ip_cross_call`` with norm2 for ``ip``; ``cross_control_route`` for ``ctl``)."""
    B, N, C = hidden_states.shape
    hs = hidden_states.contiguous()
    n = B * N
    wq, bq = _panel_weight(attn.to_q)
    wo, bo = _panel_weight(_out_linear(attn))
    xp = _lib.layernorm_panels(hs, norm.weight, norm.bias, norm.eps)
    q = _lib.linear_panels(xp, n, wq, C, bq).view(B, N, C)             # any N: the core's query row stride is N itself
    o = _attn2_core(attn, q, N, encoder_hidden_states, "panels", attention_mask, ip, ctl, probs_to, words_to)
    op = _lib.to_panels(o.view(n, C))
    return _lib.linear_panels(op, n, wo, C, bo, resid=hs.view(n, C)).view(B, N, C)


def norm_cross_attention_f32(norm: torch.nn.Module, attn: torch.nn.Module, hidden_states: torch.Tensor,
                             encoder_hidden_states: torch.Tensor, probs_to: Optional[torch.nn.Module] = None,
                             words_to=None) -> torch.Tensor:
    """patch.py:171-185 for an fp32 block with ``fp32_projections``: ``attn2(norm2(h), encoder_hidden_states) + h`` as
    vtm_layernorm, the q GEMM, the k / V^T GEMMs of the conditioning tokens (padded to a multiple of 8 rows), the fp32
    attention core (whatever ``fp32_attention`` says: the module forward it replaces is fp32, and 77 keys keep it cheap; the
    maps of fp32 rows are the torch restatement) and the output GEMM with the residual add in its epilogue.  The caller has
    asked ``attn2_route`` (or ``f32_cross_ok``)."""
    N = hidden_states.shape[1]
    f32 = torch.float32
    hs = hidden_states.contiguous()
    xn = _lib.layernorm(hs, norm.weight, norm.bias, norm.eps)
    q = _lib.linear_f32(xn, None, None, None, N, *_linear(attn.to_q, f32)[:2])                             # (B, N8, C)
    o = _attn2_core(attn, q, N, encoder_hidden_states, "f32", probs_to=probs_to, words_to=words_to)
    return _lib.linear_f32(o, None, None, None, N, *_linear(_out_linear(attn), f32)[:2], epilogue="resid", resid=hs,
                           out=torch.empty_like(hs))


def cross_attention(attn: torch.nn.Module, x: torch.Tensor, encoder_hidden_states, attention_mask=None,
                    probs_to: Optional[torch.nn.Module] = None, words_to=None, ctl=None, route: Optional[Attn2Route] = None,
                    **kwargs) -> torch.Tensor:
    """`self.attn2(norm_hidden_states, encoder_hidden_states=..., attention_mask=...)` (patch.py:178-183) -- the
    un-merged tokens attending to the conditioning (77 text tokens in SD) -- on the library-GEMM frame: pad to 8 rows, to_q,
    the core (``_attn2_core``), to_out; or, for everything that frame does not take, the module's own forward.  ``route``:
    what ``attn2_route`` answered for tokens like ``x``, when the caller has asked already; ``ctl``: an injecting block, whose
    caller has asked (``cross_control_route``).  ``probs_to`` / ``words_to``: a registered block gets ``attn2_probs`` / its
    LocalBlend the word maps on whichever of the two the call takes (the module path: the torch restatement)."""
    if route is None:
        route = Attn2Route("blas") if ctl is not None else _attn2_lib_route(attn, x, encoder_hidden_states, attention_mask,
                                                                             kwargs)
    if route.frame == "module":
        if probs_to is not None:
            probs_to.attn2_probs = _module_path_probs(attn, x, encoder_hidden_states, attention_mask)
        if words_to is not None:
            add_word_maps_module_path(words_to, attn, x, encoder_hidden_states, attention_mask)
        return attn(x, encoder_hidden_states=encoder_hidden_states, attention_mask=attention_mask, **kwargs)
    N = x.shape[1]
    xq = F.pad(x, (0, 0, 0, -N % 8)) if N % 8 else x
    q = _apply_linear(attn.to_q, xq, x.dtype)
    o = _attn2_core(attn, q, N, encoder_hidden_states, "blas", attention_mask, route.ip, ctl, probs_to, words_to)
    return _apply_linear(_out_linear(attn), o, o.dtype)[:, :N]


# ----------------------------------------------------------------------------------------------------
# the rest of the block as panel GEMMs (csrc/ff.hip)
# ----------------------------------------------------------------------------------------------------
# VIDTOME_FF: "panels" (default) = norm3 -> GEGLU projection with the gated activation in the GEMM's epilogue -> output
# Linear with bias and residual, all hand-written (vtm_layernorm_panels, vtm_ff_geglu, vtm_linear_panels: the 8C-wide
# projection is never written); "blas" = library GEMMs around vtm_geglu (rounds 1-2).  The same switch covers the
# cross-attention's query projection (norm2 -> panels -> vtm_linear_panels).
FF_MODE = os.environ.get("VIDTOME_FF", "panels")


def _packed(module: torch.nn.Module, name: str, tag, dev, build):
    """Weights repacked for the panel GEMMs, cached on the module under `name` and rebuilt when `tag` -- the keys
    lora.linear_params gave for the projections packed -- changes."""
    cache = module.__dict__.setdefault("_vtm_packed", {})
    hit = cache.get(name)
    if hit is None or hit[0] != tag:
        hit = cache[name] = (tag, build(), _built_here(dev))
    _built_before(hit[2], dev)
    return hit[1]


def _geglu_ff(ff: torch.nn.Module):
    """(GEGLU projection Linear, output Linear) of a Diffusers FeedForward [GEGLU, Dropout, Linear], else None."""
    net = getattr(ff, "net", None)
    if (net is not None and len(net) == 3 and net[0].__class__.__name__ == "GEGLU" and hasattr(net[0], "proj")
            and _readable_linear(net[0].proj) and _readable_linear(net[2])
            and (not ff.training or getattr(net[1], "p", 0.0) == 0.0)):      # Dropout(0.0) is the identity in any mode
        return net[0].proj, net[2]
    return None


def _geglu_dims(ff: torch.nn.Module, x: torch.Tensor):
    """(GEGLU projection, output Linear, C, D) of ``_geglu_ff`` -- the two BASE Linears (shapes and dtypes of the effective
    weights) -- where they chain C -> 2 D -> D -> C over the channels of ``x``; else None."""
    lin = _geglu_ff(ff)
    if lin is not None:
        proj, out = (lora.base_linear(m) for m in lin)
        C, D = x.shape[-1], proj.out_features // 2
        if proj.in_features == C and proj.out_features == 2 * D and out.in_features == D and out.out_features == C:
            return proj, out, C, D
    return None


def fused_ff_ok(norm: torch.nn.Module, ff: torch.nn.Module, x: torch.Tensor) -> bool:
    if FF_MODE != "panels" or not x.is_cuda or x.dtype not in (torch.float16, torch.bfloat16):
        return False
    dims = _geglu_dims(ff, x)
    if dims is None or not _plain_layernorm(norm, x):
        return False
    proj, out, C, D = dims
    return C % 64 == 0 and C <= 2048 and D % 64 == 0 and proj.weight.dtype == x.dtype and out.weight.dtype == x.dtype


def _ff_panel_weights(ff: torch.nn.Module):
    """(W1 packed in the tile order of vtm_ff_geglu, its fp32 bias in that order or None, D, W2 as k-panels, its fp32 bias or
    None) of a feed-forward ``fused_ff_ok`` accepted, cached on the two projections."""
    proj, out = _geglu_ff(ff)
    pw, pb, pkey = _linear(proj)
    D = pw.shape[0] // 2

    def pack_w1():
        t = torch.arange(D // 64, device=pw.device)[:, None] * 64 + torch.arange(64, device=pw.device)[None, :]
        order = torch.cat([t, t + D], dim=1).reshape(-1).to(torch.int32)       # tile t: 64 value rows, then their gate rows
        b = None if pb is None else pb.detach().float()[order.long()].contiguous()
        return _lib.to_panels(pw.detach().contiguous(), order), b

    w1, b1 = _packed(proj, "geglu", pkey, pw.device, pack_w1)
    w2, b2 = _panel_weight(out)
    return w1, b1, D, w2, b2


def _ff_panels(weights, xp: torch.Tensor, n: int, resid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The two GEMMs of a feed-forward ``fused_ff_ok`` accepted, over the k-panels ``xp`` of its n LayerNorm'ed rows: the GEGLU
    projection with the gated activation in its epilogue -> k-panels, the output Linear + bias (+ ``resid`` (n, C)) -> (n, C)
    token rows.  The one place vtm_ff_geglu is reached from; the panels come from vtm_layernorm_panels
    (``norm_feed_forward_residual``), vtm_layernorm_gather (``merged_feed_forward_residual``) or
    vtm_residual_replay_layernorm (``broadcast_feed_forward_residual``).  ``weights``: ``_ff_panel_weights(ff)``, which each
    caller takes AHEAD of its LayerNorm launch -- a first call packs there (vtm_to_panels), and launch order is kept."""
    w1, b1, D, w2, b2 = weights
    hp = _lib.ff_geglu(xp, n, w1, D, b1)
    return _lib.linear_panels(hp, n, w2, xp.shape[0] * 8, b2, resid=resid)        # (C / 8 panels in, C columns out)


def norm_feed_forward_residual(norm: torch.nn.Module, ff: torch.nn.Module, hidden_states: torch.Tensor) -> torch.Tensor:
    """patch.py:187-199 for the plain-LayerNorm block: ``ff(norm3(hidden_states)) + hidden_states`` as three launches:
    LayerNorm -> k-panels, GEGLU projection with the gated activation in its epilogue -> k-panels, output Linear + bias +
    residual -> token rows.  The caller has checked ``fused_ff_ok``."""
    weights = _ff_panel_weights(ff)
    hs = hidden_states.contiguous()
    n = hs.numel() // hs.shape[-1]
    xp = _lib.layernorm_panels(hs, norm.weight, norm.bias, norm.eps)
    return _ff_panels(weights, xp, n, hs.view(n, -1)).view(hidden_states.shape)


def f32_ff_ok(block: torch.nn.Module, norm: torch.nn.Module, ff: torch.nn.Module, x: torch.Tensor) -> bool:
    """The feed-forward of an fp32 block with the ``fp32_projections`` opt-in on the fp32 GEMMs (norm_feed_forward_f32)."""
    if not (_fp32_projections(block) and x.is_cuda and x.dtype == torch.float32 and _f32_layernorm_ok(norm, x)):
        return False
    dims = _geglu_dims(ff, x)
    if dims is None:
        return False
    proj, out, C, D = dims
    return D % 8 == 0 and _linear_dtype_ok(proj, torch.float32) and _linear_dtype_ok(out, torch.float32)


def norm_feed_forward_f32(norm: torch.nn.Module, ff: torch.nn.Module, hidden_states: torch.Tensor) -> torch.Tensor:
    """patch.py:187-199 for an fp32 block with ``fp32_projections``: ``ff(norm3(h)) + h`` as vtm_layernorm, the GEGLU GEMM
    with value * gelu(gate) in its epilogue (the 8C-wide projection is never written) and the output GEMM with bias and
    residual.  The caller has checked ``f32_ff_ok``."""
    proj, out = _geglu_ff(ff)
    f32 = torch.float32
    C = hidden_states.shape[-1]
    hs = hidden_states.contiguous()
    n = hs.numel() // C
    xn = _lib.layernorm(hs, norm.weight, norm.bias, norm.eps).view(1, n, C)
    h = _lib.linear_f32(xn, None, None, None, n, *_linear(proj, f32)[:2], epilogue="geglu")               # (1, n8, D)
    y = _lib.linear_f32(h, None, None, None, n, *_linear(out, f32)[:2], epilogue="resid", resid=hs.view(1, n, C),
                        out=torch.empty((1, n, C), dtype=f32, device=hs.device))
    return y.view(hidden_states.shape)


def feed_forward(ff: torch.nn.Module, x: torch.Tensor) -> torch.Tensor:
    """`self.ff(norm_hidden_states)` (patch.py:192).  The Diffusers feed-forward of SD blocks is
    [GEGLU(proj: Linear C -> 8C), Dropout, Linear 4C -> C]; when that shape is recognised the gated activation
    runs as vtm_geglu (the two Linears stay library GEMMs), otherwise the module runs unchanged."""
    lin = _geglu_ff(ff)
    # (not in training: stricter than _geglu_ff's own dropout clause, which is then true whatever the Dropout's p)
    if (lin is not None and not ff.training and x.is_cuda and x.dtype in (torch.float16, torch.bfloat16, torch.float32)
            and lora.base_linear(lin[0]).out_features % 16 == 0):
        return _apply_linear(lin[1], _lib.geglu(_apply_linear(lin[0], x)))
    return ff(x)


def ff_route(block: torch.nn.Module, hidden_states: torch.Tensor, plan: Optional["MergePlan"]) -> str:
    """How the block computes its feed-forward on hidden states like ``hidden_states`` (B F, N, C) behind the attn1 segment
    whose compute_merge gave ``plan`` (None: nothing merged).  Launches nothing; decided once per forward, and
    ``feed_forward_segment`` calls the body.  The first row that holds, "on the merged tokens" meaning: the block's
    ``merge_mlp`` opt-in (``update_patch(model, merge_mlp=True)``) is True itself AND there is a local map (``plan.keep`` and
    ``plan.inv_local``: not a site that does not merge, a single-frame chunk, local_merge_ratio <= 0 or a replayed attn1) AND
    the block is no AdaLayerNormZero one (its shift / scale / gate are per frame row):
      "merged-panels"  on the merged tokens, and ``fused_ff_ok``: ``u(ff(norm3(m(h)))) + h`` over the local levels' closures
                       (tomesd's merge_mlp) as vtm_layernorm_gather -> vtm_ff_geglu -> vtm_linear_panels -> vtm_unmerge_add
                       (``merged_feed_forward_residual``)
      "merged"         on the merged tokens, every other feed-forward (fp32 models, VIDTOME_FF=blas, a ``ff`` that is not the
                       GEGLU one, projections the panel path does not read): gathered LayerNorm with token rows out (or
                       vtm_gather_rows + the norm module), ``feed_forward``, vtm_unmerge_add (the same body)
      "panels"         over every token, no AdaLayerNormZero block, and ``fused_ff_ok``: vtm_layernorm_panels -> vtm_ff_geglu
                       -> vtm_linear_panels with the residual (``norm_feed_forward_residual``)
      "f32"            over every token, no AdaLayerNormZero block, and ``f32_ff_ok`` (an fp32 block with ``fp32_projections``):
                       vtm_layernorm and the two fp32 GEMMs (``norm_feed_forward_f32``)
      "module"         everything else, every AdaLayerNormZero block among it: ``layer_norm``, the shift / scale,
                       ``feed_forward``, the gate, the residual (``module_feed_forward_residual``)
    So an fp32 block with ``fp32_projections`` AND ``merge_mlp`` is "merged" where it merges, not "f32" (there is no merged
    fp32-GEMM body); an AdaLayerNorm (non-zero) block keeps a plain norm3 and may be "panels" or "merged-panels"; and
    ``fused_ff_ok`` is evaluated at most once.
    The global level plays no part: its merged sequence holds other chunks' anchor rows, whose feed-forward output nobody
    would read.  The matching is the one attn1 used in this forward; nothing is drawn."""
    if block.use_ada_layer_norm_zero:
        return "module"
    merged = (getattr(block, "merge_mlp", False) is True and plan is not None and plan.keep is not None
              and plan.inv_local is not None)
    if fused_ff_ok(block.norm3, block.ff, hidden_states):
        return "merged-panels" if merged else "panels"
    if merged:
        return "merged"
    return "f32" if f32_ff_ok(block, block.norm3, block.ff, hidden_states) else "module"


def module_feed_forward_residual(norm: torch.nn.Module, ff: torch.nn.Module, hidden_states: torch.Tensor, ada=None
                                 ) -> torch.Tensor:
    """patch.py:187-199 as written, the "module" feed-forward of ``ff_route``: ``ff(norm3(h)) + h`` through ``layer_norm`` and
    ``feed_forward``.  ``ada``: an AdaLayerNormZero block's (shift_mlp, scale_mlp, gate_mlp) of this forward's norm1, each
    (B F, C); None on every other block."""
    norm_hidden_states = layer_norm(norm, hidden_states)
    if ada is None:
        return feed_forward(ff, norm_hidden_states) + hidden_states
    shift_mlp, scale_mlp, gate_mlp = ada
    norm_hidden_states = norm_hidden_states * (1 + scale_mlp[:, None]) + shift_mlp[:, None]
    return gate_mlp.unsqueeze(1) * feed_forward(ff, norm_hidden_states) + hidden_states


def feed_forward_segment(block: torch.nn.Module, hidden_states: torch.Tensor, plan: Optional["MergePlan"], route: str,
                         ada=None) -> torch.Tensor:
    """The block's feed-forward segment on the body ``route`` (what ``ff_route`` answered for this call) names; ``ada`` goes to
    the "module" body alone -- no other route is taken on an AdaLayerNormZero block."""
    if route in ("merged-panels", "merged"):
        return merged_feed_forward_residual(block, hidden_states, plan, route)
    if route == "panels":
        return norm_feed_forward_residual(block.norm3, block.ff, hidden_states)
    if route == "f32":
        return norm_feed_forward_f32(block.norm3, block.ff, hidden_states)
    return module_feed_forward_residual(block.norm3, block.ff, hidden_states, ada)


def merged_feed_forward_residual(block: torch.nn.Module, hidden_states: torch.Tensor, plan: "MergePlan", route: str
                                 ) -> torch.Tensor:
    """The "merged-panels" / "merged" feed-forward of ``ff_route``: with h the hidden states joined per sample (B, L, C),
    ``y = ff(norm3(h[b, keep[b, :]]))`` over M_l rows instead of L, ``out[b, i] = y[b, inv_local[b, i]] + h[b, i]``."""
    norm, ff = block.norm3, block.ff
    fs = plan.fsize
    hj = join_frame(hidden_states.contiguous(), fs)
    B, L, C = hj.shape
    keep, inv_local = plan.keep, plan.inv_local
    Ml = keep.shape[1]
    if route == "merged-panels":
        # (the panels of all samples are one row range: sample b at rows b * M_l, like norm_feed_forward_residual's b * L)
        weights = _ff_panel_weights(ff)
        xp = _lib.layernorm_gather(hj, keep, norm.weight, norm.bias, norm.eps)
        y = _ff_panels(weights, xp, B * Ml).view(B, Ml, C)
    else:
        if _lib_layernorm_ok(norm, hj):
            xn = _lib.layernorm_gather(hj, keep, norm.weight, norm.bias, norm.eps, panels=False)
        else:
            xn = norm(_lib.gather_rows(hj, None, keep))
        y = feed_forward(ff, xn)
        if y.dtype != hj.dtype:                 # (a ff that changes the dtype: the add promotes like `ff_output + hidden_states`)
            return split_frame(torch.gather(y, 1, inv_local.long()[:, :, None].expand(-1, -1, C)) + hj, fs)
    return split_frame(_lib.unmerge_add(y.contiguous(), inv_local, hj), fs)


def cross_merge_route(block: torch.nn.Module, hidden_states: torch.Tensor, plan: Optional["MergePlan"],
                      route: "Attn2Route", encoder_hidden_states=None, encoder_attention_mask=None) -> str:
    """How the block computes its attn2 segment on hidden states like ``hidden_states`` (B F, N, C) behind the attn1 segment
    whose compute_merge gave ``plan`` (None: nothing merged), ``route`` being what ``attn2_route`` answered for this call.
    Launches nothing.
      "merged-panels"  ``u(attn2(norm2(m(h)), context)) + h`` over the local levels' closures (tomesd's merge_crossattn), every
                       merged row attending to the conditioning of the frame its kept token lives in
                       (``merged_cross_attention_residual``)
      "plain"          today's attn2 over every token, whatever ``route`` says.  Whenever ANY of these holds: the block's
                       ``merge_crossattn`` opt-in (``update_patch(model, merge_crossattn=True)``) is unset; there is no local
                       map -- a site that does not merge, a single-frame chunk, local_merge_ratio <= 0; the route is not the
                       plain "panels" frame -- "module", "blas", "f32", an AdaLayerNorm block; an ``encoder_attention_mask``
                       is present; the call is an IP-Adapter one; the block is registered for cross-attention control
                       (injecting at this step or not), attention maps or LocalBlend -- all of these read or edit per-token
                       rows; ``encoder_hidden_states`` is not a tensor with one row set per frame row (B F of them).
    The global level plays no part, as in ``ff_route``; the matching is the one attn1 used in this forward; nothing is
    drawn."""
    if (getattr(block, "merge_crossattn", False) is not True or plan is None or plan.keep is None or plan.inv_local is None
            or route.frame != "panels" or route.ip is not None or block.use_ada_layer_norm
            or encoder_attention_mask is not None
            or block.__dict__.get("vtm_cross_control") is not None or getattr(block, "vtm_attention_maps", False)
            or local_blend_of(block) is not None
            or not isinstance(encoder_hidden_states, torch.Tensor) or encoder_hidden_states.dim() != 3
            or hidden_states.dim() != 3 or encoder_hidden_states.shape[0] != hidden_states.shape[0]
            or hidden_states.shape[0] % plan.fsize or hidden_states.shape[1] * plan.fsize != plan.L):
        return "plain"
    return "merged-panels"


def merged_cross_attention_residual(block: torch.nn.Module, hidden_states: torch.Tensor, encoder_hidden_states: torch.Tensor,
                                    plan: "MergePlan") -> torch.Tensor:
    """The "merged-panels" attn2 segment of ``cross_merge_route``: with h the hidden states joined per sample (B, L, C),
    L = F N, ``y[b, j] = attn2(norm2(h[b, keep[b, j]]), encoder_hidden_states[b F + keep[b, j] // N])`` over M_l rows
    instead of L, ``out[b, i] = y[b, inv_local[b, i]] + h[b, i]``.  The kept rows are taken in frame order
    (``MergePlan.frame_order``: a permutation of the M_l rows that the unmerge map undoes), so the rows of one frame are one
    segment of the merged sequence and the core serves it with that frame's keys: vtm_layernorm_gather -> panels, the q panel
    GEMM, k / V^T of every frame row's conditioning as today (``_cross_kv``), vtm_attention_kv_segments, the output panel GEMM
    with bias, vtm_unmerge_add with the residual."""
    norm, attn = block.norm2, block.attn2
    fs = plan.fsize
    hj = join_frame(hidden_states.contiguous(), fs)
    B, L, C = hj.shape
    N = L // fs
    keep_sorted, inv_sorted, seg_off = plan.frame_order()
    Ml = keep_sorted.shape[1]
    n = B * Ml
    wq, bq = _panel_weight(attn.to_q)
    wo, bo = _panel_weight(_out_linear(attn))
    # (the panels of all samples are one row range: sample b at rows b * M_l -- what seg_off counts in)
    xp = _lib.layernorm_gather(hj, keep_sorted, norm.weight, norm.bias, norm.eps)
    q = _lib.linear_panels(xp, n, wq, C, bq)                               # (n, C)
    k, vt = _cross_kv(attn.to_k, attn.to_v, _pad_keys(encoder_hidden_states, q.dtype), C, "panels")
    o = _lib.attention_kv_segments(q, k, vt, attn.heads, seg_off, N, encoder_hidden_states.shape[1], _scale(attn, C))
    y = _lib.linear_panels(_lib.to_panels(o), n, wo, C, bo).view(B, Ml, C)
    return split_frame(_lib.unmerge_add(y, inv_sorted, hj), fs)


# ----------------------------------------------------------------------------------------------------
# patched block
# ----------------------------------------------------------------------------------------------------
def patched_self_attention_segment(block: torch.nn.Module, hidden_states: torch.Tensor,
                                   norm_hidden_states: torch.Tensor, encoder_hidden_states=None,
                                   attention_mask=None, cross_attention_kwargs=None, gate_msa=None,
                                   route: Optional[str] = None, plan_to: Optional[list] = None) -> torch.Tensor:
    """patch.py:148-169: compute_merge -> attn1(merged) -> unmerge -> + residual.  ``route``: what ``attn1_route`` answered
    for this call, when the caller has asked already.  ``plan_to``: a list of the caller's that receives this call's
    MergePlan (None at a site that does not merge) -- how the block's feed-forward reads the maps of THIS forward (``ff_route``)
    without anything being kept on the module."""
    cross_attention_kwargs = cross_attention_kwargs if cross_attention_kwargs is not None else {}
    if route is None:
        route = attn1_route(block, norm_hidden_states, encoder_hidden_states, attention_mask, cross_attention_kwargs,
                            gate_msa)
    _pag_check(block, norm_hidden_states, route)
    if sag_registered(block):
        # (these bodies hold no 16-bit q | k rows of the whole frame side by side: the restatement on norm1's output)
        _sag_check(block, norm_hidden_states)
        block.attn1_key_mass = _module_path_key_mass(block.attn1, norm_hidden_states)
    # ("module" and "blas" read the merged tokens; the other routes' projections gather through the map)
    m_a, u_a, merged = compute_merge(block, norm_hidden_states, block._tome_info, materialize=route in ("module", "blas"))
    plan = getattr(m_a, "plan", None)
    if plan_to is not None:
        plan_to.append(plan)
    attn = block.attn1
    if route == "module":
        # not the hot path (SD never masks self-attention nor makes attn1 a cross-attention; LoRA'd / custom
        # attention modules are not the plain arithmetic): run the module's own attention on the merged tokens
        # exactly as the reference does
        if pag.registered(attn) is not None:
            raise RuntimeError("vidtome_amd: this block is registered for perturbed attention (register_perturbed_attention) "
                               "but its attn1 call keeps the module's own forward, which knows nothing of it (a mask, "
                               "processor kwargs, an AdaLayerNormZero gate, PnP sharing or a module that is not the plain "
                               "arithmetic)")
        M = plan.M if plan is not None else merged.shape[1]
        attn_output = attn(merged[:, :M],
                           encoder_hidden_states=encoder_hidden_states if block.only_cross_attention else None,
                           attention_mask=attention_mask, **cross_attention_kwargs)
    else:
        # (PnP injection reads the source sample's q for every group: the live rows must be the same rows in every sample,
        # which align_batch guarantees -- the levels' indices are computed once on the batch-folded tokens, merge.py:73-76)
        aligned = plan is not None and plan.aligned
        live = (plan is not None and plan.q_rows is not None and gate_msa is None and LIVE_QUERIES
                and (_pnp_share_groups(attn) == 1 or aligned))
        q_rows = plan.q_rows if live else None
        q_count = plan.q_count if live else None
        fp32_core = getattr(block, "fp32_attention", False)
        # perturbed attention: the leading batch the bodies see (the joined chunks; the frame rows where nothing merges)
        n_org = _pag_org(attn, norm_hidden_states.shape[0] if plan is None else plan.x_joined.shape[0])
        if route == "blas":
            attn_output = self_attention(attn, merged, plan.M if plan is not None else None, q_rows, q_count,
                                         fp32_core=fp32_core, aligned=aligned, n_org=n_org)
        else:
            # the pool the projections gather from (block does not merge: per-frame attention on the tokens as they are)
            pool = (norm_hidden_states.contiguous(), None, None) if plan is None else \
                (plan.x_joined, plan.anchors_in, plan.gather_map)
            if route == "panels":
                attn_output = self_attention_panels(attn, *pool, q_rows, q_count, aligned=aligned, n_org=n_org)
            else:                                                         # "rows", "f32": the tokens' dtype says which
                attn_output = self_attention_rows(attn, *pool, q_rows, q_count, plan=plan, fp32_core=fp32_core,
                                                  aligned=aligned, n_org=n_org)
        if live:
            # rows are the chunk's local merged tokens: unmerge with the local levels' map alone
            # (= the global level's unmerge, merge.py:439-460, folded into the choice of queries)
            fs = plan.fsize
            r = join_frame(hidden_states.contiguous(), fs)
            if plan.inv_q is None:                                        # single-frame chunk: no local level
                return split_frame(attn_output[:, :plan.L] + r, fs)
            return split_frame(_lib.unmerge_add(attn_output.contiguous(), plan.inv_q, r), fs)
    if gate_msa is not None:
        attn_output = gate_msa.unsqueeze(1) * attn_output
    if plan is None:
        return attn_output[:, :hidden_states.shape[1]] + hidden_states
    return u_a(attn_output, resid=hidden_states)                          # patch.py:168-169 fused


def layer_norm(norm: torch.nn.Module, x: torch.Tensor) -> torch.Tensor:
    """`self.norm1(hidden_states)` (patch.py:146; also norm2 / norm3, patch.py:173-176, 187): a plain
    torch.nn.LayerNorm over the channel axis runs as vtm_layernorm; anything else (AdaLayerNorm variants,
    unusual shapes) is the module's own business."""
    if _lib_layernorm_ok(norm, x):
        return _lib.layernorm(x, norm.weight, norm.bias, norm.eps)
    return norm(x)


def _lib_layernorm_ok(norm: torch.nn.Module, x: torch.Tensor) -> bool:
    """``norm(x)`` is what vtm_layernorm (and vtm_layernorm_gather with token rows out) computes."""
    return (_plain_layernorm(norm, x) and x.is_cuda and x.shape[-1] % 8 == 0 and x.shape[-1] <= 2048
            and x.dtype in (torch.float16, torch.bfloat16, torch.float32))


_NO_BROADCAST = (None, "", "compute", "compute")


def broadcast_modes(block: torch.nn.Module):
    """(bc, name, attn1's mode, attn2's mode) of this forward under ``broadcast.register_attention_broadcast``: each mode
    "compute" (the segment as ever), "record" (the same, then one vtm_residual_record launch) or "reuse" (the segment is
    replaced by the replay of its cached delta).  An unregistered block: ``_NO_BROADCAST``, nothing looked at.  Launches
    nothing.  Raises, with the block's name, where a registered consumer would silently miss what a skipped segment makes."""
    hit = block.__dict__.get("vtm_broadcast")
    if hit is None:
        return _NO_BROADCAST
    bc, name = hit
    who = f"vidtome_amd: block '{name}' is registered for attention broadcast (register_attention_broadcast) but "
    if block.use_ada_layer_norm or block.use_ada_layer_norm_zero:
        raise RuntimeError(who + "is an AdaLayerNorm / AdaLayerNormZero block: its segments are modulated per timestep "
                                 "(attention broadcast on such a block is not supported)")
    mode1, mode2 = bc.step_modes(name)
    if block.attn2 is None:
        mode2 = "compute"
    if mode2 == "reuse":
        for on, what in ((getattr(block, "vtm_attention_maps", False), "attention maps (register_attention_maps)"),
                         (local_blend_of(block) is not None, "LocalBlend (register_local_blend)"),
                         (block.__dict__.get("vtm_cross_control") is not None,
                          "cross-attention control (register_cross_attention_control)")):
            if on:
                raise RuntimeError(who + f"also for {what}: this step replays attn2, which computes no map")
    if mode1 == "reuse" and sag_registered(block):
        raise RuntimeError(who + "also for self-attention guidance (register_self_attention_guidance): this step replays "
                                 "attn1, which computes no key mass")
    return bc, name, mode1, mode2


def broadcast_feed_forward_residual(bc, name: str, norm: torch.nn.Module, ff: torch.nn.Module, hidden_states: torch.Tensor
                                    ) -> torch.Tensor:
    """The whole block on a step that replays both attentions, where ``ff_route`` answers "panels": h2 = h + d1 + d2 and
    norm3(h2) as k-panels from ONE launch (vtm_residual_replay_layernorm), then ``norm_feed_forward_residual``'s two GEMMs on
    them."""
    weights = _ff_panel_weights(ff)
    h2, xp = bc.replay_layernorm(name, hidden_states, norm)
    n = h2.numel() // h2.shape[-1]
    return _ff_panels(weights, xp, n, h2.view(n, -1)).view(hidden_states.shape)


def make_diffusers_tome_block(block_class: Type[torch.nn.Module]) -> Type[torch.nn.Module]:
    """vidtome/patch.py:119-203: patched class made on the fly, named ToMeBlock, keeps ``_parent``."""

    class ToMeBlock(block_class):
        _parent = block_class

        def forward(self, hidden_states, attention_mask=None, encoder_hidden_states=None,
                    encoder_attention_mask=None, timestep=None, cross_attention_kwargs=None,
                    class_labels=None) -> torch.Tensor:
            bc, bc_name, mode1, mode2 = broadcast_modes(self)                      # broadcast.register_attention_broadcast
            plan = ada = route = None
            if mode1 == "reuse":
                # attn1 is replayed: no norm1, no compute_merge (no draw, no global-token update), so no MergePlan either --
                # merge_mlp / merge_crossattn take their paths over every token ("no local map")
                if mode2 == "reuse":
                    # (attn2's delta rides in the same launch; with the "panels" feed-forward, norm3 does too.  The replay
                    # changes neither shape nor dtype: the route asked here is the feed-forward's below)
                    route = ff_route(self, hidden_states, None)
                    if route == "panels":
                        return broadcast_feed_forward_residual(bc, bc_name, self.norm3, self.ff, hidden_states)
                hidden_states = bc.replay(bc_name, ("attn1", "attn2") if mode2 == "reuse" else ("attn1",), hidden_states)
            else:
                segment_input = hidden_states
                gate_msa = None
                if self.use_ada_layer_norm:                                        # patch.py:139-146
                    norm_hidden_states = self.norm1(hidden_states, timestep)
                elif self.use_ada_layer_norm_zero:
                    norm_hidden_states, gate_msa, *ada = self.norm1(
                        hidden_states, timestep, class_labels, hidden_dtype=hidden_states.dtype)
                else:
                    norm_hidden_states = None

                # 1. self-attention on merged tokens (the hot path)                # patch.py:148-169
                # (merge_mlp / merge_crossattn: the feed-forward and attn2 below read the maps of THIS forward's
                # compute_merge -- carried on a local)
                plans = [] if (getattr(self, "merge_mlp", False) is True
                               or getattr(self, "merge_crossattn", False) is True) else None
                seg_kw = {} if plans is None else {"plan_to": plans}
                if norm_hidden_states is None:
                    hidden_states = self_attention_segment(self, hidden_states, encoder_hidden_states, attention_mask,
                                                           cross_attention_kwargs, **seg_kw)
                else:
                    hidden_states = patched_self_attention_segment(
                        self, hidden_states, norm_hidden_states, encoder_hidden_states, attention_mask,
                        cross_attention_kwargs, gate_msa, **seg_kw)
                plan = plans[-1] if plans else None
                if mode1 == "record":
                    bc.record(bc_name, "attn1", segment_input, hidden_states)

            # 2. cross-attention                                                   # patch.py:171-185
            if mode2 == "reuse":                                                   # attn2 is replayed (with attn1's, above)
                if mode1 != "reuse":
                    hidden_states = bc.replay(bc_name, ("attn2",), hidden_states)
            elif self.attn2 is not None:
                segment_input = hidden_states
                hidden_states = cross_attention_segment(self, hidden_states, encoder_hidden_states, encoder_attention_mask,
                                                        cross_attention_kwargs, timestep, plan)
                if mode2 == "record":
                    bc.record(bc_name, "attn2", segment_input, hidden_states)

            # 3. feed-forward                                                      # patch.py:187-199
            if route is None:
                route = ff_route(self, hidden_states, plan)
            return feed_forward_segment(self, hidden_states, plan, route, ada)

    return ToMeBlock


def hook_tome_model(model: torch.nn.Module):
    """vidtome/patch.py:206-212: forward pre-hook recording the latent (H, W)."""
    def hook(module, args):
        module._tome_info["size"] = (args[0].shape[2], args[0].shape[3])
        return None

    model._tome_info["hooks"].append(model.register_forward_pre_hook(hook))


def hook_tome_module(module: torch.nn.Module):
    """vidtome/patch.py:215-231: lazily create the block generator; all blocks fork the same state so their
    draws stay in lock-step within one pass."""
    def hook(module, args):
        gmode = module._tome_info["args"].get("generator_device", None)
        if not hasattr(module, "generator"):
            module.generator = init_generator(args[0].device, mode=gmode)
        elif module.generator.device != args[0].device and (gmode or GENERATOR_MODE_DEFAULT()) == "device":
            # patch.py:221-224: the model moved to another device -> fork that device's state (opt-in stream only: the
            # default CPU stream does not depend on where the tensors live)
            module.generator = init_generator(args[0].device, fallback=module.generator, mode=gmode)
        return None

    module._tome_info["hooks"].append(module.register_forward_pre_hook(hook))


def GENERATOR_MODE_DEFAULT() -> str:
    from . import utils
    return utils.GENERATOR_MODE


def apply_patch(model: torch.nn.Module, local_merge_ratio: float = 0.9, merge_global: bool = False,
                global_merge_ratio=0.8, max_downsample: int = 2, seed: int = 123, batch_size: int = 2,
                include_control: bool = False, align_batch: bool = False, target_stride: int = 4,
                global_rand=0.5, *, generator_device: Optional[str] = None):
    """vidtome/patch.py:234-334 -- same arguments, defaults, return value and errors.

    One keyword-only addition: ``generator_device`` = None (the process default, VIDTOME_GENERATOR, "cpu" unless set) |
    "cpu" | "device".  "cpu": the block generators fork the CPU RNG state wherever the model lives -- the draw stream of the
    reference's CPU path (the parity oracle).  "device": the reference's own rule (vidtome/utils.py:18-30, patch.py:31-32,
    221-224): on a GPU they fork ``torch.cuda.get_rng_state()`` and draw on the device generator (re-forked when the model
    changes device), which reproduces a GPU run of the reference draw for draw at the price of a host read-back per draw."""
    if generator_device not in (None, "cpu", "device"):
        raise ValueError(f"generator_device must be None, 'cpu' or 'device', got {generator_device!r}")
    _lib.lib()   # fail loudly right here if the HIP library is missing: there is no fallback
    remove_patch(model)                                                            # patch.py:277
    is_diffusers = isinstance_str(model, "DiffusionPipeline") or isinstance_str(model, "ModelMixin")
    if not is_diffusers:
        if not hasattr(model, "model") or not hasattr(model.model, "diffusion_model"):
            raise RuntimeError(
                "Provided model was not a Stable Diffusion / Latent Diffusion model, as expected.")
        # the reference's LDM branch (make_tome_block, patch.py:94-116) unpacks 6 values from the 3-tuple
        # compute_merge returns and cannot run; it is out of scope here as well
        raise RuntimeError("LDM (non-diffusers) models are not supported: the reference's own LDM patch "
                           "path is broken (patch.py:105-106 vs :91)")
    diffusion_model = model.unet if hasattr(model, "unet") else model              # patch.py:290
    if isinstance_str(model, "StableDiffusionControlNetPipeline") and include_control:
        diffusion_models = [diffusion_model, model.controlnet]                     # patch.py:292-295
    else:
        diffusion_models = [diffusion_model]

    for diffusion_model in diffusion_models:
        diffusion_model._tome_info = {                                             # patch.py:298-313
            "size": None,
            "hooks": [],
            "args": {
                "max_downsample": max_downsample,
                "generator": None,
                "seed": seed,
                "batch_size": batch_size,
                "align_batch": align_batch,
                "merge_global": merge_global,
                "global_merge_ratio": global_merge_ratio,
                "local_merge_ratio": local_merge_ratio,
                "global_rand": global_rand,
                "target_stride": target_stride,
                "generator_device": generator_device,          # (not a reference key; see the docstring)
            },
        }
        hook_tome_model(diffusion_model)
        for _, module in diffusion_model.named_modules():
            if isinstance_str(module, "BasicTransformerBlock"):                    # patch.py:319
                module.__class__ = make_diffusers_tome_block(module.__class__)
                module._tome_info = diffusion_model._tome_info
                hook_tome_module(module)
                if not hasattr(module, "use_ada_layer_norm_zero"):                 # patch.py:330-332
                    module.use_ada_layer_norm = False
                    module.use_ada_layer_norm_zero = False
    return model


def _patched_roots(model: torch.nn.Module, controlnet_on_unet: bool):
    """The module trees the reference walks: the UNet (`model.unet` for a pipeline) and, if present, a ControlNet.
    `remove_patch` looks for `.controlnet` on the UNet it just unwrapped (patch.py:338-341, a quirk: a pipeline's
    ControlNet hangs off the pipeline), `update_patch` / `collect_from_patch` on the object they were given
    (patch.py:359-362, 374-377)."""
    unet = model.unet if hasattr(model, "unet") else model
    owner = unet if controlnet_on_unet else model
    return unet, ([unet, owner.controlnet] if hasattr(owner, "controlnet") else [unet])


def remove_patch(model: torch.nn.Module):
    """vidtome/patch.py:337-355: drop the hooks, give every ToMeBlock its parent class back; returns the UNet."""
    unet, roots = _patched_roots(model, controlnet_on_unet=True)
    # the launch planners' pinned counter buffers are written by asynchronous copies the LIBRARY issued (torch's host
    # allocator does not know about them): let the last ones land before the buffers go back to its pool
    if torch.cuda.is_available() and any("_vtm_match_plans" in m.__dict__ for root in roots for m in root.modules()):
        torch.cuda.synchronize()
    for root in roots:
        for module in root.modules():
            info = getattr(module, "_tome_info", None)
            if info is not None:
                for hook in info["hooks"]:
                    hook.remove()
                info["hooks"].clear()
            if module.__class__.__name__ == "ToMeBlock":
                module.__class__ = module._parent
            # the fused path's derived copies of the weights (panel-layout packs, stacked q|k weights): ~0.4-0.5 GB of fp16
            # for SD-1.5; they are rebuilt on demand if the model is patched again
            module.__dict__.pop("_vtm_packed", None)
            module.__dict__.pop("_vtm_wcache", None)
            module.__dict__.pop("_vtm_lora", None)             # folded LoRA weights (lora.linear_params)
            if hasattr(module, "processor"):                   # ... and the same on an IP-Adapter processor's projections
                ip_adapter.drop_caches(module)
            module.__dict__.pop("_vtm_match_plans", None)      # the matcher's launch planners (pinned 32-byte buffers)
            module.__dict__.pop("fp32_attention", None)        # update_patch's opt-in: a later apply_patch starts without it
            module.__dict__.pop("fp32_projections", None)      # (likewise)
            module.__dict__.pop("merge_mlp", None)             # (likewise)
            module.__dict__.pop("merge_crossattn", None)       # (likewise)
            module.__dict__.pop("vtm_attention_maps", None)    # maps.register_attention_maps' switch ...
            module.__dict__.pop("attn2_probs", None)           # ... and the map of the block's last forward
            module.__dict__.pop("vtm_sag", None)               # sag.register_self_attention_guidance's switch ...
            module.__dict__.pop("attn1_key_mass", None)        # ... and the key mass of the block's last forward
            freeu.release(module)                              # freeu.register_freeu's "vtm_freeu": hooks off, s1 .. b2 back
            module.__dict__.pop("vtm_cross_control", None)     # p2p.register_cross_attention_control's schedule and edits
            module.__dict__.pop("vtm_local_blend", None)       # blend.register_local_blend's accumulator
            module.__dict__.pop(pag.MARK, None)                # pag.register_perturbed_attention's marker (on attn1)
            module.__dict__.pop("vtm_broadcast", None)         # broadcast.register_attention_broadcast's schedule and caches
    _lib.release_workspaces()            # the cached scratch buffers of the patched path (re-created on demand)
    return roots[-1]                     # the reference returns its loop variable: the last tree walked


def update_patch(model: torch.nn.Module, **kwargs):
    """vidtome/patch.py:358-370: setattr on every module that carries ``_tome_info`` (the root included);
    returns the last tree walked, like the reference."""
    _, roots = _patched_roots(model, controlnet_on_unet=False)
    for root in roots:
        for module in root.modules():
            if hasattr(module, "_tome_info"):
                for k, v in kwargs.items():
                    setattr(module, k, v)
    return roots[-1]


def collect_from_patch(model: torch.nn.Module, attr="tome"):
    """vidtome/patch.py:373-387: {module name: getattr(module, attr)} over the patched trees."""
    _, roots = _patched_roots(model, controlnet_on_unet=False)
    found = {}
    for root in roots:
        for name, module in root.named_modules():
            if hasattr(module, attr):
                found[name] = getattr(module, attr)
    return found
