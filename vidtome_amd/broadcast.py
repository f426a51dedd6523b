"""Pyramid attention broadcast on patched blocks: replay a block's cached attn1 / attn2 contribution per frame.

    bc = AttentionBroadcast(scheduler.timesteps, num_frames=F, attn1_every=2, attn2_every=6)
    register_attention_broadcast(pipe, bc)                     # blocks=...: as for register_attention_maps
    for i, t in enumerate(scheduler.timesteps):
        bc.set_step(i)                                         # once per step, before its first UNet call
        for frame_ids, chunk in chunks:                        # every frame of the video once per step
            bc.set_frames(frame_ids)                           # where generate.py passes batch_idx; None: the whole video
            ...one UNet call on a [group 0 | group 1 | ...] x frames batch...
        x = step(...)

Pyramid Attention Broadcast (Zhao et al. 2024; Diffusers' ``apply_pyramid_attention_broadcast``): inside a window of
timesteps an attention's output barely changes from step to step, so it is computed every k-th step and replayed in between.
Per registered block and ``kind`` in ("attn1", "attn2") every step i has a mode, a pure host function of i, the timesteps
t[0 .. n), the window (lo, hi) and ``every``:

    reuse(i)  = i > 0 and lo < t[i] < hi and i % every != 0
    mode(i)   = "reuse"    if reuse(i)
                "record"   elif i + 1 < n and reuse(i + 1)
                "compute"  otherwise                                    (every=None: always "compute")

Diffusers' rule with one call per step, except that a step records only when the next one will read it.

* compute: the segment runs exactly as without the registration -- same launches, same bits.
* record:  the same, then ONE launch stores per frame d = T(float(h_after) - float(h_before)), the segment's contribution
           to the residual stream with its residual add, rounded once to the model dtype T, into row (g, frame id) of a
           whole-video cache (G, num_frames, N, C) (vtm_residual_record, csrc/broadcast.hip).  The delta rather than the
           attention output: the fused routes never materialise the latter, and the delta is the same thing on every route.
* reuse:   the segment does NOT run -- no norm, no compute_merge (no generator draw, no global-token update), no projection,
           no attention core.  h' = T(float(h) + float(d)) with d from row (g, frame id).  When both kinds reuse,
           h1 = T(h + d1), h2 = T(h1 + d2) in one launch, and where the block's feed-forward is the fused one that launch
           also writes norm3(h2) as the GEMM's panels (vtm_residual_replay_layernorm): the block is that launch and the
           feed-forward's two GEMMs.

The batch is group-major like everywhere else: sample b = g * Fg + f, G = B / Fg inferred from the call.  The cache is keyed
(group, frame id), not by call count, so it survives any chunking: every step must cover every frame once (the rule the
solver history and SEGA's momentum state), in any chunks, in any order.  A reuse whose frames were not all recorded at the
latest record step RAISES -- host bookkeeping, no device read; there is no fallback.

Streams: cache rows are written and read on the stream the block runs on.  Chunks in flight on two streams touch disjoint
frames, and a step's streams are joined before the next step (scheduler.run_step does), so a reuse never reads a row
another stream is still writing; nothing here synchronises.

Opt-in, and like ``merge_mlp`` / ``merge_crossattn`` it changes the block's output where it is switched on.  A reuse step of
attn2 on a block registered for attention maps, LocalBlend or cross-attention control, one of attn1 on a block registered
for SAG, and any AdaLayerNorm block RAISE at the forward: each would silently miss a map (or its modulation).  On an
attn1-reuse step there is no MergePlan, so ``merge_mlp`` / ``merge_crossattn`` take their plain paths.  Several UNet calls
per frame and step (SAG's second call) need an ``AttentionBroadcast`` of their own, or unregistered blocks."""
from __future__ import annotations

import math
from typing import Callable, Dict, Iterable, Optional, Sequence, Set, Tuple, Union

import torch

from . import _lib
from .maps import select_blocks
from .patch import _patched_roots

ATTR = "vtm_broadcast"
KINDS = ("attn1", "attn2")


class AttentionBroadcast:
    """The schedule and the per-block caches.  ``timesteps``: the run's timestep list t[0 .. n); ``num_frames``: the frames of
    the whole video; ``attn1_every`` / ``attn2_every``: k, an int >= 1 (1 never reuses) or None (off); ``attn1_window`` /
    ``attn2_window``: (lo, hi), a step reuses only where lo < t < hi.  Defaults as Diffusers' for spatial attention (every 2)
    and cross attention (every 6) in (100, 800)."""

    def __init__(self, timesteps: Iterable, num_frames: int, attn1_every: Optional[int] = 2, attn2_every: Optional[int] = 6,
                 attn1_window: Tuple[float, float] = (100, 800), attn2_window: Tuple[float, float] = (100, 800)):
        who = "AttentionBroadcast"
        if isinstance(timesteps, torch.Tensor):
            timesteps = timesteps.detach().cpu().tolist()
        ts = [float(t) for t in timesteps]
        if not ts or not all(math.isfinite(t) for t in ts):
            raise ValueError(f"{who}: timesteps must be a non-empty list of finite numbers")
        num_frames = int(num_frames)
        if num_frames < 1:
            raise ValueError(f"{who}: num_frames must be at least 1")
        every, windows = [], []
        for kind, k, w in (("attn1", attn1_every, attn1_window), ("attn2", attn2_every, attn2_window)):
            if k is not None and (isinstance(k, bool) or not isinstance(k, int) or k < 1):
                raise ValueError(f"{who}: {kind}_every must be None or an int >= 1, got {k!r}")
            try:
                lo, hi = (float(v) for v in w)
            except (TypeError, ValueError):
                raise ValueError(f"{who}: {kind}_window must be a pair (lo, hi), got {w!r}") from None
            if math.isnan(lo) or math.isnan(hi) or lo > hi:
                raise ValueError(f"{who}: {kind}_window must be (lo, hi) with lo <= hi, got {w!r}")
            every.append(k)
            windows.append((lo, hi))
        self.timesteps: Tuple[float, ...] = tuple(ts)
        self.num_frames = num_frames
        self.every: Tuple[Optional[int], Optional[int]] = tuple(every)
        self.windows: Tuple[Tuple[float, float], Tuple[float, float]] = tuple(windows)
        self._step: Optional[int] = None
        self._frames: Optional[Tuple[int, ...]] = None
        self._cache: Dict[Tuple[str, str], torch.Tensor] = {}
        self._recorded: Dict[Tuple[str, str], Tuple[int, Set[int]]] = {}       # the last record step and its frames
        self._rows: Dict[tuple, torch.Tensor] = {}

    # ---- the schedule: pure, on the host ----
    def _reuse(self, k: int, i: int) -> bool:
        every, (lo, hi) = self.every[k], self.windows[k]
        return every is not None and i > 0 and lo < self.timesteps[i] < hi and i % every != 0

    def _mode(self, k: int, i: int) -> str:
        if self._reuse(k, i):
            return "reuse"
        return "record" if i + 1 < len(self.timesteps) and self._reuse(k, i + 1) else "compute"

    def modes(self, i: int) -> Tuple[str, str]:
        """(attn1's mode, attn2's mode) of step ``i``, each "compute", "record" or "reuse"."""
        if isinstance(i, bool) or int(i) != i or not 0 <= int(i) < len(self.timesteps):
            raise ValueError(f"AttentionBroadcast.modes: step {i!r} does not lie in 0 .. {len(self.timesteps) - 1}")
        return self._mode(0, int(i)), self._mode(1, int(i))

    # ---- the caller's side ----
    def set_step(self, i: int) -> None:
        """The index into ``timesteps`` of the step the next UNet calls belong to."""
        self.modes(i)
        self._step = int(i)

    def set_frames(self, frame_ids: Optional[Iterable[int]] = None) -> None:
        """The absolute frame ids of the chunk the next UNet call carries (per group, in the chunk's order); None: the
        chunk is the whole video, frames 0 .. num_frames - 1."""
        if frame_ids is None:
            self._frames = None
            return
        ids = tuple(int(i) for i in frame_ids)
        if not ids or len(set(ids)) != len(ids) or min(ids) < 0 or max(ids) >= self.num_frames:
            raise ValueError(f"AttentionBroadcast.set_frames: frame ids must be distinct and lie in 0 .. {self.num_frames - 1}, "
                             f"got {list(ids)}")
        self._frames = ids

    def cache(self, name: str, kind: str) -> torch.Tensor:
        """The (G, num_frames, N, C) delta cache of block ``name`` and ``kind`` ("attn1" | "attn2"): allocated (uninitialised)
        at the block's first record; rows are valid where a record step wrote them."""
        if kind not in KINDS:
            raise ValueError(f"AttentionBroadcast.cache: kind must be one of {KINDS}, got {kind!r}")
        try:
            return self._cache[(name, kind)]
        except KeyError:
            raise RuntimeError(f"AttentionBroadcast.cache: block '{name}' has recorded no {kind} yet") from None

    def nbytes(self) -> int:
        """Device bytes the caches hold (SD-1.5 at 512 x 512: about 23 MB per frame, group and kind over all blocks)."""
        return sum(c.numel() * c.element_size() for c in self._cache.values())

    def reset(self) -> None:
        """Drop the caches and the bookkeeping (a new video, or a new run): the next record allocates again."""
        self._cache.clear()
        self._recorded.clear()
        self._rows.clear()
        self._step = None

    # ---- the patched block's side (patch.ToMeBlock.forward) ----
    def step_modes(self, who: str) -> Tuple[str, str]:
        if self._step is None:
            raise RuntimeError(f"vidtome_amd: attention broadcast on block '{who}': call set_step(i) before the step's UNet calls")
        return self._mode(0, self._step), self._mode(1, self._step)

    def _chunk(self, who: str, h: torch.Tensor) -> Tuple[Tuple[int, ...], Optional[torch.Tensor], int]:
        """(frame ids, their device int32 tensor or None for the whole video in order, G) of the call ``h`` (B, N, C) belongs to."""
        if h.dim() != 3:
            raise RuntimeError(f"vidtome_amd: attention broadcast on block '{who}': hidden states must be (B F, N, C), got "
                               f"{tuple(h.shape)}")
        ids = self._frames if self._frames is not None else tuple(range(self.num_frames))
        Fg = len(ids)
        if h.shape[0] % Fg:
            raise RuntimeError(f"vidtome_amd: attention broadcast on block '{who}': the call carries {h.shape[0]} samples, not a "
                               f"multiple of the chunk's {Fg} frames (group-major batch; give the chunk's frame ids with "
                               "set_frames before the UNet call)")
        if self._frames is None:
            return ids, None, h.shape[0] // Fg
        key = (ids, h.device)
        dev = self._rows.get(key)
        if dev is None:
            if len(self._rows) > 256:
                self._rows.clear()
            dev = self._rows[key] = torch.tensor(ids, dtype=torch.int32, device=h.device)
        return ids, dev, h.shape[0] // Fg

    def _check_cache(self, who: str, kind: str, c: torch.Tensor, h: torch.Tensor, G: int) -> None:
        want = (G, self.num_frames, h.shape[1], h.shape[2])
        if tuple(c.shape) != want or c.dtype != h.dtype or c.device != h.device:
            raise RuntimeError(f"vidtome_amd: attention broadcast on block '{who}': the {kind} cache is {tuple(c.shape)} "
                               f"{c.dtype} on {c.device}, this call needs {want} {h.dtype} on {h.device} (G, N, C, dtype and "
                               "device must not change between calls; reset() starts over)")

    def record(self, who: str, kind: str, h_before: torch.Tensor, h_after: torch.Tensor) -> None:
        """A record step's one extra launch: the delta of the segment into the rows of the chunk's frames."""
        if h_after.shape != h_before.shape or h_after.dtype != h_before.dtype:
            raise RuntimeError(f"vidtome_amd: attention broadcast on block '{who}': the {kind} segment changed the hidden "
                               f"states' shape or dtype ({tuple(h_before.shape)} {h_before.dtype} -> {tuple(h_after.shape)} "
                               f"{h_after.dtype})")
        ids, dev, G = self._chunk(who, h_before)
        c = self._cache.get((who, kind))
        if c is None:
            c = self._cache[(who, kind)] = torch.empty((G, self.num_frames) + tuple(h_before.shape[1:]), dtype=h_before.dtype,
                                                       device=h_before.device)
        self._check_cache(who, kind, c, h_before, G)
        _lib.residual_record(h_before.contiguous(), h_after.contiguous(), c, dev)
        step, seen = self._recorded.get((who, kind), (None, None))
        if step != self._step:
            seen = set()
            self._recorded[(who, kind)] = (self._step, seen)
        seen.update(ids)

    def _readable(self, who: str, kind: str, h: torch.Tensor, ids, G: int) -> torch.Tensor:
        """The cache a reuse step reads, after the bookkeeping: every frame of the chunk recorded at the latest record step."""
        k = KINDS.index(kind)
        last = next(j for j in range(self._step - 1, -1, -1) if self._mode(k, j) == "record")   # (a reuse has one before it)
        step, seen = self._recorded.get((who, kind), (None, set()))
        missing = sorted(set(ids) - seen) if step == last else sorted(ids)
        if missing:
            raise RuntimeError(f"vidtome_amd: attention broadcast on block '{who}': step {self._step} replays {kind}, but frames "
                               f"{missing} were not recorded at step {last} (every step must cover every frame once, with "
                               "set_step / set_frames before its UNet calls)")
        c = self._cache[(who, kind)]
        self._check_cache(who, kind, c, h, G)
        return c

    def replay(self, who: str, kinds: Sequence[str], h: torch.Tensor) -> torch.Tensor:
        """A reuse step of ``kinds`` (one kind, or both in the block's order): one vtm_residual_replay launch."""
        ids, dev, G = self._chunk(who, h)
        caches = [self._readable(who, kind, h, ids, G) for kind in kinds]
        return _lib.residual_replay(h.contiguous(), caches[0], caches[1] if len(caches) > 1 else None, dev)

    def replay_layernorm(self, who: str, h: torch.Tensor, norm: torch.nn.Module) -> Tuple[torch.Tensor, torch.Tensor]:
        """A step that reuses both kinds ahead of the fused feed-forward: (h2 (B F, N, C), the k-panels of norm(h2)) from one
        vtm_residual_replay_layernorm launch."""
        ids, dev, G = self._chunk(who, h)
        c1, c2 = (self._readable(who, kind, h, ids, G) for kind in KINDS)
        return _lib.residual_replay_layernorm(h.contiguous(), c1, c2, dev, norm.weight, norm.bias, norm.eps)


def _clear(block: torch.nn.Module) -> None:
    block.__dict__.pop(ATTR, None)


def register_attention_broadcast(model: torch.nn.Module, bc: AttentionBroadcast,
                                 blocks: Optional[Union[Iterable[str], Callable[[str, torch.nn.Module], bool]]] = None):
    """Switch the broadcast on for the selected patched blocks: ``model`` and ``blocks`` as for ``register_attention_maps``
    (None: every patched block of the UNet; names; or a predicate).  Registering again only replaces ``bc`` and the
    selection.  A ControlNet's block, which carries the name of a UNet block, keeps its caches under "controlnet." + name.
    Returns the selected names, sorted."""
    who = "register_attention_broadcast"
    if not isinstance(bc, AttentionBroadcast):
        raise TypeError(f"{who}: bc must be an AttentionBroadcast")
    every, chosen = select_blocks(model, blocks, who)
    for (name, blk, in_unet), on in zip(every, chosen):
        if on:
            setattr(blk, ATTR, (bc, name if in_unet else "controlnet." + name))
        else:
            _clear(blk)
    return sorted({name for (name, _, _), on in zip(every, chosen) if on})


def unregister_attention_broadcast(model: torch.nn.Module) -> None:
    """Switch the broadcast off everywhere (``remove_patch`` does the same); ``bc`` keeps its caches until ``reset``."""
    _, roots = _patched_roots(model, controlnet_on_unet=False)
    for root in roots:
        for module in root.modules():
            _clear(module)
