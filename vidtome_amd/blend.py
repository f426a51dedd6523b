"""Prompt-to-Prompt LocalBlend on patched blocks: per-word cross-attention maps from the fused attn2 path.

    lb = LocalBlend({0: LocalBlend.word_weights(77, [2]), 2: LocalBlend.word_weights(77, [2])}, num_inputs=3, num_frames=F)
    register_local_blend(pipe, lb, blocks=...)                 # the blocks of ONE resolution
    for t in timesteps:
        pnp.register_time(pipe, t)
        for frame_ids, chunk in chunks:
            lb.set_frames(frame_ids)                           # where generate.py passes batch_idx
            ...one UNet call on a [source | uncond | cond] x frames batch...
        x = pred_next_x(...)
        x = lb.blend(x, x_src)                                 # keeps the source latents outside the mask

LocalBlend accumulates, over blocks and denoising steps, the cross-attention map of a few chosen words per sample group,
pools, normalises and thresholds the sum into a mask and keeps the SOURCE latents outside it.  What it needs of a block is
one float per query row, sum_j w[j] P[i, j] with P the head-averaged probabilities: a registered block adds exactly that
into ``lb``'s fp32 accumulator (G, num_frames, N) with one vtm_attention_word_map launch per group in ``words`` on the q / k
rows its attn2 segment already holds (csrc/attention_words.hip) -- never the (B F, N, K) map.  Under cross-attention
control (p2p.py) the edited map is linear in the probabilities again,
    sum_n w[n] P_edit[i, n] = P_src[i, :] . (M (a o w)) + P_own[i, :] . (b o w),
two launches with transformed weights.  Routes the kernel does not take (fp32 blocks, more than 256 text tokens, module-path
calls) restate the same sum in torch; a block whose map cannot be read RAISES: a blend built on a silently missing block is
wrong.  The block's own output does not depend on the registration, and an unregistered block launches what it launched
before.

The batch is group-major like PnP's and P2P's: sample b = g * Fg + f.  Groups not in ``words`` (the unconditional one) are
not computed.  ``blend`` is one vtm_local_blend launch (csrc/local_blend.hip); its two deliberate differences from P2P --
``pooled > threshold * max`` for ``pooled / max > threshold``, a select for ``x_src + mask * (x - x_src)`` -- are stated
there.  P2P's ``start_blend`` is the caller's: do not call ``blend`` before that step."""
from __future__ import annotations

import math
from typing import Callable, Dict, Iterable, Optional, Sequence, Tuple, Union

import torch

from . import _lib
from .maps import select_blocks
from .patch import _patched_roots

ATTR = "vtm_local_blend"


class LocalBlend:
    """The accumulator of the chosen words' maps and the blend built on it.  ``words``: {group index in 0 ..
    num_inputs - 1: (K,) finite float weights} (group 0 is the source; at least one group, at most 8); ``num_frames``: the
    frames of the whole video; ``threshold`` and ``pool`` (the radius: window 2 pool + 1, P2P's k = 1 is pool = 1) as
    vtm_local_blend takes them.  The fp32 accumulator (len(words), num_frames, N) is allocated at the first registered
    forward, when N and the device are known."""

    def __init__(self, words: Dict[int, Sequence[float]], num_inputs: int, num_frames: int, threshold: float = 0.3,
                 pool: int = 1):
        who = "LocalBlend"
        num_inputs, num_frames = int(num_inputs), int(num_frames)
        if num_inputs < 1 or num_frames < 1:
            raise ValueError(f"{who}: num_inputs and num_frames must be at least 1")
        words = dict(words)
        if not 1 <= len(words) <= _lib.LOCAL_BLEND_MAX_GROUPS:
            raise ValueError(f"{who}: words must name 1 .. {_lib.LOCAL_BLEND_MAX_GROUPS} groups, got {len(words)}")
        rows = []
        for g in sorted(words, key=repr):
            if not isinstance(g, int) or isinstance(g, bool) or not 0 <= g < num_inputs:
                raise ValueError(f"{who}: words are keyed by the group index 0 .. {num_inputs - 1}, got {g!r}")
        self.groups: Tuple[int, ...] = tuple(sorted(words))
        for g in self.groups:
            w = torch.as_tensor(words[g])
            if not w.is_floating_point() and w.dtype not in (torch.int32, torch.int64, torch.bool, torch.uint8):
                raise TypeError(f"{who}: the weights of group {g} must be numbers, got {w.dtype}")
            w = w.detach().to(torch.float32).cpu()
            if w.dim() != 1 or w.numel() < 1:
                raise ValueError(f"{who}: the weights of group {g} must be a (K,) row, got shape {tuple(w.shape)}")
            if not bool(torch.isfinite(w).all()):
                raise ValueError(f"{who}: the weights of group {g} are not finite")
            if rows and w.numel() != rows[0].numel():
                raise ValueError(f"{who}: group {g} has {w.numel()} weights, group {self.groups[0]} has {rows[0].numel()}")
            rows.append(w)
        pool = int(pool)
        if not 0 <= pool <= _lib.LOCAL_BLEND_MAX_POOL:
            raise ValueError(f"{who}: pool = {pool}, a radius of 0 .. {_lib.LOCAL_BLEND_MAX_POOL} is taken")
        threshold = float(threshold)
        if not math.isfinite(threshold):
            raise ValueError(f"{who}: threshold must be finite")
        self.weights = torch.stack(rows).contiguous()          # (G, K) fp32 on the host
        self.num_inputs, self.num_frames, self.threshold, self.pool = num_inputs, num_frames, threshold, pool
        self._acc: Optional[torch.Tensor] = None
        self._frames: Optional[Tuple[int, ...]] = None
        self._on: Dict[torch.device, torch.Tensor] = {}
        self._rows: Dict[tuple, torch.Tensor] = {}
        self._edited: Dict[tuple, tuple] = {}

    @property
    def K(self) -> int:
        return self.weights.shape[1]

    @staticmethod
    def word_weights(K: int, token_indices: Iterable[int]) -> torch.Tensor:
        """The 0 / 1 row of K weights that is 1 on ``token_indices`` (P2P's ``alpha_layers`` of one prompt)."""
        K = int(K)
        if K < 1:
            raise ValueError("LocalBlend.word_weights: K must be at least 1")
        w = torch.zeros(K, dtype=torch.float32)
        for i in token_indices:
            if isinstance(i, bool) or int(i) != i or not 0 <= int(i) < K:
                raise ValueError(f"LocalBlend.word_weights: token index {i!r} does not lie in 0 .. {K - 1}")
            w[int(i)] = 1.0
        return w

    # ---- the caller's side ----
    def set_frames(self, frame_ids: Optional[Iterable[int]] = None) -> None:
        """The absolute frame ids of the chunk the next UNet call carries (per group, in the chunk's order); None: the
        chunk is the whole video, frames 0 .. num_frames - 1."""
        if frame_ids is None:
            self._frames = None
            return
        ids = tuple(int(i) for i in frame_ids)
        if not ids or len(set(ids)) != len(ids) or min(ids) < 0 or max(ids) >= self.num_frames:
            raise ValueError(f"LocalBlend.set_frames: frame ids must be distinct and lie in 0 .. {self.num_frames - 1}, "
                             f"got {list(ids)}")
        self._frames = ids

    def reset(self) -> None:
        """Zero the accumulator (a new video, or a new run over the same one)."""
        if self._acc is not None:
            self._acc.zero_()

    def maps(self, hw: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        """The accumulator as (G, num_frames, h, w), h w = N: ``hw``, or h = w = sqrt(N).  A view, not a copy."""
        if self._acc is None:
            raise RuntimeError("LocalBlend.maps: nothing accumulated yet (no registered block has run)")
        N = self._acc.shape[2]
        if hw is None:
            s = math.isqrt(N)
            if s * s != N:
                raise ValueError(f"LocalBlend.maps: N = {N} tokens per frame is not a square, give hw=(h, w)")
            hw = (s, s)
        h, w = int(hw[0]), int(hw[1])
        if h < 1 or w < 1 or h * w != N:
            raise ValueError(f"LocalBlend.maps: hw = {(h, w)} does not hold N = {N} tokens")
        return self._acc.view(len(self.groups), self.num_frames, h, w)

    def blend(self, x: torch.Tensor, x_src: torch.Tensor, return_mask: bool = False, hw: Optional[Tuple[int, int]] = None,
              out: Optional[torch.Tensor] = None):
        """``x`` inside the mask of the accumulated maps, ``x_src`` outside: both (num_frames, C, H, W) contiguous latents of
        one dtype; ``out`` may be x.  One vtm_local_blend launch on the current stream -- the accumulator is written on the
        streams the registered blocks ran on: with chunks in flight on several streams the caller synchronises first.
        Returns the blended latents, or (latents, mask uint8 (num_frames, H, W))."""
        return _lib.local_blend(self.maps(hw), x, x_src, self.pool, self.threshold, out=out, return_mask=return_mask)

    # ---- the patched block's side (patch.add_word_maps) ----
    def weights_on(self, device) -> torch.Tensor:
        """The (G, K) weights on ``device``, moved once."""
        device = torch.device(device)
        hit = self._on.get(device)
        if hit is None:
            hit = self._on[device] = self.weights.to(device).contiguous()
        return hit

    def edited_weights(self, edit, gi: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """((1, K) M (a o w), (1, K) b o w) on ``device`` for group slot ``gi`` under the CrossEdit ``edit``: computed once per
        (edit, words) pair."""
        device = torch.device(device)
        key = (id(edit), gi, device)
        hit = self._edited.get(key)
        if hit is None or hit[0] is not edit:
            M, a, b = edit.on(device)
            w = self.weights_on(device)[gi]
            hit = self._edited[key] = (edit, torch.mv(M, a * w).reshape(1, -1).contiguous(), (b * w).reshape(1, -1).contiguous())
        return hit[1], hit[2]

    def frame_rows(self, Fg: int, device) -> torch.Tensor:
        """The accumulator rows of the current chunk's ``Fg`` frames, int64 on ``device``."""
        ids = self._frames
        if ids is None:
            if Fg != self.num_frames:
                raise RuntimeError(f"LocalBlend: the call carries {Fg} frames per group and the video has {self.num_frames}: "
                                   "give the chunk's frame ids with set_frames before the UNet call")
            ids = tuple(range(Fg))
        elif len(ids) != Fg:
            raise RuntimeError(f"LocalBlend: set_frames named {len(ids)} frames, the call carries {Fg} per group")
        key = (ids, torch.device(device))
        hit = self._rows.get(key)
        if hit is None:
            if len(self._rows) > 256:
                self._rows.clear()
            hit = self._rows[key] = torch.tensor(ids, dtype=torch.int64, device=device)
        return hit

    def accumulator(self, N: int, device, who: str = "") -> torch.Tensor:
        """The (G, num_frames, N) accumulator, allocated (zeroed) at the first call; a later call with another token count
        or device raises."""
        device = torch.device(device)
        if self._acc is None:
            self._acc = torch.zeros((len(self.groups), self.num_frames, int(N)), dtype=torch.float32, device=device)
        elif self._acc.shape[2] != N:
            raise RuntimeError(f"vidtome_amd: LocalBlend on block '{who}': the block has {N} tokens per frame, the accumulator "
                               f"{self._acc.shape[2]} (one resolution per LocalBlend: register the blocks of one)")
        elif self._acc.device != device:
            raise RuntimeError(f"vidtome_amd: LocalBlend on block '{who}': the block runs on {device}, the accumulator lives "
                               f"on {self._acc.device}")
        return self._acc


def _clear(block: torch.nn.Module) -> None:
    block.__dict__.pop(ATTR, None)


def register_local_blend(model: torch.nn.Module, lb: LocalBlend,
                         blocks: Optional[Union[Iterable[str], Callable[[str, torch.nn.Module], bool]]] = None):
    """Let the selected patched blocks add their word maps into ``lb``: ``model`` and ``blocks`` as for
    ``register_attention_maps`` (None: every patched block of the UNet; names; or a predicate) -- select the blocks of ONE
    resolution, a block of another token count raises at its forward.  Registering again only replaces ``lb`` and the
    selection.  Works beside ``register_attention_maps`` and ``register_cross_attention_control`` on the same block.
    Returns the selected names, sorted."""
    who = "register_local_blend"
    if not isinstance(lb, LocalBlend):
        raise TypeError(f"{who}: lb must be a LocalBlend")
    every, chosen = select_blocks(model, blocks, who)
    for (name, blk, _), on in zip(every, chosen):
        if on:
            setattr(blk, ATTR, (lb, name))
        else:
            _clear(blk)
    return sorted({name for (name, _, _), on in zip(every, chosen) if on})


def unregister_local_blend(model: torch.nn.Module) -> None:
    """Switch the accumulation off everywhere (``remove_patch`` does the same); ``lb`` keeps what it holds."""
    _, roots = _patched_roots(model, controlnet_on_unet=False)
    for root in roots:
        for module in root.modules():
            _clear(module)
