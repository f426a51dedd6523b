"""Self-attention guidance (SAG; Hong et al., Diffusers' ``StableDiffusionSAGPipeline``) on patched blocks.

    register_self_attention_guidance(pipe)                     # the UNet's mid block
    sag = SelfAttentionGuidance(pipe, scale=0.75)
    sampler = GuidedDPMSolver.from_scheduler(sched, group_weights=sag.group_weights(7.5))
    for i, t in enumerate(timesteps):
        for chunk in chunks:
            out = unet(cat([x[chunk]] * 2), t, cond)                                     # leaves attn1_key_mass
            x_deg = sag.degrade(x, out, sampler, i, groups=2, frame_ids=chunk)
            d = unet(x_deg, t, uncond)                                                   # (overwrites attn1_key_mass)
            sampler.step(x, cat([out, d]), i, groups=3, frame_ids=chunk, out=x_next)

SAG blurs the regions of the predicted clean sample the mid block's self-attention looks at most, re-noises the result and
steers away from the model's prediction on it: eps = u + s (c - u) + g (u - d).  What it needs of the block is one float per
token, the attention MASS of the token as a key,
    mass[f, j] = sum_i (1 / h) sum_head P[f, head, i, j]         (its mean over j is exactly 1),
never the (B F, h, N, N) probabilities a storing attention processor materialises.  A registered block leaves
``block.attn1_key_mass`` after every forward: (B F, N) fp32, new on every forward, no autograd history, on the stream the
block ran on -- one vtm_attention_key_mass launch on the q | k row ranges of the qkv buffer the un-merged attn1 body already
holds (csrc/attention_mass.hip); every other attn1 body at an un-merged site gets it from an fp32 torch restatement of
to_q / to_k on norm1's output (patch._module_path_key_mass), or None with one warning where the projections cannot be read.
An edit is never silently dropped: a registered block RAISES when its site merges tokens, when a frame has more than 4096
tokens (the kernel's key limit), under perturbed attention and under PnP sharing.  The block's output does not depend on
the registration, and an unregistered block launches what it launched before.

``SelfAttentionGuidance.degrade`` is one vtm_sag_degrade launch per chunk (csrc/sag.hip): threshold, nearest-neighbour
upsample, x0 / eps by the sampler's prediction type, masked Gaussian blur, re-noise.  Its three deliberate differences from
the Diffusers pipeline -- the mask selects instead of multiplying, the upsample index is an integer division, the blur is
fp32 and rounded once -- are stated in include/vidtome_hip.h.  The final sum is ``GuidedDPMSolver(group_weights=...)`` over
cat([unet_out, degraded_out]): ``group_weights`` gives the weights."""
from __future__ import annotations

import math
from typing import Callable, Iterable, Optional, Union

import torch

from . import _lib
from .maps import _patched_blocks, select_blocks
from .patch import _patched_roots
from .sampler import PREDICTION_TYPES, GuidedDDIM, GuidedDPMSolver

FLAG, ATTR = "vtm_sag", "attn1_key_mass"
MID_BLOCK = "mid_block.attentions.0.transformer_blocks.0"


def _clear(block: torch.nn.Module) -> None:
    block.__dict__.pop(FLAG, None)
    block.__dict__.pop(ATTR, None)


def register_self_attention_guidance(model: torch.nn.Module,
                                     blocks: Optional[Union[Iterable[str], Callable[[str, torch.nn.Module], bool]]] = None):
    """Switch the attn1 key mass on: ``model`` is what ``apply_patch`` took.  ``blocks`` = None: the UNet's
    ``mid_block.attentions.0.transformer_blocks.0`` when it is a patched block (else this raises and asks for names); an
    iterable of module names or a predicate, as ``maps.select_blocks`` defines them.  Registering again only changes the
    selection: blocks no longer selected lose the switch and their stored mass.  Returns the selected names, sorted."""
    who = "register_self_attention_guidance"
    if blocks is None:
        every, _ = select_blocks(model, None, who)
        if not any(name == MID_BLOCK and in_unet for name, _, in_unet in every):
            raise RuntimeError(f"{who}: the UNet has no patched block {MID_BLOCK!r}: name the blocks (the keys "
                               "collect_from_patch returns)")
        chosen = [name == MID_BLOCK and in_unet for name, _, in_unet in every]
    else:
        every, chosen = select_blocks(model, blocks, who)
    for (name, blk, _), on in zip(every, chosen):
        if on:
            setattr(blk, FLAG, True)
        else:
            _clear(blk)
    return sorted({name for (name, _, _), on in zip(every, chosen) if on})


def unregister_self_attention_guidance(model: torch.nn.Module) -> None:
    """Switch the key mass off everywhere and drop the stored ones (``remove_patch`` does the same)."""
    _, roots = _patched_roots(model, controlnet_on_unet=False)
    for root in roots:
        for module in root.modules():
            _clear(module)


class SelfAttentionGuidance:
    """The host side of SAG for ``model`` (what ``apply_patch`` took): ``scale`` g of the guidance term g (u - d);
    ``blur_sigma`` and ``kernel_size`` (odd, at most 9: the blur radius is (kernel_size - 1) / 2) of the Gaussian;
    ``threshold`` of the key mass (1.0 is its mean); ``block``: the registered block's name when more than one is registered."""

    def __init__(self, model: torch.nn.Module, scale: float = 0.75, blur_sigma: float = 1.0, kernel_size: int = 9,
                 threshold: float = 1.0, block: Optional[str] = None):
        who = "SelfAttentionGuidance"
        kernel_size = int(kernel_size)
        if kernel_size < 1 or kernel_size % 2 != 1 or kernel_size > 2 * _lib.SAG_MAX_RADIUS + 1:
            raise ValueError(f"{who}: kernel_size = {kernel_size}: an odd size of 1 .. {2 * _lib.SAG_MAX_RADIUS + 1} is taken")
        self.scale, self.blur_sigma, self.threshold = float(scale), float(blur_sigma), float(threshold)
        if not self.blur_sigma > 0.0 or not math.isfinite(self.blur_sigma):
            raise ValueError(f"{who}: blur_sigma = {blur_sigma} must be positive and finite")
        if not math.isfinite(self.scale) or math.isnan(self.threshold):
            raise ValueError(f"{who}: scale must be finite and threshold a number")
        self.radius = (kernel_size - 1) // 2
        self.taps = _lib.gaussian_taps(self.radius, self.blur_sigma)
        self.model, self.block = model, block

    def group_weights(self, guidance_scale: float, cfg: bool = True):
        """What ``GuidedDPMSolver(group_weights=...)`` takes over cat([unet_out, degraded_out]): with classifier-free guidance
        (groups u, c, d) ``(1 - s + g, s, -g)``, i.e. u + s (c - u) + g (u - d); without (groups c, d) ``(1 + g, -g)``."""
        s, g = float(guidance_scale), self.scale
        return (1.0 - s + g, s, -g) if cfg else (1.0 + g, -g)

    def _registered(self):
        found = [(name, blk) for name, blk, _ in _patched_blocks(self.model) if blk.__dict__.get(FLAG) is True]
        if self.block is not None:
            found = [(name, blk) for name, blk in found if name == self.block]
        if len(found) != 1:
            raise RuntimeError(f"SelfAttentionGuidance: {len(found)} registered blocks"
                               + (f" named {self.block!r}" if self.block is not None else "")
                               + ": register one with register_self_attention_guidance, or name it with block=")
        return found[0]

    @staticmethod
    def mass_grid(size, N: int):
        """(h_m, w_m) of a block's N tokens for latents of ``size`` = (H, W): ds = ceil(sqrt(H W / N)), h_m = ceil(H / ds),
        w_m = ceil(W / ds) -- the UNet's stride-2 downsampling; raises when h_m * w_m != N."""
        H, W = int(size[0]), int(size[1])
        ds = int(math.ceil(math.sqrt(H * W / N)))
        h_m, w_m = -(-H // ds), -(-W // ds)
        if h_m * w_m != N:
            raise RuntimeError(f"SelfAttentionGuidance: {N} tokens are not the ({h_m}, {w_m}) grid of ({H}, {W}) latents at "
                               f"downsample {ds}")
        return h_m, w_m

    def degrade(self, x: torch.Tensor, model_out: torch.Tensor, sampler, i: int, *, groups: int, group: Optional[int] = None,
                frame_ids=None, mass: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                want_mask: bool = False):
        """The degraded latents of one chunk, one vtm_sag_degrade launch on the current stream.  ``x`` (n_frames, C, H, W):
        the whole-video latents; ``model_out`` (groups * F, C, H, W): the UNet output of the chunk, group-major; ``sampler``:
        a GuidedDDIM or GuidedDPMSolver, whose ``coefficients(i)`` give sqrt_alpha / sqrt_beta of step ``i`` and whose
        prediction type is used; ``group``: the group x0 / eps are taken from, ``groups - 2`` (the unconditional one) or 0
        for ``groups == 1``; ``frame_ids`` as for the samplers' ``step``.  ``mass``: fp32 (F, N) rows, default the registered
        block's ``attn1_key_mass`` rows of that group (the block's last forward: call this between the two UNet calls).
        Returns the chunk-local (F, C, H, W) degraded latents, or (them, mask uint8 (F, H, W)) with ``want_mask``."""
        who = "SelfAttentionGuidance.degrade"
        groups = int(groups)
        if groups < 1:
            raise RuntimeError(f"{who}: groups = {groups}")
        group = (groups - 2 if groups >= 2 else 0) if group is None else int(group)
        if not 0 <= group < groups:
            raise RuntimeError(f"{who}: group = {group} outside [0, {groups})")
        if isinstance(sampler, GuidedDDIM):
            sqrt_alpha, sqrt_beta = sampler.coefficients(i)[2:4]
        elif isinstance(sampler, GuidedDPMSolver):
            sqrt_alpha, sqrt_beta = sampler.coefficients(i)[0:2]
        else:
            raise RuntimeError(f"{who}: sampler must be a GuidedDDIM or a GuidedDPMSolver")
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or not isinstance(model_out, torch.Tensor) or model_out.dim() != 4:
            raise RuntimeError(f"{who}: x must be (n_frames, C, H, W) and model_out (groups * F, C, H, W)")
        H, W = x.shape[2:]
        if H * W > _lib.SAG_MAX_PLANE:
            raise RuntimeError(f"{who}: frames of {H} x {W} latents: vtm_sag_degrade takes a plane of at most "
                               f"{_lib.SAG_MAX_PLANE} elements (128 x 128 latents; two fp32 planes of it live in a "
                               "workgroup's LDS)")
        if model_out.shape[0] % groups:
            raise RuntimeError(f"{who}: model_out has {model_out.shape[0]} rows for {groups} groups")
        F = model_out.shape[0] // groups
        if mass is None:
            name, blk = self._registered()
            stored = blk.__dict__.get(ATTR)
            if stored is None:
                raise RuntimeError(f"{who}: block {name!r} holds no attn1_key_mass (no forward yet, or its projections could "
                                   "not be read)")
            if stored.shape[0] != groups * F:
                raise RuntimeError(f"{who}: block {name!r} holds the key mass of {stored.shape[0]} samples, the chunk has "
                                   f"{groups} groups of {F} frames (the degraded pass overwrites it: call degrade between "
                                   "the two UNet calls)")
            mass = stored[group * F:(group + 1) * F]
            size = blk._tome_info["size"] or (H, W)
        else:
            size = (H, W)
        if not isinstance(mass, torch.Tensor) or mass.dim() != 2:
            raise RuntimeError(f"{who}: mass must be fp32 (F, N)")
        if tuple(size) != (H, W):
            raise RuntimeError(f"{who}: the block saw latents of {tuple(size)}, x is ({H}, {W})")
        h_m, w_m = self.mass_grid(size, mass.shape[1])
        return _lib.sag_degrade(x, model_out, mass, h_m, w_m, sqrt_alpha, sqrt_beta, self.taps, self.threshold, groups=groups,
                                group=group, frame_ids=frame_ids, pred_type=PREDICTION_TYPES[sampler.prediction_type], out=out,
                                want_mask=want_mask)
