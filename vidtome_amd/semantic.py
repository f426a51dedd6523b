"""Semantic guidance (SEGA; Brack et al., Diffusers' ``SemanticStableDiffusionPipeline``) for text-only edits of a video.

    concepts = [EditConcept(scale=6.0, threshold=0.95, warmup=5), EditConcept(scale=4.0, reverse=True, mask="sum")]
    sega = SemanticGuidance(concepts, guidance_scale=7.5)              # groups: u, c, e_1, e_2
    sampler = GuidedDPMSolver.from_scheduler(sched)                    # or GuidedDDIM: the step takes ONE group
    sega.prepare(x)                                                    # the whole-video momentum, zeroed
    for i, t in enumerate(timesteps):
        for chunk in chunks:
            out = unet(cat([x[chunk]] * sega.groups), t, cat([uncond, cond, edit_1, edit_2]))
            m = sega.combine(out, i, frame_ids=chunk)                  # one vtm_semantic_guidance launch
            sampler.step(x, m, i, groups=1, frame_ids=chunk, out=x_next)

Every edit concept has its own group of the UNet output.  Its term ``g_e = s_e (e - u)`` (``-s_e`` with ``reverse``) is kept
only where its magnitude reaches the ``threshold`` quantile of its plane -- per (frame, channel) plane with ``mask="channel"``
(Diffusers' SEGA), of the channel sum per frame with ``mask="sum"`` (LEDITS++), inside a caller's region with
``"channel+region"`` / ``"sum+region"``, or in the region alone with ``"region"``.  The kept terms, weighted, join the
classifier-free combination together with a momentum buffer that follows them:

    m   = u + s (c - u) + sum_e w_apply[e] (M_e ? g_e : 0) + momentum_scale * nu
    nu' = momentum_beta * nu + (1 - momentum_beta) * sum_e w_acc[e] (M_e ? g_e : 0)

``schedule(i)`` states the step rule once: a concept ACCUMULATES (w_acc = weight) while ``i < cooldown``, it is APPLIED
(w_apply = weight) while ``warmup <= i < cooldown``, and the momentum is applied once every concept has ``i >= warmup`` --
SEGA's "momentum builds up during warm-up".  The term is not linear in the groups, so no set of ``group_weights`` expresses
it; ``combine`` is one launch per chunk (csrc/semantic.hip, contract in include/vidtome_hip.h) whose result the samplers take
with ``groups=1``.  The momentum is a whole-video fp32 tensor addressed by ``frame_ids`` like the solver's history: every step
must combine every frame exactly once, under any chunking.

A LEDITS++-style attention mask is ``LocalBlend.blend(..., return_mask=True)``'s mask passed as ``regions`` (uint8, one
(F, H, W) map per concept) with a ``"sum+region"`` concept.

Deliberate differences from Diffusers, all stated in the header:
  * the mask SELECTS, it does not multiply: equal for finite values, and a NaN / Inf in a masked-off term reaches nothing;
  * the threshold is (float)(a_lo + frac (a_hi - a_lo)) in double on exact order statistics, not torch.quantile's fp32 lerp:
    within a few 1e-6 relative of it, and the masks agree on continuous data (tests/test_semantic_host.py);
  * ``guidance_rescale`` is not combined with semantic guidance: the sampler steps one group, for which rescale is off;
  * concepts are summed with their explicit ``weight``; Diffusers' per-concept softmax re-weighting is not reproduced.
Unsupported input raises; there is no torch fallback."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import _lib

MASK_MODES = {"channel": _lib.SEGA_CHANNEL, "sum": _lib.SEGA_SUM, "region": _lib.SEGA_REGION,
              "channel+region": _lib.SEGA_CHANNEL_REGION, "sum+region": _lib.SEGA_SUM_REGION}


@dataclass(frozen=True)
class EditConcept:
    """One edit concept: ``scale`` s_e >= 0 (``reverse`` steers away: the term's sign flips), ``threshold`` the quantile in
    [0, 1] below which the term is dropped, ``warmup`` / ``cooldown`` the steps it is applied in (``cooldown`` None: to the
    end), ``weight`` its share of the sum, ``mask`` one of channel | sum | region | channel+region | sum+region."""
    scale: float = 5.0
    threshold: float = 0.9
    reverse: bool = False
    warmup: int = 10
    cooldown: Optional[int] = None
    weight: float = 1.0
    mask: str = "channel"

    def __post_init__(self):
        if self.mask not in MASK_MODES:
            raise ValueError(f"EditConcept: mask = {self.mask!r} (one of {sorted(MASK_MODES)})")
        if not 0.0 <= float(self.threshold) <= 1.0:
            raise ValueError(f"EditConcept: threshold = {self.threshold}: a quantile inside [0, 1] is taken")
        if not math.isfinite(float(self.scale)) or float(self.scale) < 0.0 or not math.isfinite(float(self.weight)):
            raise ValueError(f"EditConcept: scale = {self.scale} (finite, >= 0; reverse flips the sign), weight = {self.weight} "
                             "(finite)")
        if int(self.warmup) < 0 or (self.cooldown is not None and int(self.cooldown) < 0):
            raise ValueError(f"EditConcept: warmup = {self.warmup}, cooldown = {self.cooldown}: step counts >= 0")

    @property
    def signed_scale(self) -> float:
        return -float(self.scale) if self.reverse else float(self.scale)


class SemanticGuidance:
    """The caller-side combination of semantic guidance (module docstring).  Group order of ``model_out``: u, c, e_1 .. e_E
    (``cfg=False``: u, e_1 .. e_E, no classifier-free term)."""

    def __init__(self, concepts: Sequence[EditConcept], guidance_scale: float = 7.5, momentum_scale: float = 0.1,
                 momentum_beta: float = 0.4, cfg: bool = True):
        who = "SemanticGuidance"
        self.concepts = list(concepts)
        if any(not isinstance(c, EditConcept) for c in self.concepts):
            raise TypeError(f"{who}: concepts must be EditConcept instances")
        if len(self.concepts) > _lib.SEGA_MAX_CONCEPTS:
            raise ValueError(f"{who}: {len(self.concepts)} concepts: at most {_lib.SEGA_MAX_CONCEPTS} are taken")
        self.guidance_scale, self.momentum_scale, self.momentum_beta = float(guidance_scale), float(momentum_scale), float(momentum_beta)
        if not all(math.isfinite(v) for v in (self.guidance_scale, self.momentum_scale, self.momentum_beta)):
            raise ValueError(f"{who}: guidance_scale, momentum_scale and momentum_beta must be finite")
        self.cfg = bool(cfg)
        self.momentum: Optional[torch.Tensor] = None

    @property
    def groups(self) -> int:
        return (2 if self.cfg else 1) + len(self.concepts)

    def prepare(self, x: torch.Tensor) -> None:
        """Allocate the zeroed whole-video fp32 momentum for the latents ``x`` (n_frames, C, H, W) on the current stream."""
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or not x.is_cuda:
            raise RuntimeError("SemanticGuidance.prepare: x must be (n_frames, C, H, W) latents on the GPU (vidtome_amd has no "
                               "CPU path)")
        self.momentum = torch.zeros(x.shape, dtype=torch.float32, device=x.device)

    def schedule(self, i: int):
        """(w_apply[], w_acc[], mom_apply) of step ``i`` (module docstring): pure host logic."""
        i = int(i)
        if i < 0:
            raise IndexError(f"SemanticGuidance.schedule: step {i}")
        acc = [float(c.weight) if (c.cooldown is None or i < int(c.cooldown)) else 0.0 for c in self.concepts]
        app = [w if i >= int(c.warmup) else 0.0 for c, w in zip(self.concepts, acc)]
        return app, acc, bool(self.concepts) and all(i >= int(c.warmup) for c in self.concepts)

    def combine(self, model_out: torch.Tensor, i: int, *, frame_ids=None, regions: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, want_masks: bool = False):
        """The combined model output of step ``i`` for one chunk: ``model_out`` (groups * F, C, H, W), group-major; ``frame_ids``
        the chunk's rows of the video (None: all, in order); ``regions`` uint8 (E, F, H, W) where a concept's mask names a
        region.  Returns (F, C, H, W) in model_out's dtype -- what ``GuidedDDIM.step`` / ``GuidedDPMSolver.step`` take with
        ``groups=1`` -- or (that, masks uint8 (E, F, C, H, W)) with ``want_masks``.  Updates the momentum rows in place."""
        if self.momentum is None:
            raise RuntimeError("SemanticGuidance.combine: call prepare(x) first (it allocates the momentum)")
        app, acc, mom_apply = self.schedule(i)
        first = 2 if self.cfg else 1
        return _lib.semantic_guidance(model_out, self.groups, 0, 1 if self.cfg else -1, self.guidance_scale,
                                      list(range(first, self.groups)), [c.signed_scale for c in self.concepts],
                                      [float(c.threshold) for c in self.concepts], app, acc,
                                      [MASK_MODES[c.mask] for c in self.concepts], regions=regions, momentum=self.momentum,
                                      frame_ids=frame_ids, mom_scale=self.momentum_scale, mom_beta=self.momentum_beta,
                                      mom_apply=mom_apply, out=out, want_masks=want_masks)
