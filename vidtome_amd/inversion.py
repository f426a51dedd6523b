"""Edit-friendly DDPM inversion (Huberman-Spiegelglas et al., "An Edit Friendly DDPM Noise Space"; LEDITS++, Diffusers'
``LEditsPPPipelineStableDiffusion.invert``) of a real video, one launch per chunk: ``EditFriendlyInversion``.

    solver = GuidedDPMSolver.from_scheduler(sched, algorithm_type="sde-dpmsolver++", solver_order=2, guidance_scale=3.5)
    inv = EditFriendlyInversion(solver)
    levels = inv.noise_levels(x0, generator=g)            # (n + 1, n_frames, C, H, W); levels[n] is x0
    for i, t in enumerate(solver.timesteps):
        def process_chunk(chunk):
            out = unet(torch.cat([levels[i][chunk]] * groups), t, ...).sample
            inv.step(levels, out, i, groups=groups, frame_ids=chunk)
        scheduler.run_step(unet, chunks, len(x0), process_chunk, streams=streams)
    # the edit: sampling from the first level with the stored noise (the solver steps in sequence from step 0)
    x = levels[0].clone()
    for i in range(n):
        ... m = SemanticGuidance.combine(...) ...
        solver_edit.step(x, m, i, groups=1, noise=inv.noise[i][chunk], frame_ids=chunk)

The video is noised to every level INDEPENDENTLY (vtm_noise_levels), which is what makes the noise maps edit friendly.  Then
the levels are walked in sampling order and every step solves the stochastic solver's update for the noise that lands on the
next level (vtm_invert_step, csrc/invert_step.hip), rounds it to the model dtype, and corrects the next level with the
rounded noise.  The kernel shares the forward step's expression (csrc/solver_core.h), so sampling with the stored noise and
the same model outputs reproduces every level bit for bit.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _lib
from .noise import LEVELS, FrameNoise
from .sampler import PREDICTION_TYPES, GuidedDPMSolver, _checked_step


class EditFriendlyInversion:
    """The inversion that belongs to ``solver``, a ``GuidedDPMSolver`` with ``algorithm_type="sde-dpmsolver++"`` (a deterministic
    update has no noise to solve for).  Coefficients, group weights, ``rescale_group``, the guidance rescale, the prediction
    type, the history ring and the rule that steps come in sequence are the solver's own: this class restates none of them,
    and it steps the solver's history, so one solver serves one inversion (or one sampling pass) at a time.

    DDIM with ``eta = 1`` (DDPM ancestral sampling, the scheduler of the edit-friendly paper and of LEDITS++ before its
    DPM-Solver++ variant) is this solver at ``solver_order=1``: an identity of the coefficients,
    ``c_x x + c_x0 x0 + c_noise z == sqrt(a') x0 + sqrt(1 - a' - sigma_t^2) eps + sigma_t z``, so it needs no kernel of its
    own.  ``GuidedDDIM`` with ``0 < eta < 1`` is out of scope.

    With ``final_alpha_cumprod = 1`` the last step has no noise term (c_noise = 0): its noise map is +0, ``levels[n]`` stays the
    caller's ``x0``, and sampling's last step reconstructs the model's clean prediction at the last level, not ``x0``.  With
    ``final_alpha_cumprod < 1`` the last step is solved like every other and ``levels[n]`` (x0, taken as the last level) is
    corrected by the rounding of its noise map.

    ``noise``: (n, n_frames, ...) in the model dtype, step i's noise map in ``noise[i]``; allocated by ``noise_levels``."""

    def __init__(self, solver: GuidedDPMSolver):
        if not isinstance(solver, GuidedDPMSolver):
            raise TypeError("EditFriendlyInversion: solver must be a GuidedDPMSolver")
        if solver.algorithm_type != "sde-dpmsolver++":
            raise ValueError(f"EditFriendlyInversion: algorithm_type {solver.algorithm_type!r} is deterministic: there is no "
                             'noise to solve for (use "sde-dpmsolver++")')
        self.solver = solver
        self.noise: Optional[torch.Tensor] = None

    def level_coefficients(self) -> list:
        """[(sqrt(a_k), sqrt(1 - a_k))] for the n levels the solver steps from, in host float64."""
        return [self.solver._level(k)[:2] for k in range(len(self.solver.timesteps))]

    def noise_levels(self, x0: torch.Tensor, generator: Optional[torch.Generator] = None,
                     noise: Optional[FrameNoise] = None) -> torch.Tensor:
        """The video ``x0`` (n_frames, ...) noised to every level, one vtm_noise_levels launch over randn drawn from
        ``generator``: a NEW (n + 1, n_frames, ...) tensor, ``levels[k] = sqrt(a_k) x0 + sqrt(1 - a_k) N(0, 1)`` for k < n and
        ``levels[n] = x0``.  Also allocates ``noise`` and prepares the solver's history, on the current stream.
        ``noise=FrameNoise(seed)`` in place of ``generator``: the draws are keyed by (seed, LEVELS, level k, frame, element) --
        one vtm_frame_noise launch -- so a frame's levels depend neither on the video's length nor on a generator's state."""
        if noise is not None and not isinstance(noise, FrameNoise):
            raise TypeError("EditFriendlyInversion.noise_levels: noise must be a FrameNoise")
        if noise is not None and generator is not None:
            raise ValueError("EditFriendlyInversion.noise_levels: noise=FrameNoise(...) draws nothing from a generator: pass one "
                             "of the two")
        if not isinstance(x0, torch.Tensor) or x0.dim() < 2:
            raise RuntimeError("EditFriendlyInversion.noise_levels: x0 must be a (frames, ...) tensor")
        if not x0.is_cuda:
            raise RuntimeError("EditFriendlyInversion.noise_levels: x0 must live on the GPU (vidtome_amd has no CPU path)")
        if x0.dtype not in _lib._DT or not x0.is_contiguous():
            raise RuntimeError("EditFriendlyInversion.noise_levels: x0 must be a contiguous fp16 / bf16 / fp32 tensor")
        n = len(self.solver.timesteps)
        levels = torch.empty((n + 1,) + tuple(x0.shape), dtype=x0.dtype, device=x0.device)
        if noise is None:
            levels[:n].normal_(generator=generator)
        elif n:
            noise.with_tag(LEVELS).normal(tuple(x0.shape[1:]), 0, n_frames=x0.shape[0], steps=n, out=levels[:n])
        coef = torch.tensor(self.level_coefficients(), dtype=torch.float32).to(x0.device)
        _lib.noise_levels(x0, levels[:n], coef)
        levels[n].copy_(x0)
        self.noise = torch.empty((n,) + tuple(x0.shape), dtype=x0.dtype, device=x0.device)
        self.solver.prepare(x0)
        return levels

    def step(self, levels: torch.Tensor, model_out: torch.Tensor, i: int, *, groups: int = 2, frame_ids=None,
             want: Sequence[str] = ()):
        """Step ``i`` of the inversion for one chunk, one vtm_invert_step launch on the current stream: reads ``levels[i]``,
        writes the chunk's rows of ``noise[i]`` and corrects those rows of ``levels[i + 1]`` in place.  ``model_out`` (groups *
        F, ...), group-major: the UNet output for ``levels[i][frame_ids]``; ``groups``, ``frame_ids`` and ``want`` are
        ``GuidedDPMSolver.step``'s.  Every step must step every frame exactly once, and steps come in order.  Returns None, or
        the tuple of the chunk-local tensors ``want`` names."""
        who = "EditFriendlyInversion"
        s = self.solver
        n = len(s.timesteps)
        if not isinstance(levels, torch.Tensor) or levels.dim() < 3 or levels.shape[0] != n + 1:
            raise RuntimeError(f"{who}.step: levels must be the ({n + 1}, frames, ...) tensor noise_levels returned")
        if not 0 <= int(i) < n:
            raise IndexError(f"{who}: step {i} outside [0, {n})")
        i = int(i)
        x = levels[i]
        want, (sqrt_alpha, sqrt_beta, c_x, c_x0, c_h1, c_h2, c_noise), F, groups, weights = _checked_step(
            who, x, model_out, None, groups, frame_ids, want, lambda: s.coefficients(i), s.weights, lambda: s._in_sequence(i))
        if not levels.is_cuda:
            raise RuntimeError(f"{who}.step: levels must live on the GPU (vidtome_amd has no CPU path)")
        if not levels.is_contiguous():
            raise RuntimeError(f"{who}.step: levels must be contiguous")
        if self.noise is None or self.noise.shape != levels[:n].shape or self.noise.dtype != levels.dtype \
                or self.noise.device != levels.device:
            raise RuntimeError(f"{who}.step: noise does not fit levels {tuple(levels.shape)}: call noise_levels first")
        if len(s.history) != s.solver_order - 1 or any(h.shape != x.shape or h.device != x.device for h in s.history):
            raise RuntimeError(f"{who}.step: the solver's history does not fit levels {tuple(levels.shape)}: call noise_levels "
                               "first")
        s._current = i
        ring = len(s.history)
        eps, x0 = _lib.invert_step(x, model_out, weights, sqrt_alpha, sqrt_beta, c_x, c_x0, c_h1, c_h2, c_noise,
                                   target=levels[i + 1], z_out=self.noise[i],
                                   h1=s.history[(i - 1) % ring] if c_h1 != 0.0 else None,
                                   h2=s.history[(i - 2) % ring] if c_h2 != 0.0 else None,
                                   h_out=s.history[i % ring] if ring else None,
                                   g_ref=groups - 1 if s.rescale_group is None else s.rescale_group, frame_ids=frame_ids,
                                   pred_type=PREDICTION_TYPES[s.prediction_type],
                                   rescale=s.guidance_rescale if groups >= 2 else 0.0,
                                   want_eps="eps" in want, want_x0="x0" in want)
        asked = dict(eps=eps, x0=x0)
        return tuple(asked[w] for w in want) if want else None
