"""The caller-side step of a VidToMe pipeline as one launch per chunk: ``GuidedDDIM``.

    sampler = GuidedDDIM.from_scheduler(pipe.scheduler, guidance_scale=7.5, guidance_rescale=0.7)
    for i, t in enumerate(pipe.scheduler.timesteps):
        def process_chunk(chunk):                                # chunk: the frame indices scheduler.get_chunks gives
            unet_out = unet(torch.cat([x[chunk]] * groups), t, ...).sample
            sampler.step(x, unet_out, i, groups=groups, frame_ids=chunk, out=x_next)
        scheduler.run_step(unet, chunks, len(x), process_chunk, streams=streams)
        x, x_next = x_next, x

The reference does this in torch on the caller's stream (generate.py:239-311, invert.py:181-211): per chunk the group slice
``eps.chunk(batch_size)[-2:]``, the classifier-free-guidance combine and ``noises[chunk] = ...``, then one whole-video
``pred_next_x`` after the last chunk.  The update is per frame, so here every chunk writes its own frames of the next latents
(vtm_guided_step, csrc/guided_step.hip), which also drops the one whole-video launch that has to wait for every stream of
``run_step(..., streams=...)``.  Beyond the reference's expression (epsilon prediction, eta = 0; kept bit for bit by
``_lib.cfg_ddim``) it covers what Diffusers' DDIM step covers: v-prediction and sample prediction, ``guidance_rescale``
(``rescale_noise_cfg``: per-frame standard deviations) and ``eta > 0``.  Computed in fp32, every stored value rounded once.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import _lib

PREDICTION_TYPES = {"epsilon": _lib.PRED_EPSILON, "v_prediction": _lib.PRED_V, "sample": _lib.PRED_SAMPLE}
WANT = ("eps", "x0")


def _host_list(values, name: str) -> list:
    if isinstance(values, torch.Tensor):
        return values.detach().cpu().double().tolist() if values.dtype.is_floating_point else values.detach().cpu().tolist()
    try:
        return [v.item() if hasattr(v, "item") else v for v in values]
    except TypeError:
        raise ValueError(f"GuidedDDIM: {name} must be a sequence or a tensor") from None


class GuidedDDIM:
    """DDIM over ``alphas_cumprod`` (indexed by timestep) along ``timesteps`` (descending, as a Diffusers scheduler holds them
    after ``set_timesteps``).  ``guidance_rescale`` applies where there is guidance (``groups >= 2``); ``eta`` is Diffusers'."""

    def __init__(self, alphas_cumprod, timesteps, final_alpha_cumprod=1.0, prediction_type: str = "epsilon",
                 guidance_scale: float = 7.5, guidance_rescale: float = 0.0, eta: float = 0.0):
        if prediction_type not in PREDICTION_TYPES:
            raise ValueError(f"GuidedDDIM: unknown prediction_type {prediction_type!r} (one of {sorted(PREDICTION_TYPES)})")
        # fp32 table entries are exact in float64: the alphas are the scheduler's own values
        self.alphas = [float(a) for a in _host_list(alphas_cumprod, "alphas_cumprod")]
        self.timesteps = [int(t) for t in _host_list(timesteps, "timesteps")]
        if not self.timesteps or any(not 0 <= t < len(self.alphas) for t in self.timesteps):
            raise ValueError(f"GuidedDDIM: timesteps must be a non-empty sequence inside [0, {len(self.alphas)})")
        self.final_alpha = float(final_alpha_cumprod)
        self.prediction_type = prediction_type
        self.guidance_scale, self.guidance_rescale, self.eta = float(guidance_scale), float(guidance_rescale), float(eta)
        if not self.guidance_rescale >= 0.0 or not self.eta >= 0.0:
            raise ValueError("GuidedDDIM: guidance_rescale and eta must be >= 0")

    @classmethod
    def from_scheduler(cls, scheduler, **overrides) -> "GuidedDDIM":
        """From a Diffusers-style DDIM scheduler after ``set_timesteps``: reads ``alphas_cumprod``, ``timesteps``,
        ``final_alpha_cumprod`` and ``config.prediction_type`` (epsilon when the scheduler has none)."""
        kw = dict(final_alpha_cumprod=scheduler.final_alpha_cumprod,
                  prediction_type=getattr(getattr(scheduler, "config", None), "prediction_type", None) or "epsilon")
        kw.update(overrides)
        return cls(scheduler.alphas_cumprod, scheduler.timesteps, **kw)

    def coefficients(self, i: int, inversion: bool = False):
        """(alpha_from, alpha_to, sqrt_alpha, sqrt_beta, c_x0, c_eps, sigma) of step ``i`` in host float64.  The index rule is
        ``pred_next_x``'s (generate.py:282-298), quirks included: sampling goes from alphas[timesteps[i]] to
        alphas[timesteps[i + 1]] (the final alpha at the last step); inversion walks rev = reversed(timesteps) from
        alphas[rev[i - 1]] (the final alpha at i = 0) to alphas[rev[i]]."""
        n = len(self.timesteps)
        i = int(i)
        if not 0 <= i < n:
            raise IndexError(f"GuidedDDIM: step {i} outside [0, {n})")
        if inversion:
            if self.eta != 0.0:
                raise ValueError("GuidedDDIM: inversion is deterministic: eta must be 0")
            rev = self.timesteps[::-1]
            a_from = self.alphas[rev[i - 1]] if i > 0 else self.final_alpha
            a_to = self.alphas[rev[i]]
        else:
            a_from = self.alphas[self.timesteps[i]]
            a_to = self.alphas[self.timesteps[i + 1]] if i < n - 1 else self.final_alpha
        sigma = 0.0
        if self.eta != 0.0:
            sigma = self.eta * math.sqrt((1.0 - a_to) / (1.0 - a_from)) * math.sqrt(1.0 - a_from / a_to)
        c_eps = math.sqrt(max(1.0 - a_to - sigma * sigma, 0.0))
        return a_from, a_to, math.sqrt(a_from), math.sqrt(1.0 - a_from), math.sqrt(a_to), c_eps, sigma

    def step(self, x: torch.Tensor, model_out: torch.Tensor, i: int, *, groups: int = 2, frame_ids=None,
             inversion: bool = False, noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
             out: Optional[torch.Tensor] = None, want: Sequence[str] = ()):
        """Step ``i`` for one chunk, one vtm_guided_step launch on the current stream.  ``x`` (n_frames, C, H, W): the
        whole-video latents; ``model_out`` (groups * F, C, H, W): the UNet output of the chunk, group-major, its last two
        groups the unconditional and the conditional prediction (generate.py:276; under PnP the source group comes first and
        is not read); ``groups = 1``: no guidance (inversion).  ``frame_ids``: the chunk's F frame indices into x (what
        ``scheduler.get_chunks`` gives, any host sequence, or a device int32 tensor, which is not checked); None: the chunk is
        the whole video.  With ``eta > 0`` and no ``noise`` (F, C, H, W), randn of the chunk's shape is drawn from ``generator``.

        ``out`` receives x' in the chunk's rows and may be x (every element is read before it is written).  Without ``out``:
        a NEW tensor when ``frame_ids`` is None (all of it is written), otherwise x itself, updated IN PLACE in the chunk's rows
        -- a new tensor would hold rows nobody wrote.  Returns out, or (out, *asked) with ``want`` naming "eps" and / or "x0":
        chunk-local (F, C, H, W) tensors of the epsilon and the clean-sample prediction."""
        want = (want,) if isinstance(want, str) else tuple(want)
        if any(w not in WANT for w in want) or len(set(want)) != len(want):
            raise ValueError(f"GuidedDDIM.step: want names {want}, known: {WANT}")
        _, _, sqrt_alpha, sqrt_beta, c_x0, c_eps, sigma = self.coefficients(i, inversion)
        tensors = ((x, "x"), (model_out, "model_out")) + (((noise, "noise"),) if noise is not None else ())
        for t, name in tensors:
            if not isinstance(t, torch.Tensor) or t.dim() < 2:
                raise RuntimeError(f"GuidedDDIM.step: {name} must be a (frames, ...) tensor")
        F = x.shape[0] if frame_ids is None else len(frame_ids)
        groups = int(groups)
        if groups < 1 or model_out.shape[0] != groups * F:
            raise RuntimeError(f"GuidedDDIM.step: model_out has {model_out.shape[0]} samples, not {groups} groups x {F} frames")
        if model_out.dtype != x.dtype or (noise is not None and noise.dtype != x.dtype):
            raise RuntimeError(f"GuidedDDIM.step: dtype mismatch: x {x.dtype}, model_out {model_out.dtype}"
                               + (f", noise {noise.dtype}" if noise is not None else ""))
        for t, name in tensors:
            if not t.is_cuda:
                raise RuntimeError(f"GuidedDDIM.step: {name} must live on the GPU (vidtome_amd has no CPU path)")
        if sigma != 0.0 and noise is None:
            noise = torch.randn((F,) + tuple(model_out.shape[1:]), dtype=x.dtype, device=x.device, generator=generator)
        res = _lib.guided_step(x, model_out, sqrt_alpha, sqrt_beta, c_x0, c_eps, sigma, groups=groups, frame_ids=frame_ids,
                               pred_type=PREDICTION_TYPES[self.prediction_type], guidance=self.guidance_scale,
                               rescale=self.guidance_rescale if groups >= 2 else 0.0, noise=noise, out=out,
                               want_eps="eps" in want, want_x0="x0" in want)
        asked = dict(eps=res[1], x0=res[2])
        return res[0] if not want else (res[0],) + tuple(asked[w] for w in want)
