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

``GuidedDPMSolver`` is the same loop for multistep DPM-Solver++ (fewer UNet evaluations) and for guidance with a weight per
group (vtm_solver_step, csrc/solver_step.hip): its history lives per frame, so it too is stepped chunk by chunk.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import _lib
from .noise import FrameNoise

PREDICTION_TYPES = {"epsilon": _lib.PRED_EPSILON, "v_prediction": _lib.PRED_V, "sample": _lib.PRED_SAMPLE}
WANT = ("eps", "x0")


def _host_list(values, name: str) -> list:
    if isinstance(values, torch.Tensor):
        return values.detach().cpu().double().tolist() if values.dtype.is_floating_point else values.detach().cpu().tolist()
    try:
        return [v.item() if hasattr(v, "item") else v for v in values]
    except TypeError:
        raise ValueError(f"GuidedDDIM: {name} must be a sequence or a tensor") from None


def _checked_step(who: str, x, model_out, noise, groups, frame_ids, want, coefficients, on_groups=None, before_gpu=None):
    """What the ``step`` of both samplers checks, in the order it always did: the names in ``want``; the step's
    ``coefficients()``; x, model_out and noise as (frames, ...) tensors; the group count (then ``on_groups(groups)``, the
    sampler's own look at it); one dtype (then ``before_gpu()``); all on the GPU.  Returns (want as a tuple, the coefficients,
    F, groups, what on_groups gave)."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if any(w not in WANT for w in want) or len(set(want)) != len(want):
        raise ValueError(f"{who}.step: want names {want}, known: {WANT}")
    coef = coefficients()
    tensors = ((x, "x"), (model_out, "model_out")) + (((noise, "noise"),) if noise is not None else ())
    for t, name in tensors:
        if not isinstance(t, torch.Tensor) or t.dim() < 2:
            raise RuntimeError(f"{who}.step: {name} must be a (frames, ...) tensor")
    F = x.shape[0] if frame_ids is None else len(frame_ids)
    groups = int(groups)
    if groups < 1 or model_out.shape[0] != groups * F:
        raise RuntimeError(f"{who}.step: model_out has {model_out.shape[0]} samples, not {groups} groups x {F} frames")
    own = on_groups(groups) if on_groups else None
    if model_out.dtype != x.dtype or (noise is not None and noise.dtype != x.dtype):
        raise RuntimeError(f"{who}.step: dtype mismatch: x {x.dtype}, model_out {model_out.dtype}"
                           + (f", noise {noise.dtype}" if noise is not None else ""))
    if before_gpu:
        before_gpu()
    for t, name in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{who}.step: {name} must live on the GPU (vidtome_amd has no CPU path)")
    return want, coef, F, groups, own


def _keyed(who: str, noise, generator):
    """``noise`` of a step -> (the tensor or None, the FrameNoise or None)."""
    if not isinstance(noise, FrameNoise):
        return noise, None
    if generator is not None:
        raise ValueError(f"{who}.step: noise=FrameNoise(...) draws nothing from a generator: pass one of the two")
    return None, noise


def _asked(res, want):
    """(out, eps, x0) of a step as ``step`` returns it: out, or (out, *asked) in ``want``'s order."""
    asked = dict(eps=res[1], x0=res[2])
    return res[0] if not want else (res[0],) + tuple(asked[w] for w in want)


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
             inversion: bool = False, noise=None, generator: Optional[torch.Generator] = None,
             out: Optional[torch.Tensor] = None, want: Sequence[str] = ()):
        """Step ``i`` for one chunk, one vtm_guided_step launch on the current stream.  ``x`` (n_frames, C, H, W): the
        whole-video latents; ``model_out`` (groups * F, C, H, W): the UNet output of the chunk, group-major, its last two
        groups the unconditional and the conditional prediction (generate.py:276; under PnP the source group comes first and
        is not read); ``groups = 1``: no guidance (inversion).  ``frame_ids``: the chunk's F frame indices into x (what
        ``scheduler.get_chunks`` gives, any host sequence, or a device int32 tensor, which is not checked); None: the chunk is
        the whole video.  With ``eta > 0`` and no ``noise`` (F, C, H, W), randn of the chunk's shape is drawn from ``generator``
        -- noise that depends on the chunking.  ``noise=FrameNoise(seed)`` instead keys the noise by (seed, i, frame, element):
        one vtm_guided_step_keyed launch that draws it in place, the same bits under any chunking, order, rank or stream.

        ``out`` receives x' in the chunk's rows and may be x (every element is read before it is written).  Without ``out``:
        a NEW tensor when ``frame_ids`` is None (all of it is written), otherwise x itself, updated IN PLACE in the chunk's rows
        -- a new tensor would hold rows nobody wrote.  Returns out, or (out, *asked) with ``want`` naming "eps" and / or "x0":
        chunk-local (F, C, H, W) tensors of the epsilon and the clean-sample prediction."""
        noise, keyed = _keyed("GuidedDDIM", noise, generator)
        want, (_, _, sqrt_alpha, sqrt_beta, c_x0, c_eps, sigma), F, groups, _ = _checked_step(
            "GuidedDDIM", x, model_out, noise, groups, frame_ids, want, lambda: self.coefficients(i, inversion))
        if sigma != 0.0 and noise is None and keyed is None:
            noise = torch.randn((F,) + tuple(model_out.shape[1:]), dtype=x.dtype, device=x.device, generator=generator)
        res = _lib.guided_step(x, model_out, sqrt_alpha, sqrt_beta, c_x0, c_eps, sigma, groups=groups, frame_ids=frame_ids,
                               pred_type=PREDICTION_TYPES[self.prediction_type], guidance=self.guidance_scale,
                               rescale=self.guidance_rescale if groups >= 2 else 0.0, noise=noise, out=out,
                               want_eps="eps" in want, want_x0="x0" in want, key=keyed.key(i) if keyed else None)
        return _asked(res, want)


ALGORITHM_TYPES = ("dpmsolver++", "sde-dpmsolver++")


class GuidedDPMSolver:
    """Multistep DPM-Solver++ (Lu et al.; second order = midpoint) over ``alphas_cumprod`` (indexed by timestep) along
    ``timesteps`` (descending), one vtm_solver_step launch per chunk.  It solves the ODE DDIM solves, so it starts from the same
    DDIM-inverted latents, in 20 to 25 steps.  The contract is the formulas below (float64 on the host, folded into five
    coefficients; the launch computes in fp32); nothing is claimed about the bits of a Diffusers release.

        sampler = GuidedDPMSolver.from_scheduler(pipe.scheduler, solver_order=2, guidance_scale=7.5)
        sampler.prepare(x)                                       # the history buffers, before any side stream touches them
        for i, t in enumerate(sampler.timesteps):
            def process_chunk(chunk):
                unet_out = unet(torch.cat([x[chunk]] * groups), t, ...).sample
                sampler.step(x, unet_out, i, groups=groups, frame_ids=chunk, out=x_next)
            scheduler.run_step(unet, chunks, len(x), process_chunk, streams=streams)
            x, x_next = x_next, x

    Levels: a_k = alphas_cumprod[timesteps[k]] for k < n, a_n = final_alpha_cumprod (1.0: the last step lands on sigma = 0);
    alpha = sqrt(a), sigma = sqrt(1 - a), lambda = log(alpha) - log(sigma).  Step i goes from level i (alpha, sigma) to level
    i + 1 (alpha', sigma'); h = lambda_{i+1} - lambda_i, h0 = lambda_i - lambda_{i-1}, h1 = lambda_{i-1} - lambda_{i-2},
    r0 = h0 / h, r1 = h1 / h; m0, m1, m2 are the clean-sample predictions of steps i, i - 1, i - 2.

        order 1:  x' = (sigma'/sigma) x - alpha' (e^-h - 1) m0
        order 2:  D1 = (m0 - m1) / r0 ;   x' = (sigma'/sigma) x - alpha' (e^-h - 1) m0 - 0.5 alpha' (e^-h - 1) D1
        order 3:  D1_0 = (m0 - m1)/r0, D1_1 = (m1 - m2)/r1, D1 = D1_0 + r0/(r0 + r1) (D1_0 - D1_1), D2 = (D1_0 - D1_1)/(r0 + r1)
                  x' = (sigma'/sigma) x - alpha' (e^-h - 1) m0 + alpha' ((e^-h - 1)/h + 1) D1 - alpha' ((e^-h - 1 + h)/h^2 - 0.5) D2
        "sde-dpmsolver++", order 1 / 2:
                  x' = (sigma'/sigma) e^-h x + alpha' (1 - e^-2h) m0 [+ 0.5 alpha' (1 - e^-2h) D1] + sigma' sqrt(1 - e^-2h) noise

    At sigma' = 0 the limits are taken exactly: x' = m0.  The order of step i, ``have`` = min(i, solver_order - 1) being the
    number of earlier predictions there are: 1 when solver_order == 1, or have == 0, or i is the last step and
    (``euler_at_final``, or ``lower_order_final`` and n < 15, or a_n == 1); otherwise 2 when solver_order == 2, or have == 1, or i
    is the second-to-last step and ``lower_order_final`` and n < 15; otherwise 3.

    Guidance: m = sum_g w[g] * model_out[group g].  ``group_weights`` (one per group of the call) gives w -- e.g.
    (1 - s, s + p, -p) for perturbed-attention guidance over (uncond, cond, perturbed), (s_T, s_I - s_T, 1 - s_I) for
    InstructPix2Pix over (text + image, image, none); without it w is (1 - guidance_scale, guidance_scale) on the last two
    groups and 0 before them ((1,) for one group).  A group of weight 0 is never read.  ``guidance_rescale`` (groups >= 2)
    restores the per-frame std of group ``rescale_group`` (default: the last).

    History: solver_order - 1 whole-video fp32 tensors shaped like x, a ring over the step index (step i overwrites the
    prediction of step i - (solver_order - 1), element by element, after reading it).  ``prepare(x)`` allocates them on the
    current stream; the first ``step`` does it when nobody has, which is too late under ``run_step(streams=...)``: there the
    caller prepares first.  Step 0 restarts the history; every step must step EVERY frame exactly once (what
    ``scheduler.get_chunks`` guarantees), and steps come in order: an ``i`` that is neither the current step nor the next
    raises."""

    def __init__(self, alphas_cumprod, timesteps, final_alpha_cumprod=1.0, prediction_type: str = "epsilon",
                 solver_order: int = 2, algorithm_type: str = "dpmsolver++", lower_order_final: bool = True,
                 euler_at_final: bool = False, guidance_scale: float = 7.5, guidance_rescale: float = 0.0,
                 group_weights=None, rescale_group: Optional[int] = None):
        who = "GuidedDPMSolver"
        if prediction_type not in PREDICTION_TYPES:
            raise ValueError(f"{who}: unknown prediction_type {prediction_type!r} (one of {sorted(PREDICTION_TYPES)})")
        if algorithm_type not in ALGORITHM_TYPES:
            raise ValueError(f"{who}: unknown algorithm_type {algorithm_type!r} (one of {ALGORITHM_TYPES})")
        self.solver_order = int(solver_order)
        if not 1 <= self.solver_order <= (2 if algorithm_type == "sde-dpmsolver++" else 3):
            raise ValueError(f"{who}: solver_order {solver_order} ({algorithm_type}: 1 .. "
                             f"{2 if algorithm_type == 'sde-dpmsolver++' else 3})")
        self.alphas = [float(a) for a in _host_list(alphas_cumprod, "alphas_cumprod")]
        self.timesteps = [int(t) for t in _host_list(timesteps, "timesteps")]
        if not self.timesteps or any(not 0 <= t < len(self.alphas) for t in self.timesteps):
            raise ValueError(f"{who}: timesteps must be a non-empty sequence inside [0, {len(self.alphas)})")
        self.final_alpha = float(final_alpha_cumprod)
        levels = [self.alphas[t] for t in self.timesteps]
        if any(not 0.0 < a < 1.0 for a in levels) or not 0.0 < self.final_alpha <= 1.0:
            raise ValueError(f"{who}: every level's alphas_cumprod must lie in (0, 1) (the final one may be 1)")
        self.prediction_type, self.algorithm_type = prediction_type, algorithm_type
        self.lower_order_final, self.euler_at_final = bool(lower_order_final), bool(euler_at_final)
        self.guidance_scale, self.guidance_rescale = float(guidance_scale), float(guidance_rescale)
        if not self.guidance_rescale >= 0.0:
            raise ValueError(f"{who}: guidance_rescale must be >= 0")
        self.group_weights = None if group_weights is None else [float(w) for w in _host_list(group_weights, "group_weights")]
        self.rescale_group = None if rescale_group is None else int(rescale_group)
        self.history: list = []                   # solver_order - 1 fp32 tensors like x; step k's prediction in [k % len]
        self._current: Optional[int] = None       # the step the history belongs to

    @classmethod
    def from_scheduler(cls, scheduler, **overrides) -> "GuidedDPMSolver":
        """From a Diffusers-style scheduler after ``set_timesteps``: reads ``alphas_cumprod``, ``timesteps``,
        ``final_alpha_cumprod`` (1.0 when the scheduler has none) and, where ``config`` has them, ``prediction_type``,
        ``solver_order``, ``algorithm_type``, ``lower_order_final`` and ``euler_at_final``."""
        config = getattr(scheduler, "config", None)
        kw = dict(final_alpha_cumprod=getattr(scheduler, "final_alpha_cumprod", 1.0))
        for name in ("prediction_type", "solver_order", "algorithm_type", "lower_order_final", "euler_at_final"):
            if getattr(config, name, None) is not None:
                kw[name] = getattr(config, name)
        kw.update(overrides)
        return cls(scheduler.alphas_cumprod, scheduler.timesteps, **kw)

    def weights(self, groups: int) -> list:
        """The weight of each of the ``groups`` groups of a call."""
        groups = int(groups)
        if self.group_weights is not None:
            if len(self.group_weights) != groups:
                raise RuntimeError(f"GuidedDPMSolver: {len(self.group_weights)} group_weights for a call of {groups} groups")
            return list(self.group_weights)
        if groups < 1:
            raise RuntimeError(f"GuidedDPMSolver: groups = {groups}")
        return [1.0] if groups == 1 else [0.0] * (groups - 2) + [1.0 - self.guidance_scale, self.guidance_scale]

    def order(self, i: int, have: Optional[int] = None) -> int:
        """The order step ``i`` is taken at (class docstring)."""
        n = len(self.timesteps)
        i = int(i)
        if not 0 <= i < n:
            raise IndexError(f"GuidedDPMSolver: step {i} outside [0, {n})")
        most = min(i, self.solver_order - 1)
        have = most if have is None else int(have)
        if not 0 <= have <= most:
            raise ValueError(f"GuidedDPMSolver: have = {have} outside [0, {most}] at step {i}")
        low = self.lower_order_final and n < 15
        if self.solver_order == 1 or have == 0 or (i == n - 1 and (self.euler_at_final or low or self.final_alpha == 1.0)):
            return 1
        if self.solver_order == 2 or have == 1 or (i == n - 2 and low):
            return 2
        return 3

    def _level(self, k: int):
        a = self.alphas[self.timesteps[k]] if k < len(self.timesteps) else self.final_alpha
        alpha, sigma = math.sqrt(a), math.sqrt(1.0 - a)
        return alpha, sigma, (math.log(alpha) - math.log(sigma) if sigma > 0.0 else math.inf)

    def coefficients(self, i: int, have: Optional[int] = None):
        """(sqrt_alpha, sqrt_beta, c_x, c_x0, c_h1, c_h2, c_noise) of step ``i`` in host float64: alpha and sigma of level i, and
        x' = c_x x + c_x0 m0 + c_h1 m1 + c_h2 m2 + c_noise noise, the class docstring's update with D1 / D2 multiplied out.
        ``have``: how many earlier predictions are valid, min(i, solver_order - 1) unless given smaller."""
        order = self.order(i, have)
        alpha, sigma, lam = self._level(i)
        alpha_n, sigma_n, lam_n = self._level(i + 1)
        if sigma_n == 0.0:                         # h = inf (order 1 by the rule above): the limits, exactly
            return alpha, sigma, 0.0, 1.0, 0.0, 0.0, 0.0
        h = lam_n - lam
        sde = self.algorithm_type == "sde-dpmsolver++"
        if sde:
            c_x = sigma_n / sigma * math.exp(-h)
            lead = -alpha_n * math.expm1(-2.0 * h)                 # alpha' (1 - e^-2h)
            c_noise = sigma_n * math.sqrt(-math.expm1(-2.0 * h))
        else:
            c_x, c_noise = sigma_n / sigma, 0.0
            lead = -alpha_n * math.expm1(-h)                       # -alpha' (e^-h - 1)
        if order == 1:
            return alpha, sigma, c_x, lead, 0.0, 0.0, c_noise
        r0 = (lam - self._level(i - 1)[2]) / h
        if order == 2:
            return alpha, sigma, c_x, lead + 0.5 * lead / r0, -0.5 * lead / r0, 0.0, c_noise
        r1 = (self._level(i - 1)[2] - self._level(i - 2)[2]) / h
        c_d1 = alpha_n * (math.expm1(-h) / h + 1.0)
        c_d2 = -alpha_n * ((math.expm1(-h) + h) / (h * h) - 0.5)
        # D1 = (1 + k) D1_0 - k D1_1 and D2 = (D1_0 - D1_1) / (r0 + r1), k = r0 / (r0 + r1)
        k = r0 / (r0 + r1)
        on_d10 = c_d1 * (1.0 + k) + c_d2 / (r0 + r1)
        on_d11 = -c_d1 * k - c_d2 / (r0 + r1)
        return alpha, sigma, c_x, lead + on_d10 / r0, on_d11 / r1 - on_d10 / r0, -on_d11 / r1, c_noise

    def prepare(self, x: torch.Tensor) -> None:
        """Allocate the solver_order - 1 history tensors for the video ``x`` on the current stream and forget the step."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("GuidedDPMSolver.prepare: x must live on the GPU (vidtome_amd has no CPU path)")
        self.history = [torch.empty(x.shape, dtype=torch.float32, device=x.device) for _ in range(self.solver_order - 1)]
        self._current = None

    def _in_sequence(self, i: int) -> None:
        if i != 0 and (self._current is None or i not in (self._current, self._current + 1)):
            raise RuntimeError(f"GuidedDPMSolver.step: step {i} out of sequence (the history is at step {self._current}; "
                               "step 0 restarts it)")

    def step(self, x: torch.Tensor, model_out: torch.Tensor, i: int, *, groups: int = 2, frame_ids=None,
             noise=None, generator: Optional[torch.Generator] = None,
             out: Optional[torch.Tensor] = None, want: Sequence[str] = ()):
        """Step ``i`` for one chunk, one vtm_solver_step launch on the current stream.  ``x``, ``model_out`` (groups * F, C, H,
        W, group-major), ``frame_ids``, ``out`` (it may be x; without it a NEW tensor when ``frame_ids`` is None, otherwise x
        itself IN PLACE), ``want`` and the result are ``GuidedDDIM.step``'s.  With "sde-dpmsolver++" and no ``noise`` (F, C, H,
        W), randn of the chunk's shape is drawn from ``generator``; ``noise=FrameNoise(seed)`` keys it per frame instead (one
        vtm_solver_step_keyed launch), as in ``GuidedDDIM.step``."""
        noise, keyed = _keyed("GuidedDPMSolver", noise, generator)
        want, (sqrt_alpha, sqrt_beta, c_x, c_x0, c_h1, c_h2, c_noise), F, groups, weights = _checked_step(
            "GuidedDPMSolver", x, model_out, noise, groups, frame_ids, want, lambda: self.coefficients(i), self.weights,
            lambda: self._in_sequence(int(i)))
        i = int(i)
        if len(self.history) != self.solver_order - 1 or any(h.shape != x.shape or h.device != x.device for h in self.history):
            if i != 0:
                raise RuntimeError(f"GuidedDPMSolver.step: the history of step {i} does not fit x {tuple(x.shape)} on {x.device}")
            self.prepare(x)
        self._current = i
        if c_noise != 0.0 and noise is None and keyed is None:
            noise = torch.randn((F,) + tuple(model_out.shape[1:]), dtype=x.dtype, device=x.device, generator=generator)
        ring = len(self.history)
        res = _lib.solver_step(x, model_out, weights, sqrt_alpha, sqrt_beta, c_x, c_x0, c_h1, c_h2, c_noise,
                               h1=self.history[(i - 1) % ring] if c_h1 != 0.0 else None,
                               h2=self.history[(i - 2) % ring] if c_h2 != 0.0 else None,
                               h_out=self.history[i % ring] if ring else None,
                               g_ref=groups - 1 if self.rescale_group is None else self.rescale_group, frame_ids=frame_ids,
                               pred_type=PREDICTION_TYPES[self.prediction_type],
                               rescale=self.guidance_rescale if groups >= 2 else 0.0, noise=noise, out=out,
                               want_eps="eps" in want, want_x0="x0" in want, key=keyed.key(i) if keyed else None)
        return _asked(res, want)
