"""Frame-keyed noise: ``FrameNoise``, the stochastic operand of a step addressed per frame like every other.

    noise = FrameNoise(seed=1234)                                # one per sampling run; the same on every rank
    x = FrameNoise(seed=1234, tag=INIT).normal((4, 64, 64), step=0, n_frames=n, dtype=torch.float16)[0]
    for i, t in enumerate(timesteps):
        def process_chunk(chunk):
            sampler.step(x, unet_out, i, groups=groups, frame_ids=chunk, noise=noise, out=x_next)

A ``torch.Generator`` is a stream: the noise a frame gets depends on where the frame sits in the step's chunk draw, and
``ChunkScheduler`` draws a new cut every step; under ``chunk_parallel`` every rank has a generator of its own.  Here the noise
of element e of frame f at step i is a pure function of (seed, tag, i, f, e) -- Philox4x32-10 keyed by the seed, counted by
(e >> 2, f, i, tag), Box-Muller on its output (include/vidtome_hip.h, "Frame-keyed noise"; csrc/philox.h).  So a stochastic
step's bits depend neither on the chunking, nor on the chunks' order, nor on the rank or stream that runs a chunk, and a step
that is handed a ``FrameNoise`` draws its noise inside its own launch (vtm_guided_step_keyed / vtm_solver_step_keyed): no randn
launch, no noise tensor.  It reproduces no other library's stream.
"""
from __future__ import annotations

import operator
from typing import Optional, Sequence

import torch

from . import _lib

INIT, STEP, LEVELS = _lib.NOISE_INIT, _lib.NOISE_STEP, _lib.NOISE_LEVELS      # the named tags
USER_TAG = _lib.NOISE_USER                                                    # a caller's own tags start here
MAX_ABS = 5.7683             # |z| <= sqrt(48 ln 2) = 5.76823 by construction (u1 >= 2^-24)


class FrameNoise:
    """N(0, 1) noise as a pure function of (``seed``, ``tag``, step, frame, element).  ``seed``: an int in [0, 2^64);
    ``tag``: what the noise is for -- ``STEP`` (a sampler's stochastic term, the default), ``INIT`` (the initial latents),
    ``LEVELS`` (edit-friendly inversion's levels; ``noise_levels`` sets it itself), or a caller's own from ``USER_TAG`` up.
    Two uses that share seed, tag, step and frame share their noise: that is the point, and the reason for the tags."""

    def __init__(self, seed: int, tag: int = STEP):
        try:
            self.seed, self.tag = operator.index(seed), operator.index(tag)
        except TypeError:
            raise TypeError("FrameNoise: seed and tag must be integers") from None
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError(f"FrameNoise: seed {self.seed} outside [0, 2^64)")
        if not (self.tag in (INIT, STEP, LEVELS) or USER_TAG <= self.tag < 2 ** 32):
            raise ValueError(f"FrameNoise: tag {self.tag} is neither INIT, STEP, LEVELS nor a user tag in [{USER_TAG}, 2^32)")

    def with_tag(self, tag: int) -> "FrameNoise":
        """The same seed under another tag."""
        return FrameNoise(self.seed, tag)

    def key(self, step: int):
        """(seed, step, tag) as the keyed launches take it."""
        try:
            step = operator.index(step)
        except TypeError:
            raise TypeError("FrameNoise: step must be an integer") from None
        if not 0 <= step < 2 ** 32:
            raise ValueError(f"FrameNoise: step {step} outside [0, 2^32)")
        return self.seed, step, self.tag

    def normal(self, shape: Sequence[int], step: int, frame_ids=None, n_frames: Optional[int] = None, steps: int = 1,
               dtype: torch.dtype = torch.float32, device=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The noise of frames ``frame_ids`` at steps ``step .. step + steps - 1`` as a (steps, F, *shape) tensor, one
        vtm_frame_noise launch on the current stream.  ``shape``: a frame's (C, H, W).  ``frame_ids``: a host sequence of
        whole-video frame indices (checked against ``n_frames`` when given) or a device int32 tensor (taken as it is); None:
        frames 0 .. ``n_frames`` - 1.  ``out``: a contiguous tensor of that shape to fill (it fixes dtype and device);
        otherwise a new one of ``dtype`` on ``device`` (default: the current GPU).  The fp32 normal is rounded once to a 16-bit
        dtype, so ``normal(dtype=fp16)`` is ``normal(dtype=fp32).half()`` bit for bit."""
        who = "FrameNoise.normal"
        try:
            shape = tuple(operator.index(v) for v in shape)
            steps = operator.index(steps)
        except TypeError:
            raise TypeError(f"{who}: shape must be a sequence of integers and steps an integer") from None
        if not shape or any(v < 1 for v in shape) or steps < 0:
            raise ValueError(f"{who}: shape {shape} must be a frame's non-empty (C, H, W) and steps >= 0")
        seed, step, tag = self.key(step)
        if steps and step + steps - 1 >= 2 ** 32:
            raise ValueError(f"{who}: steps {step} .. {step + steps - 1} leave [0, 2^32)")
        if frame_ids is None:
            if n_frames is None:
                raise ValueError(f"{who}: without frame_ids, n_frames says how many frames")
            F = operator.index(n_frames)
            if F < 0:
                raise ValueError(f"{who}: n_frames = {F}")
        else:
            F = frame_ids.numel() if isinstance(frame_ids, torch.Tensor) else len(frame_ids)
        full = (steps, F) + shape
        if out is None:
            if dtype not in _lib._DT:
                raise RuntimeError(f"{who}: dtype {dtype} is not fp16 / bf16 / fp32")
            device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            if device.type != "cuda":
                raise RuntimeError(f"{who}: device {device}: vidtome_amd has no CPU path")
            out = torch.empty(full, dtype=dtype, device=device)
        elif not isinstance(out, torch.Tensor) or tuple(out.shape) != full:
            raise RuntimeError(f"{who}: out must be a {full} tensor")
        return _lib.frame_noise(out, seed, step, tag, frame_ids=frame_ids, n_frames=n_frames)
