"""Frame-keyed noise: the keyed step launch against torch.randn + the tensor-noise launch, fp16: one JSON line.

    python tools/frame_noise_step.py [--reps 30] [--out profiles/frame_noise_step.json]

Event-timed in ONE process on the same inputs, the two forms interleaved repetition by repetition so they share the clock:
  keyed    sampler.step(..., noise=FrameNoise(seed)): one launch (vtm_guided_step_keyed / vtm_solver_step_keyed) that draws
           the chunk's noise where it is used -- 10 Philox rounds and one logf / sqrtf / sinpif / cospif per two elements
  randn    sampler.step(..., generator=g): torch.randn of the chunk's shape, then the tensor-noise launch that reads it
           (vtm_guided_step / vtm_solver_step) -- one launch and one F * E read more
  stored   sampler.step(..., noise=z) on noise drawn beforehand: the tensor-noise launch alone, for the split of `randn`
Shape: the cfg-2 chunk, F = 16 frames of 4 x 64 x 64 (rows 8 .. 23 of a 32-frame video), two groups.  Samplers: DDIM with
eta = 1, and "sde-dpmsolver++" at orders 1 and 2 (step 7 of 20 of Stable Diffusion's schedule; the solver's history is set
up by the steps before it, untimed).  Reports median and min / max in microseconds, whether the keyed and the randn min-max
ranges are disjoint and whether the keyed median is the slower one.  Nothing is asserted about the times; the keyed step is
checked against the tensor-noise step on vtm_frame_noise's output, bit for bit."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP = 7


def _timed(variants, warmup, reps):
    """Event times in us of every variant, interleaved repetition by repetition -> {name: {median, min, max}}."""
    times = {k: [] for k in variants}
    for rep in range(warmup + reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    return {k: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
            for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vidtome_amd import FrameNoise, GuidedDDIM, GuidedDPMSolver
    dev, dt = "cuda", torch.float16
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    alphas = torch.cumprod(1.0 - betas, dim=0)
    timesteps = ((np.arange(20) * 50)[::-1] + 1).tolist()
    n_frames, lo, Fr, shape = 32, 8, 16, (4, 64, 64)
    rows = list(range(lo, lo + Fr))
    samplers = {"ddim eta=1": lambda: GuidedDDIM(alphas, timesteps, eta=1.0),
                "sde-dpmsolver++ order=1": lambda: GuidedDPMSolver(alphas, timesteps, algorithm_type="sde-dpmsolver++", solver_order=1),
                "sde-dpmsolver++ order=2": lambda: GuidedDPMSolver(alphas, timesteps, algorithm_type="sde-dpmsolver++", solver_order=2)}
    result = {"tool": "frame_noise_step", "device": torch.cuda.get_device_name(0), "dtype": "fp16", "reps": args.reps,
              "unit": "us", "chunk": f"{Fr}x4x64x64 of {n_frames}", "groups": 2, "shapes": {}}
    noise = FrameNoise(20240607)
    for name, make in samplers.items():
        g = torch.Generator().manual_seed(len(name))
        x = torch.randn((n_frames,) + shape, generator=g).to(device=dev, dtype=dt)
        mo = torch.randn((2 * Fr,) + shape, generator=g).to(device=dev, dtype=dt)
        gen = torch.Generator(device=dev).manual_seed(1)
        z = noise.normal(shape, STEP, frame_ids=rows, dtype=dt)[0]
        outs = {k: torch.zeros_like(x) for k in ("keyed", "randn", "stored")}
        steppers = {k: make() for k in outs}
        with torch.no_grad():
            for s in steppers.values():                   # the history of a multistep solver: the steps before STEP, on the chunk
                if hasattr(s, "prepare"):
                    s.prepare(x)
                    for i in range(STEP):
                        s.step(x, mo, i, frame_ids=rows, noise=noise, out=torch.empty_like(x))
            variants = {"keyed": lambda: steppers["keyed"].step(x, mo, STEP, frame_ids=rows, noise=noise, out=outs["keyed"]),
                        "randn": lambda: steppers["randn"].step(x, mo, STEP, frame_ids=rows, generator=gen, out=outs["randn"]),
                        "stored": lambda: steppers["stored"].step(x, mo, STEP, frame_ids=rows, noise=z, out=outs["stored"])}
            for fn in variants.values():
                fn()
            torch.cuda.synchronize()
            same = torch.equal(outs["keyed"][lo:lo + Fr].view(torch.int16), outs["stored"][lo:lo + Fr].view(torch.int16))
            assert same and bool(torch.isfinite(outs["keyed"][lo:lo + Fr]).all()), name
            # the timed repetitions re-step a history that step STEP has already overwritten: the same work on other values
            r = _timed(variants, args.warmup, args.reps)
        k, t = r["keyed"], r["randn"]
        r["ranges_disjoint"] = bool(k["max"] < t["min"] or t["max"] < k["min"])
        r["keyed_slower"] = bool(k["median"] > t["median"])
        r["keyed_equals_stored_bitwise"] = same
        result["shapes"][name] = r
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
