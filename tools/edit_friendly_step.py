"""Edit-friendly inversion: the vtm_invert_step launch against a torch restatement of the same chain, fp16: one JSON line.

    python tools/edit_friendly_step.py [--reps 30] [--out profiles/edit_friendly_step.json]

Event-timed in ONE process on the same inputs, the two forms interleaved repetition by repetition so they share the clock:
  kernel   _lib.invert_step: one launch per chunk (combine, rescale, prediction, mu, the noise map, the corrected level, the
           fp32 history)
  torch    what Diffusers' LEditsPPPipelineStableDiffusion.invert strings together per chunk (compute_noise_sde_dpm_pp_2nd and
           the guidance in front of it), in the model's dtype: the classifier-free combine, rescale_noise_cfg, the clean-sample
           prediction, mu, z = (target - mu) / c_noise, target = mu + c_noise z, the history in fp32 -- every intermediate
           rounded to fp16
Shapes: the cfg-2 chunk, F = 16 frames of 4 x 64 x 64 (rows 8 .. 23 of a 32-frame video: slices, so torch gathers nothing),
groups 1 and 2, orders 1 and 2, with and without guidance rescale (which needs two groups).  Coefficients: step 7 of 20 of
Stable Diffusion's schedule.  Reports median and min / max in microseconds, whether the two min-max ranges are disjoint and
whether the kernel's median is the slower one.  Nothing is asserted about the times; the two noise maps are compared (fp16
intermediates cost the torch form a few ulps)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S_CFG, PHI = 3.5, 0.7


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


def invert_torch(x, mo, groups, rescale, coef, target, z_out, h1, h_out):
    """The chain on the chunk's slices, in their dtype (epsilon prediction); writes z_out, target and h_out in place."""
    sa, sb, c_x, c_x0, c_h1, _, c_noise = coef
    if groups == 1:
        m = mo
    else:
        u, c = mo.chunk(2)
        m = u + S_CFG * (c - u)
        if rescale > 0.0:
            std_c = c.std(dim=list(range(1, c.ndim)), keepdim=True)
            std_m = m.std(dim=list(range(1, m.ndim)), keepdim=True)
            m = rescale * (m * (std_c / std_m)) + (1.0 - rescale) * m
    x0 = (x - sb * m) / sa
    mu = c_x * x + c_x0 * x0
    if c_h1 != 0.0:
        mu = mu + (c_h1 * h1).to(x.dtype)
    z = (target - mu) / c_noise
    z_out.copy_(z)
    target.copy_(mu + c_noise * z)
    h_out.copy_(x0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vidtome_amd import GuidedDPMSolver, _lib
    dev, dt = "cuda", torch.float16
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    alphas = torch.cumprod(1.0 - betas, dim=0)
    timesteps = ((np.arange(20) * 50)[::-1] + 1).tolist()
    n_frames, lo, Fr, shape = 32, 8, 16, (4, 64, 64)
    rows = list(range(lo, lo + Fr))
    result = {"tool": "edit_friendly_step", "device": torch.cuda.get_device_name(0), "dtype": "fp16", "reps": args.reps,
              "unit": "us", "chunk": f"{Fr}x4x64x64", "shapes": {}}
    for groups in (1, 2):
        for order in (1, 2):
            for rescale in (0.0, PHI) if groups == 2 else (0.0,):
                coef = GuidedDPMSolver(alphas, timesteps, algorithm_type="sde-dpmsolver++", solver_order=order).coefficients(7)
                g = torch.Generator().manual_seed(10 * groups + order)
                x = torch.randn((n_frames,) + shape, generator=g).to(device=dev, dtype=dt)
                mo = torch.randn((groups * Fr,) + shape, generator=g).to(device=dev, dtype=dt)
                start = torch.randn((n_frames,) + shape, generator=g).to(device=dev, dtype=dt)
                h1 = torch.randn((n_frames,) + shape, generator=g).to(dev)
                weights = (1.0,) if groups == 1 else (1.0 - S_CFG, S_CFG)
                ours = {"target": start.clone(), "z": torch.zeros_like(x), "h": torch.zeros_like(h1)}
                theirs = {"target": start.clone(), "z": torch.zeros_like(x), "h": torch.zeros_like(h1)}

                def kernel():
                    _lib.invert_step(x, mo, weights, *coef, target=ours["target"], z_out=ours["z"],
                                     h1=h1 if coef[4] != 0.0 else None, h_out=ours["h"], frame_ids=rows, rescale=rescale)

                def composed():
                    invert_torch(x[lo:lo + Fr], mo, groups, rescale, coef, theirs["target"][lo:lo + Fr], theirs["z"][lo:lo + Fr],
                                 h1[lo:lo + Fr], theirs["h"][lo:lo + Fr])

                with torch.no_grad():
                    kernel(), composed()
                    diff = (ours["z"].float() - theirs["z"].float()).abs()
                    assert bool(torch.isfinite(ours["z"]).all()) and bool(torch.isfinite(theirs["z"]).all())
                    # the timed repetitions re-correct an already corrected level: the same work on other values
                    r = _timed({"kernel": kernel, "torch": composed}, args.warmup, args.reps)
                k, t = r["kernel"], r["torch"]
                r["ranges_disjoint"] = bool(k["max"] < t["min"] or t["max"] < k["min"])
                r["kernel_slower"] = bool(k["median"] > t["median"])
                r["max_abs_noise_difference_to_torch"] = float(f"{float(diff.max()):.3e}")
                r["max_abs_noise"] = float(f"{float(ours['z'].float().abs().max()):.3e}")
                result["shapes"][f"groups={groups} order={order} rescale={rescale}"] = r
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
