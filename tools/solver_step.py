"""The guided DPM-Solver++ step of one chunk, fused (GuidedDPMSolver.step: one vtm_solver_step launch) against the torch
composition a caller writes without it, fp16: one JSON line.

    python tools/solver_step.py [--reps 50] [--out profiles/solver_step.json]

Per case, event-timed in ONE process on the same inputs, the variants interleaved repetition by repetition so they share the
clock (tools/guided_step.py's measurement).  The torch composition is the weighted sum over ``model_out.chunk(groups)``, the
guidance rescale (per-frame ``std``), the prediction type, the second-order multistep update from an fp32 history tensor, and
the two indexed stores ``x_next[chunk] = ...`` / ``history[chunk] = x0``.  Two settings: ``epsilon`` (epsilon prediction, no
rescale) and ``v_rescale`` (v-prediction, guidance_rescale 0.7).  Cases: 16 frames of 4 x 64 x 64 with 2 groups (CFG) and
with 3 (perturbed-attention weights), 16 frames of 4 x 96 x 96 with 2.  Reports median and min / max in microseconds; a
difference is real only when the min-max ranges do not overlap.  Both are launch-bound: nothing is asserted about the times;
the two results are compared."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from attention_maps_block import _timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vidtome_amd import GuidedDPMSolver
    dev, dt, step = "cuda", torch.float16, 7
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    alphas, timesteps = torch.cumprod(1.0 - betas, dim=0), torch.arange(951, -1, -50)
    result = {"tool": "solver_step", "device": torch.cuda.get_device_name(0), "dtype": "fp16", "reps": args.reps, "unit": "us",
              "cases": {}}
    for frames, side, groups in ((16, 64, 2), (16, 64, 3), (16, 96, 2)):
        g = torch.Generator().manual_seed(side + groups)
        x = torch.randn(frames, 4, side, side, generator=g).to(device=dev, dtype=dt)
        mo = torch.randn(groups * frames, 4, side, side, generator=g).to(device=dev, dtype=dt)
        ids = torch.arange(frames, device=dev)
        ids32 = ids.to(torch.int32)
        weights = (1.0 - 7.5, 7.5) if groups == 2 else (1.0 - 7.5, 7.5 + 3.0, -3.0)
        case = {}
        for name, pred, rescale in (("epsilon", "epsilon", 0.0), ("v_rescale", "v_prediction", 0.7)):
            s = GuidedDPMSolver(alphas, timesteps, prediction_type=pred, solver_order=2, group_weights=weights,
                                guidance_rescale=rescale)
            sa, sb, cx, c0, c1 = s.coefficients(step)[:5]
            fused_out, torch_out = torch.empty_like(x), torch.empty_like(x)
            for i in range(step):                                        # the history of the steps before
                s.step(x, mo, i, groups=groups, frame_ids=ids32, out=fused_out)
            hist = s.history[0].clone()

            def fused():
                s.step(x, mo, step, groups=groups, frame_ids=ids32, out=fused_out)

            def composed():
                m = sum(w * t for w, t in zip(weights, mo.chunk(groups)))
                if rescale:
                    ratio = mo.chunk(groups)[-1].std(dim=(1, 2, 3), keepdim=True) / m.std(dim=(1, 2, 3), keepdim=True)
                    m = rescale * (m * ratio) + (1 - rescale) * m
                xc = x[ids]
                x0 = (xc - sb * m) / sa if pred == "epsilon" else sa * xc - sb * m
                torch_out[ids] = (cx * xc + c0 * x0 + c1 * hist[ids]).to(dt)
                hist[ids] = x0.float()

            fused()
            composed()
            d = float((fused_out.float() - torch_out.float()).abs().max())
            # the composition rounds to fp16 after every operation: a few fp16 steps of the largest value
            assert d < 0.02 * float(torch_out.float().abs().max()), d
            case[name] = _timed({"fused": fused, "torch": composed}, args.warmup, args.reps)
            case[name]["max_abs_difference"] = float(f"{d:.3e}")
        result["cases"][f"{frames} x 4 x {side} x {side}, {groups} groups"] = case
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
