"""Semantic guidance: the vtm_semantic_guidance launch against a torch restatement of the Diffusers chain, fp16: one JSON line.

    python tools/semantic_step.py [--reps 30] [--out profiles/semantic_step.json]

Event-timed in ONE process on the same inputs, the two forms interleaved repetition by repetition so they share the clock:
  kernel   _lib.semantic_guidance: one launch per chunk (classifier-free term, E concepts, momentum applied and updated)
  torch    what SemanticStableDiffusionPipeline strings together per concept, in the model's dtype: scale * (e - u), abs,
           flatten(2), float(), torch.quantile, where, the weighted sum, then the momentum update and the final sum
           ("sum": LEDITS++'s channel sum of |g| before the quantile)
Shapes: C = 4; F = 16 at 64 x 64 with E = 1 and E = 3 in "channel" and in "sum" mode; F = 16 at 96 x 96 and F = 4 at
128 x 128 with E = 3, "channel".  Reports median and min / max in microseconds, whether the two min-max ranges are disjoint
and whether the kernel's median is the slower one.  Nothing is asserted about the times; the two results are compared (a
few elements may differ by a whole term where torch.quantile's fp32 threshold falls on the other side of a value)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALES, QS, WEIGHTS = (5.0, -4.0, 3.0), (0.9, 0.95, 0.75), (1.0, 0.5, 1.5)
S_CFG, MOM_SCALE, MOM_BETA = 7.5, 0.1, 0.4


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


def sega_torch(mo, E, mode, momentum):
    """The Diffusers chain in mo's dtype (quantile in fp32); returns (combined output, new momentum)."""
    parts = mo.chunk(2 + E)
    u, c = parts[0], parts[1]
    edit = torch.zeros_like(u)
    for e in range(E):
        g = SCALES[e] * (parts[2 + e] - u)
        a = torch.abs(g)
        if mode == "sum":
            a = a.sum(dim=1, keepdim=True)
        thr = torch.quantile(a.flatten(start_dim=2).to(torch.float32), QS[e], dim=2, keepdim=False)
        g = torch.where(a >= thr.to(a.dtype)[:, :, None, None], g, torch.zeros_like(g))
        edit = edit + WEIGHTS[e] * g
    out = u + S_CFG * (c - u) + edit + MOM_SCALE * momentum
    return out, MOM_BETA * momentum + (1 - MOM_BETA) * edit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vidtome_amd import _lib
    dev, dt = "cuda", torch.float16
    result = {"tool": "semantic_step", "device": torch.cuda.get_device_name(0), "dtype": "fp16", "reps": args.reps, "unit": "us",
              "shapes": {}}
    cases = [(16, 64, 1, "channel"), (16, 64, 3, "channel"), (16, 64, 1, "sum"), (16, 64, 3, "sum"), (16, 96, 3, "channel"),
             (4, 128, 3, "channel")]
    for Fr, H, E, mode in cases:
        g = torch.Generator().manual_seed(H + E)
        mo = torch.randn((2 + E) * Fr, 4, H, H, generator=g).to(device=dev, dtype=dt)
        mom32 = (torch.randn(Fr, 4, H, H, generator=g) * 0.5).to(dev)
        mom16 = mom32.to(dt)
        out = torch.empty(Fr, 4, H, H, dtype=dt, device=dev)
        code = _lib.SEGA_SUM if mode == "sum" else _lib.SEGA_CHANNEL
        work = mom32.clone()

        def kernel():
            return _lib.semantic_guidance(mo, 2 + E, 0, 1, S_CFG, list(range(2, 2 + E)), SCALES[:E], QS[:E], WEIGHTS[:E],
                                          WEIGHTS[:E], [code] * E, momentum=work, mom_scale=MOM_SCALE, mom_beta=MOM_BETA,
                                          mom_apply=True, out=out)

        def composed():
            return sega_torch(mo, E, mode, mom16)

        with torch.no_grad():
            ours = kernel().float()
            theirs, their_mom = composed()
            diff = (ours - theirs.float()).abs()
            mom_diff = (work - their_mom.float()).abs()
            assert bool(torch.isfinite(ours).all()) and bool(torch.isfinite(theirs).all())
            key = f"{Fr}x4x{H}x{H} E={E} {mode}"
            r = _timed({"kernel": kernel, "torch": composed}, args.warmup, args.reps)
        k, t = r["kernel"], r["torch"]
        r["ranges_disjoint"] = bool(k["max"] < t["min"] or t["max"] < k["min"])
        r["kernel_slower"] = bool(k["median"] > t["median"])
        r["max_abs_difference_to_torch"] = float(f"{float(diff.max()):.3e}")
        r["elements_off_by_more_than_0.05"] = int((diff > 0.05).sum())
        r["momentum_elements_off_by_more_than_0.05"] = int((mom_diff > 0.05).sum())
        r["elements"] = diff.numel()
        result["shapes"][key] = r
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
