#!/usr/bin/env python3
"""What FreeU costs in front of the up-block resnets: one JSON line, also written to profiles/freeu_block.json.

    python tools/freeu_block.py [--reps 20] [--warmup 5] [--out profiles/freeu_block.json]

Per workload, the FreeU calls of one UNet forward (all fp16), timed three ways on the same tensors:
* "hip":            _lib.freeu (vtm_freeu, version 1) in place on each concatenation;
* "torch_diffusers": a torch restatement of Diffusers' op chain on the two halves -- the slice multiply, the upcast rule
                     (fp32 unless H and W are powers of two; if this build's FFT refuses fp16 the chain is run in fp32 and
                     "fft_dtype" says so), fftn, fftshift, the mask, ifftshift, ifftn, .real, the cast back;
* "hip_v2" / "torch_original": version 2 against the original repository's chain (the same filter; the backbone scaled by
                     1 + (b - 1) * the min-max-normalised channel mean).
Workloads (B, plane sides, backbone | skip channels per call):
    cfg-2      32   8, 16    1280|1280 1280|1280 1280|640 at the first side, 1280|640 640|640 640|320 at the second
    cfg-5      32   12, 24   the same
    sdxl-32     4   32       1280|1280 1280|1280 1280|640
    sdxl-64     4   64       640|640 640|640 640|320
Device events around the calls of a workload, median and [min, max] of --reps after --warmup, the variants alternating
inside every repetition; the tensors are restored from a pristine copy outside the timed region (the calls are in place).
"gbps" is one read plus one write of the TOUCHED planes (B * (C_h // 2 + C_s) * P * 2 bytes, twice) over the median.
"max_abs_diff" compares hip and torch results at the timed size.  One process; run it under a time limit."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from vidtome_amd import _lib  # noqa: E402

DEV = "cuda"
B1, S1, B2, S2 = 1.5, 0.9, 1.6, 0.2
SD = ((1280, 1280), (1280, 1280), (1280, 640)), ((1280, 640), (640, 640), (640, 320))
WORKLOADS = {
    "cfg-2": (32, [(c, 8, B1, S1) for c in SD[0]] + [(c, 16, B2, S2) for c in SD[1]]),
    "cfg-5": (32, [(c, 12, B1, S1) for c in SD[0]] + [(c, 24, B2, S2) for c in SD[1]]),
    "sdxl-32": (4, [(c, 32, B1, S1) for c in SD[0]]),
    "sdxl-64": (4, [(c, 64, B2, S2) for c in (SD[1][1], SD[1][1], SD[1][2])]),
}


def event_ms(fns, reps, warmup):
    """Median and [min, max] ms per variant, the variants alternating inside every repetition; fns: {name: (prepare, run)},
    prepare runs outside the timed region."""
    for _ in range(warmup):
        for prepare, run in fns.values():
            prepare()
            run()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, (prepare, run) in fns.items():
            prepare()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            run()
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e))
    return {k: {"ms": round(statistics.median(v), 4), "spread_ms": [round(min(v), 4), round(max(v), 4)], "reps": reps}
            for k, v in times.items()}


def _pow2(n):
    return n & (n - 1) == 0


def fourier_filter(x_in, scale, fft_dtype):
    x = x_in.to(fft_dtype)
    H, W = x.shape[-2:]
    f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(x.shape, device=x.device)
    mask[..., H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = scale
    f = torch.fft.ifftshift(f * mask, dim=(-2, -1))
    return torch.fft.ifftn(f, dim=(-2, -1)).real.to(x_in.dtype)


def diffusers_chain(hidden, res, b, s, fft_dtype):
    half = hidden.shape[1] // 2
    hidden[:, :half] = hidden[:, :half] * b
    return hidden, fourier_filter(res, s, fft_dtype)


def original_chain(hidden, res, b, s, fft_dtype):
    half = hidden.shape[1] // 2
    n = hidden.shape[0]
    mean = hidden.mean(1).unsqueeze(1)
    hi = mean.view(n, -1).max(-1)[0][:, None, None, None]
    lo = mean.view(n, -1).min(-1)[0][:, None, None, None]
    mean = (mean - lo) / (hi - lo)
    hidden[:, :half] = hidden[:, :half] * ((b - 1) * mean + 1)
    return hidden, fourier_filter(res, s, fft_dtype)


def fft_dtype_for(side):
    """Diffusers' rule: fp16 stays fp16 at power-of-two sizes, everything else goes to fp32 -- unless this FFT refuses fp16."""
    if not _pow2(side):
        return torch.float32, "fp32 (not a power of two)"
    try:
        torch.fft.fftn(torch.zeros(1, 1, side, side, dtype=torch.float16, device=DEV), dim=(-2, -1))
        torch.cuda.synchronize()
        return torch.float16, "fp16"
    except RuntimeError as exc:
        return torch.float32, "fp32 (this FFT refuses fp16: %s)" % str(exc).splitlines()[0][:80]


def workload(name, reps, warmup):
    B, calls = WORKLOADS[name]
    g = torch.Generator().manual_seed(0)
    pristine, cat, hidden, res, fft = [], [], [], [], []
    ramp = lambda side: torch.linspace(-1, 1, side * side).reshape(1, 1, side, side)
    for (C_h, C_s), side, b, s in calls:
        x = torch.randn(B, C_h + C_s, side, side, generator=g)
        x[:, :C_h] += ramp(side)                                   # version 2 divides by the spread of the mean map
        x = x.to(torch.float16).to(DEV)
        pristine.append(x)
        cat.append(torch.empty_like(x))
        hidden.append(torch.empty_like(x[:, :C_h]))
        res.append(torch.empty_like(x[:, C_h:]))
        fft.append(fft_dtype_for(side))

    def restore_cat():
        for c, p in zip(cat, pristine):
            c.copy_(p)

    def restore_halves():
        for h, r, p, (chan, _, _, _) in zip(hidden, res, pristine, calls):
            h.copy_(p[:, :chan[0]])
            r.copy_(p[:, chan[0]:])

    def hip(version):
        def run():
            for c, (chan, _, b, s) in zip(cat, calls):
                _lib.freeu(c, chan[0], b, s, version)
        return run

    outs = {}

    def torch_chain(chain, key):
        def run():
            outs[key] = [chain(h, r, b, s, f[0]) for h, r, (_, _, b, s), f in zip(hidden, res, calls, fft)]
        return run

    fns = {"hip": (restore_cat, hip(1)), "torch_diffusers": (restore_halves, torch_chain(diffusers_chain, "d")),
           "hip_v2": (restore_cat, hip(2)), "torch_original": (restore_halves, torch_chain(original_chain, "o"))}
    out = event_ms(fns, reps, warmup)
    touched = sum(B * (chan[0] // 2 + chan[1]) * side * side * 2 * 2 for chan, side, _, _ in calls)
    for k in out:
        out[k]["gbps"] = round(touched / out[k]["ms"] / 1e6, 1)
    # agreement at the timed size
    for version, key, chain in ((1, "d", diffusers_chain), (2, "o", original_chain)):
        restore_cat(), restore_halves()
        hip(version)()
        torch_chain(chain, key)()
        diff = 0.0
        for c, (h, r) in zip(cat, outs[key]):
            diff = max(diff, float((c.float() - torch.cat([h, r], 1).float()).abs().max()))
        out["hip" if version == 1 else "hip_v2"]["max_abs_diff_to_torch"] = round(diff, 5)
    out["touched_bytes"] = touched
    out["B"] = B
    out["calls"] = ["%d|%d @ %dx%d" % (chan[0], chan[1], side, side) for chan, side, _, _ in calls]
    out["fft_dtype"] = sorted({f[1] for f in fft})
    out["hip_faster_than_torch"] = {"version_1": out["hip"]["ms"] < out["torch_diffusers"]["ms"],
                                    "version_2": out["hip_v2"]["ms"] < out["torch_original"]["ms"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freeu_block.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("freeu_block: no GPU: nothing is measured on a CPU")
    result = {"device": torch.cuda.get_device_name(0), "dtype": "fp16", "factors": dict(b1=B1, s1=S1, b2=B2, s2=S2)}
    for name in WORKLOADS:
        result[name] = workload(name, args.reps, args.warmup)
        print("%s: done" % name, file=sys.stderr, flush=True)     # (a sign of life per workload for whoever set the time limit)
        torch.cuda.empty_cache()
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
