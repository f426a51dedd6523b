"""Speed of the fp32 attention core (csrc/attention_f32.hip).

    timeout -k 10 600 python tools/fp32_attention.py [--reps 10]

For each full-size launch: ms per launch (median of --reps after a warm-up) and the executed TFLOP/s as a fraction of the
MI355X fp32 matrix peak (157.3 TFLOP/s); executed flops = 4 * B * Mq_live * Mk * C.  Then one cfg-2 pass of an fp32
SD-1.5 stand-in (top, mid and un-merged sites) with and without `fp32_attention`.  Prints one JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 157.3e12
SHAPES = [("cfg-2 top block", 2, 8, 40, 34816, 52224), ("cfg-2 mid block", 2, 8, 80, 8704, 13056),
          ("cfg-5 top block", 2, 5, 64, 64513, 90319), ("cfg-2 down2 (d = 160)", 32, 8, 160, 256, 256)]


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def kernels(reps):
    from vidtome_amd import _lib
    for name, B, h, d, Mq, Mk in SHAPES:
        C = h * d
        g = torch.Generator(device="cuda").manual_seed(1)
        q = torch.randn(B, (Mq + 7) // 8 * 8, C, device="cuda", generator=g)
        k = torch.randn(B, (Mk + 7) // 8 * 8, C, device="cuda", generator=g)
        vt = torch.randn(B, C, (Mk + 7) // 8 * 8, device="cuda", generator=g)
        for dt in (torch.float32, torch.float16):
            qq, kk, vv = q.to(dt), k.to(dt), vt.to(dt)
            t0 = time.time()
            med, lo, hi = _time(lambda: _lib.attention_kv(qq, kk, vv, h, Mq, Mk, d ** -0.5), reps)
            fl = 4.0 * B * Mq * Mk * C
            print(json.dumps({"shape": name, "dtype": str(dt).split(".")[-1], "ms": round(med, 3), "ms_min": round(lo, 3),
                              "ms_max": round(hi, 3), "tflops": round(fl / med / 1e9, 2),
                              "fraction_of_fp32_peak": round(fl / med / 1e-3 / PEAK, 3),
                              "wall_s": round(time.time() - t0, 2)}), flush=True)


def block_pass(reps):
    import vidtome_amd
    from vidtome_amd import sites as S
    B, F, latent = 2, 16, (64, 64)
    sl = [s for s in S.sd15_sites() if s.name in ("down0.0", "down1.0", "down2.0", "mid")]
    unet = S.SiteUNet(sl, seed=3).to(device="cuda", dtype=torch.float32)
    vidtome_amd.apply_patch(unet, local_merge_ratio=0.9, merge_global=True, global_merge_ratio=0.8, batch_size=B)
    unet.set_size(latent)
    hiddens = [S.synthetic_hidden(s, B, F, latent, torch.float32, "cuda", seed=40 + i) for i, s in enumerate(sl)]
    with torch.no_grad():
        for _ in range(2):                      # the global level reaches its steady state
            S.run_segment_pass(unet, hiddens)
        for flag in (False, True):
            vidtome_amd.update_patch(unet, fp32_attention=flag)
            med, lo, hi = _time(lambda: S.run_segment_pass(unet, hiddens), reps)
            print(json.dumps({"pass": "cfg-2 fp32 stand-in (4 sites)", "fp32_attention": flag, "ms": round(med, 2),
                              "ms_min": round(lo, 2), "ms_max": round(hi, 2)}), flush=True)
    vidtome_amd.remove_patch(unet)


def clocks():
    try:
        import subprocess
        out = subprocess.run(["rocm-smi", "--showclocks"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                             timeout=30).stdout
        return [l.strip() for l in out.splitlines() if "sclk" in l.lower()][:2]
    except Exception as e:     # (reporting only)
        return [repr(e)]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    kernels(args.reps)
    print(json.dumps({"sclk_after_kernels": clocks()}), flush=True)
    block_pass(max(3, args.reps // 2))
