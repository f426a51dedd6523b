#!/usr/bin/env python3
"""What DoRA adapters cost: one JSON line.

    python tools/dora_block.py [--reps 10] [--warmup 3]

* fold: the device time of folding all 160 block projections of SD-1.5 (16 transformer blocks x 10 projections) with a
  rank-64 DoRA adapter, vtm_dora_norms + vtm_dora_fold per projection (one-off per adapter state), next to vtm_lora_fold
  on the same operands; and the host wall time of the first `lora.linear_params` call on every DoRA-wrapped projection
  (operand concatenation, the two launches, the bias), synchronised at the end.
* cfg2_top_segment: the cfg-2 top-block segment (up3.0, batch 2, 16 frames at 512 x 512, local merge 0.5 + global merge
  0.5, steady-state passes of sites.ClipStream) with a rank-64 DoRA adapter on its four attn1 projections, timed as in
  tools/lora_block.py: unadapted, dora_fused (folded weights on the HIP path) and dora_module (the recogniser forced to
  refuse the DoRA layers: what a DoRA user got before DoRA folded -- attention over the materialised merged tokens on
  torch SDPA, the stand-in's DoRA forward per projection).
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lora_block as lb  # noqa: E402  (puts the repository and tests/ on sys.path)
import torch  # noqa: E402

import vidtome_amd  # noqa: E402
from vidtome_amd import _lib, lora, sites  # noqa: E402
from dora_standin import wrap_dora  # noqa: E402


def _event_ms(fn, reps):
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return {"ms": round(statistics.median(times), 3), "spread_ms": [round(min(times), 3), round(max(times), 3)]}


def fold_times(sl, r=64, reps=5):
    unet = lb.build(sl, True)
    projs = [m for m in unet.modules() if type(m) is torch.nn.Linear and m.weight.dim() == 2]
    g = torch.Generator().manual_seed(0)
    ops = []
    for m in projs:
        co, ci = m.weight.shape
        w = m.weight.detach()
        ops.append((w, (torch.randn(co, r, generator=g) * 0.01).to(lb.DEV), (torch.randn(r, ci, generator=g) * ci ** -0.5).to(lb.DEV),
                    w.float().norm(dim=1)))
    dora = lambda: [_lib.dora_fold(w, up, down, mag, r) for w, up, down, mag in ops]
    plain = lambda: [_lib.lora_fold(w, up, down) for w, up, down, _ in ops]
    dora(), plain()                                   # warm-up
    out = {"projections": len(ops), "rank": r, "dora_device": _event_ms(dora, reps), "lora_device": _event_ms(plain, reps)}
    wrapped = wrap_dora(unet, rank=r, seed=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for m in wrapped:
        lora.linear_params(m)
    torch.cuda.synchronize()
    out["dora_linear_params_first_call_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
    out["wrapped"] = len(wrapped)
    return out


def segment(sl, B, F, latent, reps, warmup):
    base = lb.patch(lb.build(sl, False), B, latent, False)
    do = lb.build(sl, False)
    wrap_dora(do, rank=64, seed=1)
    do_mod = copy.deepcopy(do)
    lb.patch(do, B, latent, False)
    lb.patch(do_mod, B, latent, False)
    variants = {}
    for name, unet, on in (("unadapted", base, False), ("dora_fused", do, False), ("dora_module", do_mod, True)):
        st = lb.stream_for(unet, sl, B, F, latent, False)
        with lb.module_path(on):
            st.populate()
        variants[name] = (st, on)
    res = lb.time_variants(variants, reps, warmup)
    for u in (base, do, do_mod):
        vidtome_amd.remove_patch(u)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/dora_block.py needs a GPU"
    sl = sites.sd15_sites()
    res = {"fold": fold_times(sl)}
    top = [s for s in sl if s.name == "up3.0"]
    res["cfg2_top_segment"] = segment(top, 2, 16, (64, 64), a.reps, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
