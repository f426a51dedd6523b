#!/usr/bin/env python3
"""What LoHa / LoKr (LyCORIS) adapters cost: one JSON line, also written to profiles/lycoris_block.json.

    python tools/lycoris_block.py [--reps 10] [--warmup 3] [--out profiles/lycoris_block.json]

* fold: the device time of folding all 160 block projections of SD-1.5 (16 transformer blocks x 10 projections) with one
  LoHa adapter of rank 64 (vtm_loha_delta + vtm_delta_fold per projection) and one LoKr adapter (w1 full, w2 of rank 8
  multiplied out by vtm_lora_fold, vtm_lokr_delta + vtm_delta_fold), one-off per adapter state, next to vtm_lora_fold at
  rank 64 on the same weights; and the host wall time of the first `lora.linear_params` call on every wrapped projection
  (operand conversion and the launches), synchronised at the end.
* cfg2_top_segment: the cfg-2 top-block segment (up3.0, batch 2, 16 frames at 512 x 512, local merge 0.5 + global merge
  0.5, steady-state passes of sites.ClipStream) with the adapter on its four attn1 projections, timed as in
  tools/lora_block.py: unadapted, fused (folded weights on the HIP path) and module (the recogniser forced to refuse the
  layers: what a LyCORIS user got before these folded -- attention over the materialised merged tokens on torch SDPA,
  the stand-in's forward per projection).
One process; run it under a time limit.
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
from lycoris_standin import kron_split, wrap_lycoris  # noqa: E402

KINDS = {"loha": dict(kind="loha", rank=64), "lokr": dict(kind="lokr", rank=8, forms=("full", "lowrank"))}


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


def fold_times(sl, r=64, r_kr=8, reps=5):
    unet = lb.build(sl, True)
    projs = [m for m in unet.modules() if type(m) is torch.nn.Linear and m.weight.dim() == 2]
    g = torch.Generator().manual_seed(0)
    rn = lambda rows, cols, std: (torch.randn(rows, cols, generator=g) * std).to(lb.DEV)
    ops = []
    for m in projs:
        co, ci = m.weight.shape
        (a1, a2), (b1, b2) = kron_split(co), kron_split(ci)
        ops.append(dict(w=m.weight.detach(), up=rn(co, r, 0.01), down=rn(r, ci, ci ** -0.5),
                        loha=(rn(co, r, 0.01), rn(r, ci, 1.0), rn(co, r, 0.01), rn(r, ci, 1.0)),
                        lokr=(rn(a1, b1, 0.1), rn(a2, r_kr, 0.1), rn(r_kr, b2, 1.0))))

    def lokr_one(o):
        w1, w2a, w2b = o["lokr"]
        w2 = _lib.lora_fold(torch.zeros(w2a.shape[0], w2b.shape[1], device=lb.DEV), w2a, w2b)
        return _lib.delta_fold(o["w"], _lib.lokr_delta(w1, w2))

    loha = lambda: [_lib.delta_fold(o["w"], _lib.loha_delta(*o["loha"])) for o in ops]
    lokr = lambda: [lokr_one(o) for o in ops]
    plain = lambda: [_lib.lora_fold(o["w"], o["up"], o["down"]) for o in ops]
    loha(), lokr(), plain()                           # warm-up
    out = {"projections": len(ops), "loha_rank": r, "lokr_w2_rank": r_kr, "loha_device": _event_ms(loha, reps),
           "lokr_device": _event_ms(lokr, reps), "lora_rank64_device": _event_ms(plain, reps)}
    for kind, opts in KINDS.items():
        wrapped = wrap_lycoris(lb.build(sl, True), seed=1, **opts)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for m in wrapped:
            lora.linear_params(m)
        torch.cuda.synchronize()
        out[f"{kind}_linear_params_first_call_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        out["wrapped"] = len(wrapped)
    return out


def segment(sl, B, F, latent, reps, warmup):
    base = lb.patch(lb.build(sl, False), B, latent, False)
    models, variants = [base], {}
    for kind, opts in KINDS.items():
        fused = lb.build(sl, False)
        wrap_lycoris(fused, seed=1, **opts)
        module = copy.deepcopy(fused)
        models += [lb.patch(fused, B, latent, False), lb.patch(module, B, latent, False)]
    names = ["unadapted"] + [f"{k}_{v}" for k in KINDS for v in ("fused", "module")]
    for name, unet in zip(names, models):
        on = name.endswith("_module")
        st = lb.stream_for(unet, sl, B, F, latent, False)
        with lb.module_path(on):
            st.populate()
        variants[name] = (st, on)
    res = lb.time_variants(variants, reps, warmup)
    for u in models:
        vidtome_amd.remove_patch(u)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lycoris_block.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/lycoris_block.py needs a GPU"
    sl = sites.sd15_sites()
    res = {"what": "fold: ms for all 160 SD-1.5 block projections (device events, median and [min, max] of 5); "
                   "cfg2_top_segment: ms per steady pass of up3.0 (B = 2, 16 frames 512x512; device events, median and "
                   "[min, max] of --reps after --warmup, variants alternating), adapters on the four attn1 projections",
           "device": torch.cuda.get_device_name(0), "fold": fold_times(sl)}
    top = [s for s in sl if s.name == "up3.0"]
    res["cfg2_top_segment"] = segment(top, 2, 16, (64, 64), a.reps, a.warmup)
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
