"""Perturbed-attention-guidance (PAG) attn1 segment (norm1 through residual) at the cfg-2 top and mid blocks, fp16, three
samples [uncond | cond | perturbed] of 16 frames of a 64 x 64 latent: one JSON line.

    python tools/pag_block.py [--reps 30] [--out profiles/pag_block.json]

Per site, event-timed in ONE process on the same inputs, the variants interleaved repetition by repetition so they share
the clock:
  pag_fused    a PAG processor on attn1, recognised: the cores run for two samples, the third is one V projection
  pag_module   the same block on the module path (what the block ran before PAG was recognised): merged tokens
               materialised, the processor's library GEMMs and torch SDPA
  plain_fused  a plain processor: the fused segment over all three samples (no guidance; the cost PAG is compared with)
The top block merges (local_merge_ratio 0.9, global level at 0.8): every repetition is the second chunk of a step -- the
anchors the first chunk stored and the block generator's state are put back before each call, outside the timed region --
once with the local chunk on the src side of the global level (live, compacted queries) and once on the dst side.
Reports median and min / max in microseconds; a difference is real only when the min-max ranges do not overlap."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, F, LATENT = 3, 16, (64, 64)


def _timed(variants, warmup, reps):
    """Event times in us of every variant (prepare, run), interleaved repetition by repetition -> {name: {median, min, max}}."""
    times = {k: [] for k in variants}
    for rep in range(warmup + reps):
        for name, (prepare, fn) in variants.items():
            prepare()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    return {k: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
            for k, v in times.items()}


def _variant(site, name, coin, hs):
    """(prepare, run) of one variant: its own patched model, the first chunk run once to store the anchors."""
    import pag_standin as PS
    import vidtome_amd
    from vidtome_amd import patch as vpatch, sites as S
    unet = S.SiteUNet([site], seed=0).to(device="cuda", dtype=torch.float16)
    PS.install(unet, 3, name="plain" if name == "plain_fused" else None)
    vidtome_amd.apply_patch(unet, local_merge_ratio=0.9, merge_global=True, global_merge_ratio=0.8, batch_size=B,
                            global_rand=coin)
    unet.set_size(LATENT)
    blk = unet.blocks[0]
    torch.manual_seed(123)
    blk.generator = vpatch.init_generator(hs[0].device)
    route = vpatch.attn1_route

    def segment(h):
        if name == "pag_module":
            vpatch.attn1_route = lambda *a, **kw: "module"
        try:
            return vpatch.self_attention_segment(blk, h)
        finally:
            vpatch.attn1_route = route
    segment(hs[0])
    anchors, state = getattr(blk, "global_tokens", None), blk.generator.get_state()

    def prepare():
        blk.global_tokens = anchors
        blk.generator.set_state(state)
    return prepare, lambda: segment(hs[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vidtome_amd import sites as S
    result = {"tool": "pag_block", "device": torch.cuda.get_device_name(0), "dtype": "fp16", "reps": args.reps, "unit": "us",
              "batch": "3 x 16 frames, 64 x 64 latent, [uncond | cond | perturbed]", "sites": {}}
    for site in [s for s in S.sd15_sites() if s.name in ("down0.0", "mid")]:
        N = (LATENT[0] // site.downsample) ** 2
        hs = [S.synthetic_hidden(site, B, F, LATENT, torch.float16, "cuda", seed=1 + j, clip_seed=7, regime="corr01")
              for j in range(2)]
        for side, coin in (("local chunk src", 0.0), ("local chunk dst", 1.0)) if site.name != "mid" else (("un-merged", 0.5),):
            with torch.no_grad():
                variants = {name: _variant(site, name, coin, hs) for name in ("pag_fused", "pag_module", "plain_fused")}
                outs = {}
                for name, (prepare, fn) in variants.items():
                    prepare()
                    outs[name] = fn().float()
                d = float((outs["pag_fused"] - outs["pag_module"]).abs().max())
                assert d < 2e-2 * max(1.0, float(outs["pag_module"].abs().max())), d
                times = _timed(variants, args.warmup, args.reps)
            times["pag_fused / plain_fused"] = round(times["pag_fused"]["median"] / times["plain_fused"]["median"], 3)
            times["pag_fused / pag_module"] = round(times["pag_fused"]["median"] / times["pag_module"]["median"], 3)
            result["sites"][f"{site.name} C={site.channels} N={N} {side}"] = times
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
