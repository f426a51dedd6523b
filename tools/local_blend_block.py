"""attn2 segment (norm2 through residual) with LocalBlend's word maps, cfg-2 top and mid blocks, fp16: one JSON line.

    python tools/local_blend_block.py [--reps 30] [--out profiles/local_blend_block.json]

Per site, event-timed in ONE process on the same inputs -- a [source | uncond | cond] x 8 frames batch, words on groups 0
and 2 -- the variants interleaved repetition by repetition so they share the clock:
  fused        norm_cross_attention_residual as an unregistered block runs it (vtm_attention_kv)
  fused_words  the same with ``words_to``: one vtm_attention_word_map launch per group in ``words`` adds the group's word
               map into the LocalBlend accumulator (this is what register_local_blend costs)
  full_maps    what a user writes without it: ``probs_to`` (register_attention_maps: one vtm_attention_probs launch, a fresh
               (B F, N, 77) fp32 map) and, per group, ``map[rows] @ w`` and ``index_add_`` into an accumulator of their own
Reports median and min / max in microseconds; a difference is real only when the min-max ranges do not overlap.  Nothing is
asserted about the times; the two accumulators are compared.  The same run times one ``LocalBlend.blend`` (vtm_local_blend)
on 16 x 4 x 64 x 64 fp16 latents, for maps of 16 x 16 and of 64 x 64 tokens."""
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vidtome_amd import LocalBlend, _lib, patch as vpatch, sites as S
    dev, dt = "cuda", torch.float16
    G, Fr, keys = 3, 8, 77
    words = {0: LocalBlend.word_weights(keys, [2, 5]), 2: LocalBlend.word_weights(keys, [2, 6])}
    result = {"tool": "local_blend_block", "device": torch.cuda.get_device_name(0), "dtype": "fp16", "reps": args.reps,
              "unit": "us", "batch": f"{G} groups x {Fr} frames, words on groups {sorted(words)}", "sites": {}}
    for site in [s for s in S.sd15_sites() if s.name in ("up3.0", "up2.0")]:
        N = (64 // site.downsample) ** 2
        h = S.synthetic_hidden(site, G, Fr, (64, 64), dt, dev, seed=1)
        text = torch.randn(G * Fr, keys, 768, generator=torch.Generator().manual_seed(3)).to(device=dev, dtype=dt)
        unet = S.SiteUNet([site], seed=0, full=True).to(device=dev, dtype=dt)
        blk = unet.blocks[0]
        attn = blk.attn2
        assert vpatch.fused_cross_ok(blk.norm2, attn, h, text, None, {})
        lb = LocalBlend(words, G, Fr)
        holder = torch.nn.Module()
        own = torch.zeros((len(words), Fr, N), dtype=torch.float32, device=dev)      # the user's accumulator
        rows = torch.arange(Fr, device=dev)
        w_dev = lb.weights_on(dev)
        launches = []
        core = _lib.attention_word_map

        def fused():
            return vpatch.norm_cross_attention_residual(blk.norm2, attn, h, text)

        def fused_words():
            return vpatch.norm_cross_attention_residual(blk.norm2, attn, h, text, words_to=(lb, site.name))

        def full_maps():
            out = vpatch.norm_cross_attention_residual(blk.norm2, attn, h, text, probs_to=holder)
            for gi, g in enumerate(lb.groups):
                own[gi].index_add_(0, rows, torch.matmul(holder.attn2_probs[g * Fr:(g + 1) * Fr], w_dev[gi]))
            return out

        with torch.no_grad():
            _lib.attention_word_map = lambda *a, **k: (launches.append(1), core(*a, **k))[1]
            try:
                out = fused_words()
            finally:
                _lib.attention_word_map = core
            assert launches == [1] * len(words), "the word-map launches did not run"
            assert torch.equal(out, fused()), "the word maps changed the segment's output"
            full_maps()
            d = float((lb.maps().view(len(words), Fr, N) - own).abs().max())
            assert d < 1e-5, d
            key = f"{site.name} C={site.channels} N={N} keys={keys}"
            result["sites"][key] = _timed({"fused": fused, "fused_words": fused_words, "full_maps": full_maps},
                                          args.warmup, args.reps)
            result["sites"][key]["max_abs_accumulator_difference"] = float(f"{d:.3e}")
            result["sites"][key]["full_map_bytes"] = holder.attn2_probs.numel() * 4
            result["sites"][key]["word_map_bytes_per_forward"] = len(words) * Fr * N * 4
    # the blend tail
    Fv = 16
    g = torch.Generator().manual_seed(5)
    x = torch.randn(Fv, 4, 64, 64, generator=g).to(device=dev, dtype=dt)
    x_src = torch.randn(Fv, 4, 64, 64, generator=g).to(device=dev, dtype=dt)
    result["blend"] = {"latents": "16 x 4 x 64 x 64 fp16", "groups": len(words), "pool": 1}
    for side in (16, 64):
        lb = LocalBlend(words, G, Fv)
        lb.accumulator(side * side, dev).copy_(torch.rand(len(words), Fv, side * side, generator=g) ** 8)
        out = torch.empty_like(x)
        with torch.no_grad():
            result["blend"][f"map {side} x {side}"] = _timed({"blend": lambda: lb.blend(x, x_src, out=out)},
                                                             args.warmup, args.reps)["blend"]
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
