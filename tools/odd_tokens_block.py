"""attn2 and un-merged attn1 segments at token counts that are no multiple of 8 (480 x 848 video), fp16: one JSON line.

    python tools/odd_tokens_block.py [--reps 30] [--test-log LOG] [--out profiles/odd_tokens_block.json]

Sites: 30 x 53 = 1590 tokens per frame at C = 640 and 15 x 27 = 405 at C = 1280, 16 frames, batch 2.  Per site and segment,
event-timed in ONE process on the same inputs, the variants interleaved repetition by repetition so they share the clock:
  attn2  fused    norm_cross_attention_residual: LayerNorm -> panels, q GEMM, vtm_attention_kv on the dense (B F, N, C)
                  queries, output GEMM with bias and residual
         parent   what N % 8 != 0 took before: vtm_layernorm, cross_attention() (F.pad of the tokens to Np rows, library
                  GEMMs for q and out around the core, a slice) and the residual add
  attn1  fused    unmerged_self_attention_residual: norm1 -> panels, one q | k | v GEMM, vtm_transpose_cols, the core per
                  frame, output GEMM with bias and residual
         parent   patched_self_attention_segment at a site that does not merge: vtm_layernorm, self_attention_panels
                  (gather into 256-row panels per frame, one V^T GEMM per frame), a slice and the residual add
Reports median and min / max in microseconds; a difference is real only when the min-max ranges do not overlap.  Nothing is
asserted about the times.  ``--test-log``: the output of `pytest -s tests/test_gpu_odd_tokens.py`; the worst err/scale of
its float64 checks goes into the JSON per segment and dtype."""
import argparse
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from masked_cross_block import _timed  # noqa: E402


def worst_errors(path):
    """{segment: {dtype: worst err/scale}} from the printed figures of tests/test_gpu_odd_tokens.py."""
    worst = {}
    pat = re.compile(r"odd-N (attn2 segment|un-merged attn1 segment|patched block).*?torch\.(float16|bfloat16).*?err/scale=([0-9.e+-]+)")
    with open(path) as f:
        for line in f:
            for seg, dt, err in pat.findall(line):
                d = worst.setdefault(seg, {})
                d[dt] = max(d.get(dt, 0.0), float(err))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--test-log", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import vidtome_amd
    from vidtome_amd import patch as vpatch, sites as S
    dev, dt = "cuda", torch.float16
    B, Fr, keys, latent = 2, 16, 77, (60, 106)
    result = {"tool": "odd_tokens_block", "device": torch.cuda.get_device_name(0), "dtype": "fp16", "reps": args.reps,
              "unit": "us", "frames": Fr, "batch": B, "sites": {}}
    for name, ds, C, (gh, gw) in (("up2.0", 2, 640, (30, 53)), ("up1.0", 4, 1280, (15, 27))):
        N = gh * gw
        unet = S.SiteUNet([S.Site(name, ds, C, 8)], seed=0, full=True).to(device=dev, dtype=dt)
        # max_downsample = 1: neither site merges (the un-merged attn1 segment is what is timed)
        vidtome_amd.apply_patch(unet, local_merge_ratio=0.5, merge_global=True, global_merge_ratio=0.5, batch_size=B,
                                max_downsample=1)
        unet.set_size(latent)
        blk = unet.blocks[0]
        blk.generator = vpatch.init_generator(torch.device(dev), mode=None)
        g = torch.Generator().manual_seed(1)
        h = S.regime_tokens("corr05", B, Fr, N, C, g).reshape(B * Fr, N, C).to(device=dev, dtype=dt)
        text = torch.randn(B * Fr, keys, 768, generator=torch.Generator().manual_seed(3)).to(device=dev, dtype=dt)
        assert N % 8 and vpatch.fused_cross_ok(blk.norm2, blk.attn2, h, text, None, {})
        assert vpatch.unmerged_self_attention_ok(blk, h)

        def cross_fused():
            return vpatch.norm_cross_attention_residual(blk.norm2, blk.attn2, h, text)

        def cross_parent():
            return vpatch.cross_attention(blk.attn2, vpatch.layer_norm(blk.norm2, h), text) + h

        def self_fused():
            return vpatch.unmerged_self_attention_residual(blk, h)

        def self_parent():
            return vpatch.patched_self_attention_segment(blk, h, vpatch.layer_norm(blk.norm1, h))

        with torch.no_grad():
            for a, b in ((cross_fused, cross_parent), (self_fused, self_parent)):
                ref = a().float()
                d = float((b().float() - ref).abs().max())
                assert d < 2e-3 * max(1.0, float(ref.abs().max())), (a.__name__, d)
            key = f"{name} C={C} N={N} ({gh} x {gw}) N%8={N % 8}"
            result["sites"][key] = _timed({"attn2 fused": cross_fused, "attn2 parent": cross_parent,
                                           "attn1 fused": self_fused, "attn1 parent": self_parent}, args.warmup, args.reps)
        vidtome_amd.remove_patch(unet)
    if args.test_log:
        result["float64 checks, worst err/scale"] = worst_errors(args.test_log)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
