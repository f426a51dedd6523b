"""attn2 segment (norm2 through residual) with and without the cross-attention map, cfg-2 top and mid blocks, fp16: one JSON line.

    python tools/attention_maps_block.py [--reps 30] [--out profiles/attention_maps_block.json]

Per site, event-timed in ONE process on the same inputs, the variants interleaved repetition by repetition so they share
the clock:
  fused        norm_cross_attention_residual as an unregistered block runs it (vtm_attention_kv)
  fused_maps   the same with ``probs_to``: one vtm_attention_probs launch beside the core leaves the (B F, N, 77) fp32 map
  storing      what gave a map before: LayerNorm + a module forward with a storing processor -- three library GEMMs, the
               (B F heads, N, 77) probabilities materialised in the model's dtype (baddbmm + softmax, as Diffusers'
               AttnProcessor computes them), their mean over the heads kept, bmm with v, the output GEMM -- + the residual add
Reports median and min / max in microseconds; a difference is real only when the min-max ranges do not overlap.  Nothing is
asserted about the times; the two maps are compared (the storing processor rounds scores and probabilities to fp16)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class StoringAttention(torch.nn.Module):
    """attn2's module forward with a storing processor, on the projections of ``src``: Diffusers' AttnProcessor arithmetic
    (get_attention_scores: baddbmm in the model's dtype, softmax), the head-mean of the probabilities kept in ``probs``."""

    def __init__(self, src: torch.nn.Module):
        super().__init__()
        self.heads, self.scale = src.heads, src.scale
        self.to_q, self.to_k, self.to_v, self.to_out = src.to_q, src.to_k, src.to_v, src.to_out
        self.probs = None

    def forward(self, x, encoder_hidden_states=None, attention_mask=None, **kw):
        n, N, C = x.shape
        h = self.heads
        sh = lambda t: t.view(n, t.shape[1], h, C // h).permute(0, 2, 1, 3).reshape(n * h, t.shape[1], C // h)
        q, k, v = sh(self.to_q(x)), sh(self.to_k(encoder_hidden_states)), sh(self.to_v(encoder_hidden_states))
        p = torch.baddbmm(torch.empty(n * h, N, k.shape[1], dtype=q.dtype, device=q.device), q, k.transpose(1, 2), beta=0,
                          alpha=self.scale).softmax(dim=-1)                     # (B F heads, N, K) in the model's dtype
        self.probs = p.view(n, h, N, -1).float().mean(1)
        o = torch.bmm(p, v).view(n, h, N, C // h).permute(0, 2, 1, 3).reshape(n, N, C)
        return self.to_out[0](o)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vidtome_amd import _lib, patch as vpatch, sites as S
    dev, dt = "cuda", torch.float16
    B, Fr, keys = 2, 16, 77
    result = {"tool": "attention_maps_block", "device": torch.cuda.get_device_name(0), "dtype": "fp16", "reps": args.reps,
              "unit": "us", "sites": {}}
    for site in [s for s in S.sd15_sites() if s.name in ("up3.0", "up2.0")]:
        N = (64 // site.downsample) ** 2
        h = S.synthetic_hidden(site, B, Fr, (64, 64), dt, dev, seed=1)
        text = torch.randn(B * Fr, keys, 768, generator=torch.Generator().manual_seed(3)).to(device=dev, dtype=dt)
        unet = S.SiteUNet([site], seed=0, full=True).to(device=dev, dtype=dt)
        blk = unet.blocks[0]
        attn = StoringAttention(blk.attn2)
        holder = torch.nn.Module()
        launches = []
        core = _lib.attention_probs
        assert vpatch.fused_cross_ok(blk.norm2, attn, h, text, None, {})

        def fused():
            return vpatch.norm_cross_attention_residual(blk.norm2, attn, h, text)

        def fused_maps():
            return vpatch.norm_cross_attention_residual(blk.norm2, attn, h, text, probs_to=holder)

        def storing():
            return attn(vpatch.layer_norm(blk.norm2, h), encoder_hidden_states=text) + h

        with torch.no_grad():
            _lib.attention_probs = lambda *a, **k: (launches.append(1), core(*a, **k))[1]
            try:
                out = fused_maps()
            finally:
                _lib.attention_probs = core
            assert launches == [1], "the probabilities launch did not run"
            assert torch.equal(out, fused()), "the map changed the segment's output"
            storing()
            d = float((holder.attn2_probs - attn.probs).abs().max())
            assert tuple(holder.attn2_probs.shape) == (B * Fr, N, keys) and d < 1e-2, d
            key = f"{site.name} C={site.channels} N={N} keys={keys}"
            result["sites"][key] = _timed({"fused": fused, "fused_maps": fused_maps, "storing": storing}, args.warmup, args.reps)
            result["sites"][key]["max_abs_map_difference_to_storing"] = float(f"{d:.3e}")
            result["sites"][key]["map_bytes"] = holder.attn2_probs.numel() * 4
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
