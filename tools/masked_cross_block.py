"""Masked attn2 segment (norm2 through residual) at the cfg-2 top and mid blocks, fp16: one JSON line.

    python tools/masked_cross_block.py [--reps 30] [--out profiles/masked_cross_block.json]

The conditioning is 77 text tokens with an ``encoder_attention_mask`` in Diffusers' additive form, (B F, 1, 77) of 0 / -10000,
that hides the last 20 keys.  Per site, event-timed in ONE process on the same inputs, the variants interleaved repetition
by repetition so they share the clock:
  fused     the recognised mask: norm_cross_attention_residual with the core on vtm_attention_kv_bias
  module    the recogniser refuses: LayerNorm + the module's own forward (three library GEMMs, torch SDPA with the mask, the
            output GEMM) + the residual add -- what every masked call was before the kernel
  unmasked  today's norm_cross_attention_residual without a mask (vtm_attention_kv): what the mask costs on the fused path
Reports median and min / max in microseconds; a difference is real only when the min-max ranges do not overlap.  Nothing is
asserted about the times."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class MaskedSDPA(torch.nn.Module):
    """attn2's module forward as Diffusers' AttnProcessor2_0 computes it, on the projections of ``src``."""

    def __init__(self, src: torch.nn.Module):
        super().__init__()
        self.heads, self.scale = src.heads, src.scale
        self.to_q, self.to_k, self.to_v, self.to_out = src.to_q, src.to_k, src.to_v, src.to_out

    def forward(self, x, encoder_hidden_states=None, attention_mask=None, **kw):
        n, N, _ = x.shape
        sh = lambda t: t.view(n, t.shape[1], self.heads, -1).transpose(1, 2)
        q, k, v = self.to_q(x), self.to_k(encoder_hidden_states), self.to_v(encoder_hidden_states)
        mask = None if attention_mask is None else attention_mask[:, None].expand(-1, self.heads, -1, -1)
        o = F.scaled_dot_product_attention(sh(q), sh(k), sh(v), attn_mask=mask, scale=self.scale)
        return self.to_out[0](o.transpose(1, 2).reshape(n, N, -1))


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
    B, Fr, keys, hidden_keys = 2, 16, 77, 20
    result = {"tool": "masked_cross_block", "device": torch.cuda.get_device_name(0), "dtype": "fp16", "reps": args.reps,
              "unit": "us", "mask": f"last {hidden_keys} of {keys} keys at -10000", "sites": {}}
    mask = torch.zeros(B * Fr, 1, keys, device=dev, dtype=dt)
    mask[..., keys - hidden_keys:] = -10000.0
    for site in [s for s in S.sd15_sites() if s.name in ("up3.0", "up2.0")]:
        N = (64 // site.downsample) ** 2
        h = S.synthetic_hidden(site, B, Fr, (64, 64), dt, dev, seed=1)
        text = torch.randn(B * Fr, keys, 768, generator=torch.Generator().manual_seed(3)).to(device=dev, dtype=dt)
        unet = S.SiteUNet([site], seed=0, full=True).to(device=dev, dtype=dt)
        blk = unet.blocks[0]
        attn = MaskedSDPA(blk.attn2)
        launches = []
        core = _lib.attention_kv_bias
        assert vpatch.fused_cross_ok(blk.norm2, attn, h, text, mask, {})

        def fused():
            return vpatch.norm_cross_attention_residual(blk.norm2, attn, h, text, attention_mask=mask)

        def module():
            return attn(vpatch.layer_norm(blk.norm2, h), encoder_hidden_states=text, attention_mask=mask) + h

        def unmasked():
            return vpatch.norm_cross_attention_residual(blk.norm2, attn, h, text)

        with torch.no_grad():
            _lib.attention_kv_bias = lambda *a, **k: (launches.append(1), core(*a, **k))[1]
            try:
                ref = fused().float()
            finally:
                _lib.attention_kv_bias = core
            assert launches == [1], "the bias launch did not run"
            d = float((module().float() - ref).abs().max())
            assert d < 2e-2 * max(1.0, float(ref.abs().max())), d
            key = f"{site.name} C={site.channels} N={N} keys={keys} hidden={hidden_keys}"
            result["sites"][key] = _timed({"fused": fused, "module": module, "unmasked": unmasked}, args.warmup, args.reps)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
