"""Self-attention guidance: the mid block's attn1 segment with and without the key mass, and the degrade step against its
torch composition, fp16: one JSON line.

    python tools/sag_block.py [--reps 30] [--out profiles/sag_block.json]

Event-timed in ONE process on the same inputs, the variants interleaved repetition by repetition so they share the clock:
  plain        the cfg-2 mid block's attn1 segment (norm1 through residual; 2 x 16 frames of 8 x 8 tokens, C = 1280) as an
               unregistered block runs it (unmerged_self_attention_residual)
  registered   the same on a block registered for self-attention guidance: one vtm_attention_key_mass launch beside the core
  storing      what gave the map before: LayerNorm + a module forward with a storing processor -- three library GEMMs, the
               (B F heads, N, N) probabilities materialised in the model's dtype (baddbmm + softmax, as Diffusers'
               AttnProcessor computes them), their head mean summed over the queries, bmm with v, the output GEMM -- + the
               residual add
  degrade      SelfAttentionGuidance.degrade's launch (vtm_sag_degrade) at 16 x 4 x 64 x 64 and 16 x 4 x 96 x 96 latents
  degrade_torch  its torch composition in the model's dtype, as the Diffusers pipeline strings it together: pred_x0,
               threshold + nearest interpolate, reflect pad + depthwise conv2d, the masked mix, add_noise
Reports median and min / max in microseconds; a difference is real only when the min-max ranges do not overlap.  Nothing is
asserted about the times; the masses and the degraded latents of the two forms are compared."""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class StoringSelfAttention(torch.nn.Module):
    """attn1's module forward with a storing processor, on the projections of ``src``; ``mass``: the head mean of the
    probabilities summed over the queries."""

    def __init__(self, src: torch.nn.Module):
        super().__init__()
        self.heads, self.scale = src.heads, src.scale
        self.to_q, self.to_k, self.to_v, self.to_out = src.to_q, src.to_k, src.to_v, src.to_out
        self.mass = None

    def forward(self, x):
        n, N, C = x.shape
        h = self.heads
        sh = lambda t: t.view(n, N, h, C // h).permute(0, 2, 1, 3).reshape(n * h, N, C // h)
        q, k, v = sh(self.to_q(x)), sh(self.to_k(x)), sh(self.to_v(x))
        p = torch.baddbmm(torch.empty(n * h, N, N, dtype=q.dtype, device=q.device), q, k.transpose(1, 2), beta=0,
                          alpha=self.scale).softmax(dim=-1)                     # (B F heads, N, N) in the model's dtype
        self.mass = p.view(n, h, N, N).float().mean(1).sum(1)
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


def degrade_torch(x, m, mass, h_m, w_m, sa, sb, taps, threshold):
    """Epsilon prediction, in the tensors' dtype."""
    Fr, C, H, W = x.shape
    x0 = (x - sb * m) / sa
    mask = (mass > threshold).view(Fr, 1, h_m, w_m).to(x.dtype)
    mask = F.interpolate(mask, size=(H, W), mode="nearest")
    r = taps.numel() // 2
    k2 = (taps[:, None] * taps[None, :]).to(x.dtype).expand(C, 1, -1, -1)
    blur = F.conv2d(F.pad(x0, (r, r, r, r), mode="reflect"), k2, groups=C)
    deg = blur * mask + x0 * (1 - mask)
    return sa * deg + sb * m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import vidtome_amd
    from vidtome_amd import _lib, patch as vpatch, sites as S
    dev, dt = "cuda", torch.float16
    B, Fr = 2, 16
    result = {"tool": "sag_block", "device": torch.cuda.get_device_name(0), "dtype": "fp16", "reps": args.reps, "unit": "us",
              "segment": {}, "degrade": {}}
    site = next(s for s in S.sd15_sites() if s.name == "mid")
    N = (64 // site.downsample) ** 2
    h = S.synthetic_hidden(site, B, Fr, (64, 64), dt, dev, seed=1)
    unet = S.SiteUNet([site], seed=0, full=True).to(device=dev, dtype=dt)
    vidtome_amd.apply_patch(unet, local_merge_ratio=0.5, merge_global=True, global_merge_ratio=0.5, batch_size=B)
    unet.set_size((64, 64))
    blk = unet.blocks[0]
    attn = StoringSelfAttention(blk.attn1)
    assert vpatch.unmerged_self_attention_ok(blk, h), "the mid block does not take the un-merged panel body"

    def plain():
        blk.__dict__.pop("vtm_sag", None)
        return vpatch.self_attention_segment(blk, h)

    def registered():
        blk.__dict__["vtm_sag"] = True
        return vpatch.self_attention_segment(blk, h)

    def storing():
        return attn(vpatch.layer_norm(blk.norm1, h)) + h

    with torch.no_grad():
        assert torch.equal(registered(), plain()), "the key mass changed the segment's output"
        storing()
        mass = blk.attn1_key_mass
        d = float((mass - attn.mass).abs().max())
        assert tuple(mass.shape) == (B * Fr, N) and d < 5e-2, d
        key = f"mid C={site.channels} N={N} frames={B * Fr}"
        result["segment"][key] = _timed({"plain": plain, "registered": registered, "storing": storing}, args.warmup, args.reps)
        result["segment"][key]["max_abs_mass_difference_to_storing"] = float(f"{d:.3e}")
        result["segment"][key]["storing_probability_bytes"] = B * Fr * site.heads * N * N * 2
        blk.__dict__.pop("vtm_sag", None)

        taps = _lib.gaussian_taps(4, 1.0)
        taps_t = torch.tensor(taps, device=dev)
        sa, sb = math.sqrt(0.37), math.sqrt(0.63)
        for H in (64, 96):
            g = torch.Generator().manual_seed(H)
            x = torch.randn(16, 4, H, H, generator=g).to(device=dev, dtype=dt)
            m = torch.randn(16, 4, H, H, generator=g).to(device=dev, dtype=dt)
            h_m = H // 8
            ms = (torch.rand(16, h_m * h_m, generator=g) * 2).to(dev)
            out = torch.empty_like(x)

            def degrade():
                return _lib.sag_degrade(x, m, ms, h_m, h_m, sa, sb, taps, 1.0, out=out)

            def composed():
                return degrade_torch(x, m, ms, h_m, h_m, sa, sb, taps_t, 1.0)

            dd = float((degrade().float() - composed().float()).abs().max())
            assert dd < 5e-2, dd
            key = f"16x4x{H}x{H}"
            result["degrade"][key] = _timed({"degrade": degrade, "degrade_torch": composed}, args.warmup, args.reps)
            result["degrade"][key]["max_abs_difference_to_torch"] = float(f"{dd:.3e}")
    vidtome_amd.remove_patch(unet)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
