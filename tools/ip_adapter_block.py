"""IP-Adapter attn2 segment (norm2 through residual) at the cfg-2 top and mid blocks, fp16: one JSON line.

    python tools/ip_adapter_block.py [--reps 30] [--out profiles/ip_adapter_block.json]

Per site and adapter set (one 4-token adapter; a 16 + 257-token pair), event-timed in ONE process, the variants
interleaved repetition by repetition so they share the clock:
  plain     no adapter: today's norm_cross_attention_residual (the floor)
  fused     the IP-Adapter path: one vtm_attention_kv_sets launch
  composed  the same host path with the core as 1 + n vtm_attention_kv launches and torch adds
  module    the recogniser refuses: LayerNorm + the module's own forward (library GEMMs, torch SDPA per term) + residual
Reports median and min / max in microseconds; a difference is real only when the min-max ranges do not overlap.

    python tools/ip_adapter_block.py --masks [--reps 30] [--out profiles/ip_adapter_masks.json]

The region-mask case (``cross_attention_kwargs={"ip_adapter_masks": [...]}``): two adapters of 16 and 4 tokens, one image each,
the first masked to the left half of the frame and the second to the top half, at the same two sites, measured the same way:
  fused     one vtm_attention_kv_sets_masked launch (the mask downsample included, as at every forward)
  module    the recogniser refuses: the processor's loop over images, its downsample, fp16 multiplies and adds"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def composed_core(_lib):
    def core(q, k, vt, heads, Mq, sets, scale):
        out = None
        for s, n, w in sets:
            o = _lib.attention_kv_range(q, k, vt, heads, Mq, s, n, scale)     # (the set where it lies: no copy)
            out = o if out is None and w == 1.0 else (o * w if out is None else out + o * w)
        return out
    return core


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


def masked(args):
    from ip_adapter_mask_standin import install
    from vidtome_amd import _lib, ip_adapter, patch as vpatch, sites as S
    dev, dt = "cuda", torch.float16
    B, F = 2, 16
    tokens, scales = (16, 4), (1.0, 0.6)
    result = {"tool": "ip_adapter_block --masks", "device": torch.cuda.get_device_name(0), "dtype": "fp16", "reps": args.reps,
              "unit": "us", "sites": {}}
    left, top = torch.zeros(1, 1, 64, 64, device=dev), torch.zeros(1, 1, 64, 64, device=dev)
    left[..., :32] = 1
    top[:, :, :32] = 1
    kw = {"ip_adapter_masks": [left, top]}
    for site in [s for s in S.sd15_sites() if s.name in ("up3.0", "up2.0")]:
        N = (64 // site.downsample) ** 2
        h = S.synthetic_hidden(site, B, F, (64, 64), dt, dev, seed=1)
        g = torch.Generator().manual_seed(3)
        text = torch.randn(B * F, 77, 768, generator=g).to(device=dev, dtype=dt)
        ims = [torch.randn(B * F, 1, t, 768, generator=g).to(device=dev, dtype=dt) for t in tokens]
        enc = (text, ims)
        unet = S.SiteUNet([site], seed=0, full=True).to(device=dev, dtype=dt)
        blk = unet.blocks[0]
        install(unet, tokens, scales)
        launches = []
        core = _lib.attention_kv_sets_masked

        def fused():
            ip = vpatch.ip_cross_call(blk.attn2, h, enc, None, kw, blk.norm2)
            return vpatch.norm_cross_attention_residual(blk.norm2, blk.attn2, h, None, ip)

        def module():
            refuse, ip_adapter.is_ip_processor = ip_adapter.is_ip_processor, lambda attn: False
            try:
                return vpatch.cross_attention(blk.attn2, vpatch.layer_norm(blk.norm2, h), enc, None, **kw) + h
            finally:
                ip_adapter.is_ip_processor = refuse

        with torch.no_grad():
            _lib.attention_kv_sets_masked = lambda *a, **k: (launches.append(1), core(*a, **k))[1]
            try:
                ref = fused().float()
            finally:
                _lib.attention_kv_sets_masked = core
            assert launches == [1], "the masked launch did not run"
            d = float((module().float() - ref).abs().max())
            assert d < 2e-2 * max(1.0, float(ref.abs().max())), d
            key = f"{site.name} C={site.channels} N={N} adapters={'+'.join(map(str, tokens))} half-frame masks"
            result["sites"][key] = _timed({"fused": fused, "module": module}, args.warmup, args.reps)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--masks", action="store_true", help="the region-mask case (see the module docstring)")
    args = ap.parse_args()
    if args.masks:
        line = json.dumps(masked(args))
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    from ip_adapter_standin import image_states, install
    from lora_standin import SDPAAttention
    from vidtome_amd import _lib, ip_adapter, patch as vpatch, sites as S
    dev, dt = "cuda", torch.float16
    B, F = 2, 16
    fused_core = _lib.attention_kv_sets
    result = {"tool": "ip_adapter_block", "device": torch.cuda.get_device_name(0), "dtype": "fp16", "reps": args.reps,
              "unit": "us", "sites": {}}
    for site in [s for s in S.sd15_sites() if s.name in ("up3.0", "up2.0")]:
        N = (64 // site.downsample) ** 2
        h = S.synthetic_hidden(site, B, F, (64, 64), dt, dev, seed=1)
        text = torch.randn(B * F, 77, 768, generator=torch.Generator().manual_seed(3)).to(device=dev, dtype=dt)
        for tokens, scales in (((4,), (0.6,)), ((16, 257), (0.7, 0.3))):
            unet = S.SiteUNet([site], seed=0, full=True).to(device=dev, dtype=dt)
            blk = unet.blocks[0]
            plain_attn = SDPAAttention(blk.attn2)
            install(unet, tokens, scales)
            ims = image_states(tokens, B * F, 768, dt, dev)
            enc = (text, ims)

            def ip_path():
                ip = vpatch.ip_cross_call(blk.attn2, h, enc, None, {}, blk.norm2)
                return vpatch.norm_cross_attention_residual(blk.norm2, blk.attn2, h, None, ip)

            def composed():
                _lib.attention_kv_sets = composed_core(_lib)
                try:
                    return ip_path()
                finally:
                    _lib.attention_kv_sets = fused_core

            def module():
                refuse, ip_adapter.is_ip_processor = ip_adapter.is_ip_processor, lambda attn: False
                try:
                    return vpatch.cross_attention(blk.attn2, vpatch.layer_norm(blk.norm2, h), enc, None) + h
                finally:
                    ip_adapter.is_ip_processor = refuse

            variants = {
                "plain": lambda: vpatch.norm_cross_attention_residual(blk.norm2, plain_attn, h, text),
                "fused": ip_path,
                "composed": composed,
                "module": module,
            }
            times = {k: [] for k in variants}
            with torch.no_grad():
                ref = variants["fused"]().float()
                for name in ("composed", "module"):
                    d = float((variants[name]().float() - ref).abs().max())
                    assert d < 2e-2 * max(1.0, float(ref.abs().max())), (name, d)
                for rep in range(args.warmup + args.reps):
                    for name, fn in variants.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fn()
                        e1.record()
                        e1.synchronize()
                        if rep >= args.warmup:
                            times[name].append(e0.elapsed_time(e1) * 1e3)
            key = f"{site.name} C={site.channels} N={N} adapters={'+'.join(map(str, tokens))}"
            result["sites"][key] = {k: {"median": round(statistics.median(v), 1), "min": round(min(v), 1),
                                        "max": round(max(v), 1)} for k, v in times.items()}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
