"""attn2 segment (norm2 through residual) under Prompt-to-Prompt cross-attention control, cfg-2 top and mid blocks, fp16, a
[source | uncond | cond] x frames batch with the cond group edited: one JSON line.

    python tools/cross_control_block.py [--reps 30] [--out profiles/cross_control_block.json]

Per site, event-timed in ONE process on the same inputs, the variants interleaved repetition by repetition so they share
the clock:
  unregistered  norm_cross_attention_residual as a block without the control runs it (vtm_attention_kv)
  fused         norm_cross_attention_residual with ``ctl=``: the plain core on [source | uncond], vtm_cross_edit_values and
                ONE vtm_attention_kv_sets_src launch on the cond group
  composed_kv   the same edit from the pieces that existed before: V' = M diag(a) V and V'' = diag(b) V in torch, two
                vtm_attention_kv launches on the cond group (the source's q / k on V', its own on V'') plus an add
  torch_probs   what a Prompt-to-Prompt processor does: LayerNorm + three library GEMMs, the (B F heads, N, 77)
                probabilities materialised in the model's dtype, the cond group's replaced by
                (P_src @ M) * a + P_own * b, bmm with v, the output GEMM + the residual add
Reports median and min / max in microseconds; a difference is real only when the min-max ranges do not overlap.  Nothing is
asserted about the times; the three edited outputs are compared."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def _edit(K):
    """A word swap with a fractional alpha_words, re-weighted: three words change places, one becomes two, two are scaled."""
    from vidtome_amd import CrossEdit
    m = torch.eye(K)
    m[3:7] = 0
    m[3, 5], m[4, 3], m[5, 4], m[6, 6], m[6, 7] = 1.0, 1.0, 1.0, 0.5, 0.5
    eq = torch.ones(K)
    eq[4], eq[10] = 2.0, 0.5
    return CrossEdit.replace(m, 0.8).reweight(eq)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vidtome_amd import _lib, patch as vpatch, sites as S
    dev, dt = "cuda", torch.float16
    G, Fr, K = 3, args.frames, 77
    result = {"tool": "cross_control_block", "device": torch.cuda.get_device_name(0), "dtype": "fp16", "reps": args.reps,
              "unit": "us", "groups": G, "frames": Fr, "sites": {}}
    edit = _edit(K)
    M, a, b = edit.on(dev)
    for site in [s for s in S.sd15_sites() if s.name in ("up3.0", "up2.0")]:
        N = (64 // site.downsample) ** 2
        C, heads = site.channels, site.heads
        h = S.synthetic_hidden(site, G, Fr, (64, 64), dt, dev, seed=1)
        text = torch.randn(G * Fr, K, 768, generator=torch.Generator().manual_seed(3)).to(device=dev, dtype=dt)
        unet = S.SiteUNet([site], seed=0, full=True).to(device=dev, dtype=dt)
        blk = unet.blocks[0]
        norm, attn = blk.norm2, blk.attn2
        assert vpatch.fused_cross_ok(norm, attn, h, text, None, {})
        ctl = (G, {2: edit}, site.name)
        scale = attn.scale
        own, src = slice(2 * Fr, 3 * Fr), slice(0, Fr)

        def unregistered():
            return vpatch.norm_cross_attention_residual(norm, attn, h, text)

        def fused():
            return vpatch.norm_cross_attention_residual(norm, attn, h, text, ctl=ctl)

        def composed_kv():
            n = G * Fr * N
            wq, bq = vpatch._panel_weight(attn.to_q)
            wo, bo = vpatch._panel_weight(vpatch._out_linear(attn))
            xp = _lib.layernorm_panels(h, norm.weight, norm.bias, norm.eps)
            q = _lib.linear_panels(xp, n, wq, C, bq).view(G * Fr, N, C)
            k, vt = vpatch._cross_kv(attn.to_k, attn.to_v, vpatch._pad_keys(text, dt), C)
            v_own = vt[own, :, :K].float()
            pad = (0, k.shape[1] - K)
            vt1 = torch.nn.functional.pad(torch.matmul(v_own, (M * a).t()).to(dt), pad)      # (M diag(a) V)^T
            vt2 = torch.nn.functional.pad((v_own * b).to(dt), pad)                            # (diag(b) V)^T
            o = torch.empty_like(q)
            _lib.attention_kv(q[:2 * Fr], k[:2 * Fr], vt[:2 * Fr], heads, N, K, scale, out=o[:2 * Fr])
            o[own] = _lib.attention_kv(q[src], k[src], vt1, heads, N, K, scale) \
                + _lib.attention_kv(q[own], k[own], vt2, heads, N, K, scale)
            return _lib.linear_panels(_lib.to_panels(o.view(n, C)), n, wo, C, bo, resid=h.view(n, C)).view(G * Fr, N, C)

        def torch_probs():
            x = vpatch.layer_norm(norm, h)
            nb, d = G * Fr, C // heads
            sh = lambda t: t.view(nb, t.shape[1], heads, d).permute(0, 2, 1, 3).reshape(nb * heads, t.shape[1], d)
            q, kk, v = sh(attn.to_q(x)), sh(attn.to_k(text)), sh(attn.to_v(text))
            p = torch.baddbmm(torch.empty(nb * heads, N, K, dtype=dt, device=dev), q, kk.transpose(1, 2), beta=0,
                              alpha=scale).softmax(dim=-1).view(nb, heads, N, K)
            p[own] = torch.matmul(p[src], M.to(dt)) * a.to(dt) + p[own] * b.to(dt)
            o = torch.bmm(p.view(nb * heads, N, K), v).view(nb, heads, N, d).permute(0, 2, 1, 3).reshape(nb, N, C)
            return attn.to_out[0](o) + h

        with torch.no_grad():
            base, out = unregistered(), fused()
            assert torch.equal(out[:2 * Fr], base[:2 * Fr]), "an unedited group changed"
            osc = float(out.float().abs().max())
            d_kv = float((out - composed_kv()).float().abs().max()) / osc
            d_t = float((out - torch_probs()).float().abs().max()) / osc
            moved = float((out[own] - base[own]).float().abs().max()) / osc
            assert d_kv < 1e-2 and d_t < 5e-2, (d_kv, d_t)      # (the same edit three ways; torch_probs rounds P to fp16)
            key = f"{site.name} C={C} N={N} keys={K}"
            result["sites"][key] = _timed({"unregistered": unregistered, "fused": fused, "composed_kv": composed_kv,
                                           "torch_probs": torch_probs}, args.warmup, args.reps)
            result["sites"][key].update(max_abs_difference_to_composed_kv_over_scale=float(f"{d_kv:.3e}"),
                                        max_abs_difference_to_torch_probs_over_scale=float(f"{d_t:.3e}"),
                                        edit_over_scale=float(f"{moved:.3e}"),
                                        probs_bytes_torch=G * Fr * heads * N * K * 2)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
