"""Speed of the fp32 projection GEMMs (csrc/linear_f32.hip) and of the fp32 block with `fp32_projections`.

    timeout -k 10 900 python tools/fp32_block.py [--reps 10]

1. Every new GEMM at the cfg-2 / cfg-5 top-block and cfg-2 mid-block shapes against F.linear (hipBLASLt) on the same
   operands (the library gets the gathered rows materialised, the residual as a separate add): ms per call (median of --reps
   after a warm-up, device events) and executed TFLOP/s as a fraction of the MI355X fp32 matrix peak (157.3 TFLOP/s).
2. The fp32 SD-1.5 stand-in full block (sites.SiteUNet(..., full=True): norm1 / attn1 on merged tokens, attn2 over 77
   conditioning tokens, GEGLU feed-forward) at cfg-2 sizes, per site (top, mid, un-merged), with and without
   `fp32_projections`, each with `fp32_attention` on and off.
Prints one JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 157.3e12
# (name, B, n rows per sample, K, N, epilogue, transposed, rows gathered through a map)
GEMMS = [
    ("cfg-2 top attn1 q|k", 2, 52224, 320, 640, "none", False, True),
    ("cfg-2 top attn1 V^T", 2, 52224, 320, 320, "none", True, True),
    ("cfg-2 top attn1 q (live rows)", 2, 34816, 320, 320, "none", False, True),
    ("cfg-2 top attn1 out", 2, 34816, 320, 320, "none", False, False),
    ("cfg-2 top attn2 q", 1, 131072, 320, 320, "none", False, False),
    ("cfg-2 top attn2 out + resid", 1, 131072, 320, 320, "resid", False, False),
    ("cfg-2 top FF GEGLU", 1, 131072, 320, 2560, "geglu", False, False),
    ("cfg-2 top FF out + resid", 1, 131072, 1280, 320, "resid", False, False),
    ("cfg-2 mid attn1 q|k", 2, 13056, 640, 1280, "none", False, True),
    ("cfg-2 mid attn1 V^T", 2, 13056, 640, 640, "none", True, True),
    ("cfg-2 mid attn2 out + resid", 1, 32768, 640, 640, "resid", False, False),
    ("cfg-2 mid FF GEGLU", 1, 32768, 640, 5120, "geglu", False, False),
    ("cfg-2 mid FF out + resid", 1, 32768, 2560, 640, "resid", False, False),
    ("cfg-5 top attn1 q|k", 2, 90319, 320, 640, "none", False, True),
    ("cfg-5 top FF GEGLU", 1, 262144, 320, 2560, "geglu", False, False),
    ("cfg-5 top FF out + resid", 1, 262144, 1280, 320, "resid", False, False),
]


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def gemms(reps):
    from vidtome_amd import _lib
    F = torch.nn.functional
    for name, B, n, K, N, epi, tr, mapped in GEMMS:
        g = torch.Generator(device="cuda").manual_seed(n + K)
        P = n + n // 4 if mapped else n
        x0 = torch.randn(B, P, K, device="cuda", generator=g)
        rows = torch.randint(0, P, (B, n), device="cuda", generator=g, dtype=torch.int32) if mapped else None
        W = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5
        bias = torch.randn(N, device="cuda", generator=g)
        Nout = N // 2 if epi == "geglu" else N
        resid = torch.randn(B, n, Nout, device="cuda", generator=g) if epi == "resid" else None
        out = torch.empty((B, Nout, n) if tr else (B, n, Nout), device="cuda")
        hip = lambda: _lib.linear_f32(x0, None, rows, None, n, W, bias, epilogue=epi, resid=resid, transposed=tr, out=out)
        xg = torch.stack([x0[b, rows[b].long()] for b in range(B)]) if mapped else x0
        if epi == "resid":
            lib = lambda: torch.add(F.linear(xg, W, bias), resid)
        else:
            lib = lambda: F.linear(xg, W, bias)             # (GEGLU: the library writes the 2D-wide product, no activation)
        fl = 2.0 * B * n * K * N
        res = {"gemm": name, "B": B, "n": n, "K": K, "N": N, "epilogue": epi, "transposed": tr}
        for tag, fn in (("hip", hip), ("F.linear", lib)):
            ms = _time(fn, reps)
            res[tag + "_ms"] = round(ms, 3)
            res[tag + "_fraction_of_fp32_peak"] = round(fl / ms / 1e-3 / PEAK, 3)
        print(json.dumps(res), flush=True)
        del x0, xg, out, resid
        torch.cuda.empty_cache()


def _torch_cross_forward(self, x, encoder_hidden_states=None, attention_mask=None):
    """Diffusers' Attention for the stand-in's attn2 (it has no forward of its own): the module path an fp32 block takes
    without ``fp32_projections`` (library GEMMs and torch's attention)."""
    F = torch.nn.functional
    B, N, C = x.shape
    h = self.heads
    ctx = x if encoder_hidden_states is None else encoder_hidden_states
    sh = lambda t: t.reshape(B, -1, h, C // h).transpose(1, 2)
    o = F.scaled_dot_product_attention(sh(self.to_q(x)), sh(self.to_k(ctx)), sh(self.to_v(ctx)), scale=self.scale)
    return self.to_out[0](o.transpose(1, 2).reshape(B, N, C))


def block_pass(reps):
    import vidtome_amd
    from vidtome_amd import sites as S
    S.CrossAttention.forward = _torch_cross_forward
    B, F, latent = 2, 16, (64, 64)
    sl = [s for s in S.sd15_sites() if s.name in ("down0.0", "down1.0", "down2.0")]
    kind = {"down0.0": "top (merged, d = 40)", "down1.0": "mid (merged, d = 80)", "down2.0": "un-merged (d = 160)"}
    unet = S.SiteUNet(sl, seed=3, full=True).to(device="cuda", dtype=torch.float32)
    vidtome_amd.apply_patch(unet, local_merge_ratio=0.9, merge_global=True, global_merge_ratio=0.8, batch_size=B)
    unet.set_size(latent)
    hiddens = [S.synthetic_hidden(s, B, F, latent, torch.float32, "cuda", seed=40 + i) for i, s in enumerate(sl)]
    g = torch.Generator(device="cuda").manual_seed(5)
    cond = torch.randn(B, 1, 77, 768, device="cuda", generator=g).expand(B, F, 77, 768).reshape(B * F, 77, 768).contiguous()
    with torch.no_grad():
        for _ in range(2):                      # the global level reaches its steady state
            S.run_block_pass(unet, hiddens, cond)
        for proj in (False, True):
            for att in (False, True):
                vidtome_amd.update_patch(unet, fp32_projections=proj, fp32_attention=att)
                for blk, h, s in zip(unet.blocks, hiddens, sl):
                    ms = _time(lambda: blk(h, encoder_hidden_states=cond), reps)
                    print(json.dumps({"block": f"cfg-2 fp32 {kind[s.name]}", "fp32_projections": proj, "fp32_attention": att,
                                      "ms": round(ms, 2)}), flush=True)
    vidtome_amd.remove_patch(unet)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    gemms(args.reps)
    block_pass(args.reps)
