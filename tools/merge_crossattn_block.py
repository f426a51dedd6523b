"""merge_crossattn (update_patch(model, merge_crossattn=True): attn2 on the merged local tokens, keys routed per frame) at the
cfg-2 top site (C = 320) and the C = 640 site, fp16, the bench's batch (2 x 16 frames of a 64 x 64 latent), its ratios (local
0.5, global 0.5) and corr01 tokens: one JSON line.

    python tools/merge_crossattn_block.py [--reps 20] [--repeats 3] [--out profiles/merge_crossattn_block.json]

Per site, event-timed in ONE process on the same inputs, the variants alternating repetition by repetition so they share the
clock, warmed, and the whole alternating measurement repeated ``--repeats`` times (>= 3):
  attn2_segment  off: norm_cross_attention_residual (vtm_layernorm_panels -> q panel GEMM -> k / V^T panel GEMMs ->
                 vtm_attention_kv -> vtm_to_panels -> output panel GEMM + residual) over all L rows -- the parent's path, the
                 baseline; on: merged_cross_attention_residual (vtm_frame_order -> vtm_layernorm_gather -> q panel GEMM -> the
                 same k / V^T GEMMs -> vtm_attention_kv_segments -> vtm_to_panels -> output panel GEMM -> vtm_unmerge_add)
                 over M_l rows on the plan of the block's own compute_merge, the frame order computed inside the timed
                 region as a forward computes it; on_order_cached: the same with the plan's cached order (information: what
                 vtm_frame_order costs)
  block          the whole patched block forward (attn1 segment, attn2 over 77 x 768 conditioning that differs per frame
                 row, feed-forward), the second chunk of a step: the anchors the first chunk stored and the generator's state
                 are put back before each call, outside the timed region.  Four variants: no flag, merge_crossattn,
                 merge_mlp, both
Reported per variant: the median of every repeat, the median of those, and ``spread`` = max - min of the repeats' medians --
the run-to-run spread a difference has to exceed.  A verdict ``faster_beyond_spread`` / ``slower_beyond_spread`` is given only
where the repeats' ranges are disjoint.  ``rows`` is M_l / L of the run and the longest segment, ``rel_l2_on_vs_off`` the
relative L2 difference of the block output between flag on and flag off -- information only: the flag changes results by
design."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, F, LATENT, LOCAL, GLOBAL = 2, 16, (64, 64), 0.5, 0.5
SITES = ("up3.0", "up2.0")


def _timed(variants, warmup, reps):
    """Event times in us of every variant (prepare, run), interleaved repetition by repetition -> {name: median}."""
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
    return {k: statistics.median(v) for k, v in times.items()}


def _repeated(variants, warmup, reps, repeats):
    runs = [_timed(variants, warmup, reps) for _ in range(repeats)]
    out = {}
    for k in variants:
        meds = [r[k] for r in runs]
        out[k] = {"medians": [round(m, 1) for m in meds], "median": round(statistics.median(meds), 1),
                  "spread": round(max(meds) - min(meds), 1)}
    return out


def _verdict(t, base, new):
    """``new`` against ``base``: the difference of the medians, and whether the repeats' ranges are disjoint."""
    gain = t[base]["median"] - t[new]["median"]
    return {"base": base, "new": new, "base - new": round(gain, 1), "new / base": round(t[new]["median"] / t[base]["median"], 3),
            "faster_beyond_spread": bool(max(t[new]["medians"]) < min(t[base]["medians"])),
            "slower_beyond_spread": bool(min(t[new]["medians"]) > max(t[base]["medians"]))}


def _site(site, args):
    import vidtome_amd
    from vidtome_amd import patch as vpatch, sites as S
    dt = torch.float16
    unet = S.SiteUNet([site], seed=0, full=True).to(device="cuda", dtype=dt)
    vidtome_amd.apply_patch(unet, local_merge_ratio=LOCAL, merge_global=True, global_merge_ratio=GLOBAL, batch_size=B,
                            target_stride=4, global_rand=0.5)
    unet.set_size(LATENT)
    blk = unet.blocks[0]
    hs = [S.synthetic_hidden(site, B, F, LATENT, dt, "cuda", seed=1 + j, clip_seed=7, regime="corr01") for j in range(2)]
    cond = (torch.randn(B * F, 77, 768, generator=torch.Generator().manual_seed(6)) * 0.5).to(device="cuda", dtype=dt)
    torch.manual_seed(123)
    blk.generator = vpatch.init_generator(hs[0].device)
    blk(hs[0], encoder_hidden_states=cond)                       # the first chunk of the step stores the anchors
    anchors, state = getattr(blk, "global_tokens", None), blk.generator.get_state()

    def prepare():
        blk.global_tokens = anchors
        blk.generator.set_state(state)

    def flags(cross, mlp):
        def f():
            prepare()
            vidtome_amd.update_patch(unet, merge_crossattn=cross, merge_mlp=mlp)
        return f

    # the plan (and the hidden states in front of attn2) of the second chunk, taken from a flag-on forward
    seen = {}
    orig = vpatch.merged_cross_attention_residual

    def tap(block, h, enc, plan):
        seen.update(h=h, plan=plan)
        return orig(block, h, enc, plan)
    vpatch.merged_cross_attention_residual = tap
    try:
        flags(True, False)()
        out_on = blk(hs[1], encoder_hidden_states=cond).float()
    finally:
        vpatch.merged_cross_attention_residual = orig
    flags(False, False)()
    out_off = blk(hs[1], encoder_hidden_states=cond).float()
    h, plan = seen["h"], seen["plan"]
    assert vpatch.fused_cross_ok(blk.norm2, blk.attn2, h, cond, None, {})
    Ml, L = plan.keep.shape[1], plan.L
    seg = plan.frame_order()[2]
    nothing = lambda: None

    def on_with_order():
        plan._frame_order = None
        return vpatch.merged_cross_attention_residual(blk, h, cond, plan)

    segment = {"off": (nothing, lambda: vpatch.norm_cross_attention_residual(blk.norm2, blk.attn2, h, cond)),
               "on": (nothing, on_with_order),
               "on_order_cached": (plan.frame_order, lambda: vpatch.merged_cross_attention_residual(blk, h, cond, plan))}
    run = lambda: blk(hs[1], encoder_hidden_states=cond)
    block = {"off": (flags(False, False), run), "crossattn": (flags(True, False), run), "mlp": (flags(False, True), run),
             "both": (flags(True, True), run)}
    ts, tb = _repeated(segment, args.warmup, args.reps, args.repeats), _repeated(block, args.warmup, args.reps, args.repeats)
    ts["verdict"] = _verdict(ts, "off", "on")
    tb["verdict crossattn vs off"] = _verdict(tb, "off", "crossattn")
    tb["verdict both vs mlp"] = _verdict(tb, "mlp", "both")
    res = {"rows": {"M_l": Ml, "L": L, "M_l / L": round(Ml / L, 4), "longest segment": int((seg[1:] - seg[:-1]).max()),
                    "N": L // F},
           "rel_l2_on_vs_off": float((out_on - out_off).norm() / out_off.norm()),
           "attn2_segment": ts, "block": tb}
    vidtome_amd.remove_patch(unet)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("--repeats must be at least 3")
    from vidtome_amd import sites as S
    result = {"tool": "merge_crossattn_block", "device": torch.cuda.get_device_name(0), "dtype": "fp16", "reps": args.reps,
              "repeats": args.repeats, "unit": "us", "data": "corr01",
              "batch": f"{B} x {F} frames, {LATENT[0]} x {LATENT[1]} latent, local {LOCAL}, global {GLOBAL}", "sites": {}}
    with torch.no_grad():
        for site in [s for name in SITES for s in S.sd15_sites() if s.name == name]:
            N = (LATENT[0] // site.downsample) ** 2
            result["sites"][f"{site.name} C={site.channels} N={N}"] = _site(site, args)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
