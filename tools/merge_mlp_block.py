"""merge_mlp (update_patch(model, merge_mlp=True): the feed-forward on the merged local tokens) at the cfg-2 top site (C = 320)
and the C = 640 site, fp16, the bench's batch (2 x 16 frames of a 64 x 64 latent), its ratios (local 0.5, global 0.5) and
corr01 tokens: one JSON line.

    python tools/merge_mlp_block.py [--reps 20] [--repeats 3] [--out profiles/merge_mlp_block.json]

Per site, event-timed in ONE process on the same inputs, flag off and flag on alternating repetition by repetition so they
share the clock, warmed, and the whole alternating measurement repeated ``--repeats`` times (>= 3):
  ff_segment   flag off: norm_feed_forward_residual (vtm_layernorm_panels -> vtm_ff_geglu -> vtm_linear_panels + residual)
               over all L rows -- the parent's path; flag on: merged_feed_forward_residual (vtm_layernorm_gather -> vtm_ff_geglu
               -> vtm_linear_panels -> vtm_unmerge_add) over M_l rows, on the plan of the block's own compute_merge
  block        the whole patched block forward (attn1 segment, attn2 over 77 x 768 conditioning, feed-forward), the second
               chunk of a step: the anchors the first chunk stored and the generator's state are put back before each call,
               outside the timed region
Reported per variant: the median of every repeat, the median of those, and ``spread`` = max - min of the repeats' medians --
the run-to-run spread a difference has to exceed.  ``rows`` is M_l / L of the run, ``rel_l2_on_vs_off`` the relative L2
difference of the block output between flag on and flag off -- information only: the flag changes results by design."""
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


def _verdict(t):
    """on is faster than off by more than the spread either shows."""
    gain = t["off"]["median"] - t["on"]["median"]
    t["off - on"] = round(gain, 1)
    t["on / off"] = round(t["on"]["median"] / t["off"]["median"], 3)
    t["faster_beyond_spread"] = bool(gain > max(t["off"]["spread"], t["on"]["spread"])
                                     and max(t["on"]["medians"]) < min(t["off"]["medians"]))
    return t


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

    def flag(on):
        def f():
            prepare()
            vidtome_amd.update_patch(unet, merge_mlp=on)
        return f

    # the plan (and the hidden states in front of the feed-forward) of the second chunk, taken from a flag-on forward
    seen = {}
    orig = vpatch.merged_feed_forward_residual

    def tap(block, h, plan, route):
        seen.update(h=h, plan=plan, route=route)
        return orig(block, h, plan, route)
    vpatch.merged_feed_forward_residual = tap
    try:
        flag(True)()
        out_on = blk(hs[1], encoder_hidden_states=cond).float()
    finally:
        vpatch.merged_feed_forward_residual = orig
    flag(False)()
    out_off = blk(hs[1], encoder_hidden_states=cond).float()
    h, plan = seen["h"], seen["plan"]
    assert seen["route"] == "merged-panels" and vpatch.fused_ff_ok(blk.norm3, blk.ff, h)
    Ml, L = plan.keep.shape[1], plan.L
    nothing = lambda: None
    segment = {"off": (nothing, lambda: vpatch.norm_feed_forward_residual(blk.norm3, blk.ff, h)),
               "on": (nothing, lambda: vpatch.merged_feed_forward_residual(blk, h, plan, "merged-panels"))}
    block = {"off": (flag(False), lambda: blk(hs[1], encoder_hidden_states=cond)),
             "on": (flag(True), lambda: blk(hs[1], encoder_hidden_states=cond))}
    res = {"rows": {"M_l": Ml, "L": L, "M_l / L": round(Ml / L, 4)},
           "rel_l2_on_vs_off": float((out_on - out_off).norm() / out_off.norm()),
           "ff_segment": _verdict(_repeated(segment, args.warmup, args.reps, args.repeats)),
           "block": _verdict(_repeated(block, args.warmup, args.reps, args.repeats))}
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
    result = {"tool": "merge_mlp_block", "device": torch.cuda.get_device_name(0), "dtype": "fp16", "reps": args.reps,
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
