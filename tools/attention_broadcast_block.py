"""Attention broadcast (vidtome_amd.AttentionBroadcast) at the cfg-2 top site (C = 320, 4096 tokens) and the C = 640 site, fp16,
the bench's batch (2 x 16 frames of a 64 x 64 latent), its ratios (local 0.5, global 0.5) and corr01 tokens -- the shapes of
tools/merge_mlp_block.py: one JSON line.

    python tools/attention_broadcast_block.py [--reps 30] [--out profiles/attention_broadcast_block.json]

Per site the whole patched block forward (attn1 segment, attn2 over 77 x 768 conditioning, feed-forward), event-timed in ONE
process on the same inputs, the second chunk of a step (the anchors the first chunk stored and the generator's state are put
back before each call, outside the timed region), four variants interleaved repetition by repetition so they share the clock:
  unregistered    the block as the parent commit runs it: the baseline, not the code under test
  record/record   both segments computed, one vtm_residual_record launch behind each
  compute/reuse   attn1 computed, attn2 replaced by one vtm_residual_replay launch
  reuse/reuse     vtm_residual_replay_layernorm -> vtm_ff_geglu -> vtm_linear_panels
Reported per variant: median, min and max of the repetitions, in us.  ``differs`` says for each variant whether its range
is disjoint from the unregistered block's: a pair whose ranges overlap is not claimed either way."""
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
# a 4-step schedule whose every step lies in the window: with every = 2, step 0 records and step 1 reuses
TIMESTEPS, WIDE = [750, 500, 250, 0], (-1, 1000)
VARIANTS = {"record/record": (dict(attn1_every=2, attn2_every=2), 0), "compute/reuse": (dict(attn1_every=None, attn2_every=2), 1),
            "reuse/reuse": (dict(attn1_every=2, attn2_every=2), 1)}


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

    def prepare(marker, step):
        def f():
            blk.global_tokens = anchors
            blk.generator.set_state(state)
            if marker is None:
                blk.__dict__.pop("vtm_broadcast", None)
            else:
                blk.__dict__["vtm_broadcast"] = marker
                marker[0].set_step(step)
        return f

    run = lambda: blk(hs[1], encoder_hidden_states=cond)
    variants = {"unregistered": (prepare(None, None), run)}
    want = {}
    for name, (kw, step) in VARIANTS.items():
        bc = vidtome_amd.AttentionBroadcast(TIMESTEPS, F, attn1_window=WIDE, attn2_window=WIDE, **kw)
        vidtome_amd.register_attention_broadcast(unet, bc)
        marker = blk.__dict__["vtm_broadcast"]
        want[name] = tuple(name.split("/"))
        assert bc.modes(step) == want[name], (name, bc.modes(step))
        prepare(marker, 0)()
        run()                                                    # step 0 fills the caches a reuse at step 1 reads
        variants[name] = (prepare(marker, step), run)
    times = {k: [] for k in variants}
    for rep in range(args.warmup + args.reps):
        for name, (prep, fn) in variants.items():
            prep()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    res = {k: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
           for k, v in times.items()}
    base = res["unregistered"]
    res["differs"] = {k: bool(v["max"] < base["min"] or v["min"] > base["max"]) for k, v in res.items() if k != "unregistered"}
    res["minus_unregistered"] = {k: round(res[k]["median"] - base["median"], 1) for k in VARIANTS}
    res["cache_bytes_per_kind"] = B * F * hs[1].shape[1] * hs[1].shape[2] * 2
    vidtome_amd.remove_patch(unet)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vidtome_amd import sites as S
    result = {"tool": "attention_broadcast_block", "device": torch.cuda.get_device_name(0), "dtype": "fp16", "reps": args.reps,
              "unit": "us", "data": "corr01", "interleaved": True,
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
