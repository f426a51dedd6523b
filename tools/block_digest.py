"""Digest of what vidtome_amd/patch.py launches and computes, for a bit-for-bit A/B of two versions of the host layer on ONE
built library: one line per call -- case name, the ordered vidtome_amd._lib wrappers it went through, sha256 of its output,
sha256 of ``module.global_tokens``.

    VIDTOME_HIP_LIB=<libvidtome_hip.so> python tools/block_digest.py [--package DIR] [--out FILE]

``--package DIR``: the directory that holds the ``vidtome_amd`` package to import (default: this tree).  Two runs on the same
library compare with `diff`: every input is seeded on the CPU, and so is every draw of the block generator.

Cases (fp16 unless named; batch 2, 4 frames, latent 16 x 16, local_merge_ratio 0.5, the self-attention segment of one site):
  route/*      one call per row of the attn1 route table (tests/test_gpu_attn1_route.py), `merge_global=False`
  chunks/*     the rows / panels / f32 / blas routes over four chunks of one clip with `merge_global=True`: the first stores its
               tokens, the second has the local chunk on the src side (the coin threshold `global_rand` is switched per chunk, as
               `smoke()` does), the third on the dst side behind anchors that carry content ids, the fourth is ONE frame.  The
               tool fails unless a local-is-src chunk with compacted queries, a local-is-dst chunk, a folded-key launch
               (d = 40) and a single-frame chunk all occurred, and prints which did
  pnp/*        PnP shared probabilities with `align_batch=True` (live query rows under sharing)
  nolive/*     the rows route with LIVE_QUERIES off
  unmerged/*   sites that do not merge (`max_downsample=1`, 64 tokens): bf16 C = 640, fp32 C = 320 with fp32_projections
  cross/*      `cross_attention`, `norm_cross_attention_residual` and the whole block forward: plain, masked, IP-Adapter,
               IP-Adapter with region masks, and 250 tokens (no multiple of 8), under both FF_MODEs; the whole forward of an fp32
               block with fp32_projections
  cross/* side the block forward behind the public ``register_*`` functions alone, under both FF_MODEs, at 256 and at 10 x 25 =
               250 tokens: maps registered (plain, masked, IP-Adapter), a LocalBlend registered (plain, IP-Adapter),
               cross-attention control at an injecting step (four groups: the source, an identity, an edited one, one without an
               edit) with maps and blend registered, and control outside its schedule with maps, with a blend, with both.  These
               lines carry two more hashes: ``attn2_probs`` and the LocalBlend accumulator
  ff/*         the block's feed-forward tail through the block forward and the public API alone (FF_CASES; the route and the
               tail's wrappers of each row: tests/test_gpu_ff_route.py): every row of ``patch.ff_route``'s table without and with
               ``merge_mlp``, an AdaLayerNormZero stand-in at a site that does not merge, and attention broadcast
               (FF_BROADCAST_CASES: one line per step -- a record step, then the reuse of attn1, of attn2 or of both).  The one
               forward that raises is a line too, its wrappers up to there and the exception's type: an fp16 block with fp32
               feed-forward weights, whose mixed-dtype GEMM torch refuses on the host"""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
B, FRAMES, LATENT = 2, 4, (16, 16)
SPIED = ("layernorm", "layernorm_panels", "gather_rows", "gather_panels", "to_panels", "transpose_cols", "linear_rows",
         "linear_panels", "linear_f32", "attention", "attention_kv", "attention_kv_bias", "attention_kv_sets",
         "attention_kv_sets_masked", "attention_kv_sets_src", "cross_edit_values", "attention_probs", "attention_word_map",
         "compact_queries", "fold_keys", "compose", "anchor_maps", "unmerge_add", "ff_geglu", "geglu", "layernorm_gather",
         "residual_record", "residual_replay", "residual_replay_layernorm")

# name -> (dtype, C, heads, options); the expected route of each row is tests/test_gpu_attn1_route.py's table
ROUTE_CASES = {
    "fp16 C=320 heads 8": (torch.float16, 320, 8, {}),
    "fp16 C=64 heads 8": (torch.float16, 64, 8, {}),
    "bf16 C=320": (torch.bfloat16, 320, 8, {}),
    "fp16 C=640": (torch.float16, 640, 8, {}),
    "fp16 C=640 bias on to_v": (torch.float16, 640, 8, {"v_bias": True}),
    "fp16 C=480 heads 12": (torch.float16, 480, 12, {}),
    "fp16 block, fp32 to_out": (torch.float16, 320, 8, {"f32_out": True}),
    "fp32 C=320": (torch.float32, 320, 8, {}),
    "fp32 C=320 fp32_projections": (torch.float32, 320, 8, {"fp32_projections": True}),
    "PROJ_MODE=rows C=640": (torch.float16, 640, 8, {"proj_mode": "rows"}),
    "PROJ_MODE=panels C=320": (torch.float16, 320, 8, {"proj_mode": "panels"}),
    "PROJ_MODE=blas C=320": (torch.float16, 320, 8, {"proj_mode": "blas"}),
    "un-merged fp16 C=640": (torch.float16, 640, 8, {"unmerged": True}),
    "un-merged fp16 C=320": (torch.float16, 320, 8, {"unmerged": True}),
    "PnP sharing fp16 C=320": (torch.float16, 320, 8, {"pnp": True}),
    "attention_mask given": (torch.float16, 320, 8, {"mask": True}),
}


def sha(t):
    if t is None:
        return "-"
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:24]


class Spy:
    """Records the names of the _lib wrappers that run inside the `with` block, in order; every wrapper calls through."""

    def __init__(self, _lib, names=SPIED):
        self._lib, self.names, self.calls, self.kwargs = _lib, names, [], []

    def __enter__(self):
        self.orig = {n: getattr(self._lib, n) for n in self.names}
        for n, fn in self.orig.items():
            setattr(self._lib, n, self._wrap(n, fn))
        return self

    def _wrap(self, name, fn):
        def spied(*a, **kw):
            self.calls.append(name)
            self.kwargs.append(kw)
            return fn(*a, **kw)
        return spied

    def __exit__(self, *exc):
        for n, fn in self.orig.items():
            setattr(self._lib, n, fn)


def site_block(vidtome_amd, S, dtype, C, heads, unmerged=False, full=False, seed=0, **patch_kw):
    """A patched one-site model and its block: 256 tokens per frame, or 64 at a site that does not merge."""
    site = S.Site("site", 2 if unmerged else 1, C, heads)
    unet = S.SiteUNet([site], seed=seed, full=full).to(device=DEV, dtype=dtype).eval()
    vidtome_amd.apply_patch(unet, local_merge_ratio=0.5, batch_size=B, max_downsample=1 if unmerged else 2, **patch_kw)
    unet.set_size(LATENT)
    blk = unet.blocks[0]
    blk.generator = torch.Generator().manual_seed(123)
    return unet, site, blk


class CountingAttention(torch.nn.Module):
    """attn1's own forward for the "module" route: counts its calls and returns zeros."""
    calls = 0

    def forward(self, x, encoder_hidden_states=None, attention_mask=None, **kw):
        self.calls += 1
        return torch.zeros_like(x)


def route_case(vidtome_amd, name):
    """(model, block, hidden states, attention_mask, restore) of one ROUTE_CASES row; call ``restore()`` afterwards."""
    from vidtome_amd import patch as vpatch, sites as S
    dtype, C, heads, opt = ROUTE_CASES[name]
    unet, site, blk = site_block(vidtome_amd, S, dtype, C, heads, unmerged=opt.get("unmerged", False))
    attn = blk.attn1
    if opt.get("v_bias"):
        g = torch.Generator().manual_seed(9)
        attn.to_v.bias = torch.nn.Parameter(torch.randn(C, generator=g).to(device=DEV, dtype=dtype))
    if opt.get("f32_out"):
        attn.to_out[0].float()
    if opt.get("fp32_projections"):
        vidtome_amd.update_patch(unet, fp32_projections=True)
    if opt.get("pnp"):
        attn.injection_schedule, attn.t, attn.vtm_num_inputs = [981], 981, B
    mask = None
    if opt.get("mask"):
        attn.__class__ = type("Attention", (CountingAttention, type(attn)), {})
        mask = torch.zeros(B * FRAMES, 1, 128, dtype=dtype, device=DEV)
    keep = vpatch.PROJ_MODE, vpatch.FUSED_PROJ
    if "proj_mode" in opt:
        vpatch.PROJ_MODE, vpatch.FUSED_PROJ = opt["proj_mode"], opt["proj_mode"] != "blas"
    h = S.synthetic_hidden(site, B, FRAMES, LATENT, dtype, DEV, seed=50, clip_seed=7)

    def restore():
        vpatch.PROJ_MODE, vpatch.FUSED_PROJ = keep
        vidtome_amd.remove_patch(unet)
    return unet, blk, h, mask, restore


def emit(out, name, spy, y, blk):
    out.append(f"{name} | {' '.join(spy.calls)} | out {sha(y)} | anchors {sha(getattr(blk, 'global_tokens', None))}")


def run_routes(vidtome_amd, out):
    from vidtome_amd import _lib, patch as vpatch
    for name in ROUTE_CASES:
        torch.manual_seed(123)
        unet, blk, h, mask, restore = route_case(vidtome_amd, name)
        try:
            with torch.no_grad(), Spy(_lib) as spy:
                y = vpatch.self_attention_segment(blk, h, None, mask, None)
            emit(out, f"route/{name}", spy, y, blk)
        finally:
            restore()


def run_chunks(vidtome_amd, out, name, dtype, C, seen, fp32_projections=False, proj_mode=None, pnp=False, live=True,
               chunks=((FRAMES, None), (FRAMES, 0.0), (FRAMES, 1.0), (1, 1.0)), **patch_kw):
    """Chunks of one clip through one merging site with a global level; ``chunks``: (frames, coin threshold) per chunk."""
    from vidtome_amd import _lib, patch as vpatch, sites as S
    torch.manual_seed(123)
    unet, site, blk = site_block(vidtome_amd, S, dtype, C, 8, merge_global=True, global_merge_ratio=0.5, **patch_kw)
    if fp32_projections:
        vidtome_amd.update_patch(unet, fp32_projections=True)
    if pnp:
        blk.attn1.injection_schedule, blk.attn1.t, blk.attn1.vtm_num_inputs = [981], 981, B
    keep = vpatch.PROJ_MODE, vpatch.FUSED_PROJ, vpatch.LIVE_QUERIES
    if proj_mode is not None:
        vpatch.PROJ_MODE, vpatch.FUSED_PROJ = proj_mode, proj_mode != "blas"
    vpatch.LIVE_QUERIES = live
    try:
        for ck, (frames, coin) in enumerate(chunks):
            if coin is not None:
                unet._tome_info["args"]["global_rand"] = coin
            h = S.synthetic_hidden(site, B, frames, LATENT, dtype, DEV, seed=50 + ck, clip_seed=7)
            with torch.no_grad(), Spy(_lib) as spy:
                y = vpatch.self_attention_segment(blk, h)
            emit(out, f"{name} chunk {ck}", spy, y, blk)
            if "anchor_maps" in spy.calls:                       # a global level ran
                seen.add("local-is-src, compacted queries" if "compact_queries" in spy.calls else "local-is-dst")
                if frames == 1:
                    seen.add("single-frame chunk")
            if any(n == "attention_kv" and kw.get("k_fold") is not None for n, kw in zip(spy.calls, spy.kwargs)) and C // 8 == 40:
                seen.add("folded-key launch (d = 40)")
    finally:
        vpatch.PROJ_MODE, vpatch.FUSED_PROJ, vpatch.LIVE_QUERIES = keep
        vidtome_amd.remove_patch(unet)


def run_unmerged(vidtome_amd, out):
    from vidtome_amd import _lib, patch as vpatch, sites as S
    for name, dtype, C, f32p in (("bf16 C=640", torch.bfloat16, 640, False), ("fp32 C=320 fp32_projections", torch.float32, 320, True),
                                 ("fp32 C=320", torch.float32, 320, False)):
        torch.manual_seed(123)
        unet, site, blk = site_block(vidtome_amd, S, dtype, C, 8, unmerged=True)
        if f32p:
            vidtome_amd.update_patch(unet, fp32_projections=True)
        h = S.synthetic_hidden(site, B, FRAMES, LATENT, dtype, DEV, seed=50, clip_seed=7)
        with torch.no_grad(), Spy(_lib) as spy:
            y = vpatch.self_attention_segment(blk, h)
        emit(out, f"unmerged/{name}", spy, y, blk)
        vidtome_amd.remove_patch(unet)


def run_cross(vidtome_amd, out):
    """attn2 of a full block (C = 320, 77 text tokens of width 768): the two public bodies and the block forward."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ip_adapter_mask_standin
    import ip_adapter_standin
    from vidtome_amd import _lib, patch as vpatch, sites as S
    dt, C, T = torch.float16, 320, 77
    g = torch.Generator().manual_seed(3)
    text = torch.randn(B * FRAMES, T, 768, generator=g).to(device=DEV, dtype=dt)
    keep_bias = torch.arange(T)[None, :] < torch.tensor([57, 30] * FRAMES)[:, None]
    bias = ((1 - keep_bias.to(dt)) * -10000.0).unsqueeze(1).to(DEV)
    left, top = torch.zeros(1, 1, *LATENT, device=DEV), torch.zeros(1, 1, *LATENT, device=DEV)
    left[..., :LATENT[1] // 2] = 1
    top[:, :, :LATENT[0] // 2] = 1
    keep_ff = vpatch.FF_MODE
    try:
        for ff_mode in ("panels", "blas"):
            vpatch.FF_MODE = ff_mode
            for kind in ("plain", "masked", "ip-adapter", "ip-adapter region masks"):
                torch.manual_seed(123)
                unet, site, blk = site_block(vidtome_amd, S, dt, C, 8, full=True)
                enc, mask, kw = text, None, {}
                if kind == "masked":
                    mask = bias
                elif kind == "ip-adapter":
                    ip_adapter_standin.install(unet, (4, 16), (0.6, 0.3))
                    enc = (text, ip_adapter_standin.image_states((4, 16), B * FRAMES, 768, dt, DEV))
                elif kind == "ip-adapter region masks":
                    ip_adapter_mask_standin.install(unet, (16, 4), (1.0, 0.6))
                    ims = [torch.randn(B * FRAMES, 1, t, 768, generator=g).to(device=DEV, dtype=dt) for t in (16, 4)]
                    enc, kw = (text, ims), {"ip_adapter_masks": [left, top]}
                h = S.synthetic_hidden(site, B, FRAMES, LATENT, dt, DEV, seed=50, clip_seed=7)
                tag = f"cross/FF_MODE={ff_mode} {kind}"
                with torch.no_grad():
                    for n_tok in (h.shape[1], 250):
                        hn = h[:, :n_tok].contiguous()
                        if kind == "ip-adapter region masks" and n_tok == 250:
                            continue                                     # (region masks are given for the whole token grid)
                        with Spy(_lib) as spy:
                            y = vpatch.cross_attention(blk.attn2, vpatch.layer_norm(blk.norm2, hn), enc, mask, **kw)
                        emit(out, f"{tag} cross_attention N={n_tok}", spy, y, blk)
                        if isinstance(enc, tuple) and n_tok == 250:
                            continue                                     # (the panel path of an IP-Adapter call asks N % 8 == 0)
                        with Spy(_lib) as spy:
                            ip = vpatch.ip_cross_call(blk.attn2, hn, enc, mask, kw) if isinstance(enc, tuple) else None
                            y = vpatch.norm_cross_attention_residual(blk.norm2, blk.attn2, hn, None if ip else enc, ip,
                                                                     attention_mask=mask)
                        emit(out, f"{tag} norm_cross_attention_residual N={n_tok}", spy, y, blk)
                    with Spy(_lib) as spy:
                        y = blk(h, encoder_hidden_states=enc, encoder_attention_mask=mask, cross_attention_kwargs=kw or None)
                    emit(out, f"{tag} block forward", spy, y, blk)
                vidtome_amd.remove_patch(unet)
    finally:
        vpatch.FF_MODE = keep_ff


SIDE_CASES = (                      # (name, conditioning, registered, control step: None | "in" | "out", also at 250 tokens)
    ("maps plain", "plain", ("maps",), None, True),
    ("maps masked", "masked", ("maps",), None, True),
    ("maps ip-adapter", "ip-adapter", ("maps",), None, True),
    ("blend plain", "plain", ("blend",), None, True),
    ("blend ip-adapter", "ip-adapter", ("blend",), None, True),
    ("control injecting, maps and blend", "plain", ("maps", "blend"), "in", True),
    ("control outside the schedule, maps", "plain", ("maps",), "out", False),
    ("control outside the schedule, blend", "plain", ("blend",), "out", False),
    ("control outside the schedule, maps and blend", "plain", ("maps", "blend"), "out", False),
)


# attn2 route rows (tests/test_gpu_attn2_route.py holds the expected frame and core of each):
# name -> (conditioning, FF_MODE, latent, dtype, options)
CROSS_ROUTE_CASES = {
    "plain": ("plain", "panels", LATENT, torch.float16, {}),
    "plain N=250": ("plain", "panels", (10, 25), torch.float16, {}),
    "masked": ("masked", "panels", LATENT, torch.float16, {}),
    "ip-adapter": ("ip-adapter", "panels", LATENT, torch.float16, {}),
    "ip-adapter N=250": ("ip-adapter", "panels", (10, 25), torch.float16, {}),
    "ip-adapter region masks": ("ip-adapter region masks", "panels", LATENT, torch.float16, {}),
    "FF_MODE=blas plain": ("plain", "blas", LATENT, torch.float16, {}),
    "FF_MODE=blas plain N=250": ("plain", "blas", (10, 25), torch.float16, {}),
    "FF_MODE=blas masked": ("masked", "blas", LATENT, torch.float16, {}),
    "FF_MODE=blas ip-adapter": ("ip-adapter", "blas", LATENT, torch.float16, {}),
    "fp16 block, fp32 to_out": ("plain", "panels", LATENT, torch.float16, {"f32_out": True}),
    "a bool mask": ("bool mask", "panels", LATENT, torch.float16, {"counting": True}),
    "processor kwargs": ("plain", "panels", LATENT, torch.float16, {"counting": True, "kwargs": {"scale": 1.0}}),
    "fp32 fp32_projections": ("plain", "panels", LATENT, torch.float32, {"fp32_projections": True}),
    "fp32": ("plain", "panels", LATENT, torch.float32, {"counting": True}),
    "control injecting": ("plain", "panels", LATENT, torch.float16, {"control": "in"}),
    "control injecting N=250": ("plain", "panels", (10, 25), torch.float16, {"control": "in"}),
    "FF_MODE=blas control injecting": ("plain", "blas", LATENT, torch.float16, {"control": "in"}),
}


def cross_case(vidtome_amd, kind, latent=LATENT, dt=torch.float16, registered=(), control=None, f32_out=False, counting=False,
               fp32_projections=False, kwargs=None):
    """(model, block, hidden states, conditioning, mask, cross_attention_kwargs, LocalBlend or None) of one full block (C = 320,
    77 text tokens of width 768) at ``latent``: everything is switched on through the public ``register_*`` functions; the
    timestep is stamped as ``pnp.register_time`` stamps it.  ``counting``: attn2's own forward counts its calls and returns
    zeros (the site stand-ins have none)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cross_control_standin
    import ip_adapter_mask_standin
    import ip_adapter_standin
    from vidtome_amd import sites as S
    C, T, n = 320, 77, B * FRAMES
    g = torch.Generator().manual_seed(3)
    text = torch.randn(n, T, 768, generator=g).to(device=DEV, dtype=dt)
    torch.manual_seed(123)
    unet, site, blk = site_block(vidtome_amd, S, dt, C, 8, full=True)
    unet.set_size(latent)
    enc, mask, kw = text, None, dict(kwargs or {})
    if kind == "masked":
        keep = torch.arange(T)[None, :] < torch.tensor([57, 30] * FRAMES)[:, None]
        mask = ((1 - keep.to(dt)) * -10000.0).unsqueeze(1).to(DEV)
    elif kind == "bool mask":
        mask = torch.ones(n, 1, T, dtype=torch.bool, device=DEV)
    elif kind == "ip-adapter":
        ip_adapter_standin.install(unet, (4, 16), (0.6, 0.3))
        enc = (text, ip_adapter_standin.image_states((4, 16), n, 768, dt, DEV))
    elif kind == "ip-adapter region masks":
        ip_adapter_mask_standin.install(unet, (16, 4), (1.0, 0.6))
        left, top = torch.zeros(1, 1, *latent, device=DEV), torch.zeros(1, 1, *latent, device=DEV)
        left[..., :latent[1] // 2] = 1
        top[:, :, :latent[0] // 2] = 1
        enc = (text, [torch.randn(n, 1, t, 768, generator=g).to(device=DEV, dtype=dt) for t in (16, 4)])
        kw["ip_adapter_masks"] = [left, top]
    if f32_out:
        blk.attn2.to_out[0].float()
    if fp32_projections:
        vidtome_amd.update_patch(unet, fp32_projections=True)
    if counting:
        blk.attn2.__class__ = type("Attention", (CountingAttention, type(blk.attn2)), {})
        if kw:                                               # (processor kwargs send attn1 to its own forward too)
            blk.attn1.__class__ = type("Attention", (CountingAttention, type(blk.attn1)), {})
    groups = 4 if control else B
    lb = None
    if "maps" in registered:
        vidtome_amd.register_attention_maps(unet)
    if "blend" in registered:
        w = torch.rand(2, T, generator=g)
        lb = vidtome_amd.LocalBlend({0: w[0], groups // 2: w[1]}, groups, n // groups)
        vidtome_amd.register_local_blend(unet, lb)
    if control:
        swap = cross_control_standin.edit_of(cross_control_standin.specs(T)["replace"])
        edits = {1: vidtome_amd.CrossEdit.identity(T), 2: swap}
        vidtome_amd.register_cross_attention_control(unet, [981], groups, edits)
        blk.attn2.t = 981 if control == "in" else 941
    h = S.synthetic_hidden(site, B, FRAMES, latent, dt, DEV, seed=50, clip_seed=7)
    return unet, blk, h, enc, mask, kw, lb


def run_cross_side(vidtome_amd, out):
    """attn2's side launches and its controlled core, through the block forward alone."""
    from vidtome_amd import _lib, patch as vpatch
    keep_ff = vpatch.FF_MODE
    try:
        for ff_mode in ("panels", "blas"):
            vpatch.FF_MODE = ff_mode
            for name, kind, registered, control, odd in SIDE_CASES:
                for latent in (LATENT, (10, 25)) if odd else (LATENT,):
                    unet, blk, h, enc, mask, kw, lb = cross_case(vidtome_amd, kind, latent, registered=registered,
                                                                 control=control)
                    with torch.no_grad(), Spy(_lib) as spy:
                        y = blk(h, encoder_hidden_states=enc, encoder_attention_mask=mask, cross_attention_kwargs=kw or None)
                    emit(out, f"cross/FF_MODE={ff_mode} {name} block forward N={h.shape[1]}", spy, y, blk)
                    out[-1] += f" | probs {sha(getattr(blk, 'attn2_probs', None))} | blend {sha(None if lb is None else lb._acc)}"
                    vidtome_amd.remove_patch(unet)
    finally:
        vpatch.FF_MODE = keep_ff


def run_f32_blocks(vidtome_amd, out):
    """The whole forward of an fp32 block (C = 320) with the fp32_projections opt-in (without it attn2 is the module's own
    forward, which the site stand-ins do not have)."""
    from vidtome_amd import _lib, sites as S
    text = torch.randn(B * FRAMES, 77, 768, generator=torch.Generator().manual_seed(3)).to(DEV)
    torch.manual_seed(123)
    unet, site, blk = site_block(vidtome_amd, S, torch.float32, 320, 8, full=True)
    vidtome_amd.update_patch(unet, fp32_projections=True)
    h = S.synthetic_hidden(site, B, FRAMES, LATENT, torch.float32, DEV, seed=50, clip_seed=7)
    with torch.no_grad(), Spy(_lib) as spy:
        y = blk(h, encoder_hidden_states=text)
    emit(out, "cross/fp32 C=320 fp32_projections block forward", spy, y, blk)
    vidtome_amd.remove_patch(unet)


# feed-forward rows: name -> (dtype, C, heads, options)
FF_CASES = {
    "fp16 C=320": (torch.float16, 320, 8, {}),
    "bf16 C=640": (torch.bfloat16, 640, 8, {}),
    "fp16 C=160 heads 4": (torch.float16, 160, 4, {}),
    "FF_MODE=blas": (torch.float16, 320, 8, {"ff_mode": "blas"}),
    "fp32": (torch.float32, 320, 8, {"counting": True}),
    "fp32 fp32_projections": (torch.float32, 320, 8, {"fp32_projections": True}),
    "a non-GEGLU ff": (torch.float16, 320, 8, {"plain_ff": True}),
    "a LayerNorm subclass as norm3": (torch.float16, 320, 8, {"other_norm3": True}),
    "fp32 ff weights in an fp16 block": (torch.float16, 320, 8, {"f32_ff": True, "raises": True}),
    # (at a site that does not merge: the gate of attn1 is per frame row, patch.py:165, and so fits un-merged tokens alone)
    "AdaLayerNormZero": (torch.float16, 320, 8, {"ada_zero": True, "unmerged": True}),
    "AdaLayerNormZero merge_mlp": (torch.float16, 320, 8, {"ada_zero": True, "unmerged": True, "merge_mlp": True}),
    "merge_mlp fp16": (torch.float16, 320, 8, {"merge_mlp": True}),
    "merge_mlp FF_MODE=blas": (torch.float16, 320, 8, {"merge_mlp": True, "ff_mode": "blas"}),
    "merge_mlp fp32 fp32_projections": (torch.float32, 320, 8, {"merge_mlp": True, "fp32_projections": True}),
    "merge_mlp single-frame chunk": (torch.float16, 320, 8, {"merge_mlp": True, "frames": 1}),
    "merge_mlp un-merged site": (torch.float16, 320, 8, {"merge_mlp": True, "unmerged": True}),
}
# broadcast rows: name -> (FF_CASES row of the block, attn1_every, attn2_every); steps 0 (record) and 1 (reuse) of each
FF_BROADCAST_CASES = {
    "attn1 reuse": ("fp16 C=320", 2, None),
    "attn2 reuse": ("fp16 C=320", None, 2),
    "both reuse fp16": ("fp16 C=320", 2, 2),
    "both reuse FF_MODE=blas": ("FF_MODE=blas", 2, 2),
    "both reuse fp32 fp32_projections": ("fp32 fp32_projections", 2, 2),
}


class OtherNorm(torch.nn.LayerNorm):
    """Computes a LayerNorm, but is not the class the fused paths read."""


class PlainFF(torch.nn.Module):
    """A feed-forward that is not the GEGLU one."""

    def __init__(self, C):
        super().__init__()
        self.net = torch.nn.ModuleList([torch.nn.Linear(C, C)])

    def forward(self, x):
        return self.net[0](x)


class AdaZeroNorm1(torch.nn.Module):
    """An AdaLayerNormZero norm1: a LayerNorm of its input and four seeded (B F, C) tensors -- gate_msa, shift_mlp, scale_mlp,
    gate_mlp."""

    def __init__(self, n, C, dtype, seed=17):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.parts = [(torch.randn(n, C, generator=g) * 0.25).to(device=DEV, dtype=dtype) for _ in range(4)]

    def forward(self, x, timestep=None, class_labels=None, hidden_dtype=None):
        return (torch.nn.functional.layer_norm(x, x.shape[-1:]), *self.parts)


def ff_case(vidtome_amd, name):
    """(model, block, hidden states, text conditioning, restore) of one FF_CASES row: a full block (77 text tokens of width 768)
    set up through ``apply_patch`` / ``update_patch`` alone; call ``restore()`` afterwards."""
    from vidtome_amd import patch as vpatch, sites as S
    dt, C, heads, opt = FF_CASES[name]
    frames = opt.get("frames", FRAMES)
    text = torch.randn(B * frames, 77, 768, generator=torch.Generator().manual_seed(3)).to(device=DEV, dtype=dt)
    torch.manual_seed(123)
    unet, site, blk = site_block(vidtome_amd, S, dt, C, heads, unmerged=opt.get("unmerged", False), full=True)
    if opt.get("fp32_projections"):
        vidtome_amd.update_patch(unet, fp32_projections=True)
    if opt.get("merge_mlp"):
        vidtome_amd.update_patch(unet, merge_mlp=True)
    if opt.get("counting"):                                  # (attn2 of a plain fp32 block is the module's own forward)
        blk.attn2.__class__ = type("Attention", (CountingAttention, type(blk.attn2)), {})
    if opt.get("plain_ff"):
        blk.ff = PlainFF(C).to(device=DEV, dtype=dt)
    if opt.get("other_norm3"):
        norm3 = OtherNorm(C).to(device=DEV, dtype=dt)
        norm3.load_state_dict(blk.norm3.state_dict())
        blk.norm3 = norm3
    if opt.get("f32_ff"):
        blk.ff.float()
    if opt.get("ada_zero"):
        blk.norm1, blk.use_ada_layer_norm_zero = AdaZeroNorm1(B * frames, C, dt), True
    keep_ff = vpatch.FF_MODE
    vpatch.FF_MODE = opt.get("ff_mode", "panels")
    h = S.synthetic_hidden(site, B, frames, LATENT, dt, DEV, seed=50, clip_seed=7)

    def restore():
        vpatch.FF_MODE = keep_ff
        vidtome_amd.remove_patch(unet)
    return unet, blk, h, text, restore


def run_ff(vidtome_amd, out):
    """The feed-forward tail of every FF_CASES row, and of every FF_BROADCAST_CASES row at its two steps."""
    from vidtome_amd import _lib

    def forward(tag, blk, h, text, raises=False):
        with torch.no_grad(), Spy(_lib) as spy:
            try:
                y = blk(h, encoder_hidden_states=text)
            except RuntimeError as e:                        # (raised on the host: see the docstring)
                if not raises:
                    raise
                out.append(f"{tag} | {' '.join(spy.calls)} | raised {type(e).__name__}")
                return
        if raises:
            raise SystemExit(f"block_digest: {tag} was to raise")
        emit(out, tag, spy, y, blk)

    for name in FF_CASES:
        unet, blk, h, text, restore = ff_case(vidtome_amd, name)
        try:
            forward(f"ff/{name} block forward", blk, h, text, FF_CASES[name][3].get("raises", False))
        finally:
            restore()
    for name, (row, every1, every2) in FF_BROADCAST_CASES.items():
        unet, blk, h, text, restore = ff_case(vidtome_amd, row)
        try:
            bc = vidtome_amd.AttentionBroadcast([999, 666, 333, 0], FRAMES, attn1_every=every1, attn2_every=every2,
                                                attn1_window=(0, 1000), attn2_window=(0, 1000))
            vidtome_amd.register_attention_broadcast(unet, bc)
            for step in (0, 1):
                bc.set_step(step)
                forward(f"ff/broadcast {name} step {step} ({' '.join(bc.modes(step))})", blk, h, text)
        finally:
            restore()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=ROOT, help="directory holding the vidtome_amd package to import")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    assert os.path.dirname(os.path.abspath(vpatch.__file__)) == os.path.join(os.path.abspath(args.package), "vidtome_amd")
    out, seen = [], set()
    run_routes(vidtome_amd, out)
    f16, f32 = torch.float16, torch.float32
    run_chunks(vidtome_amd, out, "chunks/rows fp16 C=320", f16, 320, seen)
    run_chunks(vidtome_amd, out, "chunks/panels fp16 C=640", f16, 640, seen)
    run_chunks(vidtome_amd, out, "chunks/f32 C=320 fp32_projections", f32, 320, seen, fp32_projections=True)
    run_chunks(vidtome_amd, out, "chunks/blas fp32 C=320", f32, 320, seen)
    run_chunks(vidtome_amd, out, "chunks/blas fp16 C=320 PROJ_MODE=blas", f16, 320, seen, proj_mode="blas")
    want = {"local-is-src, compacted queries", "local-is-dst", "folded-key launch (d = 40)", "single-frame chunk"}
    three = ((FRAMES, None), (FRAMES, 0.0), (FRAMES, 1.0))
    run_chunks(vidtome_amd, out, "pnp/aligned rows fp16 C=320", f16, 320, set(), pnp=True, chunks=three, align_batch=True)
    run_chunks(vidtome_amd, out, "pnp/aligned panels fp16 C=640", f16, 640, set(), pnp=True, chunks=three, align_batch=True)
    run_chunks(vidtome_amd, out, "pnp/unaligned rows fp16 C=320", f16, 320, set(), pnp=True, chunks=three)
    run_chunks(vidtome_amd, out, "nolive/rows fp16 C=320", f16, 320, set(), live=False, chunks=three)
    run_unmerged(vidtome_amd, out)
    run_cross(vidtome_amd, out)
    run_f32_blocks(vidtome_amd, out)
    run_cross_side(vidtome_amd, out)
    run_ff(vidtome_amd, out)
    torch.cuda.synchronize()
    out.append("occurred in chunks/*: " + "; ".join(sorted(seen)))
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    if seen != want:
        raise SystemExit(f"block_digest: did not occur: {sorted(want - seen)}")


if __name__ == "__main__":
    main()
