#!/usr/bin/env python3
"""What LoRA adapters cost on the patched blocks: one JSON line.

    python tools/lora_block.py [--reps 10] [--warmup 3]

cfg-2 (SD-1.5, the 16 transformer-block sites as whole blocks, batch 2, 16 frames at 512 x 512, local merge 0.5 + global
merge 0.5, steady-state passes of sites.ClipStream) with rank-64 PEFT-style adapters on all eight projections of every
block (the stand-ins of tests/lora_standin.py), timed with device events in one process, the variants in alternating
order per repetition:
  * unadapted: the plain model on the fused path;
  * lora_fused: the adapted model (folded weights, vidtome_amd/lora.py);
  * lora_module: the adapted model on the module path, i.e. what LoRA users got before folding (the recogniser forced to
    refuse the LoRA layers; attention modules compute with torch SDPA);
and the same three for the cfg-3 top site (batch 3 [source | uncond | cond], align_batch, PnP shared probabilities), whose
module path is the reference's sa_forward arithmetic (materialised probabilities of the source sample, repeated per group).
A variant that runs out of device memory is reported as such.  Also: the fold time of every adapted projection of the
cfg-2 model at r = 4 / 64 / 128, and whether the fused LoRA outputs equal the folded twin's bit for bit.
"""
import argparse
import contextlib
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import vidtome_amd  # noqa: E402
from vidtome_amd import _lib, lora, sites  # noqa: E402
from lora_standin import SDPAAttention, folded_twin, wrap_lora  # noqa: E402

DEV = torch.device("cuda:0")


class PnPModuleAttention(SDPAAttention):
    """The reference's PnP self-attention forward (utils/pnp_utils.py:47-95) at an injection step: q / k of the source
    sample, the probabilities materialised and repeated for every group; otherwise SDPA."""

    def forward(self, x, encoder_hidden_states=None, attention_mask=None, **kw):
        n = getattr(self, "vtm_num_inputs", None)
        if encoder_hidden_states is not None or n is None or getattr(self, "t", None) not in getattr(self, "injection_schedule", ()):
            return super().forward(x, encoder_hidden_states, attention_mask, **kw)
        Bx, N, C = x.shape
        h, d = self.heads, C // self.heads
        hb = lambda t: t.view(t.shape[0], N, h, d).transpose(1, 2).reshape(t.shape[0] * h, N, d)
        src = Bx // n
        q, k, v = hb(self.to_q(x)[:src]), hb(self.to_k(x)[:src]), hb(self.to_v(x))
        attn = (torch.einsum("b i d, b j d -> b i j", q, k) * self.scale).softmax(dim=-1).repeat(n, 1, 1)
        o = torch.einsum("b i j, b j d -> b i d", attn, v).view(Bx, h, N, d).transpose(1, 2).reshape(Bx, N, C)
        return self.to_out[1](self.to_out[0](o))


def build(sl, full, pnp_B=0, seed=0):
    unet = sites.SiteUNet(sl, seed=seed, full=full).to(device=DEV, dtype=torch.float16)
    for blk in unet.blocks:
        blk.attn1 = PnPModuleAttention(blk.attn1)
        if full:
            blk.attn2 = SDPAAttention(blk.attn2)
        if pnp_B:
            blk.attn1.injection_schedule, blk.attn1.t, blk.attn1.vtm_num_inputs = [981], 981, pnp_B
    return unet


def patch(unet, B, latent, align):
    vidtome_amd.apply_patch(unet, local_merge_ratio=0.5, merge_global=True, global_merge_ratio=0.5, batch_size=B,
                            align_batch=align)
    unet.set_size(latent)
    return unet


_RECOGNISE = lora.recognise


@contextlib.contextmanager
def module_path(on=True):
    """The recogniser refuses LoRA layers: the patched block runs the modules' own forwards for them."""
    if on:
        lora.recognise = lambda m: "plain" if _RECOGNISE(m) == lora.PLAIN else None
    try:
        yield
    finally:
        lora.recognise = _RECOGNISE


def time_variants(variants, reps, warmup):
    """variants: {name: (ClipStream, module_path)} -> {name: {"ms": median, "spread_ms": [min, max]} or {"oom": ...}}."""
    res = {n: [] for n in variants}
    dead = {}
    counter = {n: 0 for n in variants}

    def one(name):
        stream, on = variants[name]
        with module_path(on):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            stream.step(counter[name])
            e.record()
            torch.cuda.synchronize()
            counter[name] += 1
            return s.elapsed_time(e)

    names = list(variants)
    for rep in range(warmup + reps):
        order = names if rep % 2 == 0 else names[::-1]
        for n in order:
            if n in dead:
                continue
            try:
                t = one(n)
            except torch.cuda.OutOfMemoryError as exc:
                dead[n] = str(exc).split("\n")[0][:200]
                torch.cuda.empty_cache()
                continue
            if rep >= warmup:
                res[n].append(t)
    out = {}
    for n in names:
        if n in dead:
            out[n] = {"oom": dead[n]}
        else:
            out[n] = {"ms": round(statistics.median(res[n]), 3), "spread_ms": [round(min(res[n]), 3), round(max(res[n]), 3)],
                      "reps": len(res[n])}
    return out


def stream_for(unet, sl, B, F, latent, full):
    torch.manual_seed(123)
    cond = torch.randn(B * F, 77, 768, generator=torch.Generator().manual_seed(3)).to(DEV, torch.float16) if full else None
    return sites.ClipStream(unet, sl, B, F, latent, torch.float16, DEV, n_sets=3, chunks_per_step=8, cond=cond,
                            regime="corr01")


def workload(sl, B, F, latent, full, align, pnp, reps, warmup):
    base = patch(build(sl, full, B if pnp else 0), B, latent, align)
    lo = build(sl, full, B if pnp else 0)
    wrap_lora(lo, ranks=(64,), seed=1)
    lo_mod = copy.deepcopy(lo)
    patch(lo, B, latent, align)
    patch(lo_mod, B, latent, align)
    variants = {}
    for name, unet, on in (("unadapted", base, False), ("lora_fused", lo, False), ("lora_module", lo_mod, True)):
        st = stream_for(unet, sl, B, F, latent, full)
        try:
            with module_path(on):
                st.populate()
        except torch.cuda.OutOfMemoryError as exc:
            variants[name] = None
            print(f"{name}: populate ran out of memory: {str(exc).splitlines()[0]}", file=sys.stderr)
            torch.cuda.empty_cache()
            continue
        variants[name] = (st, on)
    oom = {n: {"oom": "while populating the anchors"} for n, v in variants.items() if v is None}
    res = time_variants({n: v for n, v in variants.items() if v is not None}, reps, warmup)
    res.update(oom)
    for u in (base, lo, lo_mod):
        vidtome_amd.remove_patch(u)
    return res


def twin_check(sl, B, F, latent):
    """Fused LoRA outputs vs the plain model holding vtm_lora_fold's outputs: two steady passes, bit for bit."""
    lo = build(sl, True)
    wrap_lora(lo, ranks=(64,), seed=1)
    twin = folded_twin(lo)
    outs = []
    for unet in (lo, twin):
        patch(unet, B, latent, False)
        st = stream_for(unet, sl, B, F, latent, True)
        st.populate()
        outs.append([[o.clone() for o in st.step(c)] for c in range(2)])
        vidtome_amd.remove_patch(unet)
    return all(torch.equal(a, b) for pa, pb in zip(*outs) for a, b in zip(pa, pb))


def fold_times(sl, ranks=(4, 64, 128), reps=5):
    """Device time of folding every adapted projection of the cfg-2 model (one vtm_lora_fold each) at rank r."""
    unet = build(sl, True)
    projs = [m for m in unet.modules() if type(m) is torch.nn.Linear and m.weight.dim() == 2]
    out = {}
    g = torch.Generator().manual_seed(0)
    for r in ranks:
        ops = []
        for m in projs:
            co, ci = m.weight.shape
            ops.append((m.weight.detach(), (torch.randn(co, r, generator=g) * 0.01).to(DEV),
                        (torch.randn(r, ci, generator=g) * ci ** -0.5).to(DEV)))
        for w, up, down in ops:                       # warm-up
            _lib.lora_fold(w, up, down)
        times = []
        for _ in range(reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for w, up, down in ops:
                _lib.lora_fold(w, up, down)
            e.record()
            torch.cuda.synchronize()
            times.append(s.elapsed_time(e))
        out[f"r{r}"] = {"ms_all_projections": round(statistics.median(times), 3), "projections": len(ops),
                        "spread_ms": [round(min(times), 3), round(max(times), 3)]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/lora_block.py needs a GPU"
    sl = sites.sd15_sites()
    res = {"what": "ms per pass (device events, median of --reps after --warmup, variants alternating); cfg2 = 16 SD-1.5 "
                   "whole-block sites, B = 2, 16 frames 512x512; cfg3_top = up3.0 under PnP, B = 3, align_batch; rank-64 "
                   "adapters on all eight projections of every block"}
    res["cfg2"] = workload(sl, 2, 16, (64, 64), True, False, False, a.reps, a.warmup)
    top = [s for s in sl if s.name == "up3.0"]
    res["cfg3_top"] = workload(top, 3, 16, (64, 64), False, True, True, a.reps, a.warmup)
    res["fold"] = fold_times(sl)
    res["fused_equals_folded_twin"] = twin_check(sl, 2, 16, (64, 64))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
