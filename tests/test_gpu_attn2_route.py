"""Which attn2 frame and core a patched block call runs, against a literal table of attn2's routes (patch.attn2_route): one
block forward per row -- batch 2, 4 frames, latent 16 x 16 (256 tokens per frame) or 10 x 25 (250: no multiple of 8), C = 320,
8 heads, 77 text tokens of width 768 -- with the vidtome_amd._lib wrappers spied (every spy calls through).  The rows are
built by tools/block_digest.py, whose digest of such calls is what profiles/attn2_route_bitwise.txt compares.  (AdaLayerNorm
rows: tests/test_attn2_route_host.py -- the site stand-ins have no AdaLayerNorm.)"""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

CORES = {"attention_kv", "attention_kv_bias", "attention_kv_sets", "attention_kv_sets_masked", "attention_kv_sets_src",
         "cross_edit_values"}
CONTROLLED = {"attention_kv", "cross_edit_values", "attention_kv_sets_src"}
# case -> (frame, the core wrappers that ran in attn2)
EXPECTED = {
    "plain": ("panels", {"attention_kv"}),
    "plain N=250": ("panels", {"attention_kv"}),
    "masked": ("panels", {"attention_kv_bias"}),
    "ip-adapter": ("panels", {"attention_kv_sets"}),
    "ip-adapter N=250": ("blas", {"attention_kv_sets"}),                    # the panels frame asks N % 8 == 0 of this call
    "ip-adapter region masks": ("panels", {"attention_kv_sets_masked"}),
    "FF_MODE=blas plain": ("blas", {"attention_kv"}),
    "FF_MODE=blas plain N=250": ("blas", {"attention_kv"}),
    "FF_MODE=blas masked": ("blas", {"attention_kv_bias"}),
    "FF_MODE=blas ip-adapter": ("blas", {"attention_kv_sets"}),
    "fp16 block, fp32 to_out": ("blas", {"attention_kv"}),
    "a bool mask": ("module", set()),
    "processor kwargs": ("module", set()),
    "fp32 fp32_projections": ("f32", {"attention_kv"}),
    "fp32": ("module", set()),
    "control injecting": ("panels", CONTROLLED),
    "control injecting N=250": ("panels", CONTROLLED),
    "FF_MODE=blas control injecting": ("blas", CONTROLLED),
}
# what attn2's frame launched besides its core: (wrappers that must have run there, wrappers that must not have)
FRAME = {
    "panels": ({"layernorm_panels", "linear_panels", "to_panels"}, {"layernorm", "linear_f32"}),
    "f32": ({"layernorm", "linear_f32"}, {"layernorm_panels", "linear_panels"}),
    "blas": ({"layernorm"}, {"layernorm_panels", "linear_panels", "linear_f32"}),
    "module": ({"layernorm"}, {"layernorm_panels", "linear_panels", "linear_f32"}),
}


@pytest.fixture(scope="module")
def digest():
    spec = importlib.util.spec_from_file_location(
        "block_digest", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "block_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_table_names_every_case(digest):
    assert set(EXPECTED) == set(digest.CROSS_ROUTE_CASES)
    assert {frame for frame, _ in EXPECTED.values()} == set(FRAME)


@pytest.mark.filterwarnings("ignore:vidtome_amd")
@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_block_call_takes_its_route(digest, case, monkeypatch):
    import vidtome_amd
    from vidtome_amd import _lib
    from vidtome_amd import patch as vpatch
    monkeypatch.setattr(vpatch, "_warned", set())
    frame, cores = EXPECTED[case]
    kind, ff_mode, latent, dt, opt = digest.CROSS_ROUTE_CASES[case]
    monkeypatch.setattr(vpatch, "FF_MODE", ff_mode)
    unet, blk, h, enc, mask, kw, _ = digest.cross_case(vidtome_amd, kind, latent, dt, **opt)
    spied = {"segment": [], "at": None}
    real_segment = vpatch.self_attention_segment

    def self_attention_segment(*a, **k):
        y = real_segment(*a, **k)
        spied["at"] = len(spied["spy"].calls)               # attn2's launches start here ...
        return y
    monkeypatch.setattr(vpatch, "self_attention_segment", self_attention_segment)
    try:
        control = vpatch.cross_control(blk)
        assert (control is not None) == ("control" in opt)
        with torch.no_grad(), digest.Spy(_lib) as spy:
            spied["spy"] = spy
            out = blk(h, encoder_hidden_states=enc, encoder_attention_mask=mask, cross_attention_kwargs=kw or None)
        torch.cuda.synchronize()
    finally:
        vidtome_amd.remove_patch(unet)
    # ... and end where the feed-forward's begin: its first launch is the last layernorm_panels (FF_MODE "panels": the fused
    # feed-forward), else the last layernorm
    ff_norm = "layernorm_panels" if ff_mode == "panels" and dt != torch.float32 else "layernorm"
    end = len(spy.calls) - 1 - spy.calls[::-1].index(ff_norm)
    attn2 = spy.calls[spied["at"]:end]
    ran = set(attn2)
    must, must_not = FRAME[frame]
    assert ran & CORES == cores, (case, attn2)
    assert must <= ran and not (must_not & ran), (case, frame, attn2)
    assert getattr(blk.attn2, "calls", 0) == (1 if frame == "module" else 0)          # attn2's own forward
    assert out.shape == h.shape and out.dtype == h.dtype and bool(torch.isfinite(out).all())
