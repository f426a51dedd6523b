"""Which feed-forward body a patched block call runs, against a literal table of the feed-forward's routes (patch.ff_route): one
block forward per route, one of a step that replays both attentions (attention broadcast) and one of an AdaLayerNormZero
stand-in -- batch 2, 4 frames, latent 16 x 16, C = 320, 8 heads, 77 text tokens of width 768 -- with the vidtome_amd._lib
wrappers spied (every spy calls through).  Each forward must launch exactly the tail's wrappers, in order, and give bit for bit
what the named body gives when called directly on the hidden states in front of the feed-forward (the same block with a zero
feed-forward hands those out).  The rows are built by tools/block_digest.py, whose digest of such calls is what
profiles/ff_route_bitwise.txt compares."""
import importlib.util
import os

import pytest
import torch

import standin

pytestmark = pytest.mark.gpu

# case -> (the row of block_digest.FF_CASES, the route, the _lib wrappers of the tail in order)
EXPECTED = {
    "panels": ("fp16 C=320", "panels", ["layernorm_panels", "ff_geglu", "linear_panels"]),
    "f32": ("fp32 fp32_projections", "f32", ["layernorm", "linear_f32", "linear_f32"]),
    "module": ("FF_MODE=blas", "module", ["layernorm", "geglu"]),
    "merged-panels": ("merge_mlp fp16", "merged-panels", ["layernorm_gather", "ff_geglu", "linear_panels", "unmerge_add"]),
    "merged": ("merge_mlp FF_MODE=blas", "merged", ["layernorm_gather", "geglu", "unmerge_add"]),
    "AdaLayerNormZero": ("AdaLayerNormZero", "module", ["layernorm", "geglu"]),
}


@pytest.fixture(scope="module")
def digest():
    spec = importlib.util.spec_from_file_location(
        "block_digest", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "block_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _forward(digest, blk, h, text, monkeypatch):
    """One spied block forward from the block generator's first state: (output, the wrappers from ff_route's call on, the routes
    ff_route answered, the MergePlans of the forward)."""
    from vidtome_amd import _lib
    from vidtome_amd import patch as vpatch
    seen = {"routes": [], "plans": [], "at": None}
    real_route, real_merge = vpatch.ff_route, vpatch.compute_merge

    def ff_route(*a):
        seen["at"] = len(seen["spy"].calls)
        seen["routes"].append(real_route(*a))
        return seen["routes"][-1]

    def compute_merge(*a, **k):
        res = real_merge(*a, **k)
        seen["plans"].append(getattr(res[0], "plan", None))
        return res
    blk.generator = torch.Generator().manual_seed(123)
    with monkeypatch.context() as m:
        m.setattr(vpatch, "ff_route", ff_route)
        m.setattr(vpatch, "compute_merge", compute_merge)
        with torch.no_grad(), digest.Spy(_lib) as spy:
            seen["spy"] = spy
            out = blk(h, encoder_hidden_states=text)
    torch.cuda.synchronize()
    return out, spy.calls[seen["at"]:], seen["routes"], seen["plans"]


def _in_front_of_the_feed_forward(digest, blk, h, text, monkeypatch):
    """The hidden states the feed-forward gets: the same forward with a zero feed-forward (``0 + h``)."""
    ff, blk.ff = blk.ff, standin.Zero()
    try:
        return _forward(digest, blk, h, text, monkeypatch)[0]
    finally:
        blk.ff = ff


def test_the_table_names_every_route(digest):
    assert {route for _, route, _ in EXPECTED.values()} == {"merged-panels", "merged", "panels", "f32", "module"}
    assert {row for row, _, _ in EXPECTED.values()} <= set(digest.FF_CASES)


@pytest.mark.filterwarnings("ignore:vidtome_amd")
@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_block_forward_runs_the_body_its_route_names(digest, case, monkeypatch):
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    row, route, tail = EXPECTED[case]
    unet, blk, h, text, restore = digest.ff_case(vidtome_amd, row)
    try:
        _forward(digest, blk, h, text, monkeypatch)                                   # (packs the weights)
        out, ran, routes, plans = _forward(digest, blk, h, text, monkeypatch)
        assert routes == [route] and ran == tail, (case, routes, ran)
        pre = _in_front_of_the_feed_forward(digest, blk, h, text, monkeypatch)
        norm, ff = blk.norm3, blk.ff
        with torch.no_grad():
            if case == "AdaLayerNormZero":
                # vidtome/patch.py:187-199 written out
                _, _, shift_mlp, scale_mlp, gate_mlp = blk.norm1(h)
                norm_hidden_states = vpatch.layer_norm(norm, pre) * (1 + scale_mlp[:, None]) + shift_mlp[:, None]
                want = gate_mlp.unsqueeze(1) * vpatch.feed_forward(ff, norm_hidden_states) + pre
            elif route in ("merged-panels", "merged"):
                assert len(plans) == 1 and plans[0].keep is not None
                want = vpatch.merged_feed_forward_residual(blk, pre, plans[0], route)
            elif route == "panels":
                want = vpatch.norm_feed_forward_residual(norm, ff, pre)
            elif route == "f32":
                want = vpatch.norm_feed_forward_f32(norm, ff, pre)
            else:
                want = vpatch.module_feed_forward_residual(norm, ff, pre)
        torch.cuda.synchronize()
    finally:
        restore()
    assert out.shape == h.shape and out.dtype == h.dtype and bool(torch.isfinite(out).all())
    assert not torch.equal(out, pre)
    assert torch.equal(out, want), case


@pytest.mark.filterwarnings("ignore:vidtome_amd")
def test_a_step_that_replays_both_attentions_runs_the_fused_tail(digest, monkeypatch):
    """Both modes "reuse" and the route "panels": the whole forward is vtm_residual_replay_layernorm and the two panel GEMMs, and
    gives what ``norm_feed_forward_residual`` gives on h + d1 + d2."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    row, every1, every2 = digest.FF_BROADCAST_CASES["both reuse fp16"]
    unet, blk, h, text, restore = digest.ff_case(vidtome_amd, row)
    try:
        bc = vidtome_amd.AttentionBroadcast([999, 666, 333, 0], digest.FRAMES, attn1_every=every1, attn2_every=every2,
                                            attn1_window=(0, 1000), attn2_window=(0, 1000))
        vidtome_amd.register_attention_broadcast(unet, bc)
        bc.set_step(0)
        out0, ran0, routes0, _ = _forward(digest, blk, h, text, monkeypatch)
        assert bc.modes(0) == ("record", "record") and routes0 == ["panels"]
        # (the block's first forward: the two feed-forward weights are packed ahead of the LayerNorm launch)
        assert ran0 == ["to_panels", "to_panels", "layernorm_panels", "ff_geglu", "linear_panels"], ran0
        bc.set_step(1)
        assert bc.modes(1) == ("reuse", "reuse")
        from vidtome_amd import _lib
        with torch.no_grad(), digest.Spy(_lib) as spy:
            out = blk(h, encoder_hidden_states=text)
        assert spy.calls == ["residual_replay_layernorm", "ff_geglu", "linear_panels"], spy.calls
        # a zero feed-forward is not the GEGLU one: the same step replays both deltas in ONE launch and adds nothing
        ff, blk.ff = blk.ff, standin.Zero()
        try:
            with torch.no_grad(), digest.Spy(_lib) as spy:
                h2 = blk(h, encoder_hidden_states=text)
        finally:
            blk.ff = ff
        assert spy.calls == ["residual_replay", "layernorm"], spy.calls
        with torch.no_grad():
            want = vpatch.norm_feed_forward_residual(blk.norm3, blk.ff, h2)
        torch.cuda.synchronize()
    finally:
        restore()
    assert not torch.equal(h2, h) and bool(torch.isfinite(out).all())
    assert out0.shape == out.shape and torch.equal(out, want)
