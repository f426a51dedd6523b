"""CPU tests of the feed-forward's route (``patch.ff_route``) and its one dispatch (``patch.feed_forward_segment``): every cell of
the route table on stand-in blocks (no GPU: the tokens only pretend to be on one), that the route launches nothing, that a
block forward evaluates ``fused_ff_ok`` at most once, and where the AdaLayerNormZero modulation goes."""
import inspect

import pytest
import torch

import standin
from test_masked_cross_host import FakeCuda
from test_merge_mlp_host import OtherNorm, PlainFF, _plan

HEADS, B, F, N = 2, 2, 4, 16
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32

# configuration -> (dtype, C, the route with the flag off, with the flag on and a plan, with the flag on and no local map).
# Read off the table in ff_route's docstring: the merged routes ask for the flag, a local map and no AdaLayerNormZero;
# "merged-panels" / "panels" ask for fused_ff_ok (16-bit tokens, FF_MODE "panels", the GEGLU feed-forward with weights of the
# tokens' dtype, a plain LayerNorm, C and D multiples of 64); "f32" asks for fp32 tokens and the fp32_projections opt-in.
CONFIGS = {
    "fp16": (F16, 64, "panels", "merged-panels", "panels"),
    "bf16": (BF16, 64, "panels", "merged-panels", "panels"),
    "fp32": (F32, 64, "module", "merged", "module"),
    "fp32 + fp32_projections": (F32, 64, "f32", "merged", "f32"),
    "FF_MODE = blas": (F16, 64, "module", "merged", "module"),
    "non-GEGLU ff": (F16, 64, "module", "merged", "module"),
    "non-plain norm3": (F16, 64, "module", "merged", "module"),
    "fp32 ff weights in an fp16 block": (F16, 64, "module", "merged", "module"),
    "C % 64 != 0": (F16, 96, "module", "merged", "module"),
    "AdaLayerNormZero": (F16, 64, "module", "module", "module"),
    "AdaLayerNorm": (F16, 64, "panels", "merged-panels", "panels"),
}
FLAGS = ("flag off", "flag on with a plan", "flag on without a local map")


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


class AdaZeroNorm1(torch.nn.Module):
    """An AdaLayerNormZero norm1: hands back its input and the four modulation tensors it was made with."""

    def __init__(self, parts):
        super().__init__()
        self.parts = parts

    def forward(self, hs, timestep, class_labels, hidden_dtype=None):
        return (hs, *self.parts)


def _patched(dtype=F16, C=64):
    import vidtome_amd
    unet = standin.StandInUNet(C, HEADS, full=True, cond_dim=32).to(dtype)
    vidtome_amd.apply_patch(unet, batch_size=B)
    return unet, list(unet.blocks())[-1]


def _tokens(dtype=F16, C=64):
    return torch.zeros(B * F, N, C, dtype=dtype).as_subclass(FakeCuda)


def _configured(what, monkeypatch):
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    dtype, C = CONFIGS[what][:2]
    unet, blk = _patched(dtype, C)
    if what == "fp32 + fp32_projections":
        vidtome_amd.update_patch(unet, fp32_projections=True)
    elif what == "FF_MODE = blas":
        monkeypatch.setattr(vpatch, "FF_MODE", "blas")
    elif what == "non-GEGLU ff":
        blk.ff = PlainFF(C).to(dtype)
    elif what == "non-plain norm3":
        blk.norm3 = OtherNorm(C).to(dtype)
    elif what == "fp32 ff weights in an fp16 block":
        blk.ff.float()
    elif what == "AdaLayerNormZero":
        blk.use_ada_layer_norm_zero = True
    elif what == "AdaLayerNorm":
        blk.use_ada_layer_norm = True
    return unet, blk, _tokens(dtype, C)


@pytest.mark.parametrize("flag", FLAGS)
@pytest.mark.parametrize("what", sorted(CONFIGS))
def test_every_cell_of_the_table(built, monkeypatch, what, flag):
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    unet, blk, x = _configured(what, monkeypatch)
    if flag != "flag off":
        vidtome_amd.update_patch(unet, merge_mlp=True)
    plan = _plan(local=flag != "flag on without a local map")
    assert vpatch.ff_route(blk, x, plan) == CONFIGS[what][2 + FLAGS.index(flag)]
    if flag != "flag on with a plan":                        # a site that does not merge hands no plan at all: the same answer
        assert vpatch.ff_route(blk, x, None) == CONFIGS[what][2 + FLAGS.index(flag)]


def test_the_predicates_answer_what_the_table_reads(built, monkeypatch):
    """The two predicates on the configurations above, after their shape chain moved into one helper."""
    from vidtome_amd import patch as vpatch
    for what, (dtype, C, off, on, _) in CONFIGS.items():
        with monkeypatch.context() as m:
            unet, blk, x = _configured(what, m)
            assert vpatch.fused_ff_ok(blk.norm3, blk.ff, x) == (what in ("fp16", "bf16", "AdaLayerNorm", "AdaLayerNormZero")), what
            assert vpatch.f32_ff_ok(blk, blk.norm3, blk.ff, x) == (what == "fp32 + fp32_projections"), what
            assert not vpatch.fused_ff_ok(blk.norm3, blk.ff, torch.zeros(B * F, N, C, dtype=dtype)), what     # not on a GPU


def test_route_launches_nothing(built, monkeypatch):
    """Every function of the library's Python layer is replaced by one that fails: each route is still answered."""
    import vidtome_amd
    from vidtome_amd import _lib, patch as vpatch

    def boom(*a, **k):
        raise AssertionError("ff_route called into the library")
    wrappers = [n for n, f in vars(_lib).items() if inspect.isfunction(f) and f.__module__ == _lib.__name__]
    assert {"layernorm", "layernorm_panels", "layernorm_gather", "ff_geglu", "linear_panels", "linear_f32", "geglu", "to_panels",
            "gather_rows", "unmerge_add", "residual_replay_layernorm"} <= set(wrappers)
    seen = set()
    for what in ("fp16", "fp32", "fp32 + fp32_projections", "AdaLayerNormZero"):
        with monkeypatch.context() as m:
            unet, blk, x = _configured(what, m)
            vidtome_amd.update_patch(unet, merge_mlp=True)
            for name in wrappers:
                m.setattr(_lib, name, boom)
            seen |= {vpatch.ff_route(blk, x, _plan()), vpatch.ff_route(blk, x, None)}
    assert seen == {"merged-panels", "merged", "panels", "f32", "module"}


# ---------------------------------------------------------------------------------------------------
# the block forward: fused_ff_ok at most once
# ---------------------------------------------------------------------------------------------------
def _count_fused_ff_ok(monkeypatch, vpatch):
    calls = []
    real = vpatch.fused_ff_ok
    monkeypatch.setattr(vpatch, "fused_ff_ok", lambda *a: calls.append(1) or real(*a))
    return calls


def _stub_segments(monkeypatch, vpatch, seen):
    def segment(block, hs, *a, **kw):
        if "plan_to" in kw:
            kw["plan_to"].append(_plan())
        return hs

    def merged(block, hs, plan, route):
        seen.append(route)
        return hs + 1

    monkeypatch.setattr(vpatch, "self_attention_segment", segment)
    monkeypatch.setattr(vpatch, "cross_attention_segment", lambda block, hs, *a: hs)
    monkeypatch.setattr(vpatch, "merged_feed_forward_residual", merged)
    monkeypatch.setattr(vpatch, "norm_feed_forward_residual", lambda norm, ff, hs: seen.append("panels") or hs + 2)
    monkeypatch.setattr(vpatch, "module_feed_forward_residual", lambda norm, ff, hs, ada=None: seen.append("module") or hs + 4)


def test_fused_ff_ok_runs_at_most_once_per_forward(built, monkeypatch):
    import vidtome_amd
    from vidtome_amd import AttentionBroadcast, patch as vpatch
    unet, blk = _patched()
    x, seen = _tokens(), []
    _stub_segments(monkeypatch, vpatch, seen)
    calls = _count_fused_ff_ok(monkeypatch, vpatch)
    # a plain forward
    assert torch.equal(blk(x), x + 2) and seen == ["panels"] and len(calls) == 1
    # a merge_mlp forward
    vidtome_amd.update_patch(unet, merge_mlp=True)
    del seen[:], calls[:]
    assert torch.equal(blk(x), x + 1) and seen == ["merged-panels"] and len(calls) == 1
    vidtome_amd.update_patch(unet, merge_mlp=False)
    # a step that replays both attentions: the fused tail, and (FF_MODE = blas) the one replay launch + the module body
    bc = AttentionBroadcast([999, 666, 333, 0], F, attn1_every=2, attn2_every=2, attn1_window=(0, 1000), attn2_window=(0, 1000))
    vidtome_amd.register_attention_broadcast(unet, bc)
    bc.set_step(1)
    assert vpatch.broadcast_modes(blk)[2:] == ("reuse", "reuse")
    replays = []
    monkeypatch.setattr(vpatch, "broadcast_feed_forward_residual", lambda bc, name, norm, ff, hs: seen.append("replay + panels") or hs + 3)
    monkeypatch.setattr(bc, "replay", lambda who, kinds, hs: replays.append(tuple(kinds)) or hs + 8)
    del seen[:], calls[:]
    assert torch.equal(blk(x), x + 3) and seen == ["replay + panels"] and len(calls) == 1 and not replays
    monkeypatch.setattr(vpatch, "FF_MODE", "blas")
    del seen[:], calls[:]
    assert torch.equal(blk(x), x + 8 + 4) and seen == ["module"] and len(calls) == 1
    assert replays == [("attn1", "attn2")]                     # both deltas in ONE replay launch


# ---------------------------------------------------------------------------------------------------
# the dispatch
# ---------------------------------------------------------------------------------------------------
def test_dispatch_hands_the_modulation_to_the_module_body_alone(built, monkeypatch):
    from vidtome_amd import patch as vpatch
    unet, blk = _patched()
    x, plan, ada = _tokens(), _plan(), (object(), object(), object())
    got = []
    # (stand-ins with the bodies' own parameter lists: an ``ada`` handed to any of the first three would be a TypeError)
    monkeypatch.setattr(vpatch, "merged_feed_forward_residual", lambda block, hs, plan, route: got.append((route, block, hs, plan)))
    monkeypatch.setattr(vpatch, "norm_feed_forward_residual", lambda norm, ff, hs: got.append(("panels", norm, ff, hs)))
    monkeypatch.setattr(vpatch, "norm_feed_forward_f32", lambda norm, ff, hs: got.append(("f32", norm, ff, hs)))
    monkeypatch.setattr(vpatch, "module_feed_forward_residual", lambda norm, ff, hs, ada=None: got.append(("module", norm, ff, hs, ada)))
    for route in ("merged-panels", "merged", "panels", "f32", "module"):
        vpatch.feed_forward_segment(blk, x, plan, route, ada)
    assert got == [("merged-panels", blk, x, plan), ("merged", blk, x, plan), ("panels", blk.norm3, blk.ff, x),
                   ("f32", blk.norm3, blk.ff, x), ("module", blk.norm3, blk.ff, x, ada)]
    del got[:]
    vpatch.feed_forward_segment(blk, x, None, "module")
    assert got == [("module", blk.norm3, blk.ff, x, None)]


def test_module_body_is_the_reference_expression(built, monkeypatch):
    """layer_norm(norm3) -> shift / scale -> feed_forward -> gate -> + h, reached through the module's globals."""
    from vidtome_amd import patch as vpatch
    unet, blk = _patched(F32)
    g = torch.Generator().manual_seed(4)
    h = torch.randn(B * F, N, 64, generator=g)
    shift, scale, gate = (torch.randn(B * F, 64, generator=g) for _ in range(3))
    through = []
    real_ln, real_ff = vpatch.layer_norm, vpatch.feed_forward
    monkeypatch.setattr(vpatch, "layer_norm", lambda norm, x: through.append("layer_norm") or real_ln(norm, x))
    monkeypatch.setattr(vpatch, "feed_forward", lambda ff, x: through.append("feed_forward") or real_ff(ff, x))
    with torch.no_grad():
        got = vpatch.module_feed_forward_residual(blk.norm3, blk.ff, h, (shift, scale, gate))
        want = gate.unsqueeze(1) * blk.ff(blk.norm3(h) * (1 + scale[:, None]) + shift[:, None]) + h
        assert torch.equal(got, want) and through == ["layer_norm", "feed_forward"]
        assert torch.equal(vpatch.module_feed_forward_residual(blk.norm3, blk.ff, h), blk.ff(blk.norm3(h)) + h)


def test_forward_unpacks_norm1_into_the_dispatch(built, monkeypatch):
    """An AdaLayerNormZero block: the forward hands norm1's shift / scale / gate, in that order, to the dispatch."""
    from vidtome_amd import patch as vpatch
    unet, blk = _patched()
    x = _tokens()
    parts = [torch.full((B * F, 64), float(i), dtype=F16) for i in range(4)]           # gate_msa, shift_mlp, scale_mlp, gate_mlp
    blk.use_ada_layer_norm_zero = True
    blk.norm1 = AdaZeroNorm1(parts)
    blk.attn2 = None
    got = {}
    monkeypatch.setattr(vpatch, "patched_self_attention_segment", lambda block, hs, nhs, enc, mask, kw, gate_msa, **k:
                        got.update(gate_msa=gate_msa) or hs)
    monkeypatch.setattr(vpatch, "feed_forward_segment", lambda block, hs, plan, route, ada: got.update(route=route, ada=ada) or hs)
    blk(x)
    assert got["gate_msa"] is parts[0] and got["route"] == "module"
    assert len(got["ada"]) == 3 and all(a is b for a, b in zip(got["ada"], parts[1:]))
