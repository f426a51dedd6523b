"""CPU tests of attn2's routing (patch.attn2_route) against a literal table: case -> (frame, the core wrappers its core
dispatch launches, an IP-Adapter call or not).  Every row is asked of ``attn2_route`` and then taken through ONE block forward
whose launches are stubbed: the panels and f32 bodies are replaced by stand-ins that run ``patch._attn2_core`` on zero query
rows with library projections, ``cross_attention`` is the real one, and the core wrappers of vidtome_amd._lib are fakes that
record their names.  No GPU, no launch.  The same forwards count the calls of ``ip_adapter.recognise`` and of
``fused_attention_ok`` on attn2."""
import re

import pytest
import torch

import cross_control_standin as CC
import ip_adapter_mask_standin as IPM
import ip_adapter_standin as IPS
import standin
from test_masked_cross_host import ACCEPTED, REFUSED, FakeCuda

C, HEADS, B, N, T, D = 64, 2, 2, 16, 77, CC.COND_DIM
F16, F32 = torch.float16, torch.float32
CORES = ("attention_kv", "attention_kv_bias", "attention_kv_sets", "attention_kv_sets_masked", "cross_edit_values",
         "attention_kv_sets_src")
CONTROLLED = "attention_kv cross_edit_values attention_kv_sets_src"     # identity run, then the edited group's two launches
OK_MASK = "fp16 (B, 1, K)"

# case -> options of ``_build``
CASES = {
    "plain": {},
    "accepted mask": {"mask": ACCEPTED[OK_MASK]},
    "processor kwargs": {"kwargs": {"scale": 1.0}},
    "CPU tokens": {"cuda": False},
    "C = 160, 2 heads": {"c": 160},
    "FF_MODE = blas": {"ff_mode": "blas"},
    "a non-plain norm2": {"tweak": "other norm2"},
    "fp32 to_out in an fp16 block": {"tweak": "fp32 to_out"},
    "fp32, fp32_projections": {"dtype": F32, "opt_in": True},
    "fp32": {"dtype": F32},
    "fp32, fp32_projections, accepted mask": {"dtype": F32, "opt_in": True, "mask": ACCEPTED["fp32 (B, 1, K)"]},
    "IP-Adapter N = 16": {"ip": "plain"},
    "IP-Adapter N = 12": {"ip": "plain", "n": 12},
    "IP-Adapter region masks": {"ip": "region"},
    "IP-Adapter with a mask": {"ip": "plain", "mask": ACCEPTED[OK_MASK]},
    "IP-Adapter FF_MODE = blas": {"ip": "plain", "ff_mode": "blas"},
    "AdaLayerNorm plain": {"ada": True},
    "AdaLayerNorm accepted mask": {"ada": True, "mask": ACCEPTED[OK_MASK]},
    "AdaLayerNorm IP-Adapter": {"ada": True, "ip": "plain"},
    "control": {"control": True},
    "control FF_MODE = blas": {"control": True, "ff_mode": "blas"},
    "control with a mask": {"control": True, "mask": ACCEPTED[OK_MASK]},
    "norm2 gives fp32 tokens from fp16 hidden states": {"tweak": "fp32 norm2 output"},
}
CASES.update({f"refused mask: {what}": {"mask": make} for what, make in REFUSED.items() if what != "None"})

# case -> (frame, core wrappers in launch order, an IP-Adapter call was recognised) | the text a refusal raises with
EXPECTED = {
    "plain": ("panels", "attention_kv", False),
    "accepted mask": ("panels", "attention_kv_bias", False),
    "processor kwargs": ("module", "", False),
    "CPU tokens": ("module", "", False),
    "C = 160, 2 heads": ("blas", "attention_kv", False),                    # C % 64 != 0, head dim 80
    "FF_MODE = blas": ("blas", "attention_kv", False),
    "a non-plain norm2": ("blas", "attention_kv", False),
    "fp32 to_out in an fp16 block": ("blas", "attention_kv", False),
    "fp32, fp32_projections": ("f32", "attention_kv", False),
    "fp32": ("module", "", False),
    "fp32, fp32_projections, accepted mask": ("module", "", False),
    "IP-Adapter N = 16": ("panels", "attention_kv_sets", True),
    "IP-Adapter N = 12": ("blas", "attention_kv_sets", True),
    "IP-Adapter region masks": ("panels", "attention_kv_sets_masked", True),
    "IP-Adapter with a mask": ("module", "", False),
    "IP-Adapter FF_MODE = blas": ("blas", "attention_kv_sets", True),
    "AdaLayerNorm plain": ("blas", "attention_kv", False),
    "AdaLayerNorm accepted mask": ("module", "", False),
    "AdaLayerNorm IP-Adapter": ("blas", "attention_kv_sets", True),
    "control": ("panels", CONTROLLED, False),
    "control FF_MODE = blas": ("blas", CONTROLLED, False),
    "control with a mask": "an attention_mask is not taken",
    "norm2 gives fp32 tokens from fp16 hidden states": ("module", "", False),
}
EXPECTED.update({name: ("module", "", False) for name in CASES if name.startswith("refused mask: ")})
# asked of attn2_route with the HIDDEN states alone this row is "blas"; the forward asks again with the normed tokens
PRE_NORM = {"norm2 gives fp32 tokens from fp16 hidden states": ("blas", False)}


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


class OtherNorm(torch.nn.LayerNorm):
    """Computes a LayerNorm, but is not the class the fused path reads."""


class Fp32Norm(torch.nn.LayerNorm):
    """A norm2 whose output is fp32 whatever it is given (a module-path LayerNorm under autocast does the reverse)."""

    def forward(self, x):
        return super().forward(x).float()


class AdaNorm(torch.nn.Module):
    """AdaLayerNorm's call: (tokens, timestep)."""

    def __init__(self, c):
        super().__init__()
        self.norm = torch.nn.LayerNorm(c)

    def forward(self, x, timestep):
        return self.norm(x)


class CountingForward(torch.nn.Module):
    """attn2's own forward (the module path): counts its calls and returns zeros."""
    calls = 0

    def forward(self, x, encoder_hidden_states=None, attention_mask=None, **kw):
        self.calls += 1
        return torch.zeros_like(x)


class Case:
    pass


def _build(name):
    """The patched block, its inputs and the registered control of one CASES row."""
    import vidtome_amd
    from vidtome_amd import pnp
    opt = CASES[name]
    dtype, c, n = opt.get("dtype", F16), opt.get("c", C), opt.get("n", N)
    case = Case()
    case.unet = unet = CC.ControlUNet(c, heads=HEADS).to(dtype)
    vidtome_amd.apply_patch(unet, batch_size=1)
    case.blk = blk = unet.block
    if opt.get("ada"):
        blk.use_ada_layer_norm = True
        blk.norm1, blk.norm2 = AdaNorm(c).to(dtype), AdaNorm(c).to(dtype)
    tweak = opt.get("tweak")
    if tweak == "other norm2":
        blk.norm2 = OtherNorm(c).to(dtype)
    elif tweak == "fp32 to_out":
        blk.attn2.to_out[0].float()
    elif tweak == "fp32 norm2 output":
        blk.norm2 = Fp32Norm(c).to(dtype)
    if opt.get("opt_in"):
        vidtome_amd.update_patch(unet, fp32_projections=True)
    text = torch.zeros(B, T, D, dtype=dtype)
    case.enc, case.kwargs = text, dict(opt.get("kwargs", {}))
    if opt.get("ip"):
        region = opt["ip"] == "region"
        proc = (IPM if region else IPS).PROCESSOR_CLASSES["IPAdapterAttnProcessor2_0"](c, D, (4,), (0.6,)).to(dtype)
        blk.attn2 = IPS.IPAttention(blk.attn2, proc)
        if region:
            case.enc = (text, [torch.zeros(B, 1, 4, D, dtype=dtype)])
            case.kwargs = {"ip_adapter_masks": [torch.ones(1, 1, 4, 4)]}
        else:
            case.enc = (text, IPS.image_states((4,), B, D, dtype, "cpu"))
    else:
        blk.attn2.__class__ = type("Attention", (CountingForward, type(blk.attn2)), {})
    case.mask = opt["mask"]() if "mask" in opt else None
    x = torch.zeros(B, n, c, dtype=dtype)
    case.x = x.as_subclass(FakeCuda) if opt.get("cuda", True) else x
    case.control = None
    if opt.get("control"):
        pnp.register_time(standin.Pipe(unet), 981)
        edits = {1: CC.edit_of(CC.specs()["replace"])}
        assert vidtome_amd.register_cross_attention_control(unet, [981], 2, edits) == [CC.BLOCK]
    case.ff_mode = opt.get("ff_mode", "panels")
    return case


def _module_calls(blk):
    return blk.attn2.processor.calls if hasattr(blk.attn2, "processor") else blk.attn2.calls


def _stub_launches(monkeypatch, vpatch, seen):
    """Everything of a block forward that launches, except the attn2 routing under test: attn1's and the feed-forward's
    segments are no-ops, the norms are the modules' own, the panels and f32 bodies run the core dispatch alone, the core
    wrappers record their names."""
    from vidtome_amd import _lib

    def fake(name):
        def f(q, *a, out=None, **kw):
            seen["cores"].append(name)
            return torch.zeros_like(q) if out is None else out
        return f

    def frame(name):
        def body(norm, attn, hidden_states, encoder_hidden_states, ip=None, attention_mask=None, probs_to=None, words_to=None,
                 ctl=None):
            seen["frames"].append(name)
            vpatch._attn2_core(attn, torch.zeros_like(hidden_states), hidden_states.shape[1], encoder_hidden_states, "blas",
                               attention_mask, ip, ctl)
            return hidden_states
        return body

    real_cross = vpatch.cross_attention

    def cross_attention(*a, **kw):
        seen["frames"].append("cross_attention")
        return real_cross(*a, **kw)
    for name in CORES:
        monkeypatch.setattr(_lib, name, fake(name))
    monkeypatch.setattr(vpatch, "self_attention_segment", lambda blk, hs, *a, **kw: hs)
    monkeypatch.setattr(vpatch, "patched_self_attention_segment", lambda blk, hs, *a, **kw: hs)
    monkeypatch.setattr(vpatch, "norm_cross_attention_residual", frame("panels"))
    monkeypatch.setattr(vpatch, "norm_cross_attention_f32",
                        lambda norm, attn, hs, enc, probs_to=None, words_to=None: frame("f32")(norm, attn, hs, enc))
    monkeypatch.setattr(vpatch, "cross_attention", cross_attention)
    monkeypatch.setattr(vpatch, "layer_norm", lambda norm, x: norm(x.to(norm.weight.dtype)))
    monkeypatch.setattr(vpatch, "fused_ff_ok", lambda *a: False)
    monkeypatch.setattr(vpatch, "f32_ff_ok", lambda *a: False)
    monkeypatch.setattr(vpatch, "feed_forward", lambda ff, x: torch.zeros_like(x))


def _forward(case):
    with torch.no_grad():
        return case.blk(case.x, encoder_hidden_states=case.enc, encoder_attention_mask=case.mask, timestep=torch.tensor(981),
                        cross_attention_kwargs=case.kwargs or None)


def test_the_table_names_every_case():
    assert set(EXPECTED) == set(CASES)
    assert {"module", "blas", "panels", "f32"} == {e[0] for e in EXPECTED.values() if isinstance(e, tuple)}
    assert sum(name.startswith("refused mask: ") for name in CASES) == len(REFUSED) - 1


@pytest.mark.filterwarnings("ignore:vidtome_amd")
@pytest.mark.parametrize("name", sorted(CASES))
def test_route_and_forward_of_every_row(built, name, monkeypatch):
    import vidtome_amd
    from vidtome_amd import ip_adapter
    from vidtome_amd import patch as vpatch
    case, expected = _build(name), EXPECTED[name]
    blk = case.blk
    monkeypatch.setattr(vpatch, "FF_MODE", case.ff_mode)
    control = vpatch.cross_control(blk)
    assert (control is not None) == bool(CASES[name].get("control"))
    ask = lambda: vpatch.attn2_route(blk, case.x, case.enc, case.mask, case.kwargs, control)
    seen = {"cores": [], "frames": []}
    _stub_launches(monkeypatch, vpatch, seen)
    if isinstance(expected, str):                                   # a refusal: the same text from the route and the forward
        for call in (ask, lambda: _forward(case)):
            with pytest.raises(RuntimeError, match=rf"'{re.escape(CC.BLOCK)}'.*{re.escape(expected)}"):
                call()
        assert seen == {"cores": [], "frames": []} and _module_calls(blk) == 0
        assert vpatch.cross_control_route(blk, case.x, case.enc, None, case.kwargs, control) == "panels"   # without the mask
        return
    # 1. the route function alone: launches nothing, calls the module's forward never
    route = ask()
    want_frame, want_ip = PRE_NORM.get(name, (expected[0], expected[2]))
    assert route.frame == want_frame and (route.ip is not None) == want_ip and isinstance(route.ip, (type(None), ip_adapter.Call))
    assert seen == {"cores": [], "frames": []} and _module_calls(blk) == 0
    if control is not None:
        assert vpatch.cross_control_route(blk, case.x, case.enc, case.mask, case.kwargs, control) == route.frame
    # 2. one block forward, counted
    counts = {"recognise": 0, "fused_attention_ok": {}}
    real_recognise, real_ok, keep = ip_adapter.recognise, vpatch.fused_attention_ok, []

    def recognise(*a, **kw):
        counts["recognise"] += 1
        return real_recognise(*a, **kw)

    def fused_attention_ok(attn, x, *a, **kw):
        if attn is blk.attn2:
            keep.append(x)                                          # (alive: ids are not reused)
            counts["fused_attention_ok"][id(x)] = counts["fused_attention_ok"].get(id(x), 0) + 1
        return real_ok(attn, x, *a, **kw)
    monkeypatch.setattr(ip_adapter, "recognise", recognise)
    monkeypatch.setattr(vpatch, "fused_attention_ok", fused_attention_ok)
    out = _forward(case)
    assert out.shape == case.x.shape
    frame = seen["frames"][0] if seen["frames"] else None
    assert len(seen["frames"]) == 1
    if frame == "cross_attention":
        frame = "module" if _module_calls(blk) else "blas"
    assert (frame, " ".join(seen["cores"])) == expected[:2], (name, seen)
    assert _module_calls(blk) == (1 if expected[0] == "module" else 0)
    assert counts["recognise"] <= 1, counts
    assert all(n == 1 for n in counts["fused_attention_ok"].values()), counts
    assert len(counts["fused_attention_ok"]) <= (2 if name in PRE_NORM else 1), counts
    vidtome_amd.remove_patch(case.unet)


def test_public_predicates_state_the_same_rules(built, monkeypatch):
    """``fused_cross_ok``, ``f32_cross_ok`` and ``ip_cross_call`` answer what the route answers, row by row."""
    from vidtome_amd import patch as vpatch
    for name, expected in sorted(EXPECTED.items()):
        opt = CASES[name]
        if isinstance(expected, str) or opt.get("control") or opt.get("ada") or name in PRE_NORM:
            continue
        case = _build(name)
        blk = case.blk
        monkeypatch.setattr(vpatch, "FF_MODE", case.ff_mode)
        args = (case.x, case.enc, case.mask, case.kwargs)
        frame, _, is_ip = expected
        assert vpatch.fused_cross_ok(blk.norm2, blk.attn2, *args) is (frame == "panels" and not is_ip), name
        assert vpatch.f32_cross_ok(blk, blk.norm2, blk.attn2, *args) is (frame == "f32"), name
        assert (vpatch.ip_cross_call(blk.attn2, *args, blk.norm2) is not None) == (is_ip and frame == "panels"), name
        assert (vpatch.ip_cross_call(blk.attn2, *args) is not None) == is_ip, name
