"""CPU tests of masked cross-attention's host side: the mask recogniser (patch.key_bias), what the routing predicates do
with a mask and without one, where cross_attention sends a call, and that the export is declared and bound."""
import os

import pytest
import torch

import standin
from ip_adapter_standin import IPAttention, PROCESSOR_CLASSES, image_states

C, HEADS, D, B, N, T = 64, 2, 64, 2, 16, 77
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeCuda(torch.Tensor):          # the predicates need x.is_cuda; emulate it without a device
    @property
    def is_cuda(self):
        return True


class CountingCross(standin.CrossAttention):
    """A computing attn2 that counts its calls (the module path)."""
    calls = 0

    def forward(self, x, encoder_hidden_states=None, attention_mask=None, **kw):
        self.calls += 1
        return torch.zeros_like(x)


def _x(dtype=torch.float16):
    return torch.zeros(B, N, C, dtype=dtype).as_subclass(FakeCuda)


def _diffusers_bias(lengths, dtype=torch.float16):
    """What Diffusers' UNet makes of an encoder_attention_mask (B, K): (1 - mask) * -10000, unsqueezed to (B, 1, K)."""
    keep = torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]
    return ((1 - keep.to(dtype)) * -10000.0).unsqueeze(1)


ACCEPTED = {
    "fp16 (B, 1, K)": lambda: _diffusers_bias([57, 30]),
    "bf16 (B, 1, K)": lambda: _diffusers_bias([57, 30], torch.bfloat16),
    "fp32 (B, 1, K)": lambda: _diffusers_bias([57, 30], torch.float32),
    "one row for every sample (1, 1, K)": lambda: _diffusers_bias([57]),
    "-inf values": lambda: torch.zeros(B, 1, T).masked_fill(torch.arange(T) >= 50, float("-inf")),
    "a row expanded over the samples": lambda: _diffusers_bias([57]).expand(B, 1, T),
}
REFUSED = {
    "None": lambda: None,
    "a bool mask": lambda: torch.ones(B, 1, T, dtype=torch.bool),
    "an integer mask": lambda: torch.ones(B, 1, T, dtype=torch.int64),
    "a 2-D mask (B, K)": lambda: torch.zeros(B, T, dtype=torch.float16),
    "a 4-D mask": lambda: torch.zeros(B, 1, 1, T, dtype=torch.float16),
    "a per-query mask (B, N, K)": lambda: torch.zeros(B, N, T, dtype=torch.float16),
    "a key count above the conditioning's": lambda: torch.zeros(B, 1, T + 3, dtype=torch.float16),
    "a key count below the conditioning's": lambda: torch.zeros(B, 1, T - 1, dtype=torch.float16),
    "another batch": lambda: torch.zeros(B + 1, 1, T, dtype=torch.float16),
    "another device": lambda: torch.zeros(B, 1, T, dtype=torch.float16, device="meta"),
    "a list": lambda: [[0.0] * T] * B,
}


def test_recogniser_accepts_the_published_form():
    from vidtome_amd import patch as vpatch
    for what, make in ACCEPTED.items():
        m = make()
        rows = vpatch.key_bias(m, B, T, torch.device("cpu"))
        assert rows is not None, what
        assert rows.dtype == torch.float32 and tuple(rows.shape) == (m.shape[0], T) and rows.stride(1) == 1, what
        assert torch.equal(rows, m[:, 0].float()), what
    assert vpatch.key_bias(ACCEPTED["fp16 (B, 1, K)"](), B, T) is not None          # no device asked


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_recogniser_refuses_every_other_form(what):
    from vidtome_amd import patch as vpatch
    assert vpatch.key_bias(REFUSED[what](), B, T, torch.device("cpu")) is None


def test_predicates_with_and_without_a_mask():
    """fused_cross_ok takes what the recogniser takes and nothing else; f32_cross_ok keeps refusing every mask; without a mask
    all of them answer what they answered before."""
    from vidtome_amd import patch as vpatch
    a, norm = standin.CrossAttention(C, HEADS, D).half(), torch.nn.LayerNorm(C).half()
    enc = torch.zeros(B, T, D, dtype=torch.float16)
    assert vpatch.fused_cross_ok(norm, a, _x(), enc, None, {}) is True
    for what, make in ACCEPTED.items():
        assert vpatch.fused_cross_ok(norm, a, _x(), enc, make(), {}) is True, what
    for what, make in REFUSED.items():
        if what != "None":
            assert vpatch.fused_cross_ok(norm, a, _x(), enc, make(), {}) is False, what
    ok = ACCEPTED["fp16 (B, 1, K)"]()
    # everything else fused_cross_ok asks is still asked with a mask
    assert vpatch.fused_cross_ok(norm, a, _x(), enc, ok, {"scale": 1.0}) is False
    assert vpatch.fused_cross_ok(torch.nn.LayerNorm(C), a, _x(), enc, ok, {}) is False
    assert vpatch.fused_cross_ok(norm, a, _x(), (enc, [enc]), ok, {}) is False
    assert vpatch.fused_cross_ok(norm, a, torch.zeros(B, N, C, dtype=torch.float16), enc, ok, {}) is False     # not on the GPU
    # fp32 models, with or without fp32_projections
    a32, n32, e32 = standin.CrossAttention(C, HEADS, D), torch.nn.LayerNorm(C), enc.float()
    blk = torch.nn.Module()
    for opt_in in (False, True):
        blk.fp32_projections = opt_in
        assert vpatch.f32_cross_ok(blk, n32, a32, _x(torch.float32), e32, None, {}) is opt_in
        for make in ACCEPTED.values():
            assert vpatch.f32_cross_ok(blk, n32, a32, _x(torch.float32), e32, make().float(), {}) is False
            assert vpatch.fused_cross_ok(n32, a32, _x(torch.float32), e32, make().float(), {}) is False
    assert vpatch.fused_cross_ok(n32, a32, _x(torch.float32), e32, None, {}) is False


def test_ip_adapter_call_with_a_mask_keeps_the_module_path():
    from vidtome_amd import patch as vpatch
    a = IPAttention(standin.CrossAttention(C, HEADS, D), PROCESSOR_CLASSES["IPAdapterAttnProcessor2_0"](C, D, (4,), (0.6,))).half()
    enc = (torch.zeros(B, T, D, dtype=torch.float16), image_states((4,), B, D, torch.float16, "cpu"))
    norm = torch.nn.LayerNorm(C).half()
    ok = ACCEPTED["fp16 (B, 1, K)"]()
    assert vpatch.ip_cross_call(a, _x(), enc, None, {}, norm) is not None
    assert vpatch.ip_cross_call(a, _x(), enc, ok, {}, norm) is None
    assert vpatch.ip_cross_call(a, _x(), enc, ok, {}) is None
    assert vpatch.fused_cross_ok(norm, a, _x(), enc, ok, {}) is False
    assert vpatch.fused_cross_ok(norm, a, _x(), enc[0], ok, {}) is False            # the processor is not a plain one


def test_cross_attention_sends_the_call_where_it_belongs(monkeypatch):
    """The library-GEMM dispatch (VIDTOME_FF=blas): an accepted mask reaches _lib.attention_kv_bias as fp32 rows, no mask
    reaches _lib.attention_kv, every refused form -- and an fp32 model with any mask -- is the module's own forward."""
    from vidtome_amd import _lib
    from vidtome_amd import patch as vpatch
    a = CountingCross(C, HEADS, D).half()
    enc = torch.zeros(B, T, D, dtype=torch.float16)
    seen = {"bias": [], "plain": 0}

    def fake_bias(q, k, vt, heads, Mq, Mk, scale, bias):
        seen["bias"].append(bias)
        assert (heads, Mq, Mk) == (HEADS, N, T) and tuple(k.shape) == (B, 80, C) and tuple(vt.shape) == (B, C, 80)
        return torch.zeros_like(q)

    def fake_plain(q, k, vt, heads, Mq, Mk, scale, **kw):
        seen["plain"] += 1
        return torch.zeros_like(q)
    monkeypatch.setattr(_lib, "attention_kv_bias", fake_bias)
    monkeypatch.setattr(_lib, "attention_kv", fake_plain)
    out = vpatch.cross_attention(a, _x(), enc, None)
    assert tuple(out.shape) == (B, N, C) and seen["plain"] == 1 and not seen["bias"] and a.calls == 0
    for i, (what, make) in enumerate(ACCEPTED.items()):
        m = make()
        out = vpatch.cross_attention(a, _x(), enc, m)
        assert tuple(out.shape) == (B, N, C) and len(seen["bias"]) == i + 1 and a.calls == 0, what
        rows = seen["bias"][-1]
        assert rows.dtype == torch.float32 and torch.equal(rows, m[:, 0].float()), what
    assert seen["plain"] == 1
    n_bias = len(seen["bias"])
    for i, (what, make) in enumerate((w, m) for w, m in REFUSED.items() if w != "None"):
        vpatch.cross_attention(a, _x(), enc, make())
        assert a.calls == i + 1 and len(seen["bias"]) == n_bias and seen["plain"] == 1, what
    a32 = CountingCross(C, HEADS, D)
    vpatch.cross_attention(a32, _x(torch.float32), enc.float(), ACCEPTED["fp32 (B, 1, K)"]())
    assert a32.calls == 1 and len(seen["bias"]) == n_bias


def test_attn1_mask_keeps_its_own_path():
    """A mask on attn1 never meets the recogniser: attn1's route asks `attention_mask is not None` as the segments did, and
    every form the recogniser takes on attn2 sends attn1 to its module forward."""
    import inspect
    from vidtome_amd import patch as vpatch
    for fn in (vpatch.attn1_route, vpatch.self_attention_segment, vpatch.patched_self_attention_segment):
        assert "key_bias" not in inspect.getsource(fn)
    assert "attention_mask is" in inspect.getsource(vpatch.attn1_route)
    blk = standin.BasicTransformerBlock(C, HEADS).half()
    assert vpatch.attn1_route(blk, _x()) != "module"                       # (only the mask sends it there)
    for what, make in ACCEPTED.items():
        assert vpatch.attn1_route(blk, _x(), None, make()) == "module", what


def test_header_declares_and_lib_binds_the_export():
    from vidtome_amd import _lib
    from vidtome_amd import build
    hdr = open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    assert "int vtm_attention_kv_bias(" in hdr and "vtm_attention_kv_bias" in _lib.exported_symbols()
    assert "#define VTM_ABI_VERSION 2" in hdr                    # the export is additive: the ABI version stays
    assert "attention_bias.hip" in build.SOURCES
    assert callable(_lib.attention_kv_bias)


def test_wrapper_refuses_bad_operands_before_any_launch():
    from vidtome_amd import _lib
    q, k, vt = torch.zeros(B, N, C), torch.zeros(B, 80, C), torch.zeros(B, C, 80)
    bias = torch.zeros(B, T)
    with pytest.raises(RuntimeError, match="fp16 / bf16"):
        _lib.attention_kv_bias(q, k, vt, HEADS, N, T, 0.125, bias)             # fp32 operands
    h = lambda t: t.half()
    for bad in (bias.half(), torch.zeros(B, T - 1), torch.zeros(B + 1, T), torch.zeros(B, 1, T), torch.zeros(B, 2 * T)[:, ::2],
                torch.zeros(B, T, device="meta"), None):
        with pytest.raises(RuntimeError, match="bias must be"):
            _lib.attention_kv_bias(h(q), h(k), h(vt), HEADS, N, T, 0.125, bad)
