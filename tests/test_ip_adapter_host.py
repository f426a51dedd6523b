"""CPU tests of the IP-Adapter recogniser (vidtome_amd/ip_adapter.py, patch.ip_cross_call): what the fused path accepts, what
keeps the module path, and that the key sets it builds are what the decoupled cross-attention formula says."""
import pytest
import torch

import standin
from ip_adapter_standin import IPAttention, PROCESSOR_CLASSES, image_states
from lora_standin import PeftLinear

C, HEADS, D, B, N, T = 64, 2, 64, 2, 16, 77


class FakeCuda(torch.Tensor):          # the predicates need x.is_cuda; emulate it without a device
    @property
    def is_cuda(self):
        return True


def _attn(num_tokens=(4,), scale=(0.6,), name="IPAdapterAttnProcessor2_0", dtype=torch.float16):
    src = standin.CrossAttention(C, HEADS, D)
    a = IPAttention(src, PROCESSOR_CLASSES[name](C, D, num_tokens, scale))
    return a.to(dtype)


def _x(dtype=torch.float16):
    return torch.zeros(B, N, C, dtype=dtype).as_subclass(FakeCuda)


def _enc(num_tokens=(4,), dtype=torch.float16, images=1):
    return (torch.zeros(B, T, D, dtype=dtype), image_states(num_tokens, B, D, dtype, "cpu", images=images))


def _call(a, enc=None, x=None, mask=None, kwargs=None, norm=None):
    from vidtome_amd import patch as vpatch
    x = _x() if x is None else x
    enc = _enc(tuple(a.processor.num_tokens)) if enc is None else enc
    return vpatch.ip_cross_call(a, x, enc, mask, kwargs if kwargs is not None else {}, norm)


@pytest.mark.parametrize("name", ["IPAdapterAttnProcessor", "IPAdapterAttnProcessor2_0", "IPAdapterXFormersAttnProcessor"])
def test_the_three_processor_names_are_recognised(name):
    ip = _call(_attn(name=name))
    assert ip is not None and ip.text.shape == (B, T, D) and [tuple(i.shape) for i in ip.images] == [(B, 4, D)]
    assert ip.scales == [0.6] and len(ip.k_proj) == len(ip.v_proj) == 1


def test_unknown_processor_name_keeps_the_module_path():
    assert _call(_attn(name="UnknownIPProcessor")) is None
    a = standin.CrossAttention(C, HEADS, D).half()               # no processor at all: not an IP-Adapter call
    assert _call(a, enc=_enc()) is None


def test_image_tensor_shapes_and_the_legacy_split():
    a = _attn((4, 16), (0.7, 0.3))
    ip = _call(a)
    assert [i.shape[1] for i in ip.images] == [4, 16]
    ip = _call(a, enc=_enc((4, 16), images=3))                   # (B, m, T_a, D): m * T_a keys per adapter
    assert [tuple(i.shape) for i in ip.images] == [(B, 12, D), (B, 48, D)]
    text, ims = _enc((4, 16))
    assert _call(a, enc=(text, tuple(ims))) is not None          # a tuple of images is as good as a list
    one = _attn((4,), (0.5,))
    legacy = torch.arange(B * (T + 4) * D, dtype=torch.float16).view(B, T + 4, D)
    ip = _call(one, enc=legacy)
    assert ip is not None and torch.equal(ip.text, legacy[:, :T]) and torch.equal(ip.images[0], legacy[:, T:])
    assert _call(a, enc=torch.zeros(B, T + 20, D, dtype=torch.float16)) is None      # legacy form with two adapters
    assert _call(one, enc=torch.zeros(B, 4, D, dtype=torch.float16)) is None         # nothing left for the text


def test_masks_and_cross_attention_kwargs():
    a = _attn()
    assert _call(a, kwargs={"ip_adapter_masks": None}) is not None
    assert _call(a, kwargs={"ip_adapter_masks": [None]}) is not None
    assert _call(a, kwargs={"ip_adapter_masks": [torch.ones(1, N, 1)]}) is None
    assert _call(a, kwargs={"scale": 1.0}) is None
    assert _call(a, kwargs={"ip_adapter_masks": None, "scale": 1.0}) is None
    assert _call(a, mask=torch.zeros(B, 1, T)) is None


def test_what_the_recogniser_refuses():
    refused = {}
    a = _attn((4, 16), (0.7, 0.3))
    a.processor.scale = [0.7, [0.3, 0.1]]
    refused["list-valued scale"] = (a, None)
    a = _attn((4, 16), (0.7, 0.3))
    a.processor.scale = [0.7]
    refused["fewer scales than adapters"] = (a, None)
    a = _attn((4, 16), (0.7, 0.3))
    a.processor.num_tokens = [4]
    refused["fewer num_tokens than adapters"] = (a, None)
    a = _attn((4, 16), (0.7, 0.3))
    a.processor.to_v_ip = torch.nn.ModuleList(list(a.processor.to_v_ip)[:1])
    refused["to_k_ip / to_v_ip lengths differ"] = (a, None)
    a = _attn((4, 16), (0.7, 0.3))
    refused["fewer image tensors than adapters"] = (a, _enc((4,)))
    a = _attn()
    a.processor.to_k_ip[0] = torch.nn.Linear(D, C, bias=True).half()
    refused["bias on to_k_ip"] = (a, None)
    a = _attn()
    a.processor.to_v_ip[0] = torch.nn.Linear(D, C // 2, bias=False).half()
    refused["out_features != C"] = (a, None)
    a = _attn()
    a.processor.to_k_ip[0] = torch.nn.Linear(D, C, bias=False)
    refused["fp32 to_k_ip in an fp16 block"] = (a, None)
    a = _attn()
    a.processor.to_k_ip[0] = torch.nn.Sequential(torch.nn.Linear(D, C, bias=False).half())
    refused["to_k_ip not a Linear"] = (a, None)
    a = _attn()
    mods = list(a.processor.to_k_ip)
    del a.processor.to_k_ip
    a.processor.to_k_ip = mods
    refused["to_k_ip not a ModuleList"] = (a, None)
    a = _attn()
    a.processor.num_tokens = [0]
    refused["num_tokens not positive"] = (a, None)
    a = _attn()
    a.processor.scale = [True]
    refused["bool scale"] = (a, None)
    a = _attn()
    refused["image width differs from to_k_ip's"] = (a, (torch.zeros(B, T, D).half(), [torch.zeros(B, 4, D // 2).half()]))
    a = _attn()
    refused["image batch differs"] = (a, (torch.zeros(B, T, D).half(), [torch.zeros(B + 1, 4, D).half()]))
    a = _attn()
    refused["text not 3-D"] = (a, (torch.zeros(B * T, D).half(), [torch.zeros(B, 4, D).half()]))
    a = _attn()
    refused["a 3-tuple"] = (a, (torch.zeros(B, T, D).half(), [torch.zeros(B, 4, D).half()], None))
    a = _attn()
    a.group_norm = torch.nn.GroupNorm(1, C)
    refused["what fused_attention_ok refuses: group_norm"] = (a, None)
    a = _attn()
    a.to_q = torch.nn.Sequential(a.to_q)
    refused["what fused_attention_ok refuses: to_q not a Linear"] = (a, None)
    for what, (a, enc) in refused.items():
        assert _call(a, enc=enc) is None, what
    # fp32 models keep the module path, with or without fp32_projections
    a32 = _attn(dtype=torch.float32)
    assert _call(a32, enc=_enc(dtype=torch.float32), x=_x(torch.float32)) is None


def test_lora_on_the_adapter_projections_is_read_through_the_fold_recogniser():
    a = _attn()
    base = a.processor.to_k_ip[0]
    wrapped = PeftLinear(base)
    wrapped.update_layer("a0", torch.randn(4, D).half(), torch.randn(C, 4).half(), 0.5)
    a.processor.to_k_ip[0] = wrapped
    assert _call(a) is not None
    wrapped.fan_in_fan_out = True                                # ... and refused when the fold recogniser refuses it
    assert _call(a) is None


def test_tuple_never_reaches_dim_in_the_plain_predicates():
    """The parent commit called ``encoder_hidden_states.dim()`` on the tuple: AttributeError in attn2."""
    from vidtome_amd import patch as vpatch
    a = _attn(name="UnknownIPProcessor")
    norm = torch.nn.LayerNorm(C).half()
    enc = _enc()
    assert vpatch.fused_cross_ok(norm, a, _x(), enc, None, {}) is False
    blk = torch.nn.Module()
    blk.fp32_projections = True
    assert vpatch.f32_cross_ok(blk, norm.float(), a.float(), _x(torch.float32), enc, None, {}) is False
    out = vpatch.cross_attention(a.float(), torch.zeros(B, N, C), (enc[0].float(), [i.float() for i in enc[1]]))
    assert out.shape == (B, N, C) and a.processor.calls == 1     # the module path ran, on the CPU


def test_panel_path_asks_what_fused_cross_ok_asks():
    a = _attn()
    norm = torch.nn.LayerNorm(C).half()
    assert _call(a, norm=norm) is not None
    assert _call(a, norm=torch.nn.LayerNorm(C)) is None          # fp32 norm weights in an fp16 block
    assert _call(a, x=torch.zeros(B, N + 4, C, dtype=torch.float16).as_subclass(FakeCuda), norm=norm) is None   # N % 8


def test_key_sets_are_what_the_formula_says():
    from vidtome_amd import ip_adapter
    assert ip_adapter.key_sets(77, [4], [0.6]) == ([(0, 77, 1.0), (80, 4, 0.6)], [0], 88)
    assert ip_adapter.key_sets(77, [4, 16, 257], [0.7, -0.3, 1.5]) == (
        [(0, 77, 1.0), (80, 4, 0.7), (88, 16, -0.3), (104, 257, 1.5)], [0, 1, 2], 368)
    assert ip_adapter.key_sets(154, [4, 16], [0.7, 0.3]) == ([(0, 154, 1.0), (160, 4, 0.7), (168, 16, 0.3)], [0, 1], 184)
    # a zero scale takes no keys at all; the later adapters close up
    assert ip_adapter.key_sets(77, [4, 16], [0.0, 0.3]) == ([(0, 77, 1.0), (80, 16, 0.3)], [1], 96)
    assert ip_adapter.key_sets(77, [4, 16], [0.7, 0]) == ([(0, 77, 1.0), (80, 4, 0.7)], [0], 88)
    assert ip_adapter.key_sets(77, [4, 16], [0.0, 0.0]) == ([(0, 77, 1.0)], [], 80)
    for sets, _, end in (ip_adapter.key_sets(77, [4, 16, 257], [1.0, 1.0, 1.0]), ip_adapter.key_sets(80, [8], [1.0])):
        assert all(s % 8 == 0 for s, _, _ in sets) and end % 8 == 0
        assert all(a[0] + a[1] <= b[0] for a, b in zip(sets, sets[1:])) and sets[-1][0] + sets[-1][1] <= end


def test_scale_is_read_at_every_call():
    a = _attn((4, 16), (0.7, 0.3))
    assert _call(a).scales == [0.7, 0.3]
    a.processor.scale = [0.0, 1.25]                              # what pipe.set_ip_adapter_scale does
    assert _call(a).scales == [0.0, 1.25]


def test_header_declares_and_lib_binds_the_export():
    import os
    from vidtome_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vidtome_hip.h")).read()
    assert "int vtm_attention_kv_sets(" in hdr and "vtm_attention_kv_sets" in _lib.exported_symbols()
    assert "#define VTM_ABI_VERSION 2" in hdr                    # the export is additive: the ABI version stays
