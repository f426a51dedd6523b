"""CPU tests of the routing at token counts that are no multiple of 8 (widescreen frames: 480 x 848 gives 1590 and 405 tokens
per frame, 360 x 640 gives 60): attn2's fused segment and the un-merged attn1 segment take any N, every other refusal stands,
and the IP-Adapter call keeps asking N % 8 == 0 of its panel path."""
import pytest
import torch

import standin
from ip_adapter_standin import IPAttention, PROCESSOR_CLASSES, image_states
from test_masked_cross_host import ACCEPTED, FakeCuda

C, HEADS, D, B, T = 64, 2, 64, 2, 77
ODD = (12, 20, 100, 405)


def _x(N, dtype=torch.float16, C=C):
    return torch.zeros(B, N, C, dtype=dtype).as_subclass(FakeCuda)


def _cross():
    return standin.CrossAttention(C, HEADS, D).half(), torch.nn.LayerNorm(C).half(), torch.zeros(B, T, D, dtype=torch.float16)


@pytest.mark.parametrize("N", ODD)
def test_fused_cross_ok_takes_any_token_count(N):
    from vidtome_amd import patch as vpatch
    a, norm, enc = _cross()
    assert N % 8
    assert vpatch.fused_cross_ok(norm, a, _x(N), enc, None, {}) is True
    for what in ("fp16 (B, 1, K)", "one row for every sample (1, 1, K)", "-inf values"):
        assert vpatch.fused_cross_ok(norm, a, _x(N), enc, ACCEPTED[what](), {}) is True, what


def test_every_other_refusal_of_fused_cross_ok_stands():
    from vidtome_amd import patch as vpatch
    a, norm, enc = _cross()
    N = 100
    ok = ACCEPTED["fp16 (B, 1, K)"]()
    for mask in (None, ok):
        assert vpatch.fused_cross_ok(norm, a, _x(N), enc, mask, {}) is True
        assert vpatch.fused_cross_ok(norm, a, _x(N), enc, mask, {"scale": 1.0}) is False                    # kwargs
        assert vpatch.fused_cross_ok(norm, a, _x(N), (enc, [enc]), mask, {}) is False                       # tuple conditioning
        assert vpatch.fused_cross_ok(norm, a, torch.zeros(B, N, C, dtype=torch.float16), enc, mask, {}) is False   # a CPU tensor
        assert vpatch.fused_cross_ok(torch.nn.LayerNorm(C), a, _x(N), enc, mask, {}) is False               # fp32 norm, fp16 block
    assert vpatch.fused_cross_ok(norm, a, _x(N), enc, torch.ones(B, 1, T, dtype=torch.bool), {}) is False   # a refused mask form
    a32, n32 = standin.CrossAttention(C, HEADS, D), torch.nn.LayerNorm(C)
    assert vpatch.fused_cross_ok(n32, a32, _x(N, torch.float32), enc.float(), None, {}) is False            # fp32 model


def test_unmerged_self_attention_ok_takes_an_odd_site():
    """360 x 640: the ds 8 site holds 6 x 10 = 60 tokens per frame and does not merge."""
    from vidtome_amd import patch as vpatch
    Cb = 640
    blk = standin.BasicTransformerBlock(Cb, 8).half()
    blk._tome_info = {"size": (45, 80), "args": {"max_downsample": 2}}
    x = _x(60, C=Cb)
    assert vpatch.unmerged_site(blk, x)
    assert vpatch.unmerged_self_attention_ok(blk, x) is True
    assert vpatch.unmerged_self_attention_ok(blk, _x(64, C=Cb)) is True
    # what it refused before, it refuses at N = 60 too
    assert vpatch.unmerged_self_attention_ok(blk, torch.zeros(B, 60, Cb, dtype=torch.float16)) is False     # a CPU tensor
    blk.norm1 = torch.nn.LayerNorm(Cb)
    assert vpatch.unmerged_self_attention_ok(blk, x) is False                                               # fp32 norm, fp16 block
    blk.norm1 = torch.nn.LayerNorm(Cb).half()
    blk._tome_info["size"] = (6, 10)                                                                        # a site that merges
    assert vpatch.unmerged_self_attention_ok(blk, x) is False


def test_ip_adapter_panel_path_still_asks_a_multiple_of_8():
    from vidtome_amd import patch as vpatch
    a = IPAttention(standin.CrossAttention(C, HEADS, D), PROCESSOR_CLASSES["IPAdapterAttnProcessor2_0"](C, D, (4,), (0.6,))).half()
    norm = torch.nn.LayerNorm(C).half()
    for N in ODD:
        enc = (torch.zeros(B, T, D, dtype=torch.float16), image_states((4,), B, D, torch.float16, "cpu"))
        assert vpatch.ip_cross_call(a, _x(N), enc, None, {}, norm) is None
        assert vpatch.ip_cross_call(a, _x(N), enc, None, {}) is not None          # cross_attention's library GEMMs take it
    enc = (torch.zeros(B, T, D, dtype=torch.float16), image_states((4,), B, D, torch.float16, "cpu"))
    assert vpatch.ip_cross_call(a, _x(16), enc, None, {}, norm) is not None
