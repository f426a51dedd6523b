"""CPU tests of the cross-attention maps' host side (vidtome_amd.maps): the switch and what clears it, the block selection,
the C-ABI surface of vtm_attention_probs and its wrapper's checks, and the torch restatement the routes without the kernel
use (patch._probs_torch / patch._module_path_probs) against float64."""
import ctypes
import os
import re
import warnings

import pytest
import torch

import attention_maps_standin as AM
import standin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 64


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


def _model(built):
    import vidtome_amd
    unet = standin.StandInUNet(C, 2, full=True, cond_dim=32)
    vidtome_amd.apply_patch(unet)
    return unet


def _names(unet):
    return [n for n, m in unet.named_modules() if m.__class__.__name__ == "ToMeBlock"]


def test_public_names():
    import vidtome_amd
    from vidtome_amd import maps
    assert vidtome_amd.register_attention_maps is maps.register_attention_maps
    assert vidtome_amd.unregister_attention_maps is maps.unregister_attention_maps
    assert {"register_attention_maps", "unregister_attention_maps"} <= set(vidtome_amd.__all__)


def test_register_unregister_and_remove_patch_set_and_clear_the_switch(built):
    import vidtome_amd
    unet = _model(built)
    names = _names(unet)
    assert len(names) == 9
    blocks = dict(unet.named_modules())
    assert vidtome_amd.register_attention_maps(unet) == sorted(names)
    assert all(blocks[n].vtm_attention_maps is True for n in names)
    assert vidtome_amd.collect_from_patch(unet, "attn2_probs") == {}           # nothing ran yet
    for n in names:
        blocks[n].attn2_probs = torch.zeros(1)                                 # (what a forward leaves)
    assert sorted(vidtome_amd.collect_from_patch(unet, "attn2_probs")) == sorted(names)
    vidtome_amd.unregister_attention_maps(unet)
    assert not any(hasattr(blocks[n], "vtm_attention_maps") or hasattr(blocks[n], "attn2_probs") for n in names)
    # the pipeline form, and remove_patch
    pipe = standin.Pipe(unet)
    vidtome_amd.register_attention_maps(pipe, names[:2])
    blocks[names[0]].attn2_probs = torch.zeros(1)
    vidtome_amd.remove_patch(pipe)
    assert not any(hasattr(blocks[n], "vtm_attention_maps") or hasattr(blocks[n], "attn2_probs") for n in names)
    with pytest.raises(RuntimeError, match="nothing is patched"):
        vidtome_amd.register_attention_maps(unet)


def test_blocks_accepts_names_and_a_predicate_and_registering_again_changes_the_selection(built):
    import vidtome_amd
    unet = _model(built)
    names = _names(unet)
    blocks = dict(unet.named_modules())
    on = lambda: sorted(n for n in names if getattr(blocks[n], "vtm_attention_maps", False))
    assert vidtome_amd.register_attention_maps(unet, names[2:4]) == sorted(names[2:4]) == on()
    blocks[names[2]].attn2_probs = torch.zeros(1)
    top = lambda name, blk: name.startswith("up_blocks.3.") and blk is blocks[name]
    vidtome_amd.register_attention_maps(unet, top)
    assert on() == sorted(n for n in names if n.startswith("up_blocks.3.")) and len(on()) == 3
    assert not hasattr(blocks[names[2]], "attn2_probs")                        # dropped with the selection
    vidtome_amd.register_attention_maps(unet, names[0])                        # one name
    assert on() == [names[0]]
    with pytest.raises(ValueError, match="not patched blocks"):
        vidtome_amd.register_attention_maps(unet, [names[0], "up_blocks.9.nothing"])
    assert on() == [names[0]]                                                  # a refused call changes nothing
    vidtome_amd.register_attention_maps(unet, [])
    assert on() == []
    vidtome_amd.remove_patch(unet)


def test_default_selection_leaves_a_controlnet_alone(built):
    import vidtome_amd

    class DiffusionPipeline:
        pass

    class StableDiffusionControlNetPipeline(DiffusionPipeline):
        def __init__(self):
            self.unet = standin.StandInUNet(C, 2, full=True, cond_dim=32)
            self.controlnet = standin.StandInUNet(C, 2, full=True, cond_dim=32)
    pipe = StableDiffusionControlNetPipeline()
    vidtome_amd.apply_patch(pipe, include_control=True)
    vidtome_amd.register_attention_maps(pipe)
    flag = lambda root: [getattr(b, "vtm_attention_maps", False) for b in root.blocks()]
    assert all(flag(pipe.unet)) and not any(flag(pipe.controlnet))
    vidtome_amd.register_attention_maps(pipe, lambda name, blk: True)          # the predicate sees a ControlNet's blocks too
    assert all(flag(pipe.controlnet))
    vidtome_amd.unregister_attention_maps(pipe)
    assert not any(flag(pipe.unet)) and not any(flag(pipe.controlnet))


def test_header_declares_and_lib_binds_the_export(built):
    from vidtome_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    decl = re.search(r"int vtm_attention_probs\((.*?)\);", hdr, re.S)
    assert decl and hasattr(ctypes.CDLL(built), "vtm_attention_probs") and "vtm_attention_probs" in _lib.exported_symbols()
    assert len(decl.group(1).split(",")) == len(_lib._SIGNATURES["vtm_attention_probs"][0]) == 19
    assert "vidtome/patch.py:178-183" in hdr[hdr.index("vtm_attention_probs --"):decl.start()]
    assert re.search(r"#define VTM_ABI_VERSION 2\b", hdr) and _lib.lib().vtm_version() == _lib.ABI_VERSION == 2
    assert "attention_probs.hip" in build.SOURCES and callable(_lib.attention_probs)


def test_wrapper_refuses_bad_operands_before_any_launch():
    from vidtome_amd import _lib
    q, k = torch.zeros(2, 16, C), torch.zeros(2, 8, C)
    with pytest.raises(RuntimeError, match="fp16 / bf16"):
        _lib.attention_probs(q, k, 2, 16, 8, 0.125)
    with pytest.raises(RuntimeError, match="fp16 / bf16"):
        _lib.attention_probs(q.half(), k.bfloat16(), 2, 16, 8, 0.125)
    with pytest.raises(RuntimeError, match="on one GPU"):
        _lib.attention_probs(q.half(), k.half(), 2, 16, 8, 0.125)              # host tensors


def _attn(dtype=torch.float32, seed=0):
    a = standin.CrossAttention(C, 2, 32)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in a.parameters():
            if p.ndim == 2:
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[-1] ** -0.5)
    return a.to(dtype)


def test_torch_restatement_against_float64():
    """patch._probs_torch, the evaluation of every route the kernel does not take: fp32, within the kernel's own bound of
    float64 on the same rows; -inf keys are exactly 0."""
    from vidtome_amd import patch as vpatch
    g = torch.Generator().manual_seed(1)
    q, k = torch.randn(3, 20, C, generator=g), torch.randn(3, 77, C, generator=g)
    bias = torch.zeros(3, 77)
    bias[1, 5:40] = float("-inf")
    bias[2, 60:] = -10000.0
    for b in (None, bias):
        got = vpatch._probs_torch(q, k, 2, 32 ** -0.5, b)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, 20, 77)
        assert float((got.double() - AM.probs64(q, k, 2, 32 ** -0.5, b)).abs().max()) <= (77 + 8) * 2.0 ** -24
    assert bool((got[1, :, 5:40] == 0).all()) and bool((got[2, :, 60:] == 0).all())


def test_module_path_map_reads_to_q_and_to_k_or_gives_none():
    from vidtome_amd import patch as vpatch
    a = _attn()
    g = torch.Generator().manual_seed(2)
    x, enc = torch.randn(2, 12, C, generator=g), torch.randn(2, 9, 32, generator=g)
    got = vpatch._module_path_probs(a, x, enc, None)
    ref = AM.probs64(a.to_q(x), a.to_k(enc), 2, a.scale)
    assert tuple(got.shape) == (2, 12, 9) and not got.requires_grad
    assert float((got.double() - ref.detach()).abs().max()) <= 1e-6
    # an IP-Adapter tuple: the text set
    assert torch.equal(vpatch._module_path_probs(a, x, (enc, [torch.zeros(2, 4, 32)]), None), got)
    # a mask of key_bias's form goes along; every other form gives None and one warning, nothing raises
    mask = torch.zeros(2, 1, 9)
    mask[0, 0, 4:] = -10000.0
    masked = vpatch._module_path_probs(a, x, enc, mask)
    assert bool((masked[0, :, 4:] == 0).all()) and torch.equal(masked[1], got[1])
    vpatch._warned.discard("maps-unreadable")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert vpatch._module_path_probs(a, x, enc, torch.zeros(2, 12, 9)) is None        # a per-query mask
        assert vpatch._module_path_probs(a, x, enc, mask == 0) is None                    # a bool mask
        a.norm_cross = torch.nn.LayerNorm(32)
        assert vpatch._module_path_probs(a, x, enc, None) is None                         # something in front of to_k
        a.norm_cross = None
        a.to_q = torch.nn.Sequential(a.to_q)
        assert vpatch._module_path_probs(a, x, enc, None) is None                         # an unreadable projection
    assert len([m for m in w if "attn2_probs is None" in str(m.message)]) == 1
