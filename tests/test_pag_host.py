"""CPU tests of the perturbed-attention (PAG) host side: vidtome_amd.pag's recogniser, split and registration, what clears the
marker, and attn1's routing with a PAG processor (patch.attn1_route).  No GPU, no launch."""
import pytest
import torch

import pag_standin as PS
import standin

C, HEADS, N = 64, 2, 16


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


class FakeCuda(torch.Tensor):          # the predicates need x.is_cuda; emulate it without a device
    @property
    def is_cuda(self):
        return True


def _x(B=3, dtype=torch.float16):
    return torch.zeros(B, N, C, dtype=dtype).as_subclass(FakeCuda)


def _block(name=None, dtype=torch.float16):
    blk = standin.BasicTransformerBlock(C, HEADS).to(dtype)
    if name is not None:
        blk.attn1 = PS.PAGAttention(blk.attn1, PS.PROCESSOR_CLASSES[name]())
    return blk


def test_groups_of_by_name_and_by_marker():
    from vidtome_amd import pag
    assert pag.groups_of(_block().attn1) is None
    assert pag.groups_of(_block("PAGIdentitySelfAttnProcessor2_0").attn1) == 2
    assert pag.groups_of(_block("PAGCFGIdentitySelfAttnProcessor2_0").attn1) == 3
    for unknown in ("PAGHunyuanAttnProcessor2_0", "PAGJointAttnProcessor2_0"):
        assert pag.groups_of(_block(unknown).attn1) is None
    plain = _block()
    plain.attn1 = PS.PAGAttention(plain.attn1, PS.PlainProcessor())
    assert type(plain.attn1.processor).__name__ == "AttnProcessor2_0" and pag.groups_of(plain.attn1) is None
    for g in (2, 3):
        plain.attn1.__dict__[pag.MARK] = g
        assert pag.groups_of(plain.attn1) == g and pag.registered(plain.attn1) == g
    del plain.attn1.__dict__[pag.MARK]
    assert pag.groups_of(plain.attn1) is None and pag.registered(plain.attn1) is None
    assert pag.registered(_block("PAGCFGIdentitySelfAttnProcessor2_0").attn1) is None


def test_split_sizes_and_errors():
    from vidtome_amd import pag
    assert pag.split(3, 3) == (2, 1)
    assert pag.split(4, 2) == (2, 2)
    assert pag.split(12, 3) == (8, 4)          # un-merged site: 3 samples of 4 frames, the last sample's frames perturbed
    assert pag.split(2, 2) == (1, 1)
    assert pag.split(48, 3) == (32, 16)
    for B, g in ((4, 3), (3, 2), (0, 3), (5, 2), (-3, 3)):
        with pytest.raises(ValueError, match="does not split"):
            pag.split(B, g)
    for g in (1, 4, 0, None):
        with pytest.raises(ValueError, match="2 or 3"):
            pag.split(6, g)


def _names(unet):
    from vidtome_amd import pag
    return sorted(n for n, m in unet.named_modules() if m.__class__.__name__ == "ToMeBlock" and pag.registered(m.attn1))


def test_register_remove_and_remove_patch(built):
    import vidtome_amd
    from vidtome_amd import pag
    unet = standin.StandInUNet(C, HEADS)
    with pytest.raises(RuntimeError, match="nothing is patched"):
        vidtome_amd.register_perturbed_attention(unet)
    vidtome_amd.apply_patch(unet, batch_size=3)
    every = sorted(n for n, m in unet.named_modules() if m.__class__.__name__ == "ToMeBlock")
    assert len(every) == 9
    with pytest.raises(ValueError, match="no patched block"):
        vidtome_amd.register_perturbed_attention(unet)                          # the stand-in has no "mid" block
    up1 = [n for n in every if n.startswith("up_blocks.1.")]
    assert vidtome_amd.register_perturbed_attention(unet, layers=("up_blocks.1",)) == up1 == _names(unet)
    assert all(pag.groups_of(m.attn1) == 3 for n, m in unet.named_modules() if n in up1)
    # registering again only changes the selection (a string is one layer name; the pipeline form)
    assert vidtome_amd.register_perturbed_attention(standin.Pipe(unet), "up_blocks.2.attentions.0", groups=2) == _names(unet)
    assert _names(unet) == ["up_blocks.2.attentions.0.transformer_blocks.0"]
    blk = dict(unet.named_modules())[_names(unet)[0]]
    assert pag.groups_of(blk.attn1) == 2
    for bad in (1, 4, True, None, 2.5):
        with pytest.raises(ValueError, match="2 or 3"):
            vidtome_amd.register_perturbed_attention(unet, "up_blocks", groups=bad)
    assert len(_names(unet)) == 1                                               # a refused call changes nothing
    vidtome_amd.remove_perturbed_attention(unet)
    assert _names(unet) == []
    assert len(vidtome_amd.register_perturbed_attention(unet, ("up_blocks.1", "up_blocks.3"))) == 6
    attns = [m.attn1 for m in unet.modules() if m.__class__.__name__ == "ToMeBlock"]
    vidtome_amd.remove_patch(unet)
    assert all(pag.MARK not in a.__dict__ for a in attns)                       # remove_patch cleared the markers


def test_register_raises_under_pnp_sharing(built):
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    unet = standin.StandInUNet(C, HEADS)
    vidtome_amd.apply_patch(unet, batch_size=3)
    blk = next(m for m in unet.modules() if m.__class__.__name__ == "ToMeBlock")
    blk.attn1.injection_schedule, blk.attn1.t, blk.attn1.vtm_num_inputs = [981], 981, 3
    assert vpatch._pnp_share_groups(blk.attn1) == 3
    with pytest.raises(RuntimeError, match="PnP"):
        vidtome_amd.register_perturbed_attention(unet, "up_blocks")
    assert _names(unet) == []
    blk.attn1.t = 500                                                           # not an injecting step: nothing is shared
    assert len(vidtome_amd.register_perturbed_attention(unet, "up_blocks")) == 9
    vidtome_amd.remove_patch(unet)


@pytest.mark.parametrize("name,B", [("PAGIdentitySelfAttnProcessor2_0", 4), ("PAGCFGIdentitySelfAttnProcessor2_0", 3)])
def test_route_of_a_pag_block(name, B):
    """A PAG processor keeps the plain block's route; a mask, processor kwargs, attn1 as a cross-attention, an AdaLayerNormZero
    gate, PnP sharing or a batch that does not split send it to the module."""
    from vidtome_amd import patch as vpatch
    blk, x = _block(name), _x(B)
    assert vpatch.attn1_route(blk, x) == vpatch.attn1_route(_block(), x) == "rows"
    assert vpatch.attn1_route(blk, x, None, torch.zeros(B, 1, N, dtype=torch.float16)) == "module"
    assert vpatch.attn1_route(blk, x, None, None, {"scale": 1.0}) == "module"
    assert vpatch.attn1_route(blk, x, None, None, {"ip_adapter_masks": [None]}) == "rows"
    assert vpatch.attn1_route(blk, x, gate_msa=torch.zeros(B, C)) == "module"
    assert vpatch.attn1_route(_block(), x, gate_msa=torch.zeros(B, C)) == "rows"      # the gate alone changes no plain route
    enc = torch.zeros(B, 77, C, dtype=torch.float16)
    assert vpatch.attn1_route(blk, x, enc) == "rows"
    blk.only_cross_attention = True
    assert vpatch.attn1_route(blk, x, enc) == "module"
    blk.only_cross_attention = False
    assert vpatch.attn1_route(blk, _x(B + 1)) == "module"                              # Diffusers raises there
    blk.attn1.injection_schedule, blk.attn1.t, blk.attn1.vtm_num_inputs = [981], 981, B
    assert vpatch.attn1_route(blk, x) == "module"
    blk.attn1.t = 500
    assert vpatch.attn1_route(blk, x) == "rows"
    f32 = _block(name, torch.float32)
    assert vpatch.attn1_route(f32, _x(B, torch.float32)) == "blas"
    f32.fp32_projections = True
    assert vpatch.attn1_route(f32, _x(B, torch.float32)) == "f32"


def test_unknown_pag_processors_take_the_module_path():
    from vidtome_amd import patch as vpatch
    for unknown in ("PAGHunyuanAttnProcessor2_0", "PAGJointAttnProcessor2_0"):
        assert vpatch.attn1_route(_block(unknown), _x()) == "module"
    assert not vpatch.fused_attention_ok(_block("PAGCFGIdentitySelfAttnProcessor2_0").attn1, _x())   # attn2 / other callers:
    # the PAG names are accepted for attn1 alone


def test_batch_attn1_sees(built):
    """The leading batch the split is taken over: ``batch_size`` where the site merges, the frame rows where it does not."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    blk = _block("PAGCFGIdentitySelfAttnProcessor2_0")
    x = _x(8)                                                                          # 8 frame rows of 16 tokens
    assert vpatch._pag_batch(blk, x) == 8                                              # nothing patched
    blk._tome_info = {"size": (4, 4), "args": {"max_downsample": 1, "batch_size": 3}}  # 16 tokens of 16: the site merges
    assert vpatch._pag_batch(blk, x) == 3 and vpatch.attn1_route(blk, x) == "rows"
    blk._tome_info["args"]["batch_size"] = 2
    assert vpatch.attn1_route(blk, x) == "module"                                      # 2 samples do not split in 3
    blk._tome_info["size"] = (8, 8)                                                    # 16 tokens of 64: un-merged
    assert vpatch._pag_batch(blk, x) == 8 and vpatch.attn1_route(blk, x) == "module"   # 8 frames do not split in 3
    assert vpatch._pag_batch(blk, _x(12)) == 12 and vpatch.attn1_route(blk, _x(12)) == "rows"
    # the registered form keeps its route and raises before any launch
    reg = _block()
    reg._tome_info = {"size": (4, 4), "args": {"max_downsample": 1, "batch_size": 2}}
    reg.attn1.__dict__["vtm_pag_groups"] = 3
    assert vpatch.attn1_route(reg, x) == "rows"
    from vidtome_amd import _lib
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
        with pytest.raises(ValueError, match="does not split"):
            vpatch.self_attention_segment(reg, x)
        with pytest.raises(ValueError, match="does not split"):
            vpatch.patched_self_attention_segment(reg, x, x)
