"""CPU tests of IP-Adapter region masks in the recogniser (vidtome_amd/ip_adapter.py, patch.ip_cross_call): the published
4-D form gives a Call with per-image rows of query weights, everything else keeps the module path; the key-set layout of
masked / unmasked / scale-0 adapters; the rows are the processor's own downsample, bit for bit."""
import os

import torch

import ip_adapter_mask_standin as mstand
import ip_adapter_standin as ustand
import standin
from ip_adapter_standin import IPAttention, image_states

C, HEADS, D, B, N, T = 64, 2, 64, 2, 16, 77


class FakeCuda(torch.Tensor):          # the predicates need x.is_cuda; emulate it without a device
    @property
    def is_cuda(self):
        return True


def _attn(num_tokens=(4, 16), scale=(0.7, 0.3), classes=mstand.PROCESSOR_CLASSES, name="IPAdapterAttnProcessor2_0"):
    src = standin.CrossAttention(C, HEADS, D)
    return IPAttention(src, classes[name](C, D, num_tokens, scale)).half()


def _x(n=N):
    return torch.zeros(B, n, C, dtype=torch.float16).as_subclass(FakeCuda)


def _enc(num_tokens=(4, 16), images=(1, 1)):
    """(text, one (B, m_a, T_a, D) tensor per adapter; m_a = 0: the 3-D form (B, T_a, D))."""
    ims = []
    for t, m in zip(num_tokens, images):
        im = image_states((t,), B, D, torch.float16, "cpu", images=max(m, 2))[0][:, :max(m, 1)]
        ims.append(im[:, 0] if m == 0 else im)
    return torch.zeros(B, T, D, dtype=torch.float16), ims


def _masks(images=(1, 1), hw=(8, 8), seed=0):
    g = torch.Generator().manual_seed(seed)
    return [None if m is None else torch.rand(1, m, *hw, generator=g) for m in images]


def _call(a, enc, masks, x=None, mask=None, norm=None):
    from vidtome_amd import patch as vpatch
    return vpatch.ip_cross_call(a, _x() if x is None else x, enc, mask, {"ip_adapter_masks": masks}, norm)


def test_published_masks_give_a_call_with_rows_of_the_processors_own_downsample():
    for name in mstand.PROCESSOR_CLASSES:
        a = _attn(name=name)
        masks = _masks((1, 3), hw=(8, 8))
        ip = _call(a, _enc(images=(1, 3)), masks)
        assert ip is not None and ip.scales == [0.7, 0.3]
        assert [tuple(i.shape) for i in ip.images] == [(B, 4, D), (B, 48, D)]      # all m_a * T_a tokens, one GEMM
        assert [tuple(r.shape) for r in ip.masks] == [(1, N), (3, N)] and all(r.dtype == torch.float32 for r in ip.masks)
        for m, rows in zip(masks, ip.masks):
            for i in range(m.shape[1]):
                want = mstand.IPAdapterMaskProcessor.downsample(m[:, i], 1, N, 1).reshape(N)
                assert torch.equal(rows[i], want)
    # the panel dispatch asks the same (norm2 given), and a mask of another resolution and aspect is the downsample's business
    a = _attn()
    masks = _masks((1, 1), hw=(12, 12))
    ip = _call(a, _enc(), masks, norm=torch.nn.LayerNorm(C).half())
    assert ip is not None
    assert torch.equal(ip.masks[1][0], mstand.IPAdapterMaskProcessor.downsample(masks[1][:, 0], 1, N, 1).reshape(N))
    wide = [torch.rand(1, 1, 4, 16), None]                                        # 32 tokens as 2 x 8... the mask's aspect
    ip = _call(a, _enc(), wide, x=_x(32))
    assert torch.equal(ip.masks[0][0], mstand.IPAdapterMaskProcessor.downsample(wide[0][:, 0], 1, 32, 1).reshape(32))
    assert ip.masks[1] is None


def test_none_entries_and_zero_scales():
    a = _attn()
    ip = _call(a, _enc(images=(0, 2)), _masks((None, 2)))                          # an unmasked 3-D adapter next to a masked one
    assert ip is not None and ip.masks[0] is None and tuple(ip.masks[1].shape) == (2, N)
    assert _call(a, _enc(), [None, None]).masks is None                            # all None: the unmasked call, as before
    a.processor.scale = [0.0, 0.3]                                                 # a masked adapter of scale 0 takes no part
    ip = _call(a, _enc(images=(2, 1)), _masks((2, 1)))
    assert ip is not None and ip.masks[0] is None and tuple(ip.masks[1].shape) == (1, N)


def test_what_keeps_the_module_path():
    ok_enc, ok_masks = _enc(images=(1, 1)), _masks((1, 1))
    assert _call(_attn(), ok_enc, ok_masks) is not None
    refused = {
        "a 3-D mask": (_attn(), ok_enc, [torch.ones(1, N, 1), None]),
        "a 3-D mask behind a 4-D one": (_attn(), ok_enc, [ok_masks[0], torch.ones(1, N, 1)]),
        "shape[0] != 1": (_attn(), ok_enc, [torch.ones(2, 1, 8, 8), None]),
        "shape[1] != m_a": (_attn(), _enc(images=(2, 1)), [torch.ones(1, 3, 8, 8), None]),
        "a 3-D image tensor with a mask": (_attn(), _enc(images=(0, 1)), ok_masks),
        "fewer masks than adapters": (_attn(), ok_enc, ok_masks[:1]),
        "a tensor instead of a list": (_attn(), ok_enc, torch.ones(2, 1, 8, 8)),
        "an integer mask": (_attn(), ok_enc, [torch.ones(1, 1, 8, 8, dtype=torch.int32), None]),
        "9 sets": (_attn(), _enc(images=(4, 4)), _masks((4, 4))),
        "9 sets, one adapter unmasked": (_attn(), _enc(images=(7, 2)), _masks((7, None))),
        "a processor whose module has no IPAdapterMaskProcessor": (_attn(classes=ustand.PROCESSOR_CLASSES), ok_enc, ok_masks),
    }
    a = _attn()
    a.processor.scale = [0.7, [0.3]]
    refused["a list-valued scale"] = (a, ok_enc, ok_masks)
    a = _attn()
    a.processor.scale = [[0.7], 0.3]
    refused["a list-valued scale on the masked adapter"] = (a, ok_enc, [ok_masks[0], None])
    for what, (a, enc, masks) in refused.items():
        assert _call(a, enc, masks) is None, what
    assert _call(_attn(), _enc(images=(4, 3)), _masks((4, 3))) is not None         # 1 + 4 + 3 = 8 sets fit
    assert _call(_attn(), ok_enc, ok_masks, mask=torch.zeros(B, 1, T)) is None     # an attention_mask
    from vidtome_amd import patch as vpatch
    assert vpatch.ip_cross_call(_attn(), _x(), ok_enc, None, {"ip_adapter_masks": ok_masks, "scale": 1.0}) is None
    a32 = _attn().float()                                                          # fp32 models
    enc32 = (ok_enc[0].float(), [i.float() for i in ok_enc[1]])
    assert vpatch.ip_cross_call(a32, _x().float().as_subclass(FakeCuda), enc32, None, {"ip_adapter_masks": ok_masks}) is None


def test_a_downsample_of_another_shape_keeps_the_module_path(monkeypatch):
    a = _attn()
    enc, masks = _enc(), _masks((1, 1))
    monkeypatch.setattr(mstand.IPAdapterMaskProcessor, "downsample",
                        staticmethod(lambda m, b, n, c: torch.ones(1, n + 1, 1)))
    assert _call(a, enc, masks) is None
    monkeypatch.setattr(mstand, "IPAdapterMaskProcessor", object())
    assert _call(a, enc, masks) is None


def test_masked_key_sets_layout():
    from vidtome_amd import ip_adapter
    mk = ip_adapter.masked_key_sets
    # no masked adapter: key_sets, every row -1
    assert mk(77, [4, 16], [0.7, 0.3], [0, 0]) == ([(0, 77, 1.0), (80, 4, 0.7), (88, 16, 0.3)], [0, 1], 104, [-1, -1, -1])
    # one image each, both masked
    assert mk(77, [16, 4], [1.0, 0.6], [1, 1]) == ([(0, 77, 1.0), (80, 16, 1.0), (96, 4, 0.6)], [0, 1], 104, [-1, 0, 1])
    # masked (3 images of 4 tokens: a set each, each on a multiple of 8) / unmasked (2 images share one set) / masked
    assert mk(77, [12, 32, 257], [0.7, -0.3, 1.5], [3, 0, 1]) == (
        [(0, 77, 1.0), (80, 4, 0.7), (88, 4, 0.7), (96, 4, 0.7), (104, 32, -0.3), (136, 257, 1.5)], [0, 1, 2], 400,
        [-1, 0, 1, 2, -1, 3])
    # a masked adapter of scale 0 takes no keys and no rows; the later ones close up
    assert mk(77, [8, 16, 20], [0.0, 0.3, 0.5], [2, 0, 2]) == (
        [(0, 77, 1.0), (80, 16, 0.3), (96, 10, 0.5), (112, 10, 0.5)], [1, 2], 128, [-1, -1, 0, 1])
    assert mk(154, [8], [0.0], [2]) == ([(0, 154, 1.0)], [], 160, [-1])
    for sets, _, end, rows in (mk(77, [12, 32, 257], [1.0, 1.0, 1.0], [3, 2, 1]), mk(80, [24], [1.0], [3])):
        assert all(s % 8 == 0 for s, _, _ in sets) and end % 8 == 0 and len(rows) == len(sets)
        assert all(a[0] + a[1] <= b[0] for a, b in zip(sets, sets[1:])) and sets[-1][0] + sets[-1][1] <= end


def test_operands_place_every_image_on_a_multiple_of_8_keys():
    """patch._ip_key_sets on the CPU (library GEMMs): 3 images of 4 tokens projected in one GEMM, then one set per image;
    the rows of k / v^T of every set are the projection of that image's tokens, the table is the Call's rows in set order."""
    from vidtome_amd import patch as vpatch
    a = _attn()
    enc, masks = _enc(images=(3, 0)), _masks((3, None))
    ip = vpatch.ip_cross_call(a, _x(), enc, None, {"ip_adapter_masks": masks})
    k, vt, sets, rows, table = vpatch._ip_key_sets(a.float(), ip, torch.float32, C, False)
    assert sets == [(0, 77, 1.0), (80, 4, 0.7), (88, 4, 0.7), (96, 4, 0.7), (104, 16, 0.3)] and rows == [-1, 0, 1, 2, -1]
    assert tuple(k.shape) == (B, 120, C) and tuple(vt.shape) == (B, C, 120)
    assert torch.equal(table, ip.masks[0]) and table.is_contiguous()
    proc = a.processor
    for i in range(3):
        s = sets[1 + i][0]
        im = enc[1][0][:, i].float()
        assert torch.allclose(k[:, s:s + 4], proc.to_k_ip[0](im), atol=1e-5)
        assert torch.allclose(vt[:, :, s:s + 4], proc.to_v_ip[0](im).transpose(1, 2), atol=1e-5)
    assert torch.allclose(k[:, 104:120], proc.to_k_ip[1](enc[1][1].float()), atol=1e-5)
    # a call whose masked adapters all have scale 0 carries no table: the unmasked launch
    a = _attn()
    a.processor.scale = [0.0, 0.3]
    ip = vpatch.ip_cross_call(a, _x(), enc, None, {"ip_adapter_masks": masks})
    assert vpatch._ip_key_sets(a.float(), ip, torch.float32, C, False)[2:] == ([(0, 77, 1.0), (80, 16, 0.3)], None, None)


def test_region_masks_do_not_reach_attn1():
    from vidtome_amd import patch as vpatch
    assert vpatch._attn1_kwargs({"ip_adapter_masks": [None]}) == {} and vpatch._attn1_kwargs(None) == {}
    assert vpatch._attn1_kwargs({"ip_adapter_masks": [None], "scale": 0.5}) == {"scale": 0.5}


def test_header_declares_and_lib_binds_the_masked_export():
    from vidtome_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vidtome_hip.h")).read()
    assert "int vtm_attention_kv_sets_masked(" in hdr and "vtm_attention_kv_sets_masked" in _lib.exported_symbols()
    assert "#define VTM_ABI_VERSION 2" in hdr                    # the export is additive: the ABI version stays
