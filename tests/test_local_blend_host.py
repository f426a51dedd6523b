"""CPU tests of LocalBlend's host side (vidtome_amd.blend): the argument checks, ``word_weights``, the registration and what
clears it, the C-ABI surface of vtm_attention_word_map / vtm_local_blend, and the blend formula (tests/local_blend_standin.py
``blend_formula``, the restatement the GPU test holds vtm_local_blend to) against a literal transcription of
Prompt-to-Prompt's ``LocalBlend.__call__``."""
import ctypes
import os
import re

import pytest
import torch

import local_blend_standin as LB
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
    from vidtome_amd import blend
    assert vidtome_amd.LocalBlend is blend.LocalBlend
    assert vidtome_amd.register_local_blend is blend.register_local_blend
    assert vidtome_amd.unregister_local_blend is blend.unregister_local_blend
    assert {"LocalBlend", "register_local_blend", "unregister_local_blend"} <= set(vidtome_amd.__all__)


def test_local_blend_argument_checks():
    from vidtome_amd import LocalBlend
    w = torch.ones(7)
    lb = LocalBlend({0: w, 2: [0.5] * 7}, num_inputs=3, num_frames=4, threshold=0.25, pool=2)
    assert lb.groups == (0, 2) and lb.K == 7 and lb.weights.dtype == torch.float32 and tuple(lb.weights.shape) == (2, 7)
    assert (lb.num_inputs, lb.num_frames, lb.threshold, lb.pool) == (3, 4, 0.25, 2)
    assert LocalBlend({1: w}, 2, 1).pool == 1 and LocalBlend({1: w}, 2, 1).threshold == 0.3
    for bad in ({3: w}, {-1: w}, {"0": w}, {True: w}, {0.0: w}, {}):
        with pytest.raises(ValueError, match="group"):
            LocalBlend(bad, 3, 4)
    with pytest.raises(ValueError, match="groups"):
        LocalBlend({g: w for g in range(9)}, 9, 4)                                   # more than 8 groups
    for bad in (float("nan"), float("inf"), float("-inf")):
        v = w.clone()
        v[3] = bad
        with pytest.raises(ValueError, match="not finite"):
            LocalBlend({0: v}, 3, 4)
    with pytest.raises(ValueError, match="8 weights"):
        LocalBlend({0: w, 1: torch.ones(8)}, 3, 4)                                   # two lengths
    with pytest.raises(ValueError, match=r"\(K,\) row"):
        LocalBlend({0: torch.ones(2, 7)}, 3, 4)
    for pool in (-1, 4):
        with pytest.raises(ValueError, match="pool"):
            LocalBlend({0: w}, 3, 4, pool=pool)
    with pytest.raises(ValueError, match="threshold"):
        LocalBlend({0: w}, 3, 4, threshold=float("nan"))
    with pytest.raises(ValueError, match="at least 1"):
        LocalBlend({0: w}, 3, 0)


def test_word_weights():
    from vidtome_amd import LocalBlend
    w = LocalBlend.word_weights(77, [2, 5, 76])
    assert w.dtype == torch.float32 and tuple(w.shape) == (77,) and float(w.sum()) == 3.0
    assert w.nonzero().reshape(-1).tolist() == [2, 5, 76]
    assert not bool(LocalBlend.word_weights(4, []).any())
    assert LocalBlend.word_weights(4, torch.tensor([1, 1])).tolist() == [0.0, 1.0, 0.0, 0.0]
    for bad in ([77], [-1], [1.5]):
        with pytest.raises(ValueError, match="token index"):
            LocalBlend.word_weights(77, bad)


def test_frames_maps_and_reset_without_a_forward():
    from vidtome_amd import LocalBlend
    lb = LocalBlend({0: torch.ones(7)}, 2, 4)
    with pytest.raises(RuntimeError, match="nothing accumulated"):
        lb.maps()
    lb.reset()                                                                        # (nothing to zero: no error)
    for bad in ([0, 0], [4], [-1], []):
        with pytest.raises(ValueError, match="set_frames"):
            lb.set_frames(bad)
    lb.set_frames([3, 1])
    assert lb.frame_rows(2, "cpu").tolist() == [3, 1] and lb.frame_rows(2, "cpu").dtype == torch.int64
    with pytest.raises(RuntimeError, match="named 2 frames"):
        lb.frame_rows(3, "cpu")
    lb.set_frames(None)
    assert lb.frame_rows(4, "cpu").tolist() == [0, 1, 2, 3]
    with pytest.raises(RuntimeError, match="set_frames"):
        lb.frame_rows(2, "cpu")
    acc = lb.accumulator(12, "cpu", "blk")
    assert tuple(acc.shape) == (1, 4, 12) and acc.dtype == torch.float32 and not bool(acc.any())
    assert lb.accumulator(12, "cpu", "blk") is acc
    with pytest.raises(RuntimeError, match=r"'blk'.*16 tokens per frame, the accumulator 12"):
        lb.accumulator(16, "cpu", "blk")
    with pytest.raises(ValueError, match="not a square"):
        lb.maps()
    assert tuple(lb.maps(hw=(3, 4)).shape) == (1, 4, 3, 4)
    with pytest.raises(ValueError, match="does not hold"):
        lb.maps(hw=(3, 5))
    acc.fill_(1.0)
    assert lb.maps(hw=(3, 4)).data_ptr() == acc.data_ptr()                            # a view
    lb.reset()
    assert not bool(acc.any())


def test_edited_weights_are_the_linear_form_and_cached():
    """sum_n w[n] P_edit[i, n] = P_src[i, :] . (M (a o w)) + P_own[i, :] . (b o w) for P_edit = a (P_src M) + b P_own."""
    from vidtome_amd import CrossEdit, LocalBlend
    K = 9
    g = torch.Generator().manual_seed(0)
    e = CrossEdit(torch.randn(K, K, generator=g), torch.randn(K, generator=g), torch.randn(K, generator=g))
    lb = LocalBlend({0: torch.randn(K, generator=g), 1: torch.randn(K, generator=g)}, 2, 1)
    w_src, w_own = lb.edited_weights(e, 1, "cpu")
    assert tuple(w_src.shape) == tuple(w_own.shape) == (1, K) and w_src.dtype == torch.float32
    p_src, p_own = torch.rand(5, K, generator=g).double(), torch.rand(5, K, generator=g).double()
    M, a, b, w = e.mapper.double(), e.src_weight.double(), e.own_weight.double(), lb.weights[1].double()
    edited = (p_src @ M) * a + p_own * b
    assert float((edited @ w - (p_src @ w_src[0].double() + p_own @ w_own[0].double())).abs().max()) < 1e-5
    assert lb.edited_weights(e, 1, "cpu")[0] is w_src                                 # once per (edit, words) pair
    assert lb.edited_weights(CrossEdit.identity(K), 1, "cpu")[0] is not w_src


def test_register_unregister_and_remove_patch(built):
    import vidtome_amd
    unet = _model(built)
    names = _names(unet)
    blocks = dict(unet.named_modules())
    lb = vidtome_amd.LocalBlend({0: torch.ones(7)}, 2, 4)
    on = lambda: sorted(n for n in names if "vtm_local_blend" in blocks[n].__dict__)
    assert vidtome_amd.register_local_blend(unet, lb) == sorted(names) == on()
    assert all(blocks[n].vtm_local_blend == (lb, n) for n in names)
    # selection forms: names, one name, a predicate; registering again replaces lb and the selection
    assert vidtome_amd.register_local_blend(unet, lb, names[2:4]) == sorted(names[2:4]) == on()
    other = vidtome_amd.LocalBlend({1: torch.ones(7)}, 2, 4)
    assert vidtome_amd.register_local_blend(unet, other, names[0]) == [names[0]] == on()
    assert blocks[names[0]].vtm_local_blend[0] is other
    top = lambda name, blk: name.startswith("up_blocks.3.") and blk is blocks[name]
    vidtome_amd.register_local_blend(unet, lb, top)
    assert on() == sorted(n for n in names if n.startswith("up_blocks.3.")) and len(on()) == 3
    with pytest.raises(ValueError, match="not patched blocks"):
        vidtome_amd.register_local_blend(unet, lb, [names[0], "up_blocks.9.nothing"])
    assert len(on()) == 3                                                             # a refused call changes nothing
    with pytest.raises(TypeError, match="LocalBlend"):
        vidtome_amd.register_local_blend(unet, {0: torch.ones(7)})
    # beside the other two switches, and cleared on its own
    vidtome_amd.register_attention_maps(unet)
    vidtome_amd.register_cross_attention_control(unet, [981], 2, {1: vidtome_amd.CrossEdit.identity(7)})
    vidtome_amd.unregister_local_blend(unet)
    assert on() == [] and all(blocks[n].vtm_attention_maps and "vtm_cross_control" in blocks[n].__dict__ for n in names)
    # the pipeline form, and remove_patch
    pipe = standin.Pipe(unet)
    vidtome_amd.register_local_blend(pipe, lb, names[:2])
    assert on() == sorted(names[:2])
    vidtome_amd.remove_patch(pipe)
    assert on() == []
    with pytest.raises(RuntimeError, match="nothing is patched"):
        vidtome_amd.register_local_blend(unet, lb)


def test_header_declares_and_lib_binds_the_exports(built):
    from vidtome_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    lib = ctypes.CDLL(built)
    for name, nargs in (("vtm_attention_word_map", 24), ("vtm_local_blend", 16)):
        decl = re.search(r"int %s\((.*?)\);" % name, hdr, re.S)
        assert decl and hasattr(lib, name) and name in _lib.exported_symbols()
        assert len(decl.group(1).split(",")) == len(_lib._SIGNATURES[name][0]) == nargs
    words = re.search(r"int vtm_attention_word_map\(", hdr)
    assert "vidtome/patch.py:178-183" in hdr[hdr.index("vtm_attention_word_map --"):words.start()]
    assert "LocalBlend" in hdr[hdr.index("vtm_attention_word_map --"):words.start()]
    declared = set(re.findall(r"\b(vtm_[a-z_0-9]+)\s*\(", hdr)) - {"vtm_match_row_pad"}
    assert declared == set(_lib.exported_symbols())
    assert re.search(r"#define VTM_ABI_VERSION 2\b", hdr) and _lib.lib().vtm_version() == _lib.ABI_VERSION == 2
    assert {"attention_words.hip", "local_blend.hip"} <= set(build.SOURCES)
    assert callable(_lib.attention_word_map) and callable(_lib.local_blend)


def test_new_kernels_do_not_spill(built):
    from vidtome_amd import build
    """Every instantiation (9 head dims x 2 dtypes; 2 element sizes): no scratch, no spilled register."""
    for src, kernel, count in (("attention_words", "attention_words_kernel", 18), ("local_blend", "local_blend_kernel", 2)):
        res = {k: v for k, v in build.kernel_resources(os.path.join(os.path.dirname(built), src + ".o")).items() if kernel in k}
        assert len(res) == count, sorted(res)
        for name, r in res.items():
            assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)


def test_wrappers_refuse_bad_operands_before_any_launch():
    from vidtome_amd import _lib
    q, k = torch.zeros(2, 16, C), torch.zeros(2, 8, C)
    w, out = torch.ones(1, 8), torch.zeros(2, 16)
    with pytest.raises(RuntimeError, match="fp16 / bf16"):
        _lib.attention_word_map(q, k, 2, 16, 8, 0.125, w, out)
    with pytest.raises(RuntimeError, match="on one GPU"):
        _lib.attention_word_map(q.half(), k.half(), 2, 16, 8, 0.125, w, out)          # host tensors
    with pytest.raises(RuntimeError, match="acc must be"):
        _lib.local_blend(torch.zeros(2, 3, 4, 4), torch.zeros(3, 4, 8, 8), torch.zeros(3, 4, 8, 8), 1, 0.3)


# ---------------------------------------------------------------------------------------------------
# the blend formula against Prompt-to-Prompt's LocalBlend.__call__
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(3, 4, 4, 8, 8, 1, 0.3), (2, 16, 16, 64, 64, 1, 0.3), (2, 5, 3, 10, 9, 1, 0.6), (2, 12, 9, 24, 27, 2, 0.6),
                                  (1, 8, 8, 8, 8, 0, 0.45)], ids=lambda c: "x".join(map(str, c)))
def test_formula_is_p2ps_local_blend(case):
    """P2P: max_pool2d -> nearest interpolate -> divide by the maximum -> gt(threshold) -> OR of the two prompts -> x_src +
    mask (x - x_src), per frame, the source prompt's map and the edited prompt's as the two groups.  ``blend_formula`` pools,
    looks the cell up, compares ``pooled > threshold * max`` and selects.  The two agree wherever the comparison is not a
    tie of roundings -- the inputs are first checked to have no pooled value within 1e-6 (relative) of threshold * max --
    and wherever the arithmetic blend does not round: the latents here are multiples of 1 / 8 below 8 in magnitude, whose
    differences and sums fp32 holds exactly (a 16-bit dtype would round them: the kernel's select does not)."""
    Fr, h, w, H, W, pool, thr = case
    g = torch.Generator().manual_seed(sum(case[:6]))
    acc = torch.rand(2, Fr, h, w, generator=g) ** 8                                  # (groups: the source, the edited prompt)
    x = torch.randint(-63, 64, (Fr, 4, H, W), generator=g).float() / 8
    x_src = torch.randint(-63, 64, (Fr, 4, H, W), generator=g).float() / 8
    pooled = torch.nn.functional.max_pool2d(acc, 2 * pool + 1, stride=1, padding=pool)
    cut = thr * acc.amax(dim=(2, 3), keepdim=True).double()
    assert float(((pooled.double() - cut).abs() / cut).min()) > 1e-6, "a pooled value sits on the threshold"
    out, mask = LB.blend_formula(acc, x, x_src, pool, thr)
    assert 0 < int(mask.sum()) < mask.numel()
    for f in range(Fr):
        x_t = torch.stack([x_src[f], x[f]])                                           # prompt 0 is the source
        want, want_mask = LB.p2p_local_blend(acc[:, f, None], x_t, pool, thr)
        assert torch.equal(mask[f], want_mask[0, 0].bool()), f
        assert torch.equal(out[f], want[1]) and torch.equal(want[0], x_src[f]), f


def test_formula_gives_an_empty_mask_for_an_all_zero_map():
    """P2P divides 0 by 0 there: NaN > threshold is false.  threshold * 0 = 0 and 0 > 0 is false as well."""
    acc = torch.zeros(2, 1, 4, 4)
    acc[1, 0, 1, 2] = 1.0
    x, x_src = torch.ones(1, 4, 8, 8), torch.zeros(1, 4, 8, 8)
    out, mask = LB.blend_formula(acc, x, x_src, 1, 0.3)
    _, only = LB.blend_formula(acc[1:], x, x_src, 1, 0.3)
    assert torch.equal(mask, only) and int(mask.sum()) == 9 * 4                      # the 3 x 3 window, 2 x 2 pixels a cell
    want, want_mask = LB.p2p_local_blend(acc[:, 0, None], torch.stack([x_src[0], x[0]]), 1, 0.3)
    assert torch.equal(mask[0], want_mask[0, 0].bool()) and torch.equal(out[0], want[1])
    assert not bool(LB.blend_formula(torch.zeros(2, 1, 4, 4), x, x_src, 1, 0.3)[1].any())
