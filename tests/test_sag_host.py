"""CPU tests of self-attention guidance: the C-ABI surface of vtm_attention_key_mass / vtm_sag_degrade (declarations, every
VTM_EINVAL path without a launch), the float64 restatement of tests/sag_standin.py against torch's own reflect padding,
conv2d and nearest interpolation at every shape the GPU tests use, the group-weight algebra, and the host semantics of
vidtome_amd.sag (register / unregister / remove_patch, the raise rules, the mass grid)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sag_standin as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NEW = ("vtm_attention_key_mass", "vtm_attention_key_mass_ws_bytes", "vtm_sag_degrade")
# the (H, W, h_m, w_m) of tests/test_gpu_sag.py
GRIDS = [(64, 64, 8, 8), (96, 96, 12, 12), (40, 72, 5, 9), (60, 60, 8, 8), (5, 5, 1, 1), (128, 128, 16, 16)]


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


def test_header_declares_exactly_the_exports_and_the_version_stays(built):
    from vidtome_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    declared = set(re.findall(r"\b(vtm_[a-z_0-9]+)\s*\(", hdr)) - {"vtm_match_row_pad"}
    lib = ctypes.CDLL(built)
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _lib.exported_symbols(), name
        assert re.search(r"^(int|size_t) " + name + r"\(", hdr, re.M), name
    assert declared == set(_lib.exported_symbols())
    assert "#define VTM_ABI_VERSION 2" in hdr and _lib.lib().vtm_version() == _lib.ABI_VERSION == 2
    assert {"attention_mass.hip", "sag.hip"} <= set(build.SOURCES)
    assert callable(_lib.attention_key_mass) and callable(_lib.sag_degrade)
    assert (_lib.KEY_MASS_MAX_KEYS, _lib.KEY_MASS_MAX_QUERIES, _lib.SAG_MAX_RADIUS, _lib.SAG_MAX_PLANE) == (4096, 65536, 4, 16384)


def test_new_kernels_use_no_scratch(built):
    """The compiler's resource figures (profiles/attention_mass_resources.txt): no scratch, no spills, two workgroups of the
    key-mass kernel per CU (<= 256 VGPRs, <= 80 KB of LDS)."""
    from vidtome_amd import build
    res = build.kernel_resources(os.path.join(os.path.dirname(built), "attention_mass.o"))
    mass = {k: v for k, v in res.items() if "attention_mass_kernel" in k}
    assert len(mass) == 18, sorted(mass)                                   # 9 head dims x fp16 / bf16
    for k, v in list(mass.items()) + list(build.kernel_resources(os.path.join(os.path.dirname(built), "sag.o")).items()):
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
        assert v["vgpr_count"] <= 256 and v.get("group_segment_fixed_size", 0) <= 80 * 1024, (k, v)


def test_key_mass_einval_paths_answer_without_a_launch(built):
    """No GPU here: a call that got as far as a launch would fail differently (VTM_ELAUNCH) or crash on the fake pointers."""
    from vidtome_amd import _lib
    L = _lib.lib()
    P, P2, O = 0x10000, 0x20000, 0x30000
    ok = dict(q=P, ldq=960, k=P2, ldk=960, out=O, ldo=64, dtype=_lib.VTM_F16, B=2, h=8, Mq=64, Mqp=64, Mk=64, Mkp=64, d=40,
              scale=40 ** -0.5, ws=None, ws_bytes=0)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vtm_attention_key_mass(a["q"], a["ldq"], a["k"], a["ldk"], a["out"], a["ldo"], a["dtype"], a["B"], a["h"],
                                        a["Mq"], a["Mqp"], a["Mk"], a["Mkp"], a["d"], a["scale"], a["ws"], a["ws_bytes"], None)
    bad = [dict(q=None), dict(k=None), dict(out=None), dict(q=P + 8), dict(k=P2 + 2), dict(out=O + 2), dict(B=0), dict(h=0),
           dict(Mq=0), dict(Mk=0), dict(Mqp=63), dict(Mkp=63), dict(d=0), dict(Mk=4097, Mkp=4097, ldo=4097),
           dict(Mq=65537, Mqp=65537), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")),
           dict(dtype=_lib.VTM_F32), dict(dtype=9), dict(ldq=324), dict(ldk=324), dict(ldq=312), dict(ldo=63), dict(d=24, h=4),
           dict(Mq=129, Mqp=129), dict(Mq=129, Mqp=129, ws=0x40000, ws_bytes=2 * 2 * 64 * 4 - 1),
           dict(Mq=129, Mqp=129, ws=0x40002, ws_bytes=1 << 20), dict(Mk=4096, Mkp=4096, ldo=4096, ldk=1 << 19)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert L.vtm_last_error().startswith(b"vtm_attention"), kw
    ws = L.vtm_attention_key_mass_ws_bytes
    assert ws(2, 128, 64) == 0 and ws(1, 1, 1) == 0
    assert ws(2, 129, 64) == 2 * 2 * 64 * 4 and ws(1, 1024, 1024) == 8 * 1024 * 4 and ws(3, 65536, 4096) == 3 * 512 * 4096 * 4
    assert ws(0, 64, 64) == 0 and ws(1, 65537, 64) == 0 and ws(1, 200, 4097) == 0


def test_sag_degrade_einval_paths_answer_without_a_launch(built):
    from vidtome_amd import _lib
    L = _lib.lib()
    taps = (ctypes.c_float * 9)(*_lib.gaussian_taps(4, 1.0))
    X, M, MASS, O = 0x10000, 0x200000, 0x400000, 0x600000
    ok = dict(x=X, n_rows=4, ids=None, m=M, mass=MASS, ld=64, h_m=8, w_m=8, dtype=_lib.VTM_F16, F=2, C=4, H=64, W=64, pred=0,
              sa=0.6, sb=0.8, taps=taps, r=4, thr=1.0, out=O, mask=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vtm_sag_degrade(a["x"], a["n_rows"], a["ids"], a["m"], a["mass"], a["ld"], a["h_m"], a["w_m"], a["dtype"],
                                 a["F"], a["C"], a["H"], a["W"], a["pred"], a["sa"], a["sb"], a["taps"], a["r"], a["thr"],
                                 a["out"], a["mask"], None)
    bad = [dict(dtype=5), dict(pred=3), dict(pred=-1), dict(x=None), dict(m=None), dict(mass=None), dict(taps=None),
           dict(out=None), dict(r=5), dict(r=-1), dict(F=-1), dict(C=0), dict(H=0), dict(W=0), dict(n_rows=1), dict(H=4),
           dict(W=4), dict(H=128, W=129), dict(H=16385, W=1, r=0), dict(h_m=0), dict(w_m=0), dict(h_m=9), dict(ld=63),
           dict(h_m=65, w_m=1, ld=128), dict(sa=float("nan")), dict(sb=float("nan")), dict(thr=float("nan")),
           dict(out=X), dict(out=X + 3 * 4 * 64 * 64 * 2), dict(out=X - 16)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert L.vtm_last_error().startswith(b"vtm_sag_degrade"), kw
    assert call(H=128, W=129) == EINVAL and b"16384" in L.vtm_last_error()
    assert call(F=0) == 0                                                  # an empty chunk: nothing to do, no launch


@pytest.mark.parametrize("H,W,h_m,w_m", GRIDS)
def test_restatement_equals_torch_reflect_conv_and_nearest(H, W, h_m, w_m):
    """blur64 == F.pad(mode="reflect") + conv2d in float64, upsample_nearest == F.interpolate(mode="nearest") -- at these
    shapes torch's float scale and the integer rule floor(y h_m / H) name the same source cell (checked here, index by
    index)."""
    g = torch.Generator().manual_seed(H * W + h_m)
    x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
    for r, sigma in ((4, 1.0), (2, 0.7), (0, 1.0)):
        t = S.taps64(r, sigma)
        assert abs(t.sum() - 1.0) <= (2 * r + 1) * 2.0 ** -24 and np.array_equal(t, t[::-1])
        k2 = torch.from_numpy(np.outer(t, t))[None, None]
        want = F.conv2d(F.pad(x.reshape(6, 1, H, W), (r, r, r, r), mode="reflect"), k2).reshape(2, 3, H, W) if r else x
        err = float(np.abs(S.blur64(x.numpy(), t) - want.numpy()).max())
        assert err <= 1e-14 * float(x.abs().max()), (r, err)
    m = torch.rand(3, h_m, w_m, generator=g, dtype=torch.float64)
    want = F.interpolate(m[None], size=(H, W), mode="nearest")[0].numpy()
    assert np.array_equal(S.upsample_nearest(m.numpy(), H, W), want)


def test_reflect_indices_and_taps():
    assert S.reflect_index(5, 4)[0].tolist() == [4, 3, 2, 1, 0, 1, 2, 3, 4]
    assert S.reflect_index(5, 4)[4].tolist() == [0, 1, 2, 3, 4, 3, 2, 1, 0]
    assert S.reflect_index(7, 2)[6].tolist() == [4, 5, 6, 5, 4]
    from vidtome_amd import _lib
    for r, sigma in ((4, 1.0), (3, 2.5), (0, 1.0), (1, 0.3)):
        assert np.array_equal(np.asarray(_lib.gaussian_taps(r, sigma)), S.taps64(r, sigma)), (r, sigma)
    assert _lib.gaussian_taps(0, 1.0) == [1.0]
    with pytest.raises(RuntimeError):
        _lib.gaussian_taps(2, 0.0)


def test_prediction_types_and_add_noise_are_consistent():
    """x = sqrt_alpha x0 + sqrt_beta eps for every prediction type (alpha + beta = 1): with an empty mask the degraded latents
    are x again, in float64 to rounding."""
    g = np.random.default_rng(0)
    x, m = g.standard_normal((2, 3, 8, 8)), g.standard_normal((2, 3, 8, 8))
    sa, sb = math.sqrt(0.3), math.sqrt(0.7)
    for pred in S.PREDS:
        out, A, mask = S.degrade64(x, m, np.zeros((2, 4), np.float32), 2, 2, pred, sa, sb, S.taps64(4, 1.0))
        assert not mask.any() and float(np.abs(out - x).max()) <= 1e-14 and bool((A >= np.abs(out) - 1e-14).all())
    out, _, mask = S.degrade64(x, m, np.full((2, 4), 1.0, np.float32), 2, 2, "epsilon", sa, sb, S.taps64(4, 1.0))
    assert not mask.any()                                                  # the threshold itself is outside the mask
    out, _, mask = S.degrade64(x, m, np.array([[2, 0, 0, 0], [0, 0, 0, 2]], np.float32), 2, 2, "epsilon", sa, sb,
                               S.taps64(4, 1.0))
    assert mask[0, :4, :4].all() and not mask[0, 4:].any() and mask[1, 4:, 4:].all() and not mask[1, :4].any()
    # the select: outside the mask x comes back whatever the neighbours are; inside it the blur moved it
    assert float(np.abs(out[0][:, 4:] - x[0][:, 4:]).max()) <= 1e-14 and float(np.abs(out[0][:, :4, :4] - x[0][:, :4, :4]).max()) > 0.1


def test_key_mass_restatement_sums_to_the_query_count():
    q, k = S.mass_operands(2, 4, 50, 37, 16, torch.float16, seed=1)
    m = S.key_mass64(q, k, 4, 50, 37, 0.25)
    assert m.shape == (2, 37) and float(np.abs(m.sum(-1) - 50).max()) <= 1e-10 and m.max() > 1.5 * 50 / 37
    # the fp32 restatement of the blocks' other routes against it
    from vidtome_amd import patch
    got = patch._key_mass_torch(q, k, 4, 0.25).double().numpy()
    assert float((np.abs(got - m) / m).max()) <= S.mass_bound(50, 37, 16, *S.score_bound(q, k, 4, 50, 37, 0.25))


def test_group_weights_algebra():
    """(1 - s + g) u + s c - g d is u + s (c - u) + g (u - d); without CFG (1 + g) c - g d is c + g (c - d)."""
    import vidtome_amd
    sag = vidtome_amd.SelfAttentionGuidance(None, scale=0.75)
    g = np.random.default_rng(1)
    u, c, d = g.standard_normal((3, 100))
    for s in (1.0, 7.5, 0.0):
        w = sag.group_weights(s)
        assert len(w) == 3 and w == (1.0 - s + 0.75, s, -0.75)
        assert float(np.abs(w[0] * u + w[1] * c + w[2] * d - (u + s * (c - u) + 0.75 * (u - d))).max()) <= 1e-13
    w = sag.group_weights(7.5, cfg=False)
    assert w == (1.75, -0.75) and float(np.abs(w[0] * c + w[1] * d - (c + 0.75 * (c - d))).max()) <= 1e-13
    s = vidtome_amd.GuidedDPMSolver(np.linspace(0.99, 0.01, 100), [80, 40], group_weights=sag.group_weights(7.5))
    assert s.weights(3) == [1.0 - 7.5 + 0.75, 7.5, -0.75]
    assert sag.radius == 4 and len(sag.taps) == 9
    for kw in (dict(kernel_size=8), dict(kernel_size=11), dict(kernel_size=0), dict(blur_sigma=0.0), dict(scale=float("nan"))):
        with pytest.raises(ValueError):
            vidtome_amd.SelfAttentionGuidance(None, **kw)


def test_all_and_exports():
    import vidtome_amd
    from vidtome_amd import sag
    names = {"SelfAttentionGuidance", "register_self_attention_guidance", "unregister_self_attention_guidance"}
    assert names <= set(vidtome_amd.__all__)
    for n in names:
        assert getattr(vidtome_amd, n) is getattr(sag, n)


def test_mass_grid():
    import vidtome_amd
    grid = vidtome_amd.SelfAttentionGuidance.mass_grid
    assert grid((64, 64), 64) == (8, 8) and grid((96, 96), 144) == (12, 12) and grid((40, 72), 45) == (5, 9)
    assert grid((60, 60), 64) == (8, 8) and grid((64, 64), 4096) == (64, 64)
    with pytest.raises(RuntimeError, match="tokens"):
        grid((64, 64), 60)


def _patched(built, **kw):
    import vidtome_amd
    unet = S.MidBlock(C=64, heads=2, **kw)
    vidtome_amd.apply_patch(unet, batch_size=S.B)
    unet.set_size(S.LATENT)
    return unet


def test_register_unregister_and_remove_patch(built):
    import vidtome_amd
    unet = _patched(built)
    blk = unet.block
    assert vidtome_amd.register_self_attention_guidance(unet) == [S.MID_NAME]
    assert blk.vtm_sag is True and not hasattr(blk, "attn1_key_mass")
    blk.attn1_key_mass = torch.zeros(2, 4)
    assert vidtome_amd.collect_from_patch(unet, "attn1_key_mass") == {S.MID_NAME: blk.attn1_key_mass}
    assert vidtome_amd.register_self_attention_guidance(unet, [S.MID_NAME]) == [S.MID_NAME]
    assert vidtome_amd.register_self_attention_guidance(unet, lambda name, b: False) == []
    assert not hasattr(blk, "vtm_sag") and not hasattr(blk, "attn1_key_mass")
    with pytest.raises(ValueError, match="not patched blocks"):
        vidtome_amd.register_self_attention_guidance(unet, ["down_blocks.0"])
    vidtome_amd.register_self_attention_guidance(unet)
    blk.attn1_key_mass = torch.zeros(2, 4)
    vidtome_amd.unregister_self_attention_guidance(unet)
    assert not hasattr(blk, "vtm_sag") and not hasattr(blk, "attn1_key_mass")
    vidtome_amd.register_self_attention_guidance(unet)
    blk.attn1_key_mass = torch.zeros(2, 4)
    vidtome_amd.remove_patch(unet)
    assert "vtm_sag" not in blk.__dict__ and "attn1_key_mass" not in blk.__dict__
    with pytest.raises(RuntimeError, match="nothing is patched"):
        vidtome_amd.register_self_attention_guidance(unet)


def test_default_selection_asks_for_names_without_a_mid_block(built):
    import attention_maps_standin as AM
    import vidtome_amd
    unet = AM.OneBlock(64, heads=2)
    vidtome_amd.apply_patch(unet, batch_size=2)
    with pytest.raises(RuntimeError, match="name the blocks"):
        vidtome_amd.register_self_attention_guidance(unet)
    assert vidtome_amd.register_self_attention_guidance(unet, ["blocks.0"]) == ["blocks.0"]
    vidtome_amd.remove_patch(unet)


def test_raise_rules_name_the_rule(built):
    """patch._sag_check on CPU tokens (it launches nothing): a merging site, more tokens than the kernel takes keys, perturbed
    attention in both forms, PnP sharing at an injection step."""
    import vidtome_amd
    from vidtome_amd import patch
    unet = _patched(built)
    blk = unet.block
    vidtome_amd.register_self_attention_guidance(unet)
    assert patch.sag_registered(blk)
    deep, shallow = torch.zeros(4, 64, 64), torch.zeros(4, 4096, 64)
    patch._sag_check(blk, deep)                                            # 8 x down: does not merge
    with pytest.raises(RuntimeError, match="self-attention guidance.*merges"):
        patch._sag_check(blk, shallow)
    blk._tome_info["size"] = None
    with pytest.raises(RuntimeError, match="merges"):
        patch._sag_check(blk, deep)
    unet.set_size((512, 512))                                              # 4097 tokens, 7.9 x down: un-merged, past the key limit
    with pytest.raises(RuntimeError, match="4097 tokens.*at most 4096 keys"):
        patch._sag_check(blk, torch.zeros(1, 4097, 64))
    patch._sag_check(blk, torch.zeros(1, 4096, 64))
    unet.set_size(S.LATENT)
    vidtome_amd.register_perturbed_attention(unet, layers=("mid",), groups=2)
    with pytest.raises(RuntimeError, match="perturbed attention"):
        patch._sag_check(blk, deep)
    vidtome_amd.remove_perturbed_attention(unet)

    class PAGCFGIdentitySelfAttnProcessor2_0:
        pass
    blk.attn1.processor = PAGCFGIdentitySelfAttnProcessor2_0()
    with pytest.raises(RuntimeError, match="perturbed attention"):
        patch._sag_check(blk, deep)
    del blk.attn1.processor
    blk.attn1.injection_schedule, blk.attn1.t, blk.attn1.vtm_num_inputs = [5], 5, 3
    with pytest.raises(RuntimeError, match="PnP"):
        patch._sag_check(blk, deep)
    blk.attn1.t = 6
    patch._sag_check(blk, deep)
    vidtome_amd.remove_patch(unet)


def test_module_path_key_mass_reads_the_projections_or_warns():
    from vidtome_amd import patch
    attn = S.AM.ComputingSelf(64, 2)
    x = torch.randn(2, 9, 64)
    got = patch._module_path_key_mass(attn, x)
    q, k = attn.to_q(x), attn.to_k(x)
    want = S.key_mass64(q.detach(), k.detach(), 2, 9, 9, attn.scale)
    assert tuple(got.shape) == (2, 9) and got.dtype == torch.float32 and not got.requires_grad
    bound = S.mass_bound(9, 9, 32, *S.score_bound(q.detach(), k.detach(), 2, 9, 9, attn.scale))
    assert float((np.abs(got.double().numpy() - want) / want).max()) <= bound
    attn.norm_q = torch.nn.LayerNorm(32)
    patch._warned.discard("sag-unreadable")
    with pytest.warns(UserWarning, match="attn1_key_mass is None"):
        assert patch._module_path_key_mass(attn, x) is None


def test_degrade_host_checks(built):
    """What SelfAttentionGuidance.degrade refuses before any device work."""
    import vidtome_amd
    unet = _patched(built)
    sag = vidtome_amd.SelfAttentionGuidance(unet)
    ddim = vidtome_amd.GuidedDDIM(np.linspace(0.99, 0.01, 100), [80, 40])
    x, m = torch.zeros(4, 4, 64, 64), torch.zeros(4, 4, 64, 64)
    with pytest.raises(RuntimeError, match="0 registered blocks"):
        sag.degrade(x, m, ddim, 0, groups=2)
    vidtome_amd.register_self_attention_guidance(unet)
    with pytest.raises(RuntimeError, match="holds no attn1_key_mass"):
        sag.degrade(x, m, ddim, 0, groups=2)
    unet.block.attn1_key_mass = torch.zeros(2, 64)
    with pytest.raises(RuntimeError, match="between the two UNet calls"):
        sag.degrade(x, m, ddim, 0, groups=2)
    with pytest.raises(RuntimeError, match="sampler"):
        sag.degrade(x, m, object(), 0, groups=2)
    with pytest.raises(RuntimeError, match="group = 2"):
        sag.degrade(x, m, ddim, 0, groups=2, group=2)
    big = torch.zeros(2, 4, 128, 136)
    with pytest.raises(RuntimeError, match="16384.*LDS"):
        sag.degrade(big, big, ddim, 0, groups=1, mass=torch.zeros(2, 16 * 17))
    with pytest.raises(RuntimeError, match="tokens"):
        sag.degrade(x, m, ddim, 0, groups=2, mass=torch.zeros(2, 60))
    vidtome_amd.remove_patch(unet)
