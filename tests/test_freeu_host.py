"""CPU tests of FreeU: the C-ABI surface of vtm_freeu / vtm_freeu_ws_bytes / vtm_freeu_lanes (declarations, every VTM_EINVAL path
without a launch, the compiler's resource figures), the four-bin identity of tests/freeu_standin.py against the FFT form at
every plane size the GPU tests use, the counted roundings, and the host semantics of vidtome_amd.freeu on stand-in up blocks
(which resnets are hooked, C_h / C_s per resnet, the factors per stage, takeover / unregister / remove_patch, every raise
rule)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import freeu_standin as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NEW = ("vtm_freeu", "vtm_freeu_ws_bytes", "vtm_freeu_lanes")


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


def test_header_declares_the_exports_and_the_version_stays(built):
    from vidtome_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    lib = ctypes.CDLL(built)
    for name in NEW:
        decl = re.search(r"^(int|size_t) %s\((.*?)\);" % name, hdr, re.M | re.S)
        assert decl, name
        params = [p.strip() for p in decl.group(2).split(",")]
        argtypes, restype = _lib._SIGNATURES[name]
        assert len(params) == len(argtypes) and restype is (ctypes.c_int if decl.group(1) == "int" else ctypes.c_size_t), name
        for p, t in zip(params, argtypes):
            want = (ctypes.c_void_p if "*" in p or p.startswith("vtm_stream_t") else ctypes.c_int64 if p.startswith("int64_t")
                    else ctypes.c_float if p.startswith("float") else ctypes.c_size_t if p.startswith("size_t") else ctypes.c_int)
            assert t is want, (name, p, t)
        assert hasattr(lib, name) and name in _lib.exported_symbols(), name
    assert len(_lib._SIGNATURES["vtm_freeu"][0]) == 13 and len(_lib._SIGNATURES["vtm_freeu_ws_bytes"][0]) == 3
    assert "#define VTM_ABI_VERSION 2" in hdr and _lib.lib().vtm_version() == _lib.ABI_VERSION == 2
    assert "freeu.hip" in build.SOURCES and callable(_lib.freeu) and _lib.FREEU_MAX_PLANE == 16384
    doc = hdr[hdr.index("vtm_freeu --"):hdr.index("int vtm_freeu_lanes")]
    for word in ("C_h / 2", "never written", "max == min", "H, W >= 2", "P <= 16384", "C_h >= 2", "C_s >= 1", "ky, kx in {0, -1}"):
        assert word in doc, word


def test_kernels_use_no_scratch(built):
    """profiles/freeu_resources.txt: no scratch, no spills, at most 160 KiB of LDS -- for every instantiation: four forms x
    three dtypes of the apply kernel, the three mean kernels and the min / max kernel."""
    from vidtome_amd import build
    res = build.kernel_resources(os.path.join(os.path.dirname(built), "freeu.o"))
    assert len([k for k in res if "freeu_apply_kernel" in k]) == 12, sorted(res)
    assert len([k for k in res if "freeu_mean_kernel" in k]) == 3 and len([k for k in res if "freeu_minmax_kernel" in k]) == 1
    assert len(res) == 16
    for k, v in res.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
        assert v.get("group_segment_fixed_size", 0) <= 160 * 1024, (k, v)
        assert v["vgpr_count"] <= 128, (k, v)                 # the 1024-thread form's budget; the others sit below it too


def test_einval_paths_answer_without_a_launch(built):
    """No GPU here: a call that got as far as a launch would fail differently (VTM_ELAUNCH) or crash on the fake pointers."""
    from vidtome_amd import _lib
    L = _lib.lib()
    X, WS = 0x10000, 0x400000
    ok = dict(x=X, dtype=_lib.VTM_F16, B=2, C_h=8, C_s=4, H=8, W=8, b=1.2, s=0.9, version=1, ws=None, ws_bytes=0)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vtm_freeu(a["x"], a["dtype"], a["B"], a["C_h"], a["C_s"], a["H"], a["W"], a["b"], a["s"], a["version"], a["ws"],
                           a["ws_bytes"], None)
    need = (2 * 64 + 2 * 2) * 4
    big = 2 ** 31 - 1
    bad = [dict(x=None), dict(x=X + 1), dict(x=X + 2, dtype=_lib.VTM_F32), dict(x=X + 1, dtype=_lib.VTM_BF16), dict(B=-1),
           dict(H=1), dict(W=1), dict(H=0), dict(H=128, W=129), dict(H=16385, W=2), dict(H=2, W=8193), dict(C_h=1), dict(C_h=0),
           dict(C_s=0), dict(C_s=-3), dict(version=0), dict(version=3), dict(dtype=9), dict(dtype=-1),
           dict(version=2), dict(version=2, ws=WS, ws_bytes=need - 1), dict(version=2, ws=None, ws_bytes=need),
           dict(version=2, ws=WS + 2, ws_bytes=need), dict(B=big, C_s=big), dict(B=2 ** 31), dict(B=big, C_h=64, C_s=1),
           dict(H=128, W=128, B=2 ** 25, version=2, ws=WS, ws_bytes=2 ** 62)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert L.vtm_last_error().startswith(b"vtm_freeu"), (kw, L.vtm_last_error())
    assert call(H=128, W=129) == EINVAL and b"16384" in L.vtm_last_error()
    assert call(B=0) == 0 and call(B=0, version=2) == 0            # an empty batch: nothing to do, no launch, no workspace
    ws = L.vtm_freeu_ws_bytes
    assert ws(2, 64, 1) == 0 and ws(32, 16384, 1) == 0
    assert ws(2, 64, 2) == need and ws(4, 16384, 2) == (4 * 16384 + 8) * 4 and ws(0, 64, 2) == 0 and ws(1, 4, 2) == 24


def test_lanes_rule_and_rounding_counts(built):
    """The form is a function of P alone; K_s / K_m are the header's formulas on it."""
    from vidtome_amd import _lib
    lanes = _lib.freeu_lanes
    assert [lanes(p) for p in (3, 4, 64, 144, 256, 257, 576, 1024, 2048, 2049, 4096, 8192, 8193, 16384, 16385)] == \
        [0, 16, 16, 16, 16, 64, 64, 64, 64, 256, 256, 256, 1024, 1024, 0]
    planes = S.boundary_planes(lanes, _lib.FREEU_MAX_PLANE)
    assert planes == [(16, 16), (6, 43), (32, 64), (3, 683), (64, 128), (3, 2731)]
    for P in range(4, _lib.FREEU_MAX_PLANE + 1, 97):
        G = lanes(P)
        assert -(-(-(-P // 8)) // G) <= (2 if G in (16, 1024) else 4), P        # the chunks a lane holds fit its registers
    rc = _lib.freeu_rounding_counts
    # R = 8 chunks-per-lane + log2(min(G, 64)) + waves;  K_s = ceil((7 R + 180) / 4) + 1;  K_m = ceil(C_h / 16) + 15
    assert rc(64, 8) == (67, 16) and rc(256, 1280) == (81, 95)                  # R = 12, 20
    assert rc(4096, 640) == (92, 55) and rc(16384, 2) == (113, 16)              # R = 16 + 6 + 4, 16 + 6 + 16
    assert rc(2048, 33) == (113, 18)                                            # R = 32 + 6
    for bad in ((3, 8), (16385, 8), (64, 1)):
        with pytest.raises(ValueError):
            rc(*bad)


def _gpu_planes():
    from vidtome_amd import _lib
    planes = [(H, W) for _, _, H, W in S.SMALL + [S.LARGEST]] + S.boundary_planes(_lib.freeu_lanes, _lib.FREEU_MAX_PLANE)
    return planes + [(8, 8), (16, 16), (2, 8192)]                                # (the hook test's; the widest tables)


def test_four_bin_identity_equals_the_fft_form(built):
    g = np.random.default_rng(7)
    for H, W in _gpu_planes() + S.IDENTITY_ONLY:
        v = g.standard_normal((2, 3, H, W))
        v[1] *= 50.0
        for s in (0.2, 0.9, 1.0, 1.4, 3.0):
            err = np.abs(S.skip64(v, s) - S.skip_fft64(v, s)).max()
            assert err <= 1e-12 * np.abs(v).max() * max(1.0, abs(s - 1.0)), (H, W, s, err)
    x = g.standard_normal((2, 12, 5, 7))
    assert np.array_equal(S.freeu64(x, 8, 1.0, 1.0)[:, :8], x[:, :8])
    out = S.freeu64(x, 8, 1.5, 0.5)
    assert np.array_equal(out[:, 4:8], x[:, 4:8]) and np.array_equal(out[:, :4], x[:, :4] * 1.5)


def test_version_2_restatement_and_its_input_condition():
    x = S.make_input(2, 8, 4, 8, 8, torch.float16, seed=1).double().numpy()
    assert S.well_spread(x, 8)
    g, (spread, mag) = S.gain64(x, 8, 1.6, 2)
    assert g.shape == (2, 1, 8, 8) and abs(g.min() - 1.0) <= 1e-15 and abs(g.max() - 1.6) <= 1e-15 and (spread > 1.0).all()
    assert not np.array_equal(g[0], g[1])
    # the input condition holds at every shape of the GPU tests (float64, checked here)
    for C_h, C_s, H, W in S.SMALL + [S.LARGEST]:
        for dt in S.DTYPES:
            assert S.well_spread(S.make_input(2, C_h, C_s, H, W, dt, seed=H * W).double().numpy(), C_h), (C_h, H, W, dt)
    x[0, :8] = 0.25                                                            # a constant map: the stated deviation, g = 1
    g, _ = S.gain64(x, 8, 1.6, 2)
    assert (g[0] == 1.0).all() and g[1].max() > 1.5
    assert not S.well_spread(x, 8)


# ---- host semantics on the stand-ins -----------------------------------------------------------------------------------------
@pytest.fixture
def recorder(monkeypatch):
    from vidtome_amd import _lib
    calls = []

    def fake(x, C_h, b, s, version=1):
        calls.append((tuple(x.shape), C_h, x.shape[1] - C_h, b, s, version, x.data_ptr()))
        return x
    monkeypatch.setattr(_lib, "freeu", fake)
    return calls


def _run(unet, **kw):
    sample, skips = unet.operands(2, torch.float32, "cpu")
    with torch.no_grad():
        unet(sample, skips)
    return unet.recorded()


def test_hooks_channels_and_factors_per_stage(recorder):
    import vidtome_amd
    unet = S.StandinUNet(unit=320, size=2)
    assert vidtome_amd.register_freeu(unet, s1=0.9, s2=0.2, b1=1.5, b2=1.6) is unet
    seen = _run(unet)
    assert [(c[1], c[2]) for c in recorder] == [(1280, 1280), (1280, 1280), (1280, 640), (1280, 640), (640, 640), (640, 320)]
    assert [(c[3], c[4]) for c in recorder] == [(1.5, 0.9)] * 3 + [(1.6, 0.2)] * 3 and {c[5] for c in recorder} == {1}
    assert [c[0][2:] for c in recorder] == [(2, 2)] * 3 + [(4, 4)] * 3
    assert [(i, j) for i, j, _ in seen] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0)]    # block 2: not hooked
    assert len(unet.up_blocks[2]._forward_pre_hooks) == 0 and all(len(r._forward_pre_hooks) == 0 for r in unet.up_blocks[2].resnets)
    for blk in unet.up_blocks[:2]:
        assert len(blk._forward_pre_hooks) == 1 and all(len(r._forward_pre_hooks) == 1 for r in blk.resnets)
        st = blk.__dict__["vtm_freeu"]
        assert len(st["handles"]) == 4 and (blk.s1, blk.s2, blk.b1, blk.b2) == (None,) * 4
    # registering again: new factors, version 2, no stacked hooks
    del recorder[:]
    vidtome_amd.register_freeu(unet, s1=0.8, s2=0.3, b1=1.1, b2=1.2, version=2)
    _run(unet)
    assert [(c[3], c[4], c[5]) for c in recorder] == [(1.1, 0.8, 2)] * 3 + [(1.2, 0.3, 2)] * 3
    for blk in unet.up_blocks[:2]:
        assert len(blk._forward_pre_hooks) == 1 and all(len(r._forward_pre_hooks) == 1 for r in blk.resnets)
    # a pipeline-like holder is taken as well
    del recorder[:]
    vidtome_amd.unregister_freeu(type("Pipe", (), {"unet": unet})())
    _run(unet)
    assert recorder == []
    for blk in unet.up_blocks:
        assert "vtm_freeu" not in blk.__dict__ and len(blk._forward_pre_hooks) == 0
        assert all(n not in blk.__dict__ for n in ("s1", "s2", "b1", "b2"))            # absent before: absent again
        assert all(len(r._forward_pre_hooks) == 0 for r in blk.resnets)


def test_the_hook_hands_over_the_tensor_the_resnet_reads(recorder):
    """In place on the very tensor: the pointer the wrapper got is the pointer the resnet saw (forward's own argument)."""
    import vidtome_amd
    unet = S.StandinUNet(unit=8, size=4)
    ptrs = []
    for blk in unet.up_blocks[:2]:
        for r in blk.resnets:
            r.register_forward_hook(lambda mod, args, out: ptrs.append(args[0].data_ptr()))
    vidtome_amd.register_freeu(unet, 0.9, 0.2, 1.5, 1.6)
    _run(unet)
    assert [c[6] for c in recorder] == ptrs and len(ptrs) == 6


def test_takeover_reads_and_nulls_the_attributes_and_unregister_restores(recorder):
    import vidtome_amd
    unet = S.StandinUNet(unit=8, size=4)
    with pytest.raises(ValueError, match=r"enable_freeu\(\.\.\.\) first or pass the factors"):
        vidtome_amd.register_freeu(unet)
    for blk in unet.up_blocks:                                                # what pipe.enable_freeu(s1, s2, b1, b2) leaves
        blk.s1, blk.s2, blk.b1, blk.b2 = 0.9, 0.2, 1.5, 1.6
    base = _run(unet)                                                         # the stand-in's own torch branch ran
    vidtome_amd.register_freeu(unet)
    for blk in unet.up_blocks[:2]:
        assert (blk.s1, blk.s2, blk.b1, blk.b2) == (None,) * 4
    assert unet.up_blocks[2].s1 == 0.9                                        # not a stage: left alone
    seen = _run(unet)
    assert [(c[3], c[4]) for c in recorder] == [(1.5, 0.9)] * 3 + [(1.6, 0.2)] * 3
    # the torch branch stayed off: block 0's first resnet saw the plain concatenation
    sample, skips = unet.operands(2, torch.float32, "cpu")
    assert torch.equal(seen[0][2], torch.cat([sample, skips[-1]], 1)) and not torch.equal(base[0][2], seen[0][2])
    # taking over again while registered reads what was found the first time
    vidtome_amd.register_freeu(unet)
    assert unet.up_blocks[0].__dict__["vtm_freeu"]["found"] == dict(s1=0.9, s2=0.2, b1=1.5, b2=1.6)
    vidtome_amd.unregister_freeu(unet)
    for blk in unet.up_blocks:
        assert (blk.s1, blk.s2, blk.b1, blk.b2) == (0.9, 0.2, 1.5, 1.6) and "vtm_freeu" not in blk.__dict__
    again = _run(unet)
    assert all(torch.equal(a[2], b[2]) for a, b in zip(base, again))
    unet.up_blocks[1].b2 = 0                                                  # falsy: Diffusers' branch would be off too
    with pytest.raises(ValueError, match=r"up_blocks\[1\].*b2 = 0"):
        vidtome_amd.register_freeu(unet)
    assert "vtm_freeu" not in unet.up_blocks[0].__dict__ and unet.up_blocks[0].s1 == 0.9      # nothing half-registered


def test_remove_patch_clears_everything(built, recorder):
    import vidtome_amd
    unet = S.StandinUNet(unit=8, size=4)
    vidtome_amd.apply_patch(unet, batch_size=2)
    for blk in unet.up_blocks:
        blk.s1, blk.s2, blk.b1, blk.b2 = 0.9, 0.2, 1.5, 1.6
    vidtome_amd.register_freeu(unet)
    assert "vtm_freeu" in unet.up_blocks[1].__dict__
    vidtome_amd.remove_patch(unet)
    for blk in unet.up_blocks:
        assert "vtm_freeu" not in blk.__dict__ and len(blk._forward_pre_hooks) == 0 and blk.b2 == 1.6
        assert all(len(r._forward_pre_hooks) == 0 for r in blk.resnets)
    _run(unet)
    assert recorder == []
    src = open(os.path.join(ROOT, "vidtome_amd", "patch.py")).read()
    body = src[src.index("def remove_patch"):src.index("def update_patch")]
    assert "freeu.release(module)" in body and body.index("freeu.release(module)") > body.index('pop("vtm_sag"')
    # the new wrappers are not on the patched block's forward path
    assert "_lib.freeu" not in src


def test_raise_rules(built, recorder):
    import vidtome_amd
    unet = S.StandinUNet(unit=8, size=4)
    with pytest.raises(ValueError, match="all of s1, s2, b1, b2 or none"):
        vidtome_amd.register_freeu(unet, s1=0.9)
    with pytest.raises(ValueError, match="version = 3"):
        vidtome_amd.register_freeu(unet, 0.9, 0.2, 1.5, 1.6, version=3)
    with pytest.raises(ValueError, match="two up blocks"):
        vidtome_amd.register_freeu(torch.nn.Linear(2, 2), 0.9, 0.2, 1.5, 1.6)
    assert all("vtm_freeu" not in blk.__dict__ for blk in unet.up_blocks)
    vidtome_amd.register_freeu(unet, 0.9, 0.2, 1.5, 1.6)
    sample, skips = unet.operands(2, torch.float32, "cpu")
    # a tensor that requires grad while grad is enabled
    with pytest.raises(RuntimeError, match="requires grad.*in-place"):
        unet(sample.clone().requires_grad_(True), skips)
    with torch.no_grad():
        unet(sample.clone().requires_grad_(True), skips)                     # grad disabled: taken
    unet.recorded()
    # no skip channels left: C_s <= 0 (resnet 1 is told its input has only the previous resnet's channels)
    blk = unet.up_blocks[0]
    with pytest.raises(ValueError, match="C_s = 0 skip channels"):
        blk.resnets[1](torch.zeros(2, blk.resnets[0].out_channels, 4, 4))
    with pytest.raises(ValueError, match="C_s = -"):
        blk.resnets[2](torch.zeros(2, 3, 4, 4))
    # resnet 0 outside its block: the channel count of hidden_states is unknown
    fresh = S.StandinUNet(unit=8, size=4)
    vidtome_amd.register_freeu(fresh, 0.9, 0.2, 1.5, 1.6)
    with pytest.raises(RuntimeError, match="outside its up block"):
        fresh.up_blocks[0].resnets[0](torch.zeros(2, 64, 4, 4))
    with pytest.raises(ValueError, match="hidden_states"):
        fresh.up_blocks[0](None, skips[-3:])


def test_lib_freeu_refuses_what_the_kernel_does_not_take(built):
    """The wrapper's own checks, each naming its argument; the device check is the last, so all of them run here."""
    from vidtome_amd import _lib
    ok = torch.zeros(2, 12, 8, 8, dtype=torch.float16)
    cases = [(dict(x=ok.double()), "x is torch.float64"), (dict(x=ok.to(torch.int32)), "x is torch.int32"),
             (dict(x=ok[:, :, :, ::2]), "x must be contiguous"), (dict(x=ok.to(memory_format=torch.channels_last)), "contiguous"),
             (dict(x=ok[0]), r"\(B, C_h \+ C_s, H, W\)"), (dict(x=None), "tensor"),
             (dict(x=torch.zeros(1, 3, 128, 129, dtype=torch.float16), C_h=2), "FREEU_MAX_PLANE = 16384"),
             (dict(x=torch.zeros(1, 3, 1, 64, dtype=torch.float16), C_h=2), "H, W >= 2"),
             (dict(C_h=1), "C_h = 1"), (dict(C_h=12), "C_s"), (dict(C_h=13), "C_s"), (dict(version=0), "version = 0"),
             (dict(), "x lives on cpu")]
    for kw, match in cases:
        a = dict(dict(x=ok, C_h=8, b=1.2, s=0.9, version=1), **kw)
        with pytest.raises(ValueError, match=match):
            _lib.freeu(a["x"], a["C_h"], a["b"], a["s"], a["version"])


def test_all_and_exports():
    import vidtome_amd
    from vidtome_amd import freeu
    assert {"register_freeu", "unregister_freeu"} <= set(vidtome_amd.__all__)
    assert vidtome_amd.register_freeu is freeu.register_freeu and vidtome_amd.unregister_freeu is freeu.unregister_freeu
