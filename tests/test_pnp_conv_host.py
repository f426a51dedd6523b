"""CPU tests of PnP feature injection (vidtome_amd.pnp.register_conv_control): the public names, the C-ABI surface of
vtm_groupnorm_silu / vtm_resnet_tail, their argument checks, and the plain-torch fallback of the closure against the
reference's recorded runs (tests/golden/pnp_conv.npz) -- including that the main branch only sees the surviving rows."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pnp_conv_standin as st
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(GOLDEN, "pnp_conv.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


def test_the_three_pnp_functions_import_from_one_module():
    from vidtome_amd.pnp import register_attention_control, register_conv_control, register_time, unregister_conv_control
    assert all(callable(f) for f in (register_attention_control, register_conv_control, register_time, unregister_conv_control))


def test_header_declares_and_lib_binds_the_exports(built):
    from vidtome_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    lib = ctypes.CDLL(built)
    for name, nargs in (("vtm_groupnorm_silu", 13), ("vtm_resnet_tail", 10)):
        decl = re.search(r"int " + name + r"\((.*?)\);", hdr, re.S)
        assert decl and hasattr(lib, name) and name in _lib.exported_symbols(), name
        assert len(decl.group(1).split(",")) == len(_lib._SIGNATURES[name][0]) == nargs
    assert "pnp_utils.py:113-114" in hdr and "pnp_utils.py:146-162" in hdr       # the reference lines they replace
    assert re.search(r"#define VTM_ABI_VERSION 2\b", hdr) and _lib.lib().vtm_version() == _lib.ABI_VERSION == 2
    assert "groupnorm.hip" in build.SOURCES


def test_argument_checks_answer_before_any_launch(built):
    """Fake (never dereferenced) pointers: every bad argument returns VTM_EINVAL from the host-side checks."""
    from vidtome_amd import _lib
    L = _lib.lib()
    gn = lambda C=32, groups=4, dtype=1, act=1, x=64, out=128, HW=16, B=2: L.vtm_groupnorm_silu(
        x, None, None, None, dtype, B, C, HW, groups, 1e-5, act, out, None)
    assert gn(C=30) == -1 and b"divide" in L.vtm_last_error()
    assert gn(dtype=7) == -1 and b"dtype" in L.vtm_last_error()
    assert gn(groups=0) == -1 and gn(act=2) == -1 and gn(HW=0) == -1 and gn(x=None) == -1 and gn(B=-1) == -1
    assert gn(x=72) == -1 and b"aligned" in L.vtm_last_error()
    assert gn(x=128) == -1 and b"alias" in L.vtm_last_error()
    assert gn(B=0) == 0                                            # nothing to do is not an error
    tail = lambda B=6, M=240, inject=0, period=0, dtype=1, scale=1.0, h=64: L.vtm_resnet_tail(
        64, h, dtype, B, M, inject, period, scale, 128, None)
    assert tail(inject=4, period=0) == -1 and b"period" in L.vtm_last_error()
    assert tail(dtype=5) == -1 and b"dtype" in L.vtm_last_error()
    assert tail(inject=7, period=2) == -1 and tail(M=0) == -1 and tail(scale=0.0) == -1 and tail(h=None) == -1
    assert tail(B=0) == 0


def _registered(case, **resnet_kw):
    from vidtome_amd import pnp
    num_inputs, B, t, shortcut, scale = case
    resnet = st.load_weights(st.StandinResnet(shortcut=shortcut, scale=scale, **resnet_kw), Z, shortcut).eval()
    model = st.model_around(resnet)
    pnp.register_conv_control(model, list(st.SCHEDULE), num_inputs)
    resnet.t = t
    return model, resnet


@pytest.mark.parametrize("n", range(len(st.CASES)))
def test_fallback_equals_the_reference_on_the_surviving_rows(n):
    case = st.CASES[n]
    assert int(Z["n_cases"]) == len(st.CASES) and tuple(Z[f"{n}/{k}"].item() for k in st.FIELDS) == case
    num_inputs, B, t, shortcut, scale = case
    model, resnet = _registered(case)
    x, temb = (torch.from_numpy(Z[f"{k}/B{B}s{int(shortcut)}"]) for k in ("x", "temb"))
    assert torch.equal(x, st.inputs(B, shortcut)[0])
    seen = []
    resnet.conv1.register_forward_hook(lambda m, a, o: seen.append(a[0].shape[0]))
    with torch.no_grad():
        y = resnet.forward(x, temb)
    want = torch.from_numpy(Z[f"{n}/out"])
    assert y.shape == want.shape and float((y - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert seen == [st.surviving_rows(num_inputs, B, t)]
    sbs = B // num_inputs
    assert seen[0] == ({6: sbs, 7: sbs + 1}[B] if st.injects(t) else B)


def test_registering_twice_keeps_one_closure_and_unregister_restores_the_class_forward():
    from vidtome_amd import pnp
    model, resnet = _registered(st.CASES[0])
    first = resnet.__dict__["forward"]
    pnp.register_conv_control(model, [1, 2], 2)
    assert resnet.__dict__["forward"] is first and resnet.injection_schedule == [1, 2] and resnet.vtm_conv_num_inputs == 2
    x, temb = st.inputs(6, True)
    resnet.t = 2
    with torch.no_grad():
        y = resnet.forward(x, temb)
        plain = st.StandinResnet.forward(resnet, x, temb)
        want = plain[:3] - resnet.conv_shortcut(x[:3]) + resnet.conv_shortcut(x[3:])      # rows 3-5 carry rows 0-2's branch
    assert float((y[:3] - plain[:3]).abs().max()) < 1e-5 and float((y[3:] - want).abs().max()) < 1e-5 and not torch.allclose(y[3:], plain[3:])
    pnp.unregister_conv_control(model)
    assert "forward" not in resnet.__dict__ and not hasattr(resnet, "injection_schedule")
    with torch.no_grad():
        assert torch.equal(resnet.forward(x, temb), plain)
    pnp.unregister_conv_control(model)                             # a second call is harmless
    with pytest.raises(ValueError):
        pnp.register_conv_control(model, [1], 1)


def test_scale_shift_and_resampling_resnets_keep_the_source_only_branch():
    """The fallback covers what the kernels do not: a scale_shift time embedding and an upsampling resnet, each against
    the all-rows statement with the injection copies applied afterwards."""
    up = torch.nn.Upsample(scale_factor=2, mode="nearest")
    for kw, resample in (({"time_embedding_norm": "scale_shift"}, None), ({}, up)):
        torch.manual_seed(0)
        resnet = st.StandinResnet(shortcut=True, **kw).eval()
        resnet.upsample = resample
        model = st.model_around(resnet)
        from vidtome_amd import pnp
        pnp.register_conv_control(model, list(st.SCHEDULE), 3)
        resnet.t = st.SCHEDULE[0]
        x, temb = st.inputs(7, True)
        seen = []
        resnet.conv1.register_forward_hook(lambda m, a, o: seen.append(a[0].shape[0]))
        with torch.no_grad():
            y = resnet.forward(x, temb)
            xs = x if resample is None else resample(x)
            h = resnet.nonlinearity(resnet.norm1(x))
            h = resnet.conv1(h if resample is None else resample(h))
            e = resnet.time_emb_proj(resnet.nonlinearity(temb))[:, :, None, None]
            if kw:
                s, b = e.chunk(2, dim=1)
                h = resnet.norm2(h) * (1 + s) + b
            else:
                h = resnet.norm2(h + e)
            h = resnet.conv2(resnet.nonlinearity(h))
            h[2:4], h[4:6] = h[:2], h[:2]
            want = (resnet.conv_shortcut(xs) + h) / resnet.output_scale_factor
        assert seen == [3, 7] and float((y - want).abs().max()) <= 1e-6 * float(want.abs().max())
