"""CPU tests of edit-friendly inversion (vidtome_amd.inversion.EditFriendlyInversion, _lib.invert_step / _lib.noise_levels,
vtm_invert_step / vtm_noise_levels): the C-ABI surface, the kernels' resources, the identity that makes DDIM with eta = 1 this
solver at order 1, and every argument error -- raised before the library is entered by the two Python layers, and returned
before any launch by the library itself."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1      # include/vidtome_hip.h VTM_EINVAL


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


def _alphas():
    """Stable Diffusion's schedule: scaled-linear betas 0.00085 .. 0.012 over 1000 steps."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def _timesteps(n):
    return ((np.arange(n) * (1000 // n))[::-1] + 1).tolist()


def _solver(n=20, **kw):
    from vidtome_amd import GuidedDPMSolver
    return GuidedDPMSolver(_alphas(), _timesteps(n), **dict(dict(algorithm_type="sde-dpmsolver++"), **kw))


def test_header_declares_and_lib_binds_the_exports(built):
    import vidtome_amd
    from vidtome_amd import _lib, build, inversion
    hdr = open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    so = ctypes.CDLL(built)
    for name, count in (("vtm_invert_step", 26), ("vtm_noise_levels", 7)):
        decl = re.search(r"int %s\((.*?)\);" % name, hdr, re.S)
        assert decl and len(decl.group(1).split(",")) == len(_lib._SIGNATURES[name][0]) == count, name
        assert hasattr(so, name) and name in _lib.exported_symbols()
    # vtm_solver_step's arguments plus target and z_out, minus noise and x_out
    forward = [a.split()[-1].lstrip("*") for a in re.search(r"int vtm_solver_step\((.*?)\);", hdr, re.S).group(1).split(",")]
    inverse = [a.split()[-1].lstrip("*") for a in re.search(r"int vtm_invert_step\((.*?)\);", hdr, re.S).group(1).split(",")]
    assert sorted(inverse) == sorted(set(forward) - {"noise", "x_out"} | {"target", "z_out"})
    doc = hdr[hdr.index("vtm_invert_step --"):hdr.index("int vtm_invert_step(")]
    for word in ("ONE CHUNK", "fp32", "h_out", "frame_ids", "VTM_EINVAL", "BIT FOR BIT", "IN PLACE", "c_noise == 0"):
        assert word in doc, word
    # additive: the ABI version stays
    assert re.search(r"#define VTM_ABI_VERSION 2\b", hdr) and _lib.lib().vtm_version() == _lib.ABI_VERSION == 2
    assert "invert_step.hip" in build.SOURCES and callable(_lib.invert_step) and callable(_lib.noise_levels)
    assert vidtome_amd.EditFriendlyInversion is inversion.EditFriendlyInversion and "EditFriendlyInversion" in vidtome_amd.__all__
    # one expression: neither source restates what solver_core.h holds
    csrc = os.path.join(ROOT, "vidtome_amd", "csrc")
    core = open(os.path.join(csrc, "solver_core.h")).read()
    for name in ("struct Solve {", "void combine(", "void load_history(", "void store_history(", "float solver_sum("):
        assert name in core, name
        for src in ("solver_step.hip", "invert_step.hip"):
            text = open(os.path.join(csrc, src)).read()
            assert name not in text and '#include "solver_core.h"' in text and "solver_sum(" in text, (src, name)


def test_kernels_do_not_spill(built):
    """(2 step kernels + the noising kernel) x 3 dtypes x (16-byte | element) accesses: no scratch, no spilled register."""
    from vidtome_amd import build
    res = build.kernel_resources(os.path.join(os.path.dirname(built), "invert_step.o"))
    step = {k: v for k, v in res.items() if "invert_step" in k}
    levels = {k: v for k, v in res.items() if "noise_levels" in k}
    assert len(step) == 12 and len(levels) == 6, sorted(res)
    for name, r in {**step, **levels}.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)


# ---------------------------------------------------------------------------------------------------
# the coefficients
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("final", [1.0, 0.9991])
@pytest.mark.parametrize("n", [10, 20])
def test_ddim_eta_one_is_the_first_order_solver(n, final):
    """DDIM's update with eta = 1, x' = sqrt(a') x0 + sqrt(1 - a' - s^2) eps + s z with eps = (x - sqrt(a) x0) / sqrt(1 - a), has
    the coefficients of "sde-dpmsolver++" at order 1 on x, x0 and z.  Both sides are float64 expressions of O(1) terms with no
    cancellation worse than 1 - a (>= 8.5e-4 on this schedule, asserted): 1e-12 leaves three digits to spare."""
    from vidtome_amd import GuidedDDIM
    ddim = GuidedDDIM(_alphas(), _timesteps(n), final_alpha_cumprod=final, eta=1.0)
    s = _solver(n, final_alpha_cumprod=final, solver_order=1)
    assert min(1.0 - float(_alphas()[t]) for t in _timesteps(n)) >= 8.5e-4
    for i in range(n):
        a_from, a_to, sa, sb, c_x0_ddim, c_eps, sigma = ddim.coefficients(i)
        got = s.coefficients(i)
        assert got[:2] == (sa, sb) and got[4] == got[5] == 0.0
        want = (c_eps / sb, c_x0_ddim - c_eps * sa / sb, sigma)
        assert np.allclose((got[2], got[3], got[6]), want, rtol=0.0, atol=1e-12), (i, got, want)
        assert (got[6] == 0.0) == (i == n - 1 and final == 1.0)


def test_level_coefficients_are_the_solvers():
    from vidtome_amd import EditFriendlyInversion
    s = _solver(20, solver_order=2)
    table = EditFriendlyInversion(s).level_coefficients()
    assert len(table) == 20
    for k, (sa, sb) in enumerate(table):
        assert (sa, sb) == s.coefficients(k)[:2] == (math.sqrt(s.alphas[s.timesteps[k]]), math.sqrt(1 - s.alphas[s.timesteps[k]]))


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
@pytest.fixture()
def no_library(monkeypatch):
    """The Python layers must refuse before the library is entered: entering it fails the test."""
    from vidtome_amd import _lib

    def entered():
        raise AssertionError("the library was entered")
    monkeypatch.setattr(_lib, "lib", entered)
    return _lib


def test_wrapper_refuses_before_the_library_is_entered(no_library):
    L = no_library
    x, mo = torch.zeros(7, 4, 8, 8), torch.zeros(6, 4, 8, 8)
    tgt, z, hist = torch.zeros(7, 4, 8, 8), torch.zeros(7, 4, 8, 8), torch.zeros(7, 4, 8, 8)
    coef = (0.9, 0.4, 0.95, 0.3)                                          # sqrt_alpha, sqrt_beta, c_x, c_x0
    ids = [4, 0, 2]
    ok = dict(frame_ids=ids, target=tgt, z_out=z, c_noise=0.2)
    for w, kw, match in (((-6.5, 7.5), dict(pred_type=3), "pred_type"),
                         ((), dict(), "weights"),
                         ((1.0,) * 9, dict(), "weights"),
                         ((1.0, float("nan")), dict(), "weights"),
                         ((1.0, 2.0, 3.0), dict(), "model_out"),                     # 6 != 3 groups x 3 frames
                         ((-6.5, 7.5), dict(rescale=-1.0), "rescale"),
                         ((-6.5, 7.5), dict(rescale=0.5, g_ref=2), "rescale > 0"),
                         ((-6.5, 7.5), dict(rescale=0.5, g_ref=-1), "rescale > 0"),
                         ((0.0, 1.0), dict(rescale=0.5, g_ref=0), "rescale > 0"),      # the reference group has no weight
                         ((-6.5, 7.5), dict(c_h1=0.1), "c_h1 != 0 needs h1"),
                         ((-6.5, 7.5), dict(c_h2=0.1, h1=hist), "c_h2 != 0 needs h2"),
                         ((-6.5, 7.5), dict(h1=hist.half(), c_h1=0.1), "h1 must be an fp32"),
                         ((-6.5, 7.5), dict(h_out=hist[:3]), "h_out must be an fp32"),
                         ((-6.5, 7.5), dict(h2=hist.double()), "h2 must be an fp32"),
                         ((-6.5, 7.5), dict(z_out=None), "z_out is required"),
                         ((-6.5, 7.5), dict(target=None), "c_noise != 0 needs target"),
                         ((-6.5, 7.5), dict(target=tgt[:3]), "target must be a tensor like x"),
                         ((-6.5, 7.5), dict(target=tgt.half()), "target must be a tensor like x"),
                         ((-6.5, 7.5), dict(z_out=z.half()), "z_out must be a tensor like x"),
                         ((-6.5, 7.5), dict(z_out=z[:, :2]), "z_out must be a tensor like x"),
                         ((-6.5, 7.5), dict(target=x), "three buffers"),
                         ((-6.5, 7.5), dict(z_out=x), "three buffers"),
                         ((-6.5, 7.5), dict(z_out=tgt), "three buffers"),
                         ((-6.5, 7.5), dict(target=None, c_noise=0.0), "must live on the GPU"),     # complete, but on the CPU
                         ((-6.5, 7.5), dict(h1=hist, h2=hist, h_out=hist, c_h1=0.1, c_h2=0.1), "must live on the GPU")):
        with pytest.raises(RuntimeError, match=match):
            L.invert_step(x, mo, w, *coef, **dict(ok, **kw))
    for bad_ids, match in (([0, 7, 1], r"outside \[0, 7\)"), ([3, 1, 3], "twice"), ([0, 1], "model_out"), (None, "model_out")):
        with pytest.raises(RuntimeError, match=match):
            L.invert_step(x, mo, (-6.5, 7.5), *coef, **dict(ok, frame_ids=bad_ids))
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        L.invert_step(x, mo.half(), (-6.5, 7.5), *coef, **ok)
    with pytest.raises(RuntimeError, match="fp16 / bf16 / fp32"):
        L.invert_step(x.double(), mo.double(), (-6.5, 7.5), *coef, **ok)
    with pytest.raises(RuntimeError, match="rescale > 0"):                          # E = 1
        L.invert_step(torch.zeros(7, 1), torch.zeros(6, 1), (-6.5, 7.5), *coef, frame_ids=ids, rescale=0.5,
                      target=torch.zeros(7, 1), z_out=torch.zeros(7, 1))

    x0, lv, cf = torch.zeros(5, 4, 8), torch.zeros(3, 5, 4, 8), torch.zeros(3, 2)
    for args, match in (((x0, lv, None), "must be a tensor"), ((x0.double(), lv.double(), cf), "fp16 / bf16 / fp32"),
                        ((x0, lv.half(), cf), "fp16 / bf16 / fp32"), ((x0, lv[:, :4], cf), r"not \(n, \*x0.shape\)"),
                        ((x0, lv[0], cf), r"not \(n, \*x0.shape\)"), ((x0, lv, cf[:2]), "coef must be"),
                        ((x0, lv, cf.double()), "coef must be"), ((x0, lv, cf.flatten()), "coef must be"),
                        ((x0, lv, cf), "must live on the GPU")):
        with pytest.raises(RuntimeError, match=match):
            L.noise_levels(*args)


def test_class_refuses_before_the_library_is_entered(no_library):
    from vidtome_amd import EditFriendlyInversion, GuidedDPMSolver
    with pytest.raises(ValueError, match="deterministic"):
        EditFriendlyInversion(GuidedDPMSolver(_alphas(), _timesteps(20)))
    with pytest.raises(TypeError, match="GuidedDPMSolver"):
        EditFriendlyInversion(object())
    n = 6
    s = _solver(n, solver_order=2)
    inv = EditFriendlyInversion(s)
    with pytest.raises(RuntimeError, match="GPU"):
        inv.noise_levels(torch.zeros(7, 4, 8, 8))
    with pytest.raises(RuntimeError, match="frames, ..."):
        inv.noise_levels(torch.zeros(7))
    levels, mo, ids = torch.zeros(n + 1, 7, 4, 8, 8), torch.zeros(6, 4, 8, 8), [0, 1, 2]
    with pytest.raises(RuntimeError, match="levels must be the"):
        inv.step(levels[:n], mo, 0, frame_ids=ids)
    with pytest.raises(RuntimeError, match="levels must be the"):
        inv.step(None, mo, 0, frame_ids=ids)
    for i in (-1, n):
        with pytest.raises(IndexError):
            inv.step(levels, mo, i, frame_ids=ids)
    with pytest.raises(RuntimeError, match="2 groups x 7 frames"):
        inv.step(levels, mo, 0)
    with pytest.raises(RuntimeError, match="3 groups x 3 frames"):
        inv.step(levels, mo, 0, groups=3, frame_ids=ids)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        inv.step(levels, mo.half(), 0, frame_ids=ids)
    with pytest.raises(ValueError, match="want"):
        inv.step(levels, mo, 0, frame_ids=ids, want=("eps", "x1"))
    with pytest.raises(RuntimeError, match="3 group_weights for a call of 2 groups"):
        EditFriendlyInversion(_solver(n, group_weights=(1.0, 2.0, -2.0))).step(levels, mo, 0, frame_ids=ids)
    # out of sequence, by the solver's own rule: nothing was stepped yet, so only step 0 may come; after step 3, only 0, 3, 4
    for i in (1, 5):
        with pytest.raises(RuntimeError, match="out of sequence"):
            inv.step(levels, mo, i, frame_ids=ids)
    s._current = 3
    for i in (2, 5):
        with pytest.raises(RuntimeError, match="out of sequence"):
            inv.step(levels, mo, i, frame_ids=ids)
    for i in (0, 3, 4):
        with pytest.raises(RuntimeError, match="GPU"):                              # in sequence: the next check refuses
            inv.step(levels, mo, i, frame_ids=ids)
    assert s._current == 3 and inv.noise is None                                    # a refused call moves nothing


def test_library_refuses_before_any_launch(built):
    """The exports' own checks: VTM_EINVAL with a message naming the call, on a machine without a GPU as well -- the checks come
    before the launch (the device pointers below are never dereferenced by the host)."""
    from vidtome_amd import _lib
    lib = _lib.lib()
    P, Q, R = 4096, 8192, 12288                                            # non-null, 16-byte aligned stand-in pointers
    good = dict(x=P, mo=P, h1=None, h2=None, dtype=_lib.VTM_F16, F=3, E=256, groups=2, w=(-6.5, 7.5), g_ref=1, ids=None, pred=0,
                rescale=0.0, sa=0.9, sb=0.4, cx=0.95, cx0=0.3, ch1=0.0, ch2=0.0, cn=0.2, tgt=Q, z=R, ho=None, eo=None, x0o=None)

    def call(**kw):
        a = dict(good, **kw)
        w = (ctypes.c_float * max(len(a["w"]), 1))(*a["w"]) if a["w"] is not None else None
        return lib.vtm_invert_step(a["x"], a["mo"], a["h1"], a["h2"], a["dtype"], a["F"], a["E"], a["groups"], w, a["g_ref"],
                                   a["ids"], a["pred"], a["rescale"], a["sa"], a["sb"], a["cx"], a["cx0"], a["ch1"], a["ch2"],
                                   a["cn"], a["tgt"], a["z"], a["ho"], a["eo"], a["x0o"], None)

    nine = (1.0,) * 9
    for kw, word in ((dict(dtype=3), "dtype"), (dict(dtype=-1), "dtype"), (dict(pred=3), "pred_type"), (dict(pred=-1), "pred_type"),
                     (dict(x=None), "required"), (dict(mo=None), "required"), (dict(w=None), "required"),
                     (dict(E=0), "sizes"), (dict(F=-1), "sizes"), (dict(F=(1 << 20) + 1), "sizes"),
                     (dict(groups=0), "sizes"), (dict(groups=9, w=nine), "sizes"),
                     (dict(rescale=-0.5), "rescale"), (dict(rescale=float("nan")), "rescale"),
                     (dict(rescale=0.5, g_ref=2), "g_ref"), (dict(rescale=0.5, g_ref=-1), "g_ref"),
                     (dict(rescale=0.5, g_ref=0, w=(0.0, 1.0)), "non-zero weight"), (dict(rescale=0.5, E=1), "E >= 2"),
                     (dict(tgt=None), "target"), (dict(ch1=0.1), "h1"), (dict(ch2=0.1), "h2"), (dict(ch1=0.1, ch2=0.1, h1=P), "h2"),
                     (dict(z=None), "z_out"), (dict(tgt=P), "three buffers"), (dict(z=P), "three buffers"),
                     (dict(z=Q), "three buffers")):
        assert call(**kw) == EINVAL, kw
        msg = lib.vtm_last_error().decode()
        assert msg.startswith("vtm_invert_step:") and word in msg, (kw, msg)
    # an empty chunk is fine, and still checked; without c_noise the target may be absent; g_ref is ignored without rescale
    assert call(F=0) == 0 and call(F=0, rescale=0.7) == 0 and call(F=0, groups=8, w=nine[:8], g_ref=7, rescale=0.7) == 0
    assert call(F=0, cn=0.0, tgt=None) == 0 and call(F=0, g_ref=99) == 0
    assert call(F=0, ch1=0.1, h1=P, ch2=-0.1, h2=P, ho=P, eo=P, x0o=P) == 0
    assert call(F=0, pred=7) == EINVAL and call(F=0, z=None) == EINVAL

    def levels(x0=P, lv=Q, coef=R, dtype=_lib.VTM_F16, n=3, size=256):
        return lib.vtm_noise_levels(x0, lv, coef, dtype, n, size, None)

    for kw, word in ((dict(dtype=3), "dtype"), (dict(x0=None), "required"), (dict(lv=None), "required"),
                     (dict(coef=None), "required"), (dict(n=-1), "sizes"), (dict(n=(1 << 20) + 1), "sizes"), (dict(size=0), "sizes"),
                     (dict(lv=P), "must not be x0")):
        assert levels(**kw) == EINVAL, kw
        msg = lib.vtm_last_error().decode()
        assert msg.startswith("vtm_noise_levels:") and word in msg, (kw, msg)
    assert levels(n=0) == 0 and levels(n=0, size=0) == EINVAL
