"""CPU tests of the guided DDIM step (vidtome_amd.sampler.GuidedDDIM, _lib.guided_step, vtm_guided_step): the C-ABI surface,
the coefficients against the scalars recorded with the reference's ``pred_next_x`` (tests/golden/ddim.npz), the eta
identities, and every argument error -- raised before the library is entered by the Python layers, and returned before any
launch by the library itself (no GPU is needed to see VTM_EINVAL: nothing is launched)."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1      # include/vidtome_hip.h VTM_EINVAL


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


def _schedule():
    """tests/golden/make_golden_chunks.py's stand-in scheduler."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    return types.SimpleNamespace(alphas_cumprod=torch.cumprod(1.0 - betas, dim=0), timesteps=torch.arange(981, -1, -20),
                                 final_alpha_cumprod=torch.tensor(1.0))


def test_header_declares_and_lib_binds_the_export(built):
    import vidtome_amd
    from vidtome_amd import _lib, build, sampler
    hdr = open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    decl = re.search(r"int vtm_guided_step\((.*?)\);", hdr, re.S)
    assert decl and len(decl.group(1).split(",")) == len(_lib._SIGNATURES["vtm_guided_step"][0]) == 22
    for name, value in (("VTM_PRED_EPSILON", 0), ("VTM_PRED_V", 1), ("VTM_PRED_SAMPLE", 2)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), hdr), name
    assert (_lib.PRED_EPSILON, _lib.PRED_V, _lib.PRED_SAMPLE) == (0, 1, 2)
    doc = hdr[hdr.index("vtm_guided_step --"):decl.start()]
    assert "generate.py:239-311" in doc and "invert.py:181-211" in doc
    assert re.search(r"#define VTM_ABI_VERSION 2\b", hdr) and _lib.lib().vtm_version() == _lib.ABI_VERSION == 2
    assert hasattr(ctypes.CDLL(built), "vtm_guided_step") and "vtm_guided_step" in _lib.exported_symbols()
    assert "guided_step.hip" in build.SOURCES and callable(_lib.guided_step)
    assert vidtome_amd.GuidedDDIM is sampler.GuidedDDIM and "GuidedDDIM" in vidtome_amd.__all__
    # what the GPU test sizes its shapes from
    src = open(os.path.join(ROOT, "vidtome_amd", "csrc", "guided_step.hip")).read()
    assert f"constexpr int GS_THREADS = {_lib.GUIDED_STEP_THREADS};" in src
    assert (_lib.guided_step_chunk(torch.float32), _lib.guided_step_chunk(torch.float16), _lib.guided_step_chunk(torch.bfloat16)) \
        == (4, 8, 8)


def test_kernels_do_not_spill(built):
    """2 kernels x 3 dtypes x (16-byte | element) accesses: no scratch, no spilled register."""
    from vidtome_amd import build
    res = {k: v for k, v in build.kernel_resources(os.path.join(os.path.dirname(built), "guided_step.o")).items()
           if "guided_step" in k}
    assert len(res) == 12, sorted(res)
    for name, r in res.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)


@pytest.mark.parametrize("case,i,inversion", [(0, 0, False), (1, 17, False), (2, 49, False), (3, 5, True), (4, 0, True)])
def test_coefficients_follow_pred_next_x(case, i, inversion):
    from vidtome_amd import GuidedDDIM
    z = np.load(os.path.join(ROOT, "tests", "golden", "ddim.npz"))
    s = GuidedDDIM.from_scheduler(_schedule())
    assert s.prediction_type == "epsilon" and s.eta == 0.0
    a_from, a_to, sqrt_alpha, sqrt_beta, c_x0, c_eps, sigma = s.coefficients(i, inversion)
    for k in (case, case + 5):                                       # the fp32 and the fp16 recording share the scalars
        apt, app, inv = z[f"{k}/meta"][:3].tolist()                  # alphas[t], the "prev" alpha of generate.py:288-298
        assert bool(inv) == inversion
        # generate.py:304-309: sampling divides by mu (of alphas[t]) and lands on the prev level, inversion the other way round
        assert (a_from, a_to) == ((app, apt) if inversion else (apt, app))          # exactly
    assert sigma == 0.0
    assert (sqrt_alpha, sqrt_beta, c_x0, c_eps) == (math.sqrt(a_from), math.sqrt(1 - a_from), math.sqrt(a_to),
                                                    math.sqrt(1 - a_to))
    # the fp32 scalars the reference derived (meta[4:8] = mu, sigma, mu_prev, sigma_prev of alphas[t] / prev)
    mu, sg, mu_p, sg_p = z[f"{case}/meta"][4:8].tolist()
    want = (mu_p, sg_p, mu, sg) if inversion else (mu, sg, mu_p, sg_p)
    assert np.allclose((sqrt_alpha, sqrt_beta, c_x0, c_eps), want, rtol=2.0 ** -22, atol=0.0)    # two fp32 roundings each


def test_eta_identities_and_constructor_errors():
    from vidtome_amd import GuidedDDIM
    sch = _schedule()
    s1 = GuidedDDIM.from_scheduler(sch, eta=1.0)
    for i in (0, 17, 48, 49):
        a_from, a_to, _, _, c_x0, c_eps, sigma = s1.coefficients(i)
        want = math.sqrt((1 - a_to) / (1 - a_from)) * math.sqrt(1 - a_from / a_to)
        assert sigma == want and (sigma > 0) == (i < 49)                     # the last step lands on alpha = 1: no noise left
        assert abs(sigma ** 2 + c_eps ** 2 - (1 - a_to)) <= 4 * 2.0 ** -53 and c_x0 == math.sqrt(a_to)
        assert GuidedDDIM.from_scheduler(sch, eta=0.5).coefficients(i)[6] == 0.5 * want
        assert GuidedDDIM.from_scheduler(sch).coefficients(i)[6] == 0.0
    with pytest.raises(ValueError, match="eta"):
        s1.coefficients(3, inversion=True)
    with pytest.raises(ValueError, match="prediction_type"):
        GuidedDDIM.from_scheduler(sch, prediction_type="velocity")
    with pytest.raises(IndexError):
        s1.coefficients(50)
    with pytest.raises(ValueError, match=">= 0"):
        GuidedDDIM.from_scheduler(sch, guidance_rescale=-0.1)
    sch.config = types.SimpleNamespace(prediction_type="v_prediction")
    assert GuidedDDIM.from_scheduler(sch).prediction_type == "v_prediction"
    assert GuidedDDIM.from_scheduler(sch, prediction_type="sample").prediction_type == "sample"
    lists = GuidedDDIM(sch.alphas_cumprod.tolist(), list(range(981, -1, -20)), eta=1.0)
    assert lists.coefficients(17) == s1.coefficients(17)


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
    coef = (0.9, 0.4, 0.95, 0.3)
    ids = [4, 0, 2]
    for kw, match in ((dict(frame_ids=ids, pred_type=3), "pred_type"),
                      (dict(frame_ids=ids, g_uncond=2), "group index"),
                      (dict(frame_ids=ids, g_cond=-2), "group index"),
                      (dict(frame_ids=ids, g_uncond=1, g_cond=1), "g_uncond == g_cond"),
                      (dict(frame_ids=ids, groups=0), "group index"),
                      (dict(frame_ids=ids, rescale=-1.0), "rescale"),
                      (dict(frame_ids=ids, rescale=0.5, g_uncond=0, g_cond=-1), "rescale > 0"),
                      (dict(frame_ids=ids, want_x=False), "no output"),
                      (dict(frame_ids=[0, 1]), "model_out"),                        # 6 != 2 groups x 2 frames
                      (dict(frame_ids=None), "model_out"),                          # 6 != 2 groups x 7 frames
                      (dict(frame_ids=[0, 7, 1]), r"outside \[0, 7\)"),
                      (dict(frame_ids=[0, -1, 1]), r"outside \[0, 7\)"),
                      (dict(frame_ids=[3, 1, 3]), "twice"),
                      (dict(frame_ids=torch.tensor([3, 1, 3])), "twice"),
                      (dict(frame_ids=torch.tensor([0.0, 1.0, 2.0])), "integer"),
                      (dict(frame_ids=[0, 1.5, 2]), "integers"),
                      (dict(frame_ids=ids, out=torch.zeros(3, 4, 8, 8)), "out must be"),
                      (dict(frame_ids=ids, noise=torch.zeros(2, 4, 8, 8)), "noise must be"),
                      (dict(frame_ids=ids, noise=torch.zeros(3, 4, 8, 8).half()), "noise must be"),
                      (dict(frame_ids=ids), "must live on the GPU")):              # everything else right: host tensors
        with pytest.raises(RuntimeError, match=match):
            L.guided_step(x, mo, *coef, **kw)
    with pytest.raises(RuntimeError, match="sigma != 0 needs noise"):
        L.guided_step(x, mo, *coef, 0.1, frame_ids=ids)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        L.guided_step(x, mo.half(), *coef, frame_ids=ids)
    with pytest.raises(RuntimeError, match="fp16 / bf16 / fp32"):
        L.guided_step(x.double(), mo.double(), *coef, frame_ids=ids)
    with pytest.raises(RuntimeError, match="rescale > 0"):                          # E = 1
        L.guided_step(torch.zeros(7, 1), torch.zeros(6, 1), *coef, frame_ids=ids, rescale=0.5)
    # an ascending run is a row offset, anything else a list to upload
    assert L._frame_rows(range(2, 5), 7, "t") == (2, None, 3) and L._frame_rows(torch.arange(2, 5), 7, "t") == (2, None, 3)
    assert L._frame_rows([4, 0, 2], 7, "t") == (0, [4, 0, 2], 3) and L._frame_rows(None, 7, "t") == (0, None, 7)


def test_sampler_refuses_before_the_library_is_entered(no_library):
    from vidtome_amd import GuidedDDIM
    s = GuidedDDIM.from_scheduler(_schedule(), eta=1.0)
    x, mo = torch.zeros(7, 4, 8, 8), torch.zeros(6, 4, 8, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        s.step(x, mo, 3, frame_ids=[0, 1, 2])
    with pytest.raises(RuntimeError, match="GPU"):
        s.step(x, mo, 3, frame_ids=[0, 1, 2], noise=torch.zeros(3, 4, 8, 8))
    with pytest.raises(RuntimeError, match="2 groups x 7 frames"):
        s.step(x, mo, 3)
    with pytest.raises(RuntimeError, match="3 groups x 3 frames"):
        s.step(x, mo, 3, groups=3, frame_ids=[0, 1, 2])
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        s.step(x, mo.half(), 3, frame_ids=[0, 1, 2])
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        s.step(x, mo, 3, frame_ids=[0, 1, 2], noise=torch.zeros(3, 4, 8, 8).half())
    with pytest.raises(ValueError, match="want"):
        s.step(x, mo, 3, frame_ids=[0, 1, 2], want=("eps", "x1"))
    with pytest.raises(ValueError, match="eta"):
        s.step(x, mo, 3, frame_ids=[0, 1, 2], inversion=True)


def test_library_refuses_before_any_launch(built):
    """vtm_guided_step's own checks: VTM_EINVAL with a message naming the call, on a machine without a GPU as well -- the
    checks come before the launch (the pointers below are never dereferenced by the host)."""
    from vidtome_amd import _lib
    lib = _lib.lib()
    P = 4096                                                               # a non-null, 16-byte aligned stand-in pointer
    good = dict(x=P, mo=P, noise=None, dtype=_lib.VTM_F16, F=3, E=256, groups=2, gu=0, gc=1, ids=None, pred=0, guidance=7.5,
                rescale=0.0, sa=0.9, sb=0.4, cx=0.95, ce=0.3, sigma=0.0, xo=P, eo=None, x0o=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vtm_guided_step(a["x"], a["mo"], a["noise"], a["dtype"], a["F"], a["E"], a["groups"], a["gu"], a["gc"], a["ids"],
                                   a["pred"], a["guidance"], a["rescale"], a["sa"], a["sb"], a["cx"], a["ce"], a["sigma"], a["xo"],
                                   a["eo"], a["x0o"], None)

    for kw, word in ((dict(dtype=3), "dtype"), (dict(dtype=-1), "dtype"), (dict(pred=3), "pred_type"), (dict(pred=-1), "pred_type"),
                     (dict(gu=2), "g_uncond"), (dict(gu=-1), "g_uncond"), (dict(gc=2), "g_cond"), (dict(gc=-2), "g_cond"),
                     (dict(gu=1), "g_uncond == g_cond"), (dict(sigma=0.1), "noise"),
                     (dict(rescale=0.5, gc=-1), "rescale"), (dict(rescale=0.5, E=1), "rescale"), (dict(rescale=-0.5), "rescale"),
                     (dict(xo=None), "no output"), (dict(x=None), "required"), (dict(mo=None), "required"),
                     (dict(E=0), "sizes"), (dict(F=-1), "sizes"), (dict(groups=0), "sizes")):
        assert call(**kw) == EINVAL, kw
        msg = lib.vtm_last_error().decode()
        assert msg.startswith("vtm_guided_step:") and word in msg, (kw, msg)
    # an empty chunk is fine, and still checked
    assert call(F=0) == 0 and call(F=0, rescale=0.7) == 0 and call(F=0, xo=None, eo=P) == 0
    assert call(F=0, pred=7) == EINVAL
