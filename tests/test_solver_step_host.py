"""CPU tests of the guided DPM-Solver++ step (vidtome_amd.sampler.GuidedDPMSolver, _lib.solver_step, vtm_solver_step): the
C-ABI surface, the coefficients against a float64 restatement of the update formulas as the class docstring writes them (D1 and
D2 are formed, nothing is multiplied out), the identities of the multistep update, and every argument error -- raised before
the library is entered by the Python layers, and returned before any launch by the library itself."""
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
    return GuidedDPMSolver(_alphas(), _timesteps(n), **kw)


def test_header_declares_and_lib_binds_the_export(built):
    import vidtome_amd
    from vidtome_amd import _lib, build, sampler
    hdr = open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    decl = re.search(r"int vtm_solver_step\((.*?)\);", hdr, re.S)
    assert decl and len(decl.group(1).split(",")) == len(_lib._SIGNATURES["vtm_solver_step"][0]) == 26
    assert re.search(r"#define VTM_SOLVER_MAX_GROUPS\s+8\b", hdr) and _lib.SOLVER_MAX_GROUPS == 8
    doc = hdr[hdr.index("vtm_solver_step --"):decl.start()]
    for word in ("ONE CHUNK", "fp32", "h_out", "frame_ids", "VTM_EINVAL"):
        assert word in doc, word
    # additive: the ABI version stays
    assert re.search(r"#define VTM_ABI_VERSION 2\b", hdr) and _lib.lib().vtm_version() == _lib.ABI_VERSION == 2
    assert hasattr(ctypes.CDLL(built), "vtm_solver_step") and "vtm_solver_step" in _lib.exported_symbols()
    assert "solver_step.hip" in build.SOURCES and callable(_lib.solver_step)
    assert vidtome_amd.GuidedDPMSolver is sampler.GuidedDPMSolver and "GuidedDPMSolver" in vidtome_amd.__all__
    # what the GPU test sizes its shapes from
    src = open(os.path.join(ROOT, "vidtome_amd", "csrc", "solver_step.hip")).read()
    assert f"constexpr int SS_THREADS = {_lib.SOLVER_STEP_THREADS};" in src


def test_kernels_do_not_spill(built):
    """2 kernels x 3 dtypes x (16-byte | element) accesses: no scratch, no spilled register."""
    from vidtome_amd import build
    res = {k: v for k, v in build.kernel_resources(os.path.join(os.path.dirname(built), "solver_step.o")).items()
           if "solver_step" in k}
    assert len(res) == 12, sorted(res)
    for name, r in res.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)


# ---------------------------------------------------------------------------------------------------
# the coefficients
# ---------------------------------------------------------------------------------------------------
def _restated_order(i, n, solver_order, have, lower_order_final, euler_at_final, a_n):
    if solver_order == 1 or have == 0 or (i == n - 1 and (euler_at_final or (lower_order_final and n < 15) or a_n == 1.0)):
        return 1
    if solver_order == 2 or have == 1 or (i == n - 2 and lower_order_final and n < 15):
        return 2
    return 3


def _restated_update(levels, i, order, sde, x, m0, m1, m2, noise):
    """x' of step i by the formulas, in float64.  levels: a_0 .. a_n."""
    alpha, sigma = np.sqrt(levels), np.sqrt(1.0 - levels)
    with np.errstate(divide="ignore"):
        lam = np.log(alpha) - np.log(sigma)
    if sigma[i + 1] == 0.0:                            # the exact limit
        return m0
    h = lam[i + 1] - lam[i]
    a_n, s_n = alpha[i + 1], sigma[i + 1]
    r0 = (lam[i] - lam[i - 1]) / h if order >= 2 else None
    if sde:
        out = s_n / sigma[i] * np.exp(-h) * x + a_n * (1 - np.exp(-2 * h)) * m0 + s_n * np.sqrt(1 - np.exp(-2 * h)) * noise
        if order == 2:
            out = out + 0.5 * a_n * (1 - np.exp(-2 * h)) * ((m0 - m1) / r0)
        return out
    out = s_n / sigma[i] * x - a_n * (np.exp(-h) - 1) * m0
    if order == 2:
        out = out - 0.5 * a_n * (np.exp(-h) - 1) * ((m0 - m1) / r0)
    if order == 3:
        r1 = (lam[i - 1] - lam[i - 2]) / h
        d10, d11 = (m0 - m1) / r0, (m1 - m2) / r1
        d1 = d10 + r0 / (r0 + r1) * (d10 - d11)
        d2 = (d10 - d11) / (r0 + r1)
        out = out + a_n * ((np.exp(-h) - 1) / h + 1) * d1 - a_n * ((np.exp(-h) - 1 + h) / h ** 2 - 0.5) * d2
    return out


# e^-h - 1 + h is formed from terms of size h with an absolute error of a few 2^-53 and divided by h^2: with h >= 0.04 on
# these schedules (asserted) its error is below 4 * 2^-53 / 0.0016 = 2.8e-13, and the r's that divide it are above 0.1
# (asserted).  Nothing else cancels worse than 1 / h.  The coefficients are O(1 .. 10).
COEF_TOL = 1e-11


@pytest.mark.parametrize("final", [1.0, 0.9991])
@pytest.mark.parametrize("n", [10, 20])
@pytest.mark.parametrize("algo,solver_order", [("dpmsolver++", 1), ("dpmsolver++", 2), ("dpmsolver++", 3),
                                               ("sde-dpmsolver++", 1), ("sde-dpmsolver++", 2)])
def test_coefficients_follow_the_formulas(algo, solver_order, n, final):
    """Every step of n = 10 (< 15: the lower-order end) and n = 20, the first two (have = 0, 1) and the last two among them,
    every ``have`` the step admits, the three switches of the order rule."""
    levels = np.array([float(_alphas()[t]) for t in _timesteps(n)] + [final])
    finite = levels[levels < 1.0]
    steps = np.diff(np.log(np.sqrt(finite)) - np.log(np.sqrt(1 - finite)))
    assert steps.min() >= 0.04 and (steps[:-1] / steps[1:]).min() > 0.1
    unit = np.eye(5)
    seen = set()
    for lower, euler in ((True, False), (False, False), (False, True)):
        s = _solver(n, final_alpha_cumprod=final, solver_order=solver_order, algorithm_type=algo, lower_order_final=lower,
                    euler_at_final=euler)
        for i in range(n):
            for have in range(min(i, solver_order - 1) + 1):
                order = _restated_order(i, n, solver_order, have, lower, euler, final)
                assert s.order(i, have) == order
                seen.add((i if i < 2 else i - n, order))
                got = s.coefficients(i, have)
                assert got == s.coefficients(i) or have < min(i, solver_order - 1)
                assert got[:2] == (math.sqrt(levels[i]), math.sqrt(1 - levels[i]))
                # the update is linear: its value at the unit vectors are the coefficients
                want = [float(_restated_update(levels, i, order, algo.startswith("sde"), *unit[k])) for k in range(5)]
                assert np.allclose(got[2:], want, rtol=0.0, atol=COEF_TOL), (i, have, order, got[2:], want)
                assert all(math.isfinite(c) for c in got)
                if order < 3:
                    assert got[5] == 0.0
                if order < 2:
                    assert got[4] == 0.0
                assert (got[6] != 0.0) == (algo.startswith("sde") and not (i == n - 1 and final == 1.0))
        if final == 1.0:
            assert s.coefficients(n - 1)[2:] == (0.0, 1.0, 0.0, 0.0, 0.0)          # sigma' = 0: the limits, exactly
    # the cases the order rule turns on were all met
    assert (0, 1) in seen and (-1, 1) in seen
    if solver_order >= 2:
        assert (1, 2) in seen and (-2, 2) in seen and ((-1, 2) in seen) == (final < 1.0)
    if solver_order == 3:
        assert ((-1, 3) in seen) == (final < 1.0) and (-2, 3) in seen and (n == 10 or (-2, 2) in seen)


@pytest.mark.parametrize("solver_order", [1, 2, 3])
def test_identities(solver_order):
    n = 20
    s = _solver(n, solver_order=solver_order, final_alpha_cumprod=0.9991, lower_order_final=False)
    levels = [float(_alphas()[t]) for t in _timesteps(n)] + [0.9991]
    for i in range(n):
        sa, sb, c_x, c_x0, c_h1, c_h2, c_noise = s.coefficients(i)
        first = _solver(n, solver_order=1, final_alpha_cumprod=0.9991).coefficients(i)
        assert c_noise == 0.0
        # every history entry equal to m0: the differences D1, D2 vanish, every order is order 1.  (The multiplied-out
        # coefficients are each O(1 / r) = O(1 .. 10): their sum is held to a few roundings of that size.)
        assert c_x == first[2] and abs(c_x0 + c_h1 + c_h2 - first[3]) <= 64 * 2.0 ** -53 * (abs(c_x0) + abs(c_h1) + abs(c_h2))
        # x0 held constant: the step lands on alpha' x0 + sigma' eps_hat, eps_hat = (x - alpha x0) / sigma
        x, x0 = 0.7, -1.3
        a_n, s_n = math.sqrt(levels[i + 1]), math.sqrt(1 - levels[i + 1])
        want = a_n * x0 + s_n * (x - sa * x0) / sb
        got = c_x * x + (c_x0 + c_h1 + c_h2) * x0
        # lambda = log(alpha / sigma) carries an absolute error of a few 2^-53, which e^-h turns into a relative one
        assert abs(got - want) <= 64 * 2.0 ** -53 * (abs(c_x * x) + (abs(c_x0) + abs(c_h1) + abs(c_h2)) * abs(x0)), (i, got, want)


def test_default_weights_and_constructor_errors():
    import types
    from vidtome_amd import GuidedDPMSolver
    s = _solver(guidance_scale=7.5)
    assert s.weights(1) == [1.0] and s.weights(2) == [-6.5, 7.5] and s.weights(3) == [0.0, -6.5, 7.5]
    assert s.weights(5) == [0.0, 0.0, 0.0, -6.5, 7.5]
    pag = _solver(group_weights=(1 - 7.5, 7.5 + 3.0, -3.0))
    assert pag.weights(3) == [-6.5, 10.5, -3.0]
    assert _solver(group_weights=torch.tensor([0.25, 0.75])).weights(2) == [0.25, 0.75]
    for kw, match in ((dict(algorithm_type="sde-dpmsolver++", solver_order=3), "solver_order"),
                      (dict(solver_order=0), "solver_order"), (dict(solver_order=4), "solver_order"),
                      (dict(algorithm_type="dpmsolver"), "algorithm_type"), (dict(prediction_type="velocity"), "prediction_type"),
                      (dict(guidance_rescale=-0.1), ">= 0"), (dict(final_alpha_cumprod=1.5), "alphas_cumprod")):
        with pytest.raises(ValueError, match=match):
            _solver(**kw)
    with pytest.raises(ValueError, match="timesteps"):
        GuidedDPMSolver(_alphas(), [])
    with pytest.raises(IndexError):
        s.coefficients(20)
    with pytest.raises(ValueError, match="have"):
        s.coefficients(5, have=2)                                                 # solver_order 2 keeps one entry
    sch = types.SimpleNamespace(alphas_cumprod=_alphas(), timesteps=torch.tensor(_timesteps(20)),
                                config=types.SimpleNamespace(prediction_type="v_prediction", solver_order=3,
                                                             algorithm_type="dpmsolver++", lower_order_final=False))
    f = GuidedDPMSolver.from_scheduler(sch, guidance_scale=3.0)
    assert (f.prediction_type, f.solver_order, f.lower_order_final, f.euler_at_final, f.final_alpha, f.guidance_scale) == \
        ("v_prediction", 3, False, False, 1.0, 3.0)
    assert GuidedDPMSolver.from_scheduler(sch, solver_order=2).coefficients(7) == _solver(solver_order=2).coefficients(7)


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
    hist = torch.zeros(7, 4, 8, 8)
    coef = (0.9, 0.4, 0.95, 0.3)                                          # sqrt_alpha, sqrt_beta, c_x, c_x0
    ids = [4, 0, 2]
    for w, kw, match in (((-6.5, 7.5), dict(pred_type=3), "pred_type"),
                         ((), dict(), "weights"),
                         ((1.0,) * 9, dict(), "weights"),
                         ((1.0, float("nan")), dict(), "weights"),
                         ((1.0, 2.0, 3.0), dict(), "model_out"),                     # 6 != 3 groups x 3 frames
                         ((-6.5, 7.5), dict(rescale=-1.0), "rescale"),
                         ((-6.5, 7.5), dict(rescale=0.5, g_ref=2), "rescale > 0"),
                         ((-6.5, 7.5), dict(rescale=0.5, g_ref=-1), "rescale > 0"),
                         ((0.0, 1.0), dict(rescale=0.5, g_ref=0), "rescale > 0"),      # the reference group has no weight
                         ((-6.5, 7.5), dict(want_x=False), "no output"),
                         ((-6.5, 7.5), dict(c_noise=0.1), "c_noise != 0 needs noise"),
                         ((-6.5, 7.5), dict(c_h1=0.1), "c_h1 != 0 needs h1"),
                         ((-6.5, 7.5), dict(c_h2=0.1, h1=hist), "c_h2 != 0 needs h2"),
                         ((-6.5, 7.5), dict(h1=hist.half(), c_h1=0.1), "h1 must be an fp32"),
                         ((-6.5, 7.5), dict(h_out=hist[:3]), "h_out must be an fp32"),
                         ((-6.5, 7.5), dict(h2=hist.double()), "h2 must be an fp32"),
                         ((-6.5, 7.5), dict(out=torch.zeros(3, 4, 8, 8)), "out must be"),
                         ((-6.5, 7.5), dict(noise=torch.zeros(2, 4, 8, 8)), "noise must be"),
                         ((-6.5, 7.5), dict(noise=torch.zeros(3, 4, 8, 8).half(), c_noise=0.1), "noise must be"),
                         ((-6.5, 7.5), dict(h1=hist, h2=hist, h_out=hist, c_h1=0.1, c_h2=0.1), "must live on the GPU")):
        with pytest.raises(RuntimeError, match=match):
            L.solver_step(x, mo, w, *coef, **dict(dict(frame_ids=ids), **kw))
    for bad_ids, match in (([0, 7, 1], r"outside \[0, 7\)"), ([3, 1, 3], "twice"), ([0, 1], "model_out"), (None, "model_out")):
        with pytest.raises(RuntimeError, match=match):
            L.solver_step(x, mo, (-6.5, 7.5), *coef, frame_ids=bad_ids)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        L.solver_step(x, mo.half(), (-6.5, 7.5), *coef, frame_ids=ids)
    with pytest.raises(RuntimeError, match="fp16 / bf16 / fp32"):
        L.solver_step(x.double(), mo.double(), (-6.5, 7.5), *coef, frame_ids=ids)
    with pytest.raises(RuntimeError, match="rescale > 0"):                          # E = 1
        L.solver_step(torch.zeros(7, 1), torch.zeros(6, 1), (-6.5, 7.5), *coef, frame_ids=ids, rescale=0.5)


def test_sampler_refuses_before_the_library_is_entered(no_library):
    x, mo = torch.zeros(7, 4, 8, 8), torch.zeros(6, 4, 8, 8)
    ids = [0, 1, 2]
    with pytest.raises(ValueError, match="solver_order"):
        _solver(algorithm_type="sde-dpmsolver++", solver_order=3)
    s = _solver(solver_order=3)
    with pytest.raises(RuntimeError, match="GPU"):
        s.step(x, mo, 0, frame_ids=ids)
    with pytest.raises(RuntimeError, match="GPU"):
        _solver(algorithm_type="sde-dpmsolver++").step(x, mo, 0, frame_ids=ids, noise=torch.zeros(3, 4, 8, 8))
    with pytest.raises(RuntimeError, match="GPU"):
        s.prepare(x)
    with pytest.raises(RuntimeError, match="2 groups x 7 frames"):
        s.step(x, mo, 0)
    with pytest.raises(RuntimeError, match="3 groups x 3 frames"):
        s.step(x, mo, 0, groups=3, frame_ids=ids)
    with pytest.raises(RuntimeError, match="3 group_weights for a call of 2 groups"):
        _solver(group_weights=(1.0, 2.0, -2.0)).step(x, mo, 0, frame_ids=ids)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        s.step(x, mo.half(), 0, frame_ids=ids)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        s.step(x, mo, 0, frame_ids=ids, noise=torch.zeros(3, 4, 8, 8).half())
    with pytest.raises(ValueError, match="want"):
        s.step(x, mo, 0, frame_ids=ids, want=("eps", "x1"))
    with pytest.raises(IndexError):
        s.step(x, mo, 20, frame_ids=ids)
    # out of sequence: nothing was stepped yet, so only step 0 may come; after step 3, only 0, 3 and 4
    for i in (1, 5):
        with pytest.raises(RuntimeError, match="out of sequence"):
            s.step(x, mo, i, frame_ids=ids)
    s._current = 3
    for i in (2, 5, 19):
        with pytest.raises(RuntimeError, match="out of sequence"):
            s.step(x, mo, i, frame_ids=ids)
    for i in (0, 3, 4):
        with pytest.raises(RuntimeError, match="GPU"):                              # in sequence: the next check refuses
            s.step(x, mo, i, frame_ids=ids)
    assert s._current == 3                                                          # a refused call moves nothing


def test_library_refuses_before_any_launch(built):
    """vtm_solver_step's own checks: VTM_EINVAL with a message naming the call, on a machine without a GPU as well -- the
    checks come before the launch (the device pointers below are never dereferenced by the host)."""
    from vidtome_amd import _lib
    lib = _lib.lib()
    P = 4096                                                               # a non-null, 16-byte aligned stand-in pointer
    good = dict(x=P, mo=P, noise=None, h1=None, h2=None, dtype=_lib.VTM_F16, F=3, E=256, groups=2, w=(-6.5, 7.5), g_ref=1,
                ids=None, pred=0, rescale=0.0, sa=0.9, sb=0.4, cx=0.95, cx0=0.3, ch1=0.0, ch2=0.0, cn=0.0, xo=P, ho=None, eo=None,
                x0o=None)

    def call(**kw):
        a = dict(good, **kw)
        w = (ctypes.c_float * max(len(a["w"]), 1))(*a["w"]) if a["w"] is not None else None
        return lib.vtm_solver_step(a["x"], a["mo"], a["noise"], a["h1"], a["h2"], a["dtype"], a["F"], a["E"], a["groups"], w,
                                   a["g_ref"], a["ids"], a["pred"], a["rescale"], a["sa"], a["sb"], a["cx"], a["cx0"], a["ch1"],
                                   a["ch2"], a["cn"], a["xo"], a["ho"], a["eo"], a["x0o"], None)

    nine = (1.0,) * 9
    for kw, word in ((dict(dtype=3), "dtype"), (dict(dtype=-1), "dtype"), (dict(pred=3), "pred_type"), (dict(pred=-1), "pred_type"),
                     (dict(x=None), "required"), (dict(mo=None), "required"), (dict(w=None), "required"),
                     (dict(E=0), "sizes"), (dict(F=-1), "sizes"), (dict(F=(1 << 20) + 1), "sizes"),
                     (dict(groups=0), "sizes"), (dict(groups=9, w=nine), "sizes"),
                     (dict(rescale=-0.5), "rescale"), (dict(rescale=float("nan")), "rescale"),
                     (dict(rescale=0.5, g_ref=2), "g_ref"), (dict(rescale=0.5, g_ref=-1), "g_ref"),
                     (dict(rescale=0.5, g_ref=0, w=(0.0, 1.0)), "non-zero weight"), (dict(rescale=0.5, E=1), "E >= 2"),
                     (dict(cn=0.1), "noise"), (dict(ch1=0.1), "h1"), (dict(ch2=0.1), "h2"), (dict(ch1=0.1, ch2=0.1, h1=P), "h2"),
                     (dict(xo=None), "no output")):
        assert call(**kw) == EINVAL, kw
        msg = lib.vtm_last_error().decode()
        assert msg.startswith("vtm_solver_step:") and word in msg, (kw, msg)
    # an empty chunk is fine, and still checked; any one output will do; g_ref is ignored without rescale
    assert call(F=0) == 0 and call(F=0, rescale=0.7) == 0 and call(F=0, groups=8, w=nine[:8], g_ref=7, rescale=0.7) == 0
    for only in ("ho", "eo", "x0o"):
        assert call(F=0, xo=None, **{only: P}) == 0
    assert call(F=0, g_ref=99) == 0 and call(F=0, cn=0.1, noise=P, ch1=0.1, h1=P, ch2=-0.1, h2=P, ho=P) == 0
    assert call(F=0, pred=7) == EINVAL and call(F=1 << 20, E=1, xo=None) == EINVAL
