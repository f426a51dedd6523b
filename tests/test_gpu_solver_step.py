"""vtm_solver_step / GuidedDPMSolver.step on the GPU against a float64 numpy restatement of the formulas of
include/vidtome_hip.h.

Every element of every output is held to

    |out - ref| <= u |ref| + gamma_16 * A + [rescale > 0] * 2^-16 * A_m,        gamma_c = c 2^-24 / (1 - c 2^-24)

u = 2^-11 (fp16), 2^-8 (bf16): half an ulp of the stored 16-bit value; 0 for fp32 outputs, whose last rounding is one of the c.
A is the sum of the absolute values of the terms of the output, each term expanded down to the inputs as the formula is
written, in float64 (the scheme of ``hold`` in test_gpu_guided_step.py); A_m is the part of A proportional to m.  Every
partial sum of the kernel's expression is bounded by A, so c roundings cost at most gamma_c * A.

c = 16 is the count of fp32 roundings on the longest path of csrc/solver_step.hip's expression, x_out under epsilon
prediction with three weighted groups (sums start from 0, so each first addition is exact):
    m    = w0 v0 + w1 v1 + w2 v2         w -> fp32 1, product 1, two additions 2                             4
    m    = m * factor                    (rescale; the factor's own error is the std term)                   1
    x0   = (x - sqrt_beta m) / sqrt_alpha    sqrt_beta -> fp32 1, product 1, subtraction 1, sqrt_alpha -> fp32 1, division 1   5
    x'   = c_x x + c_x0 x0 + c_h1 h1 + c_h2 h2 + c_noise noise     c_x0 -> fp32 1, product 1, four additions 4   6
The other paths are shorter (v-prediction: 4 + 1 + 3 + 6; the x, h1, h2, noise terms: 2 + at most 4 additions; eps, x0 and
h_out end before the last line).  The std term is test_gpu_guided_step.py's: 2^-16 is the worst case of the two-pass fp32
reduction in csrc/guided_step.hip's order (<= 128 serial additions per lane, then the butterfly and the tree), which
solver_step.hip keeps, for E <= 2^17 and frames with |mean| <= std; the inputs are N(0, 1) * s, s in [0.5, 2], so that holds.
No element is exempt.  The worst observed error / bound is printed per check (run with -s)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F32, F16, BF16]
IDS = {F32: "fp32", F16: "fp16", BF16: "bf16"}
U = {F32: 0.0, F16: 2.0 ** -11, BF16: 2.0 ** -8}
ROUNDINGS = 16                                       # counted in the module docstring
GAMMA = ROUNDINGS * 2.0 ** -24 / (1.0 - ROUNDINGS * 2.0 ** -24)
PREDS = ["epsilon", "v_prediction", "sample"]
PRED_CODE = {"epsilon": 0, "v_prediction": 1, "sample": 2}
S_CFG, P_PAG, S_T, S_I = 7.5, 3.0, 7.5, 1.5
WEIGHTS = {1: (1.0,), 2: (1.0 - S_CFG, S_CFG), 3: (1.0 - S_CFG, S_CFG + P_PAG, -P_PAG)}      # 3: perturbed-attention guidance
ROWS, N_FRAMES = [5, 0, 3], 7
SIZES = [140, 256, 1024 * 8 + 8 + 3]                 # no 16-bit vector width; a latent frame; more than one workgroup pass


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _alphas():
    """Stable Diffusion's schedule: scaled-linear betas 0.00085 .. 0.012 over 1000 steps."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def _timesteps(n):
    return ((np.arange(n) * (1000 // n))[::-1] + 1).tolist()


def _solver(n=20, **kw):
    from vidtome_amd import GuidedDPMSolver
    return GuidedDPMSolver(_alphas(), _timesteps(n), **kw)


@pytest.fixture(scope="module")
def coef():
    """(sqrt_alpha, sqrt_beta, c_x, c_x0, c_h1, c_h2, c_noise) of a third-order step, with the stochastic solver's c_noise."""
    c = _solver(solver_order=3).coefficients(7)
    assert c[4] != 0.0 and c[5] != 0.0
    return c[:6] + (_solver(algorithm_type="sde-dpmsolver++").coefficients(7)[6],)


def _draw(shape, dtype, seed, offset=0):
    """N(0, 1) * s, s in [0.5, 2], rounded to dtype; ``offset`` elements in front of it in its allocation."""
    g = torch.Generator().manual_seed(seed)
    s = 0.5 + 1.5 * float(torch.rand((), generator=g))
    t = (torch.randn(shape, generator=g) * s).to(dtype)
    if not offset:
        return t.to(DEV)
    buf = torch.empty(t.numel() + offset, dtype=dtype, device=DEV)
    buf[offset:] = t.flatten().to(DEV)
    return buf[offset:].view(shape)


def _f64(t):
    return t.detach().double().cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def reference(x, mo, noise, h1, h2, rows, w, pred, rescale, g_ref, coef):
    """The formulas in float64.  x, h1, h2 (n_frames, E), mo (groups * F, E), noise (F, E), rows: the F rows of x.  A term whose
    coefficient is 0 is absent (its operand may be None).  Returns {"x": (ref, A, A_m), "eps": ..., "x0": ...}, arrays (F, E)."""
    sa, sb, cx, cx0, ch1, ch2, cn = coef
    F = len(rows)
    X = x[list(rows)]
    m, Am = np.zeros_like(X), np.zeros_like(X)
    for g, wg in enumerate(w):
        if wg != 0:
            m, Am = m + wg * mo[g * F:(g + 1) * F], Am + np.abs(wg * mo[g * F:(g + 1) * F])
    if rescale > 0:
        ratio = mo[g_ref * F:(g_ref + 1) * F].std(axis=1, ddof=1, keepdims=True) / m.std(axis=1, ddof=1, keepdims=True)
        m, Am = m * (rescale * ratio + (1 - rescale)), Am * (np.abs(rescale * ratio) + abs(1 - rescale))
    aX = np.abs(X)
    if pred == "epsilon":
        x0, x0_x, x0_m = (X - sb * m) / sa, aX / sa, sb * Am / sa
        ep, ep_x, ep_m = m, 0 * aX, Am
    elif pred == "v_prediction":
        x0, x0_x, x0_m = sa * X - sb * m, sa * aX, sb * Am
        ep, ep_x, ep_m = sa * m + sb * X, sb * aX, sa * Am
    else:
        x0, x0_x, x0_m = m, 0 * aX, Am
        ep, ep_x, ep_m = (X - sa * m) / sb, aX / sb, sa * Am / sb
    xn, xn_x, xn_m = cx * X + cx0 * x0, abs(cx) * aX + abs(cx0) * x0_x, abs(cx0) * x0_m
    for c, t, whole_video in ((ch1, h1, True), (ch2, h2, True), (cn, noise, False)):
        if c != 0:
            t = t[list(rows)] if whole_video else t
            xn, xn_x = xn + c * t, xn_x + np.abs(c * t)
    return {"x": (xn, xn_x + xn_m, xn_m), "eps": (ep, ep_x + ep_m, ep_m), "x0": (x0, x0_x + x0_m, x0_m)}


WORST = {}


def hold(out, ref_A_Am, rescaled, label):
    """Every element within the bound; prints the worst error / bound."""
    ref, A, Am = ref_A_Am
    got = _f64(out).reshape(ref.shape)
    tol = U[out.dtype] * np.abs(ref) + GAMMA * A + (2.0 ** -16 * Am if rescaled else 0.0)
    err = np.abs(got - ref)
    ratio = float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))))
    key = IDS[out.dtype]
    WORST[key] = max(WORST.get(key, 0.0), ratio if np.isfinite(ratio) else np.inf)
    print(f"[solver_step] {key} {label}: worst error / bound {ratio:.4f}  (worst so far {WORST[key]:.4f})")
    bad = ~(err <= tol)                       # NaN counts as a miss
    assert not bad.any(), (label, int(bad.sum()), ratio)


class Inputs:
    """One chunk's operands: x, h1, h2 whole-video (7 frames), model_out / noise of the F = 3 frames ROWS."""

    def __init__(self, dtype, E, groups, seed, offset=0, rows=ROWS, n=N_FRAMES):
        self.rows, self.n, self.E, self.groups, F = rows, n, E, groups, len(rows)
        self.x = _draw((n, E), dtype, seed, offset)
        self.mo = _draw((groups * F, E), dtype, seed + 1, offset)
        self.noise = _draw((F, E), dtype, seed + 2, offset)
        self.h1, self.h2 = _draw((n, E), F32, seed + 3, offset), _draw((n, E), F32, seed + 4, offset)

    def run(self, L, coef, pred, rescale, w=None, hist=2, noise=True, g_ref=None, x=None, out=None, h2=None, h_out=None):
        """-> (x_out, eps, x0, h_out); sentinel 3.0 in the rows nobody writes."""
        c = list(coef)
        c[4], c[5], c[6] = c[4] if hist >= 1 else 0.0, c[5] if hist >= 2 else 0.0, c[6] if noise else 0.0
        x = self.x if x is None else x
        out = torch.full_like(self.x, 3.0) if out is None else out
        h_out = torch.full_like(self.h1, 3.0) if h_out is None else h_out
        res = L.solver_step(x, self.mo, WEIGHTS[self.groups] if w is None else w, *c, h1=self.h1 if hist >= 1 else None,
                            h2=(self.h2 if h2 is None else h2) if hist >= 2 else None, h_out=h_out, g_ref=g_ref, frame_ids=self.rows,
                            pred_type=PRED_CODE[pred], rescale=rescale, noise=self.noise if noise else None, out=out,
                            want_eps=True, want_x0=True)
        assert res[0] is out
        return out, res[1], res[2], h_out

    def check(self, got, coef, pred, rescale, label, w=None, hist=2, noise=True, g_ref=None):
        c = list(coef)
        c[4], c[5], c[6] = c[4] if hist >= 1 else 0.0, c[5] if hist >= 2 else 0.0, c[6] if noise else 0.0
        w = WEIGHTS[self.groups] if w is None else w
        ref = reference(_f64(self.x), _f64(self.mo), _f64(self.noise), _f64(self.h1), _f64(self.h2), self.rows, w, pred, rescale,
                        len(w) - 1 if g_ref is None else g_ref, c)
        out, eps, x0, h_out = got
        rescaled = rescale > 0
        hold(out[self.rows], ref["x"], rescaled, label + " x'")
        hold(eps, ref["eps"], rescaled, label + " eps")
        hold(x0, ref["x0"], rescaled, label + " x0")
        assert h_out.dtype == F32
        hold(h_out[self.rows], ref["x0"], rescaled, label + " h_out")
        # scatter: the other rows keep the sentinel
        others = [r for r in range(self.n) if r not in self.rows]
        assert bool((out[others] == 3.0).all()) and bool((h_out[others] == 3.0).all()), label


# ---------------------------------------------------------------------------------------------------
# dtypes x prediction types x groups x history terms x noise x rescale
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_dtypes_prediction_types(L, coef, dtype, pred):
    """F = 3 frames of 4 x 8 x 8 scattered into a 7-frame video; three groups carry the perturbed-attention weights."""
    seed = 100 * DTYPES.index(dtype) + 10 * PREDS.index(pred)
    for groups in (1, 2, 3):
        inp = Inputs(dtype, 256, groups, seed + groups)
        for hist in (0, 1, 2):
            for noise in (False, True):
                for rescale in (0.0, 0.7) if groups >= 2 else (0.0,):
                    kw = dict(hist=hist, noise=noise)
                    got = inp.run(L, coef, pred, rescale, **kw)
                    assert got[1].shape == got[2].shape == (3, 256) and got[1].dtype == dtype
                    inp.check(got, coef, pred, rescale, f"{pred} groups={groups} hist={hist} noise={noise} rescale={rescale}", **kw)


@pytest.mark.parametrize("rescale", [0.0, 0.7])
@pytest.mark.parametrize("E", SIZES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_frame_sizes(L, coef, dtype, E, rescale):
    assert SIZES[2] == L.SOLVER_STEP_THREADS * 8 + 8 + 3 and SIZES[2] % 4 == 3 and 140 % 8
    inp = Inputs(dtype, E, 3, 7 * SIZES.index(E))
    for pred in ("v_prediction", "epsilon"):
        inp.check(inp.run(L, coef, pred, rescale), coef, pred, rescale, f"E={E} {pred} rescale={rescale}")


# ---------------------------------------------------------------------------------------------------
# the weights
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescale", [0.0, 0.7])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_group_weights(L, coef, dtype, rescale):
    """A group of weight 0 is never read: full of NaN, it reaches no output (a PnP source group in front of the two guidance
    groups).  Perturbed-attention weights (1 - s, s + p, -p) and InstructPix2Pix weights (s_T, s_I - s_T, 1 - s_I), the
    latter with the rescale reference on group 0 (the fully conditioned one)."""
    inp = Inputs(dtype, 140, 3, 300)
    inp.mo[:3] = float("nan")
    w = (0.0, 1.0 - S_CFG, S_CFG)
    got = inp.run(L, coef, "epsilon", rescale, w=w)
    assert all(bool(torch.isfinite(t).all()) for t in (got[0][ROWS], got[1], got[2], got[3][ROWS]))
    inp.check(got, coef, "epsilon", rescale, f"zero-weight NaN group rescale={rescale}", w=w)
    # ... and two groups given as three with a zero in front are the two-group call, bit for bit
    two = Inputs(dtype, 140, 2, 300)
    two.mo, two.x, two.noise, two.h1, two.h2 = inp.mo[3:].clone(), inp.x, inp.noise, inp.h1, inp.h2
    for a, b in zip(got, two.run(L, coef, "epsilon", rescale)):
        assert torch.equal(_bits(a), _bits(b))
    inp = Inputs(dtype, 140, 3, 310)
    for name, w, g_ref in (("PAG", (1.0 - S_CFG, S_CFG + P_PAG, -P_PAG), None), ("InstructPix2Pix", (S_T, S_I - S_T, 1.0 - S_I), 0)):
        for pred in ("epsilon", "v_prediction"):
            got = inp.run(L, coef, pred, rescale, w=w, g_ref=g_ref)
            inp.check(got, coef, pred, rescale, f"{name} {pred} rescale={rescale}", w=w, g_ref=g_ref)


# ---------------------------------------------------------------------------------------------------
# aliasing, alignment, repeatability
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescale", [0.0, 0.7])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_aliasing(L, coef, dtype, rescale):
    """x_out is x and h_out is h2 (what the ring of a third-order solver does): the bits of the call with separate outputs."""
    for E in (140, 256):
        inp = Inputs(dtype, E, 3, 400 + E)
        apart = inp.run(L, coef, "v_prediction", rescale)
        x, h2 = inp.x.clone(), inp.h2.clone()
        alias = inp.run(L, coef, "v_prediction", rescale, x=x, out=x, h2=h2, h_out=h2)
        assert alias[0] is x and alias[3] is h2
        others = [r for r in range(N_FRAMES) if r not in ROWS]
        for a, b in zip(alias[1:3], apart[1:3]):
            assert torch.equal(_bits(a), _bits(b))
        assert torch.equal(_bits(x[ROWS]), _bits(apart[0][ROWS])) and torch.equal(_bits(x[others]), _bits(inp.x[others]))
        assert torch.equal(_bits(h2[ROWS]), _bits(apart[3][ROWS])) and torch.equal(_bits(h2[others]), _bits(inp.h2[others]))
        # h_out is h1: a second-order solver's ring of one
        h1 = inp.h1.clone()
        keep, inp.h1 = inp.h1, h1
        one = inp.run(L, coef, "v_prediction", rescale, hist=1, h_out=h1)
        inp.h1 = keep
        ref = inp.run(L, coef, "v_prediction", rescale, hist=1)
        assert torch.equal(_bits(one[0]), _bits(ref[0])) and torch.equal(_bits(h1[ROWS]), _bits(ref[3][ROWS]))
        assert torch.equal(_bits(h1[others]), _bits(inp.h1[others]))


@pytest.mark.parametrize("rescale", [0.0, 0.7])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_base_pointer_off_by_one_element(L, coef, dtype, rescale):
    """E % 8 == 0 but no operand is 16-byte aligned: the element path -- within the bound, and the SAME BITS as the aligned call
    (which of the two paths moves the data changes no result, the statistics included)."""
    inp = Inputs(dtype, 256, 3, 500, offset=1)
    assert all(t.data_ptr() % 16 == t.element_size() and t.is_contiguous() for t in (inp.x, inp.mo, inp.noise, inp.h1, inp.h2))
    got = inp.run(L, coef, "v_prediction", rescale)
    inp.check(got, coef, "v_prediction", rescale, f"off-by-one rescale={rescale}")
    aligned = Inputs(dtype, 256, 3, 500)
    assert all(t.data_ptr() % 16 == 0 for t in (aligned.x, aligned.mo, aligned.noise, aligned.h1, aligned.h2))
    assert torch.equal(_bits(aligned.mo), _bits(inp.mo))
    for a, b in zip(got, aligned.run(L, coef, "v_prediction", rescale)):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("rescale", [0.0, 0.7])
@pytest.mark.parametrize("E", SIZES)
def test_repeatable_and_frame_independent(L, coef, E, rescale):
    inp = Inputs(F16, E, 3, 600)
    first, second = inp.run(L, coef, "v_prediction", rescale), inp.run(L, coef, "v_prediction", rescale)
    for a, b in zip(first, second):
        assert torch.equal(_bits(a), _bits(b))
    for f, row in enumerate(ROWS):
        one = Inputs(F16, E, 3, 600, rows=[row])
        one.mo, one.noise = torch.stack([inp.mo[g * 3 + f] for g in range(3)]), inp.noise[f:f + 1].clone()
        alone = one.run(L, coef, "v_prediction", rescale)
        for a, b in ((first[0][row], alone[0][row]), (first[1][f], alone[1][0]), (first[2][f], alone[2][0]),
                     (first[3][row], alone[3][row])):
            assert torch.equal(_bits(a), _bits(b)), (f, E, rescale)


# ---------------------------------------------------------------------------------------------------
# GuidedDPMSolver: chunks against the whole video, on one stream and on two
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_chunks_equal_the_whole_video(dtype):
    """Four third-order steps (history none, one entry, two entries, the ring overwriting) of a 7-frame video: whole-video calls,
    the chunks [5, 0, 3], [1, 6], [2, 4], and those chunks on two HIP streams after ``prepare`` -- the same bits in the latents
    and in both history buffers after every step.  Three groups, the first of weight 0 and full of NaN, with guidance rescale."""
    n, E, groups, steps = 7, 140, 3, 4
    chunks = [[5, 0, 3], [1, 6], [2, 4]]
    kw = dict(solver_order=3, prediction_type="v_prediction", guidance_scale=S_CFG, guidance_rescale=0.7)
    x0 = _draw((n, E), dtype, 700)
    outs = [_draw((groups, n, E), dtype, 701 + k) for k in range(steps)]
    for o in outs:
        o[0] = float("nan")

    def whole():
        s, x, trace = _solver(**kw), x0, []
        for k in range(steps):
            x = s.step(x, outs[k].reshape(groups * n, E), k, groups=groups)
            trace.append((x.clone(), [h.clone() for h in s.history]))
        return trace

    def chunked(streams):
        s, x, nxt, trace = _solver(**kw), x0.clone(), torch.full_like(x0, float("nan")), []
        s.prepare(x)
        for k in range(steps):
            first = torch.cuda.current_stream()
            for st in streams:
                st.wait_stream(first)
            for j, rows in enumerate(chunks):
                with torch.cuda.stream(streams[j % len(streams)]) if streams else torch.cuda.stream(first):
                    ret = s.step(x, outs[k][:, rows].reshape(groups * len(rows), E), k, groups=groups, frame_ids=rows, out=nxt)
                    assert ret is nxt
            for st in streams:
                first.wait_stream(st)
            x, nxt = nxt, x
            trace.append((x.clone(), [h.clone() for h in s.history]))
        return trace

    want = whole()
    assert len(want[0][1]) == 2 and all(bool(torch.isfinite(t[0]).all()) for t in want)
    for streams in ([], [torch.cuda.Stream(), torch.cuda.Stream()]):
        got = chunked(streams)
        torch.cuda.synchronize()
        for k in range(steps):
            assert torch.equal(_bits(got[k][0]), _bits(want[k][0])), (k, len(streams))
            # step k wrote ring slot k % 2; the other slot holds step k - 1's prediction once there is one
            for slot in ((k % 2,) if k == 0 else (0, 1)):
                assert torch.equal(_bits(got[k][1][slot]), _bits(want[k][1][slot])), (k, slot, len(streams))


def test_generator_draws_the_noise():
    s = _solver(algorithm_type="sde-dpmsolver++")
    x, mo = _draw((3, 4, 8, 8), F16, 1), _draw((6, 4, 8, 8), F16, 2)
    drawn = s.step(x, mo, 0, generator=torch.Generator(device=DEV).manual_seed(5))
    noise = torch.randn((3, 4, 8, 8), dtype=F16, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    given = s.step(x, mo, 0, noise=noise)
    assert drawn is not x and drawn.data_ptr() != x.data_ptr() and torch.equal(_bits(drawn), _bits(given))
    assert not torch.equal(drawn, _solver().step(x, mo, 0))
    with pytest.raises(RuntimeError, match="out of sequence"):
        s.step(x, mo, 2)


# ---------------------------------------------------------------------------------------------------
# end to end: 50 steps on the ideal predictor of Gaussian data
# ---------------------------------------------------------------------------------------------------
def _simulate(order, n, x_T):
    """DPM-Solver++ of the given order in float64, from the update formulas as written (no shared code with the sampler):
    -> (final x, sum over the steps of A).  The predictor of x0 ~ N(0, 0.7^2): eps = sigma x / (alpha^2 0.49 + sigma^2)."""
    a = np.array([float(_alphas()[t]) for t in _timesteps(n)] + [1.0])
    alpha, sigma = np.sqrt(a), np.sqrt(1 - a)
    with np.errstate(divide="ignore"):
        lam = np.log(alpha) - np.log(sigma)
    x, ms, A_sum = x_T.copy(), [], np.zeros_like(x_T)
    for i in range(n):
        eps = sigma[i] * x / (alpha[i] ** 2 * 0.49 + sigma[i] ** 2)
        m0 = (x - sigma[i] * eps) / alpha[i]
        A0 = (np.abs(x) + np.abs(sigma[i] * eps)) / alpha[i]
        use = 1 if (order == 1 or i == 0 or i == n - 1) else 2 if (order == 2 or i == 1) else 3      # n = 50 >= 15, a_n = 1
        if i == n - 1:
            x, A = m0, A0
        else:
            h = lam[i + 1] - lam[i]
            e = np.exp(-h) - 1
            terms = [sigma[i + 1] / sigma[i] * x, -alpha[i + 1] * e * m0]
            A = np.abs(terms[0]) + np.abs(alpha[i + 1] * e) * A0
            if use >= 2:
                r0 = (lam[i] - lam[i - 1]) / h
                d10 = (m0 - ms[-1]) / r0
                Ad10 = (A0 + np.abs(ms[-1])) / r0
            if use == 2:
                terms.append(-0.5 * alpha[i + 1] * e * d10)
                A = A + np.abs(0.5 * alpha[i + 1] * e) * Ad10
            if use == 3:
                r1 = (lam[i - 1] - lam[i - 2]) / h
                d11 = (ms[-1] - ms[-2]) / r1
                Ad11 = (np.abs(ms[-1]) + np.abs(ms[-2])) / r1
                k = r0 / (r0 + r1)
                c1, c2 = alpha[i + 1] * (e / h + 1), alpha[i + 1] * ((e + h) / h ** 2 - 0.5)
                terms += [c1 * (d10 + k * (d10 - d11)), -c2 * (d10 - d11) / (r0 + r1)]
                A = A + (abs(c1) * (1 + 2 * k) + abs(c2) / (r0 + r1)) * Ad10 + (abs(c1) * k + abs(c2) / (r0 + r1)) * Ad11
            x = sum(terms)
        ms.append(m0)
        A_sum = A_sum + A
    return x, A_sum


def test_end_to_end_fifty_steps():
    """fp32 latents, n = 50, Stable Diffusion's schedule, the project's random chunks, orders 1 to 3.  The final latents equal a
    float64 simulation of the same formulas within n times the per-step bound: the sum over the steps of gamma_18 * A, A
    the step's sum of absolute terms from the simulation (18 = the kernel's 16 + 2 for the predictor's epsilon, which torch
    forms in fp32 as x times a coefficient: the coefficient's rounding and the product's).  Every |c_x| <= 1 and the
    predictor's x0 shrinks x's error (d x0 / d x = 0.49 alpha / (0.49 alpha^2 + sigma^2) <= 1 / alpha applied to a relative
    bound), so a step's error does not grow in the later ones.  Against the exact solution of this linear problem,
    x_T sqrt(0.49 / (alpha_T^2 0.49 + sigma_T^2)), the simulation's relative errors are 3.55e-2, 1.67e-2, 9.0e-3 (orders 1, 2,
    3); the GPU's must show order 2 below 0.6 of order 1 (simulated: 0.47) and order 3 below order 2."""
    from vidtome_amd.scheduler import ChunkScheduler
    n, frames, shape = 50, 7, (4, 8, 8)
    a = [float(_alphas()[t]) for t in _timesteps(n)]
    x_T = torch.randn((frames,) + shape, generator=torch.Generator().manual_seed(11)).to(DEV)
    exact = _f64(x_T) * math.sqrt(0.49 / (a[0] * 0.49 + 1 - a[0]))
    np.random.seed(3)
    torch.manual_seed(3)
    cut = ChunkScheduler(chunk_size=3, merge_global=False)
    gamma = 18 * 2.0 ** -24 / (1 - 18 * 2.0 ** -24)
    rel = {}
    for order in (1, 2, 3):
        s = _solver(n, solver_order=order)
        x, nxt = x_T.clone(), torch.empty_like(x_T)
        for i in range(n):
            k = math.sqrt(1 - a[i]) / (a[i] * 0.49 + 1 - a[i])
            for chunk in cut.get_chunks(frames):
                s.step(x, x[chunk.to(DEV)] * k, i, groups=1, frame_ids=chunk, out=nxt)
            x, nxt = nxt, x
        sim, A_sum = _simulate(order, n, _f64(x_T))
        err = np.abs(_f64(x) - sim)
        print(f"[solver_step] end to end order {order}: worst error / bound {float((err / (gamma * A_sum)).max()):.4f}, "
              f"relative to max |x| {float(err.max() / np.abs(sim).max()):.3e}")
        assert bool((err <= gamma * A_sum).all()), order
        rel[order] = float(np.abs(_f64(x) - exact).max() / np.abs(exact).max())
        sim_rel = float(np.abs(sim - exact).max() / np.abs(exact).max())
        print(f"[solver_step] end to end order {order}: relative error against the exact solution {rel[order]:.4e} "
              f"(float64 simulation {sim_rel:.4e})")
    assert rel[2] < 0.6 * rel[1] and rel[3] < rel[2], rel
