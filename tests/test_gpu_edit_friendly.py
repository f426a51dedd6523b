"""vtm_invert_step / vtm_noise_levels / EditFriendlyInversion on the GPU: the noise maps against a float64 numpy restatement of
the formulas of include/vidtome_hip.h, and the property the kernel exists for -- sampling with the stored noise reproduces the
corrected levels BIT FOR BIT.

Every element of z_out is held to

    |z - ref| <= u |ref| + gamma_18 * (A_mu + |target|) / |c_noise| + [rescale > 0] * 2^-16 * A_m / |c_noise|

gamma_c = c 2^-24 / (1 - c 2^-24); u = 2^-11 (fp16), 2^-8 (bf16): half an ulp of the stored 16-bit value; 0 for fp32, whose last
rounding (the division) is one of the c.  A_mu is the sum of the absolute values of the terms of mu, each expanded down to the
inputs as the formula is written, in float64 (the scheme of test_gpu_solver_step.py); A_m is the part of A_mu proportional to
m.  Every partial result of the kernel's expression is bounded by (A_mu + |target|) / |c_noise|, so c roundings cost at most
gamma_c times that.

c = 18 is the count of fp32 roundings on the longest path of csrc/invert_step.hip's expression, z_out under epsilon prediction
with three weighted groups (sums start from 0, so each first addition is exact):
    m    = w0 v0 + w1 v1 + w2 v2         w -> fp32 1, product 1, two additions 2                                         4
    m    = m * factor                    (rescale; the factor's own error is the std term)                               1
    x0   = (x - sqrt_beta m) / sqrt_alpha    sqrt_beta -> fp32 1, product 1, subtraction 1, sqrt_alpha -> fp32 1, division 1    5
    mu   = c_x x + c_x0 x0 + c_h1 h1 + c_h2 h2     c_x0 -> fp32 1, product 1, three additions 3                          5
    z    = (target - mu) / c_noise       subtraction 1, c_noise -> fp32 1, division 1                                    3
The other paths are shorter (v-prediction: 4 + 1 + 3 + 5 + 3; the x, h1, h2 terms: 2 + at most 3 additions + 3).  The std term
is test_gpu_solver_step.py's: the two-pass fp32 reduction is step_core.h's, shared by both kernels; the inputs are N(0, 1) * s,
s in [0.5, 2].  vtm_noise_levels' sqrt_alpha x0 + sqrt_beta noise is two products and one addition from an fp32 table: gamma_3.
No element is exempt.  The worst observed error / bound is printed per check (run with -s)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F32, F16, BF16]
IDS = {F32: "fp32", F16: "fp16", BF16: "bf16"}
U = {F32: 0.0, F16: 2.0 ** -11, BF16: 2.0 ** -8}


def _gamma(c):
    return c * 2.0 ** -24 / (1.0 - c * 2.0 ** -24)


GAMMA, GAMMA_LEVELS = _gamma(18), _gamma(3)          # counted in the module docstring
PREDS = ["epsilon", "v_prediction", "sample"]
PRED_CODE = {"epsilon": 0, "v_prediction": 1, "sample": 2}
S_CFG, P_PAG = 7.5, 3.0
WEIGHTS = {1: (1.0,), 2: (1.0 - S_CFG, S_CFG), 3: (1.0 - S_CFG, S_CFG + P_PAG, -P_PAG)}
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
    return GuidedDPMSolver(_alphas(), _timesteps(n), **dict(dict(algorithm_type="sde-dpmsolver++"), **kw))


@pytest.fixture(scope="module")
def coefs():
    """(sqrt_alpha, sqrt_beta, c_x, c_x0, c_h1, c_h2, c_noise) of step 7 of 20 of the stochastic solver at orders 1 and 2; under 3,
    the deterministic third-order step's coefficients with the stochastic c_noise, for the h2 term no real step of this solver
    has; under 0, the step that lands on alphas_cumprod = 1."""
    one, two = _solver(solver_order=1).coefficients(7), _solver(solver_order=2).coefficients(7)
    three = _solver(solver_order=3, algorithm_type="dpmsolver++").coefficients(7)[:6] + (two[6],)
    last = _solver(solver_order=2).coefficients(19)
    assert one[4] == 0.0 and two[4] != 0.0 and two[5] == 0.0 and three[5] != 0.0 and one[6] != 0.0 and last[2:] == (0, 1, 0, 0, 0)
    return {0: last, 1: one, 2: two, 3: three}


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


def _like(t, offset):
    """An uninitialised tensor like t with the same misalignment."""
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=DEV)
    return buf[offset:].view(t.shape)


def _f64(t):
    return t.detach().double().cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def reference(x, mo, target, h1, h2, rows, w, pred, rescale, g_ref, coef):
    """The formulas in float64.  x, target, h1, h2 (n_frames, E), mo (groups * F, E), rows: the F rows.  A term whose coefficient
    is 0 is absent.  Returns (z, A_mu + |target|, A_m), arrays (F, E), before the division by |c_noise|."""
    sa, sb, cx, cx0, ch1, ch2, cn = coef
    F = len(rows)
    X, T = x[list(rows)], target[list(rows)]
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
    elif pred == "v_prediction":
        x0, x0_x, x0_m = sa * X - sb * m, sa * aX, sb * Am
    else:
        x0, x0_x, x0_m = m, 0 * aX, Am
    mu, mu_x, mu_m = cx * X + cx0 * x0, abs(cx) * aX + abs(cx0) * x0_x, abs(cx0) * x0_m
    for c, t in ((ch1, h1), (ch2, h2)):
        if c != 0:
            mu, mu_x = mu + c * t[list(rows)], mu_x + np.abs(c * t[list(rows)])
    return (T - mu) / cn, mu_x + mu_m + np.abs(T), mu_m


WORST = {}


def hold(out, ref, tol, label):
    """Every element within the bound; prints the worst error / bound."""
    got = _f64(out).reshape(ref.shape)
    err = np.abs(got - ref)
    ratio = float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))))
    key = IDS[out.dtype]
    WORST[key] = max(WORST.get(key, 0.0), ratio if np.isfinite(ratio) else np.inf)
    print(f"[edit_friendly] {key} {label}: worst error / bound {ratio:.4f}  (worst so far {WORST[key]:.4f})")
    bad = ~(err <= tol)                       # NaN counts as a miss
    assert not bad.any(), (label, int(bad.sum()), ratio)


class Inputs:
    """One chunk's operands: x, target, h1, h2 whole-video (7 frames), model_out of the F = 3 frames ROWS."""

    def __init__(self, dtype, E, groups, seed, offset=0, rows=ROWS, n=N_FRAMES):
        self.rows, self.n, self.E, self.groups, self.offset, F = rows, n, E, groups, offset, len(rows)
        self.x = _draw((n, E), dtype, seed, offset)
        self.mo = _draw((groups * F, E), dtype, seed + 1, offset)
        self.target = _draw((n, E), dtype, seed + 2, offset)
        self.h1, self.h2 = _draw((n, E), F32, seed + 3, offset), _draw((n, E), F32, seed + 4, offset)
        self.z0, self.h0 = _draw((n, E), dtype, seed + 5, offset), _draw((n, E), F32, seed + 6, offset)

    def _kw(self, coef, w, g_ref, rescale, pred):
        return dict(h1=self.h1 if coef[4] != 0.0 else None, h2=self.h2 if coef[5] != 0.0 else None, g_ref=g_ref,
                    frame_ids=self.rows, pred_type=PRED_CODE[pred], rescale=rescale, want_eps=True, want_x0=True)

    def invert(self, L, coef, pred, rescale, w=None, g_ref=None, mo=None):
        """-> (z_out, corrected target, h_out, eps, x0); the whole-video outputs start from random contents."""
        w = WEIGHTS[self.groups] if w is None else w
        target, z, h_out = _like(self.target, self.offset), _like(self.z0, self.offset), _like(self.h0, self.offset)
        target.copy_(self.target), z.copy_(self.z0), h_out.copy_(self.h0)
        eps, x0 = L.invert_step(self.x, self.mo if mo is None else mo, w, *coef, target=target, z_out=z, h_out=h_out,
                                **self._kw(coef, w, g_ref, rescale, pred))
        return z, target, h_out, eps, x0

    def forward(self, L, coef, pred, rescale, z, w=None, g_ref=None):
        """vtm_solver_step on the same operands with noise = z[rows] -> (x_out, h_out, eps, x0)."""
        w = WEIGHTS[self.groups] if w is None else w
        noise = _like(z[self.rows], self.offset)
        noise.copy_(z[self.rows])
        out, h_out = torch.full_like(self.x, 3.0), torch.full_like(self.h1, 3.0)
        res = L.solver_step(self.x, self.mo, w, *coef, h_out=h_out, noise=noise if coef[6] != 0.0 else None, out=out,
                            **self._kw(coef, w, g_ref, rescale, pred))
        return out, h_out, res[1], res[2]

    def check_z(self, z, coef, pred, rescale, label, w=None, g_ref=None):
        w = WEIGHTS[self.groups] if w is None else w
        ref, A, Am = reference(_f64(self.x), _f64(self.mo), _f64(self.target), _f64(self.h1), _f64(self.h2), self.rows, w, pred,
                               rescale, len(w) - 1 if g_ref is None else g_ref, coef)
        tol = U[z.dtype] * np.abs(ref) + (GAMMA * A + (2.0 ** -16 * Am if rescale > 0 else 0.0)) / abs(coef[6])
        hold(z[self.rows], ref, tol, label + " z")

    def others(self):
        return [r for r in range(self.n) if r not in self.rows]


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def round_trip(L, inp, coef, pred, rescale, label, **kw):
    """invert, then the forward step with the stored noise: the corrected target, the history and the predictions, bit for
    bit; rows outside the chunk keep their bits."""
    z, target, h_out, eps, x0 = inp.invert(L, coef, pred, rescale, **kw)
    out, h_fwd, eps_fwd, x0_fwd = inp.forward(L, coef, pred, rescale, z, **kw)
    rows, others = inp.rows, inp.others()
    assert _same(out[rows], target[rows]), label
    assert _same(h_fwd[rows], h_out[rows]) and _same(eps_fwd, eps) and _same(x0_fwd, x0), label
    assert _same(target[others], inp.target[others]) and _same(z[others], inp.z0[others]), label
    assert _same(h_out[others], inp.h0[others]), label
    assert bool(torch.isfinite(z[rows]).all()), label
    return z, target, h_out


# ---------------------------------------------------------------------------------------------------
# 1. z_out against float64; 2. the round trip; 3. untouched rows
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_dtypes_prediction_types(L, coefs, dtype, pred):
    """F = 3 frames of 4 x 8 x 8 scattered into a 7-frame video; groups 1 / 2 / 3, orders 1 / 2 (and the h2 term), rescale."""
    seed = 100 * DTYPES.index(dtype) + 10 * PREDS.index(pred)
    for groups in (1, 2, 3):
        inp = Inputs(dtype, 256, groups, seed + groups)
        for order in (1, 2, 3):
            for rescale in (0.0, 0.7) if groups >= 2 else (0.0,):
                label = f"{pred} groups={groups} order={order} rescale={rescale}"
                z, _, _ = round_trip(L, inp, coefs[order], pred, rescale, label)
                inp.check_z(z, coefs[order], pred, rescale, label)


@pytest.mark.parametrize("rescale", [0.0, 0.7])
@pytest.mark.parametrize("E", SIZES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_frame_sizes(L, coefs, dtype, E, rescale):
    """Both launch shapes at a size without a 16-bit vector width, a vector size, and a second pass of the per-frame workgroup."""
    assert SIZES[2] == L.SOLVER_STEP_THREADS * 8 + 8 + 3 and SIZES[2] % 4 == 3 and 140 % 8
    inp = Inputs(dtype, E, 3, 7 * SIZES.index(E))
    for pred, order in (("v_prediction", 2), ("epsilon", 1)):
        label = f"E={E} {pred} order={order} rescale={rescale}"
        z, _, _ = round_trip(L, inp, coefs[order], pred, rescale, label)
        inp.check_z(z, coefs[order], pred, rescale, label)


@pytest.mark.parametrize("rescale", [0.0, 0.7])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_base_pointer_off_by_one_element(L, coefs, dtype, rescale):
    """E % 8 == 0 but no whole-video operand is 16-byte aligned: the element path -- within the bound, the round trip exact, and
    the SAME BITS as the aligned call."""
    inp = Inputs(dtype, 256, 3, 500, offset=1)
    assert all(t.data_ptr() % 16 == t.element_size() and t.is_contiguous() for t in (inp.x, inp.mo, inp.target, inp.h1, inp.h2))
    got = round_trip(L, inp, coefs[3], "v_prediction", rescale, f"off-by-one rescale={rescale}")
    assert all(t.data_ptr() % 16 == t.element_size() for t in got)
    inp.check_z(got[0], coefs[3], "v_prediction", rescale, f"off-by-one rescale={rescale}")
    aligned = Inputs(dtype, 256, 3, 500)
    assert all(t.data_ptr() % 16 == 0 for t in (aligned.x, aligned.mo, aligned.target, aligned.h1, aligned.h2))
    assert _same(aligned.mo, inp.mo)
    for a, b in zip(got, aligned.invert(L, coefs[3], "v_prediction", rescale)):
        assert _same(a, b)


# ---------------------------------------------------------------------------------------------------
# 4. c_noise == 0
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescale", [0.0, 0.7])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_step_without_noise(L, coefs, dtype, rescale):
    """The step that lands on alphas_cumprod = 1: z_out's rows are +0, the target keeps every bit (and may be absent), the
    history and the predictions are the forward step's."""
    for E in (140, 256):
        inp = Inputs(dtype, E, 2, 800 + E)
        z, target, h_out, eps, x0 = inp.invert(L, coefs[0], "epsilon", rescale)
        assert bool((_bits(z[ROWS]) == 0).all()) and _same(z[inp.others()], inp.z0[inp.others()])
        assert _same(target, inp.target)
        _, h_fwd, eps_fwd, x0_fwd = inp.forward(L, coefs[0], "epsilon", rescale, z)
        assert _same(h_fwd[ROWS], h_out[ROWS]) and _same(eps_fwd, eps) and _same(x0_fwd, x0)
        assert _same(h_out[inp.others()], inp.h0[inp.others()])
        z2 = inp.z0.clone()
        L.invert_step(inp.x, inp.mo, WEIGHTS[2], *coefs[0], target=None, z_out=z2, frame_ids=ROWS, rescale=rescale)
        assert _same(z2, z)


# ---------------------------------------------------------------------------------------------------
# 5. chunking independence
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescale", [0.0, 0.7])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_chunking_independence(L, coefs, dtype, rescale):
    """Five rows in one call, and as the chunks [5, 0] and [3, 1, 6]: the same bits in z_out, the target and the history."""
    rows, groups = [5, 0, 3, 1, 6], 3
    for E in (140, 256):
        whole = Inputs(dtype, E, groups, 900 + E, rows=rows)
        want = whole.invert(L, coefs[2], "v_prediction", rescale)[:3]
        got = [t.clone() for t in (whole.z0, whole.target, whole.h0)]
        mo = whole.mo.view(groups, len(rows), E)
        for lo, hi in ((0, 2), (2, 5)):
            L.invert_step(whole.x, mo[:, lo:hi].reshape(groups * (hi - lo), E).contiguous(), WEIGHTS[groups], *coefs[2],
                          target=got[1], z_out=got[0], h1=whole.h1, h_out=got[2], frame_ids=rows[lo:hi], pred_type=1, rescale=rescale)
        for a, b in zip(got, want):
            assert _same(a, b), (E, rescale)


# ---------------------------------------------------------------------------------------------------
# 6. vtm_noise_levels
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_noise_levels(L, dtype):
    """n = 3 levels of 7 frames: E = 140 (7 * 140 is no multiple of the 16-bit chunk), 256, and 256 off by one element, which
    must give the aligned call's bits."""
    n = 3
    table = torch.tensor([_solver(n, solver_order=1).coefficients(k)[:2] for k in range(n)], dtype=F32)
    coef, c = table.to(DEV), _f64(table)
    kept = {}
    for E, offset in ((140, 0), (256, 0), (256, 1)):
        x0, noise = _draw((N_FRAMES, E), dtype, 40 + E, offset), _draw((n, N_FRAMES, E), dtype, 41 + E, offset)
        levels = noise.clone() if not offset else _like(noise, offset).copy_(noise)
        assert levels.data_ptr() % 16 == offset * levels.element_size()
        before = x0.clone()
        assert L.noise_levels(x0, levels, coef) is levels
        assert _same(x0, before)
        a, b = c[:, 0, None, None] * _f64(x0)[None], c[:, 1, None, None] * _f64(noise)
        hold(levels, a + b, U[dtype] * np.abs(a + b) + GAMMA_LEVELS * (np.abs(a) + np.abs(b)), f"noise_levels E={E} offset={offset}")
        if offset:
            assert _same(levels, kept[E])
        kept[E] = levels


# ---------------------------------------------------------------------------------------------------
# 7. the whole trajectory through the classes
# ---------------------------------------------------------------------------------------------------
def _unet(x, i, groups):
    """A deterministic elementwise stand-in for the UNet: a fixed function of x and the step per group, group-major."""
    return torch.cat([torch.sin(x * (1.0 + 0.25 * g) + 0.3 * i) * 0.9 + 0.1 * g for g in range(groups)])


@pytest.mark.parametrize("final", ["alphas[0]", "1"])
@pytest.mark.parametrize("shape", [(4, 6, 7), (4, 5, 7)], ids=["E168", "E140"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_trajectory_is_reproduced_bit_for_bit(dtype, shape, final):
    """5 frames, n = 6, order 2, two chunks, two groups with guidance rescale: invert, then sample from levels[0] with the stored
    noise -- after every step the sampled video is levels[i + 1], bit for bit.  With final_alpha_cumprod = alphas[0] that
    includes the last level; with 1 the last step has no noise, its map is +0 and levels[n] is still the caller's x0."""
    from vidtome_amd import EditFriendlyInversion
    n, frames, groups, chunks = 6, 5, 2, [[3, 0, 4], [1, 2]]
    kw = dict(solver_order=2, guidance_scale=3.5, guidance_rescale=0.7,
              final_alpha_cumprod=float(_alphas()[0]) if final == "alphas[0]" else 1.0)
    x0 = _draw((frames,) + shape, dtype, 1000)
    kept = x0.clone()
    inv = EditFriendlyInversion(_solver(n, **kw))
    levels = inv.noise_levels(x0, generator=torch.Generator(device=DEV).manual_seed(7))
    assert levels.shape == (n + 1, frames) + shape and inv.noise.shape == (n, frames) + shape and _same(levels[n], x0)
    assert not any(_same(levels[a], levels[b]) for a in range(n + 1) for b in range(a))
    for i in range(n):
        for chunk in chunks:
            assert inv.step(levels, _unet(levels[i][chunk], i, groups), i, groups=groups, frame_ids=chunk) is None
    assert _same(x0, kept) and bool(torch.isfinite(levels).all()) and bool(torch.isfinite(inv.noise).all())
    if final == "1":
        assert _same(levels[n], x0) and bool((_bits(inv.noise[n - 1]) == 0).all())
    assert all(bool((inv.noise[i] != 0).any()) for i in range(n - 1))

    sampler = _solver(n, **kw)
    x, nxt = levels[0].clone(), torch.full_like(x0, float("nan"))
    for i in range(n):
        for chunk in chunks:
            sampler.step(x, _unet(x[chunk], i, groups), i, groups=groups, noise=inv.noise[i][chunk], frame_ids=chunk, out=nxt)
        x, nxt = nxt, x
        if i < n - 1 or final != "1":
            assert _same(x, levels[i + 1]), (i, final)
    assert bool(torch.isfinite(x).all())
    for a, b in zip(sampler.history, inv.solver.history):
        assert _same(a, b)
