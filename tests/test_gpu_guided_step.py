"""vtm_guided_step / GuidedDDIM.step on the GPU against a float64 numpy restatement of the formulas of include/vidtome_hip.h.

Every element of every output is held to

    |out - ref| <= u |ref| + 16 * 2^-24 * A + [rescale > 0] * 2^-16 * A_m

u = 2^-11 (fp16), 2^-8 (bf16), 2^-24 (fp32): the one rounding of the stored value.  A is the sum of the absolute values of the
terms of the output, each term expanded down to the inputs AS THE FORMULA IS WRITTEN (m = m_u + g m_c - g m_u has the three
terms |m_u|, |g m_c|, |g m_u|: the rounding error of m_c - m_u is relative to |m_c| + |m_u|, not to |m|), in float64; A_m is the
part of A that is proportional to m.  The constants are derived, not measured: at most 12 fp32 roundings lie on any term
(counting the fp32 coefficients; 16 leaves room for the second-order terms), and 2^-16 is the worst case of a two-pass fp32
reduction of <= 128 serial additions per lane followed by a tree -- which is how csrc/guided_step.hip accumulates (1024 lanes,
lane t adds its 16-byte chunks t, t + 1024, ... serially, then a butterfly over the 64 lanes and a binary tree over the 16
waves) -- for E <= 2^17 and frames with |mean| <= std.  The inputs are N(0, 1) * s with s in [0.5, 2], so that this holds.  No
element is exempt.  The worst observed error / bound is printed per check (run with -s)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F32, F16, BF16]
IDS = {F32: "fp32", F16: "fp16", BF16: "bf16"}
U = {F32: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}
HERE = os.path.dirname(os.path.abspath(__file__))
PREDS = ["epsilon", "v_prediction", "sample"]
PRED_CODE = {"epsilon": 0, "v_prediction": 1, "sample": 2}
GUIDANCE = 7.5


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def schedule():
    """tests/golden/make_golden_chunks.py's stand-in scheduler (the one tests/golden/ddim.npz was recorded with)."""
    import types
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    return types.SimpleNamespace(alphas_cumprod=torch.cumprod(1.0 - betas, dim=0), timesteps=torch.arange(981, -1, -20),
                                 final_alpha_cumprod=torch.tensor(1.0))


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
    return t.detach().float().cpu().numpy().astype(np.float64)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def reference(x, mo, noise, rows, groups, pred, guidance, rescale, coef):
    """The formulas in float64.  x (n_frames, E), mo (groups * F, E), noise (F, E) or None, rows: the F rows of x.
    Returns {"x": (ref, A, A_m), "eps": ..., "x0": ...}, every array (F, E)."""
    sa, sb, cx, ce, sg = coef
    F = len(rows)
    X = x[list(rows)]
    mu = mo[(groups - 2) * F:(groups - 1) * F] if groups >= 2 else mo[:F]
    if groups >= 2:
        mc = mo[(groups - 1) * F:]
        m = mu + guidance * (mc - mu)
        Am = (1 + abs(guidance)) * np.abs(mu) + abs(guidance) * np.abs(mc)
        if rescale > 0:
            ratio = mc.std(axis=1, ddof=1, keepdims=True) / m.std(axis=1, ddof=1, keepdims=True)
            m = m * (rescale * ratio + (1 - rescale))
            Am = Am * (np.abs(rescale * ratio) + abs(1 - rescale))
    else:
        m, Am = mu, np.abs(mu)
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
    xn, xn_x, xn_m = cx * x0 + ce * ep, cx * x0_x + ce * ep_x, cx * x0_m + ce * ep_m
    if sg != 0:
        xn, xn_x = xn + sg * noise, xn_x + np.abs(sg * noise)
    return {"x": (xn, xn_x + xn_m, xn_m), "eps": (ep, ep_x + ep_m, ep_m), "x0": (x0, x0_x + x0_m, x0_m)}


WORST = {}


def hold(out, ref_A_Am, dtype, rescaled, label, extra=0.0):
    """Every element within the bound (+ ``extra`` * A: the golden recording's own error); prints the worst error / bound."""
    ref, A, Am = ref_A_Am
    got = _f64(out).reshape(ref.shape)
    tol = U[dtype] * np.abs(ref) + 16 * 2.0 ** -24 * A + (2.0 ** -16 * Am if rescaled else 0.0) + extra * A
    err = np.abs(got - ref)
    ratio = float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))))
    WORST[IDS[dtype]] = max(WORST.get(IDS[dtype], 0.0), ratio if np.isfinite(ratio) else np.inf)
    print(f"[guided_step] {IDS[dtype]} {label}: worst error / bound {ratio:.4f}  (worst so far {WORST[IDS[dtype]]:.4f})")
    bad = ~(err <= tol)                       # NaN counts as a miss
    assert not bad.any(), (label, int(bad.sum()), ratio)


def _coef(sampler, i, inversion=False):
    return sampler.coefficients(i, inversion)[2:]


# ---------------------------------------------------------------------------------------------------
# dtypes x prediction types x rescale x eta x groups, through GuidedDDIM.step
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_dtypes_prediction_types(L, schedule, dtype, pred):
    """F = 3 frames of 4 x 8 x 8 scattered into a 7-frame video.  With 3 groups (PnP) group 0 is NaN: it is never read.  With
    one group there is no guidance, and GuidedDDIM applies guidance_rescale only where there is guidance."""
    from vidtome_amd import GuidedDDIM
    rows, n, shape = [5, 0, 3], 7, (4, 8, 8)
    F, E = len(rows), 4 * 8 * 8
    seed = 100 * DTYPES.index(dtype) + 10 * PREDS.index(pred)
    x = _draw((n,) + shape, dtype, seed)
    noise = _draw((F,) + shape, dtype, seed + 1)
    for groups in (1, 2, 3):
        mo = _draw((groups * F,) + shape, dtype, seed + 2 + groups)
        if groups == 3:
            mo[:F] = float("nan")
        mo64 = _f64(mo).reshape(groups * F, E)
        for rescale in (0.0, 0.7):
            for eta in (0.0, 1.0):
                s = GuidedDDIM.from_scheduler(schedule, prediction_type=pred, guidance_scale=GUIDANCE, guidance_rescale=rescale,
                                              eta=eta)
                coef = _coef(s, 17)
                assert (coef[4] > 0) == (eta > 0)
                out = torch.full_like(x, 3.0)
                got = s.step(x, mo, 17, groups=groups, frame_ids=rows, noise=noise if eta else None, out=out, want=("eps", "x0"))
                assert got[0] is out and got[1].shape == got[2].shape == (F,) + shape and got[1].dtype == dtype
                ref = reference(_f64(x).reshape(n, E), mo64, _f64(noise).reshape(F, E), rows, groups, pred, GUIDANCE,
                                rescale if groups >= 2 else 0.0, coef)
                label = f"{pred} groups={groups} rescale={rescale} eta={eta}"
                rescaled = rescale > 0 and groups >= 2
                hold(out[rows], ref["x"], dtype, rescaled, label + " x'")
                hold(got[1], ref["eps"], dtype, rescaled, label + " eps")
                hold(got[2], ref["x0"], dtype, rescaled, label + " x0")
                untouched = [r for r in range(n) if r not in rows]
                assert bool((out[untouched] == 3.0).all())


def test_generator_draws_the_noise(schedule):
    from vidtome_amd import GuidedDDIM
    s = GuidedDDIM.from_scheduler(schedule, eta=1.0)
    x, mo = _draw((3, 4, 8, 8), F16, 1), _draw((6, 4, 8, 8), F16, 2)
    g = torch.Generator(device=DEV).manual_seed(5)
    drawn = s.step(x, mo, 17, generator=g)
    noise = torch.randn((3, 4, 8, 8), dtype=F16, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    given = s.step(x, mo, 17, noise=noise)
    assert drawn is not x and drawn.data_ptr() != x.data_ptr() and torch.equal(_bits(drawn), _bits(given))
    assert not torch.equal(drawn, GuidedDDIM.from_scheduler(schedule).step(x, mo, 17))


# ---------------------------------------------------------------------------------------------------
# frame sizes: E = 2, no vector width, a latent frame, one full workgroup pass + one chunk + 3; a base pointer off by one
# ---------------------------------------------------------------------------------------------------
def _raw(L, x, mo, noise, coef, pred, rescale, **kw):
    return L.guided_step(x, mo, *coef, noise=noise, pred_type=PRED_CODE[pred], guidance=GUIDANCE, rescale=rescale, want_eps=True,
                         want_x0=True, **kw)


@pytest.mark.parametrize("rescale", [0.0, 0.7])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_frame_sizes(L, schedule, dtype, rescale):
    from vidtome_amd import GuidedDDIM
    coef = _coef(GuidedDDIM.from_scheduler(schedule, eta=1.0), 30)
    chunk = L.guided_step_chunk(dtype)
    sizes = [2, 140, 4 * 8 * 8, L.GUIDED_STEP_THREADS * chunk + chunk + 3]
    assert sizes[3] % chunk == 3 and 140 % 8      # (fp32's chunk of 4 divides 140: its element path is the last size's)
    F = 2
    for k, E in enumerate(sizes):
        x, noise = _draw((F, E), dtype, 7 * k), _draw((F, E), dtype, 7 * k + 1)
        # the bound's precondition, |mean| <= std in every frame of m_c and of m, is no matter of course in a frame of 2
        # elements: take the first draw that meets it (a property of the inputs, decided in float64 before anything runs)
        for attempt in range(200):
            mo = _draw((2 * F, E), dtype, 1000 * (k + 1) + attempt)
            m_c = _f64(mo)[F:]
            m = _f64(mo)[:F] + GUIDANCE * (m_c - _f64(mo)[:F])
            if all(bool(np.all(np.abs(a.mean(axis=1)) <= a.std(axis=1, ddof=1))) for a in (m_c, m)):
                break
        else:
            raise AssertionError(f"no draw of E = {E} with |mean| <= std")
        for pred in ("v_prediction", "epsilon"):
            got = _raw(L, x, mo, noise, coef, pred, rescale)
            ref = reference(_f64(x), _f64(mo), _f64(noise), range(F), 2, pred, GUIDANCE, rescale, coef)
            for o, name in zip(got, ("x", "eps", "x0")):
                hold(o, ref[name], dtype, rescale > 0, f"E={E} {pred} rescale={rescale} {name}")


@pytest.mark.parametrize("rescale", [0.0, 0.7])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_base_pointer_off_by_one_element(L, schedule, dtype, rescale):
    """E % 8 == 0 but no operand is 16-byte aligned: the element path -- within the bound, and the SAME BITS as the aligned call
    (which of the two paths moves the data changes no result, the statistics included)."""
    from vidtome_amd import GuidedDDIM
    coef = _coef(GuidedDDIM.from_scheduler(schedule, eta=1.0), 30)
    F, E = 3, 4 * 8 * 8
    shapes = ((F, E), (2 * F, E), (F, E))
    x, mo, noise = (_draw(sh, dtype, 40 + j, offset=1) for j, sh in enumerate(shapes))
    assert all(t.data_ptr() % 16 == t.element_size() and t.is_contiguous() for t in (x, mo, noise))
    got = _raw(L, x, mo, noise, coef, "v_prediction", rescale)
    ref = reference(_f64(x), _f64(mo), _f64(noise), range(F), 2, "v_prediction", GUIDANCE, rescale, coef)
    for o, name in zip(got, ("x", "eps", "x0")):
        hold(o, ref[name], dtype, rescale > 0, f"off-by-one rescale={rescale} {name}")
    aligned = _raw(L, *(t.clone() for t in (x, mo, noise)), coef, "v_prediction", rescale)
    for a, b in zip(got, aligned):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("E", [4 * 96 * 96, 4 * 128 * 128])
def test_large_frames_fp16_rescale(L, schedule, E):
    from vidtome_amd import GuidedDDIM
    coef = _coef(GuidedDDIM.from_scheduler(schedule, eta=1.0), 10)
    F = 2
    x, mo, noise = (_draw(sh, F16, 60 + j) for j, sh in enumerate(((F, E), (2 * F, E), (F, E))))
    got = _raw(L, x, mo, noise, coef, "v_prediction", 0.7)
    ref = reference(_f64(x), _f64(mo), _f64(noise), range(F), 2, "v_prediction", GUIDANCE, 0.7, coef)
    for o, name in zip(got, ("x", "eps", "x0")):
        hold(o, ref[name], F16, True, f"E={E} rescale=0.7 {name}")


# ---------------------------------------------------------------------------------------------------
# scatter and aliasing
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescale", [0.0, 0.7])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_scatter_and_aliasing(L, schedule, dtype, rescale):
    from vidtome_amd import GuidedDDIM
    coef = _coef(GuidedDDIM.from_scheduler(schedule), 17)
    rows, n, E = [6, 1, 4], 7, 140
    F = len(rows)
    x, mo = _draw((n, E), dtype, 80), _draw((2 * F, E), dtype, 81)
    canvas = _draw((n, E), dtype, 82)
    out = canvas.clone()
    res = L.guided_step(x, mo, *coef, frame_ids=rows, guidance=GUIDANCE, rescale=rescale, out=out)
    assert res[0] is out and res[1] is None and res[2] is None
    ref = reference(_f64(x), _f64(mo), None, rows, 2, "epsilon", GUIDANCE, rescale, coef)
    hold(out[rows], ref["x"], dtype, rescale > 0, f"scatter rescale={rescale}")
    others = [r for r in range(n) if r not in rows]
    assert torch.equal(_bits(out[others]), _bits(canvas[others]))                     # the other 4 rows: bit for bit
    # the ids as a device tensor, and as a CPU tensor: the same launch
    for ids in (torch.tensor(rows, dtype=torch.int32, device=DEV), torch.tensor(rows)):
        again = canvas.clone()
        L.guided_step(x, mo, *coef, frame_ids=ids, guidance=GUIDANCE, rescale=rescale, out=again)
        assert torch.equal(_bits(again), _bits(out))
    # in place: out defaults to x when the chunk is scattered, and out may be x
    for kw in (dict(), dict(out=None)):
        alias = x.clone()
        kw = dict(kw, out=alias) if "out" not in kw else kw
        got = L.guided_step(alias, mo, *coef, frame_ids=rows, guidance=GUIDANCE, rescale=rescale, **kw)[0]
        assert got is alias and torch.equal(_bits(alias[rows]), _bits(out[rows]))
        assert torch.equal(_bits(alias[others]), _bits(x[others]))
    # an ascending run is a row offset (no ids on the device): the same bits as the same run given as a device tensor
    run = _draw((2 * 3, E), dtype, 83)
    a, b = canvas.clone(), canvas.clone()
    L.guided_step(x, run, *coef, frame_ids=range(2, 5), guidance=GUIDANCE, rescale=rescale, out=a)
    L.guided_step(x, run, *coef, frame_ids=torch.tensor([2, 3, 4], dtype=torch.int32, device=DEV), guidance=GUIDANCE,
                  rescale=rescale, out=b)
    assert torch.equal(_bits(a), _bits(b)) and not torch.equal(_bits(a[2:5]), _bits(canvas[2:5]))
    assert torch.equal(_bits(a[[0, 1, 5, 6]]), _bits(canvas[[0, 1, 5, 6]]))


# ---------------------------------------------------------------------------------------------------
# repeatability: the run, and the other frames of the launch
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescale", [0.0, 0.7])
@pytest.mark.parametrize("E", [140, 4 * 8 * 8, 1024 * 8 + 8 + 3])
def test_repeatable_and_frame_independent(L, schedule, E, rescale):
    from vidtome_amd import GuidedDDIM
    coef = _coef(GuidedDDIM.from_scheduler(schedule, eta=1.0), 17)
    F = 3
    x, mo, noise = (_draw(sh, F16, 90 + j) for j, sh in enumerate(((F, E), (2 * F, E), (F, E))))
    first = _raw(L, x, mo, noise, coef, "v_prediction", rescale)
    second = _raw(L, x, mo, noise, coef, "v_prediction", rescale)
    for a, b in zip(first, second):
        assert torch.equal(_bits(a), _bits(b))
    for f in range(F):
        one = _raw(L, x[f:f + 1].clone(), torch.stack([mo[f], mo[F + f]]), noise[f:f + 1].clone(), coef, "v_prediction", rescale)
        for a, b in zip(first, one):
            assert torch.equal(_bits(a[f:f + 1]), _bits(b)), (f, E, rescale)


# ---------------------------------------------------------------------------------------------------
# the elementwise launch beyond its grid cap
# ---------------------------------------------------------------------------------------------------
def test_elementwise_beyond_the_grid_cap(L, schedule):
    """csrc/guided_step.hip caps the elementwise grid at 4096 blocks of 256 threads, one 16-byte chunk per thread and pass:
    17 fp32 frames of 4 x 256 x 256 are 1 114 112 chunks: the first pass covers 16 frames exactly, the 17th is the second pass."""
    from vidtome_amd import GuidedDDIM
    with open(os.path.join(os.path.dirname(HERE), "vidtome_amd", "csrc", "guided_step.hip")) as f:
        src = f.read()
    assert "constexpr int EW_THREADS = 256;" in src and "constexpr int64_t EW_GRID_CAP = 4096;" in src, \
        "re-derive the shape of this test from the new launch"
    F, E = 17, 4 * 256 * 256
    assert F * (E // L.guided_step_chunk(F32)) > 4096 * 256 >= (F - 1) * (E // L.guided_step_chunk(F32))
    coef = _coef(GuidedDDIM.from_scheduler(schedule), 17)
    x, mo = _draw((F, E), F32, 95), _draw((2 * F, E), F32, 96)
    torch.full((F * E * 4,), 0xFF, dtype=torch.uint8, device=DEV)       # what the output is likely allocated from: NaN patterns
    out = L.guided_step(x, mo, *coef, pred_type=PRED_CODE["v_prediction"], guidance=GUIDANCE)[0]
    ref = reference(_f64(x), _f64(mo), None, range(F), 2, "v_prediction", GUIDANCE, 0.0, coef)
    hold(out, ref["x"], F32, False, "beyond the grid cap")


# ---------------------------------------------------------------------------------------------------
# the reference's own recording (epsilon, eta = 0, sampling and inversion)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(10))
def test_against_the_reference_recording(schedule, k):
    """tests/golden/ddim.npz through GuidedDDIM.step.  The recording rounds to the tensor dtype after every operation; measured
    on the CPU it lies within 4.95 u A of float64 (u = 2^-24 / 2^-11, worst at case 2), so 5 u A is allowed for it on top of
    the kernel's own bound."""
    from vidtome_amd import GuidedDDIM
    z = np.load(os.path.join(HERE, "golden", "ddim.npz"))
    i, inversion = [(0, False), (17, False), (49, False), (5, True), (0, True)][k % 5]
    assert bool(z[f"{k}/meta"][2]) == inversion and float(z[f"{k}/meta"][3]) == GUIDANCE
    s = GuidedDDIM.from_scheduler(schedule, guidance_scale=GUIDANCE)
    x, eu, ec = (torch.from_numpy(z[f"{k}/{n}"]).to(DEV) for n in ("x", "eu", "ec"))
    dtype = x.dtype
    out, eps = s.step(x, torch.cat([eu, ec]), i, inversion=inversion, want=("eps",))
    ref = reference(_f64(x).reshape(4, -1), _f64(torch.cat([eu, ec])).reshape(8, -1), None, range(4), 2, "epsilon", GUIDANCE, 0.0,
                    _coef(s, i, inversion))
    hold(out, ref["x"], dtype, False, f"recording {k} vs float64 x'")
    hold(eps, ref["eps"], dtype, False, f"recording {k} vs float64 eps")
    rec = z[f"{k}/xn"].astype(np.float64).reshape(4, -1)
    hold(out, (rec, ref["x"][1], ref["x"][2]), dtype, False, f"recording {k} vs the recording", extra=5 * U[dtype])


# ---------------------------------------------------------------------------------------------------
# a full step over a 16-frame video in three chunks
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_full_step_in_chunks(schedule, dtype):
    from vidtome_amd import GuidedDDIM
    from vidtome_amd.scheduler import cut_frames
    n, shape, groups = 16, (4, 8, 8), 3
    s = GuidedDDIM.from_scheduler(schedule, prediction_type="v_prediction", guidance_scale=GUIDANCE, guidance_rescale=0.7, eta=1.0)
    x, noise = _draw((n,) + shape, dtype, 110), _draw((n,) + shape, dtype, 111)
    whole = _draw((groups, n) + shape, dtype, 112)                      # group-major model output of the whole video
    ranges = cut_frames(n, 5, 6)
    assert ranges == [(0, 5), (5, 11), (11, 16)]

    def run(order):
        nxt = torch.full_like(x, float("nan"))
        for c in order:
            a, b = ranges[c]
            ret = s.step(x, whole[:, a:b].reshape((groups * (b - a),) + shape), 20, groups=groups, frame_ids=torch.arange(a, b),
                         noise=noise[a:b], out=nxt)
            assert ret is nxt
        return nxt

    got = run([0, 1, 2])
    ref = reference(_f64(x).reshape(n, -1), _f64(whole).reshape(groups * n, -1), _f64(noise).reshape(n, -1), range(n), groups,
                    "v_prediction", GUIDANCE, 0.7, _coef(s, 20))
    hold(got, ref["x"], dtype, True, "full step in three chunks")
    assert torch.equal(_bits(run([2, 0, 1])), _bits(got))
    # the whole video as one chunk: the same bits again (a frame does not depend on the launch it is in)
    assert torch.equal(_bits(s.step(x, whole.reshape((groups * n,) + shape), 20, groups=groups, noise=noise)), _bits(got))
