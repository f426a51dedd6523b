"""vtm_semantic_guidance / SemanticGuidance.combine on the GPU against tests/semantic_standin.py.

Masks: mask_out is BIT-EQUAL to the standin's numpy fp32 restatement of the contract (one subtraction, one product, the
channel sum, np.sort, the double threshold formula); no element is exempt, ties included -- the arithmetic is specified
exactly.

Values: with the masks equal, every element of out and of the updated momentum is held to

    |got - ref| <= u |ref| + gamma_c * A,        gamma_c = c 2^-24 / (1 - c 2^-24)

against the float64 evaluation; u = 2^-11 (fp16), 2^-8 (bf16): half an ulp of the stored 16-bit value, 0 for fp32 (whose
last rounding is one of the c); A is the sum of the absolute values of the terms, each expanded down to the inputs (the
``hold`` scheme of test_gpu_solver_step.py): every partial sum of the kernel's expression is bounded by A.

c counts the fp32 roundings on the longest path of csrc/semantic.hip's expression, through a concept's term with six live
concepts (sums start from 0, so each first addition is exact):
    d_e  = e - u                                 subtraction 1                                           1
    g_e  = scale * d_e                           scale -> fp32 1, product 1                              2
    w g  = w_apply * g_e                         w -> fp32 1, product 1                                  2
    app  = sum of six such terms                 five additions                                          5
    m    = (u + s (c - u)) + app + mom_scale nu  the two additions after the term joins                  2
ROUNDINGS_OUT = 12.  The other paths are shorter (through c: subtraction, s -> fp32, product and three additions, 6; through
nu: mom_scale -> fp32, product, one addition, 3).  The momentum's longest path is the same up to the sum (1 + 2 + 2 + 5 = 10
with w_acc), then
    nu'  = beta nu + (1 - beta) acc              beta -> fp32 1, 1 - beta 1, product 1, addition 1       4
ROUNDINGS_MOM = 14.  Over consecutive steps the float64 recurrence is free-running, so step k's tolerance carries
|beta| times step k - 1's (and out's carries |mom_scale| times it).  The worst error / bound is printed per check (-s)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import semantic_standin as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F32, F16, BF16]
IDS = {F32: "fp32", F16: "fp16", BF16: "bf16"}
U = {F32: 0.0, F16: 2.0 ** -11, BF16: 2.0 ** -8}
ROUNDINGS_OUT, ROUNDINGS_MOM = 12, 14                       # counted in the module docstring


def _gamma(c):
    return c * 2.0 ** -24 / (1.0 - c * 2.0 ** -24)


GAMMA_OUT, GAMMA_MOM = _gamma(ROUNDINGS_OUT), _gamma(ROUNDINGS_MOM)
SHAPES = [(2, 4, 64, 64),        # baseline
          (1, 4, 5, 7),          # P = 35: fewer elements than one wave
          (1, 1, 1, 1),          # P = 1: rank_lo = hi = 0
          (3, 4, 24, 20),        # non-square, P not a power of two
          (1, 3, 96, 96),        # C = 3
          (1, 4, 128, 128)]      # the LDS limit
MODES = [S.CHANNEL, S.SUM, S.REGION, S.CHANNEL_REGION, S.SUM_REGION]
SENTINEL = -777.25


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _exact_q(P):
    """A q strictly inside (0, 1) with rank_frac == 0 (P = 1: every q has pos = 0; P = 2 has none, not used here)."""
    if P == 1:
        return 0.5
    for lo in range(P // 2, P - 1):
        q = S.exact_rank_q(lo, P)
        if q is not None:
            return q
    raise AssertionError(P)


def _quantiles(P):
    return [0.0, _exact_q(P), 0.9, 0.999, 1.0]


def _draw(shape, dtype, seed):
    """N(0, 1) * s, s in [0.5, 2], rounded to dtype."""
    g = torch.Generator().manual_seed(seed)
    s = 0.5 + 1.5 * float(torch.rand((), generator=g))
    return (torch.randn(shape, generator=g) * s).to(dtype).to(DEV)


def _regions(E, F, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((E, F, H, W), generator=g) > 0.4).to(torch.uint8).to(DEV)


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def concept(group, scale=5.0, q=0.9, w_apply=1.0, w_acc=1.0, mode=S.CHANNEL):
    return dict(group=group, scale=scale, q=q, w_apply=w_apply, w_acc=w_acc, mode=mode)


WORST = {}


def hold(got, ref, A, gamma, label, extra=0.0):
    """Every element within the bound; prints the worst error / bound.  Returns the tolerance array."""
    g = got.detach().double().cpu().numpy().reshape(ref.shape)
    tol = U[got.dtype] * np.abs(ref) + gamma * A + extra
    err = np.abs(g - ref)
    ratio = float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
    key = IDS[got.dtype]
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"[semantic] {key} {label}: worst error / bound {ratio:.4f}  (worst so far {WORST[key]:.4f})")
    bad = ~(err <= tol)                       # NaN counts as a miss
    assert not bad.any(), (label, int(bad.sum()), ratio)
    return tol


def call(L, mo, groups, gu, gc, s, cs, **kw):
    return L.semantic_guidance(mo, groups, gu, gc, s, [c["group"] for c in cs], [c["scale"] for c in cs], [c["q"] for c in cs],
                               [c["w_apply"] for c in cs], [c["w_acc"] for c in cs], [c["mode"] for c in cs], want_masks=True,
                               **kw)


def run(L, mo, groups, gu, gc, s, cs, label, regions=None, momentum=None, rows=None, ms=0.0, mb=0.0, ma=False, prev_tol=None,
        nu_ref=None):
    """One launch checked in full: masks bit-equal, out and the momentum rows to the bound, the other rows untouched.
    ``nu_ref`` / ``prev_tol``: the free-running float64 momentum of the chunk's rows and its tolerance (consecutive steps)."""
    F = mo.shape[0] // groups
    shape5 = (groups, F) + tuple(mo.shape[1:])
    before = momentum.clone() if momentum is not None else None
    out, masks = call(L, mo, groups, gu, gc, s, cs, regions=regions, momentum=momentum, frame_ids=rows, mom_scale=ms,
                      mom_beta=mb, mom_apply=ma)
    torch.cuda.synchronize()
    mo32 = mo.float().cpu().numpy().reshape(shape5)
    M, _ = S.masks(mo32, gu, cs, None if regions is None else regions.cpu().numpy())
    got_masks = masks.cpu().numpy()
    assert got_masks.shape == (len(cs), F) + tuple(mo.shape[1:]) and out.shape == (F,) + tuple(mo.shape[1:]) and out.dtype == mo.dtype
    for e, want in M.items():
        diff = got_masks[e] != want.astype(np.uint8)
        assert not diff.any(), (label, e, S.MODE_NAMES[cs[e]["mode"]], cs[e]["q"], int(diff.sum()), int(want.sum()))
    nu = None
    if momentum is not None:
        idx = list(range(F)) if rows is None else list(rows)
        nu = before[idx].double().cpu().numpy() if nu_ref is None else nu_ref
    ref, A, nu_new, A_nu = S.reference(mo32.astype(np.float64), M, gu, gc, s, cs, nu=nu, mom_scale=ms, mom_beta=mb, mom_apply=ma)
    carried = 0.0 if prev_tol is None else prev_tol
    hold(out, ref, A, GAMMA_OUT, label + " out", extra=abs(ms) * carried if ma else 0.0)
    tol = None
    if momentum is not None:
        tol = hold(momentum[idx], nu_new, A_nu, GAMMA_MOM, label + " momentum", extra=abs(mb) * carried)
        others = [r for r in range(momentum.shape[0]) if r not in idx]
        assert _same(momentum[others], before[others]), label
    return out, masks, M, nu_new, tol


def _three(groups_first, P, negative=True):
    """Three concepts: channel at 0.9, sum at an exact rank with a negative scale, channel+region at 0.999."""
    g = groups_first
    return [concept(g, 5.0, 0.9, 1.0, 1.0, S.CHANNEL), concept(g + 1, -4.0 if negative else 4.0, _exact_q(P), 0.5, 1.5, S.SUM),
            concept(g + 2, 3.0, 0.999, 2.0, 0.0, S.CHANNEL_REGION)]


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_every_shape_and_dtype(L, shape, dtype):
    """Three concepts of three modes (one with a negative scale), classifier-free term, momentum applied, at every shape."""
    F, C, H, W = shape
    mo = _draw((5 * F, C, H, W), dtype, 11 + F + H)
    momentum = _draw((F, C, H, W), F32, 5)
    run(L, mo, 5, 0, 1, 7.5, _three(2, H * W), f"{shape}", regions=_regions(3, F, H, W, 3), momentum=momentum, ms=0.1, mb=0.4, ma=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
@pytest.mark.parametrize("shape", [(3, 4, 24, 20), (1, 4, 5, 7), (1, 1, 1, 1), (2, 4, 64, 64)], ids=["3x4x24x20", "1x4x5x7", "1x1x1x1", "2x4x64x64"])
def test_every_mode_at_every_quantile(L, shape, dtype):
    """One launch per q in {0, an exact rank, 0.9, 0.999, 1} with one concept of each of the five modes."""
    F, C, H, W = shape
    mo = _draw((7 * F, C, H, W), dtype, 23 + H)
    reg = _regions(5, F, H, W, 9)
    for q in _quantiles(H * W):
        cs = [concept(2 + k, (-1) ** k * (2.0 + k), q, 1.0, 1.0, mode) for k, mode in enumerate(MODES)]
        run(L, mo, 7, 0, 1, 7.5, cs, f"{shape} q = {q:.6g}", regions=reg)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
@pytest.mark.parametrize("E", [0, 1, 3, 6])
@pytest.mark.parametrize("g_cond", [1, -1], ids=["cfg", "nocfg"])
def test_concept_counts_and_no_cfg_term(L, E, g_cond, dtype):
    F, C, H, W = 3, 4, 24, 20
    groups = 2 + E
    mo = _draw((groups * F, C, H, W), dtype, 31 + E)
    qs = _quantiles(H * W) + [0.5]
    cs = [concept(2 + k, (-1) ** k * 3.0, qs[k], 1.0 + 0.25 * k, 0.5 * k, MODES[k % 5]) for k in range(E)]
    momentum = _draw((F, C, H, W), F32, 6)
    out, _, _, _, _ = run(L, mo, groups, 0, g_cond, 7.5, cs, f"E = {E} g_cond = {g_cond}", regions=_regions(E, F, H, W, 4) if E else None,
                          momentum=momentum, ms=0.25, mb=0.6, ma=True)
    # without a momentum buffer the same call has no momentum term
    run(L, mo, groups, 0, g_cond, 7.5, cs, f"E = {E} g_cond = {g_cond} no momentum", regions=_regions(E, F, H, W, 4) if E else None)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_ties_straddle_the_selected_rank(L, dtype):
    """Operands on multiples of 1/8 (sigma 1/4, so a difference takes a few dozen values): hundreds of equal |g| around
    every rank of a 64 x 64 plane; and an all-equal plane."""
    F, C, H, W = 2, 4, 64, 64
    g = torch.Generator().manual_seed(41)
    mo = (torch.round(torch.randn((4 * F, C, H, W), generator=g) * 2.0).clamp(-12, 12) / 8.0).to(dtype).to(DEV)
    for q in (0.25, 0.5, 0.9, 0.999):
        cs = [concept(2, 0.5, q, 1.0, 1.0, S.CHANNEL), concept(3, -1.0, q, 1.0, 1.0, S.SUM)]
        _, _, M, _, _ = run(L, mo, 4, 0, 1, 7.5, cs, f"ties q = {q}")
        a = np.abs(S.edit_terms(mo.float().cpu().numpy().reshape(4, F, C, H, W), 0, 2, 0.5))[0, 0].ravel()
        lo = S.rank(q, H * W)[0]
        assert (a == np.sort(a)[lo]).sum() >= (100 if q < 0.95 else 1)               # the rank sits inside a run of equals
    flat = mo.clone()
    flat[2 * F:3 * F] = flat[0:F] + 1.0                                               # e - u == 1 everywhere, exactly
    flat[3 * F:4 * F] = flat[0:F] - 0.5
    for q in (0.0, 0.5, 1.0):
        cs = [concept(2, 2.0, q, 1.0, 1.0, S.CHANNEL), concept(3, 3.0, q, 1.0, 1.0, S.SUM)]
        _, masks, _, _, _ = run(L, flat, 4, 0, 1, 7.5, cs, f"all equal q = {q}")
        assert bool((masks == 1).all())                                               # thr == the one value: everything is kept


def test_weight_zero_concept_full_of_nan_reaches_nothing(L):
    F, C, H, W = 2, 4, 24, 20
    mo = _draw((5 * F, C, H, W), F16, 51)
    poisoned = mo.clone()
    poisoned[4 * F:] = float("nan")
    reg = _regions(3, F, H, W, 8)
    live = [concept(2, 5.0, 0.9, 1.0, 1.0, S.CHANNEL), concept(3, -4.0, 0.5, 1.0, 0.0, S.SUM_REGION)]
    dead = concept(4, 3.0, 0.5, 0.0, 0.0, S.CHANNEL_REGION)
    res = []
    for m, cs, groups in ((mo[:4 * F].contiguous(), live, 4), (poisoned, live + [dead], 5)):
        momentum = _draw((F, C, H, W), F32, 7)
        out, masks = call(L, m, groups, 0, 1, 7.5, cs, regions=reg[:len(cs)].contiguous(), momentum=momentum, mom_scale=0.1,
                          mom_beta=0.4, mom_apply=True)
        res.append((out, masks[:2], momentum))
    assert all(_same(a, b) for a, b in zip(*res)) and bool(torch.isfinite(res[1][0]).all())


def test_nan_in_one_plane_stays_in_it(L):
    F, C, H, W = 2, 4, 24, 20
    mo = _draw((3 * F, C, H, W), F16, 61)
    cs = [concept(2, 5.0, 0.9, 1.0, 1.0, S.CHANNEL)]
    clean_out, clean_masks = call(L, mo, 3, 0, 1, 7.5, cs)
    dirty = mo.clone()
    dirty[2 * F + 1, 2, 3, 5] = float("nan")                                          # concept group, frame 1, channel 2
    out, masks = call(L, dirty, 3, 0, 1, 7.5, cs)
    keep = torch.ones((F, C), dtype=torch.bool)
    keep[1, 2] = False
    assert _same(out[keep.to(DEV)], clean_out[keep.to(DEV)]) and _same(masks[0][keep.to(DEV)], clean_masks[0][keep.to(DEV)])
    # in its own plane the NaN is never selected, and the plane's mask is still the standin's (NaNs rank highest)
    want, _ = S.masks(dirty.float().cpu().numpy().reshape(3, F, C, H, W), 0, cs)
    assert np.array_equal(masks.cpu().numpy()[0], want[0].astype(np.uint8)) and int(masks[0, 1, 2, 3, 5]) == 0
    assert int(masks[0, 1, 2].sum()) > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_momentum_rows_sentinel_and_three_steps(L, dtype):
    """Rows named by frame_ids are updated to the bound and the others keep a sentinel (``run`` checks both); mom_apply = 0
    still accumulates; three consecutive steps track the free-running float64 recurrence."""
    F, C, H, W, n = 3, 4, 24, 20, 7
    rows = [5, 0, 3]
    momentum = torch.full((n, C, H, W), SENTINEL, dtype=F32, device=DEV)
    momentum[rows] = 0.0
    nu_ref, tol = np.zeros((F, C, H, W)), None
    for k in range(3):
        mo = _draw((5 * F, C, H, W), dtype, 71 + k)
        _, _, _, nu_ref, tol = run(L, mo, 5, 0, 1, 7.5, _three(2, H * W), f"step {k}", regions=_regions(3, F, H, W, k),
                                   momentum=momentum, rows=rows, ms=0.1, mb=0.4, ma=k > 0, prev_tol=tol, nu_ref=nu_ref)
        assert float(np.abs(nu_ref).max()) > 0.0                                      # step 0 (mom_apply = 0) accumulated
    assert bool((momentum[[1, 2, 4, 6]] == SENTINEL).all())
    # device-side int32 frame_ids address the same rows
    ids = torch.tensor(rows, dtype=torch.int32, device=DEV)
    a, b = momentum.clone(), momentum.clone()
    mo = _draw((5 * F, C, H, W), dtype, 79)
    reg = _regions(3, F, H, W, 5)
    oa, ma_ = call(L, mo, 5, 0, 1, 7.5, _three(2, H * W), regions=reg, momentum=a, frame_ids=rows, mom_scale=0.1, mom_beta=0.4, mom_apply=True)
    ob, mb_ = call(L, mo, 5, 0, 1, 7.5, _three(2, H * W), regions=reg, momentum=b, frame_ids=ids, mom_scale=0.1, mom_beta=0.4, mom_apply=True)
    assert _same(oa, ob) and _same(ma_, mb_) and _same(a, b)


@pytest.mark.parametrize("dtype", [F16, F32], ids=["fp16", "fp32"])
def test_chunkings_and_reruns_are_bit_equal(L, dtype):
    """Two chunkings of a 7-frame video equal the whole-video call bit for bit (out, masks, momentum); so do two runs."""
    n, C, H, W, groups = 7, 4, 24, 20, 5
    mo = _draw((groups, n, C, H, W), dtype, 81)
    reg = _regions(3, n, H, W, 2)
    start = _draw((n, C, H, W), F32, 82)
    cs = _three(2, H * W)

    def whole():
        m = start.clone()
        out, masks = call(L, mo.reshape(groups * n, C, H, W), groups, 0, 1, 7.5, cs, regions=reg, momentum=m, mom_scale=0.1,
                          mom_beta=0.4, mom_apply=True)
        return out, masks, m
    ref = whole()
    again = whole()
    assert all(_same(a, b) for a, b in zip(ref, again))
    for chunks in ([[0, 1, 2, 3], [4, 5, 6]], [[5, 0, 3], [1, 6], [2, 4]]):
        m = start.clone()
        out = torch.empty_like(ref[0])
        masks = torch.empty_like(ref[1])
        for rows in chunks:
            o, k = call(L, mo[:, rows].reshape(groups * len(rows), C, H, W).contiguous(), groups, 0, 1, 7.5, cs,
                        regions=reg[:, rows].contiguous(), momentum=m, frame_ids=rows, mom_scale=0.1, mom_beta=0.4, mom_apply=True)
            out[rows], masks[:, rows] = o, k
        assert _same(out, ref[0]) and _same(masks, ref[1]) and _same(m, ref[2]), chunks


def test_einval_leaves_out_and_momentum_untouched(L):
    F, C, H, W = 2, 4, 8, 8
    mo = _draw((3 * F, C, H, W), F16, 91)
    out = torch.full((F, C, H, W), SENTINEL, dtype=F16, device=DEV)
    momentum = torch.full((F, C, H, W), SENTINEL, dtype=F32, device=DEV)
    i32, f32, f64 = ctypes.c_int32 * 1, ctypes.c_float * 1, ctypes.c_double * 1

    def raw(H=H, lo=10, frac=0.5, mode=0, group=2, E=1, regions=None):
        return L.lib().vtm_semantic_guidance(mo.data_ptr(), L.VTM_F16, F, C, H, W, 3, 0, 1, 7.5, E, i32(group), f32(5.0), i32(lo), f64(frac),
                                             f32(1.0), f32(1.0), i32(mode), regions, momentum.data_ptr(), F, None, 0.1, 0.4, 1,
                                             out.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    for kw in (dict(lo=64), dict(frac=1.0), dict(mode=3), dict(mode=9), dict(group=3), dict(E=7), dict(H=4096)):
        assert raw(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((momentum == SENTINEL).all())
    assert raw() == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any()) and not bool((momentum == SENTINEL).any())


def _alphas():
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def test_ten_steps_through_the_solver(L):
    """SemanticGuidance.combine -> GuidedDPMSolver.step(groups=1) for ten steps of a 6-frame 16 x 16 stand-in.  Every step is
    checked from the kernel's own previous state (latents, history, momentum): the masks are bit-equal to the standin's on
    the model output the stand-in UNet gives for those latents, m and the momentum hold the bound above, and the stepped
    latents hold test_gpu_solver_step.py's bound for the m the kernel produced."""
    import test_gpu_solver_step as TS
    from vidtome_amd import EditConcept, GuidedDPMSolver, SemanticGuidance
    n, C, H, W, steps = 6, 4, 16, 16, 10
    sampler = GuidedDPMSolver(_alphas(), ((np.arange(steps) * (1000 // steps))[::-1] + 1).tolist(), solver_order=2)
    sega = SemanticGuidance([EditConcept(scale=5.0, threshold=0.9, warmup=2, cooldown=8),
                             EditConcept(scale=4.0, threshold=0.75, reverse=True, warmup=1, weight=0.5, mask="sum"),
                             EditConcept(scale=3.0, threshold=0.5, warmup=0, mask="channel+region")], guidance_scale=7.5)
    groups = sega.groups
    assert groups == 5
    x = _draw((n, C, H, W), F16, 101)
    x_next = torch.empty_like(x)
    pattern = _draw((groups, 1, C, H, W), F32, 102)
    reg_all = _regions(3, n, H, W, 103)
    sega.prepare(x)
    sampler.prepare(x)
    assert sega.momentum.dtype == F32 and not bool(sega.momentum.any())

    def unet(xc):                                                   # a stand-in: any deterministic map of the latents
        outs = [(0.9 + 0.03 * g) * xc.float() + 0.2 * torch.roll(xc.float(), g + 1, dims=-1) + 0.3 * pattern[g] for g in range(groups)]
        return torch.cat(outs).to(F16)
    chunks = [[4, 0, 2], [1, 5, 3]]
    mode_of = {name: mode for mode, name in S.MODE_NAMES.items()}
    for i in range(steps):
        app, acc, mom_apply = sega.schedule(i)
        cs = [concept(2 + k, c.signed_scale, c.threshold, app[k], acc[k], mode_of[c.mask]) for k, c in enumerate(sega.concepts)]
        coef = sampler.coefficients(i)
        hist_before = sampler.history[0].clone()
        x64 = x.double().cpu().numpy().reshape(n, -1)
        for rows in chunks:
            mo = unet(x[rows])
            reg = reg_all[:, rows].contiguous()
            before = sega.momentum.clone()
            m, masks = sega.combine(mo, i, frame_ids=rows, regions=reg, want_masks=True)
            mo32 = mo.float().cpu().numpy().reshape(groups, len(rows), C, H, W)
            M, _ = S.masks(mo32, 0, cs, reg.cpu().numpy())
            got = masks.cpu().numpy()
            for e, want in M.items():
                assert np.array_equal(got[e], want.astype(np.uint8)), (i, rows, e)
            ref, A, nu_new, A_nu = S.reference(mo32.astype(np.float64), M, 0, 1, 7.5, cs, nu=before[rows].double().cpu().numpy(),
                                               mom_scale=sega.momentum_scale, mom_beta=sega.momentum_beta, mom_apply=mom_apply)
            hold(m, ref, A, GAMMA_OUT, f"step {i} rows {rows} m")
            hold(sega.momentum[rows], nu_new, A_nu, GAMMA_MOM, f"step {i} rows {rows} momentum")
            sampler.step(x, m, i, groups=1, frame_ids=rows, out=x_next)
            want_x = TS.reference(x64, m.double().cpu().numpy().reshape(len(rows), -1), None,
                                  hist_before.double().cpu().numpy().reshape(n, -1) if coef[4] != 0.0 else None, None, rows, (1.0,),
                                  "epsilon", 0.0, 0, coef)
            TS.hold(x_next[rows], want_x["x"], False, f"step {i} rows {rows} x")
        x, x_next = x_next, x
    assert bool(torch.isfinite(x).all())
