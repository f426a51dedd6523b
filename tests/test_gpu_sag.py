"""GPU tests of self-attention guidance (run with -m gpu on an MI355X): vtm_attention_key_mass and vtm_sag_degrade through
their _lib wrappers and the C ABI against the float64 restatement of tests/sag_standin.py on the same rounded operands, then
the registered mid block and SelfAttentionGuidance.degrade.

THE BOUNDS.  Key mass: every term of a column sum is non-negative, so the bound is RELATIVE to mass_ref[j]:
((Mk + 8) + Mq + score term) 2^-24 -- the per-probability term behind the project's (Mk + 8) 2^-24 (Mk terms in the
denominator, a handful of roundings on the score, the head mean), Mq 2^-24 for the column sum (the worst case of a serial fp32
sum of Mq non-negative terms; the kernel's order is shorter), and where a score can exceed 16 log2 units
test_gpu_cross_softmax_corners.py's score term 4 ln 2 (d + 4) A with A = max sum_c |q_c k_c| scale log2(e); as there
(softmax_corners.bar) the term applies only where the operands' |score|max itself exceeds 16 (sag_standin.mass_bound).
Degrade: a counted number of fp32 roundings (sag_standin.ROUNDINGS) times 2^-24 times the magnitude sum of the terms plus
half an ulp of the output dtype, the ``hold`` scheme of test_gpu_guided_step.py; the mask is
compared on the fp32 mass, so it must be bit-equal and no element is exempt.  Every check prints its worst error / bound
(-s); profiles/attention_mass_resources.txt keeps one run's ratios."""
import math

import numpy as np
import pytest
import torch

import sag_standin as S
import softmax_corners as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = (torch.float16, torch.bfloat16)
ALL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
SENTINEL = -7.0
EINVAL = -1
# (B, h, Mq, Mk, d)
MASS_CASES = [(2, 8, 64, 64, 160),      # SD mid block at 512^2: a single query tile, written directly
              (1, 8, 144, 144, 160),    # 768^2: the second query tile is partial
              (2, 5, 257, 257, 64),     # one past every tile edge
              (1, 2, 33, 1, 8),         # one key: mass == Mq up to the 1 / h rounding
              (1, 1, 1, 65, 40),        # one query, padded contraction
              (1, 20, 70, 64, 64),      # many heads
              (1, 2, 1024, 1024, 64)]   # eight tiles through the workspace
# (F, C, H, W, h_m, w_m)
DEGRADE_CASES = [(2, 4, 64, 64, 8, 8),        # baseline
                 (1, 4, 96, 96, 12, 12),      # 768^2 latents
                 (3, 4, 40, 72, 5, 9),        # non-square
                 (1, 4, 60, 60, 8, 8),        # non-divisible upsample
                 (1, 1, 5, 5, 1, 1),          # the smallest plane for r = 4
                 (1, 4, 128, 128, 16, 16)]    # the LDS limit
SA, SB = math.sqrt(0.37), math.sqrt(1.0 - 0.37)
WORST = {}


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _ids(c):
    return "x".join(map(str, c))


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)


# ---------------------------------------------------------------------------------------------------
# 1. the key mass
# ---------------------------------------------------------------------------------------------------
def _hold_mass(got, q, k, h, Mq, Mk, d, label):
    ref = S.key_mass64(q, k, h, Mq, Mk, d ** -0.5)
    A, smax = S.score_bound(q, k, h, Mq, Mk, d ** -0.5)
    bound = S.mass_bound(Mq, Mk, d, A, smax)
    g = got.double().cpu().numpy()
    assert g.shape == ref.shape and np.isfinite(g).all(), label
    rel = float((np.abs(g - ref) / ref).max())
    total = float(np.abs(g.sum(-1) - Mq).max() / Mq)
    print(f"key mass {label} max rel err={rel:.3e} |sum - Mq| / Mq={total:.3e} bound={bound:.3e} ratio={rel / bound:.4f} "
          f"mass range [{ref.min():.3f}, {ref.max():.3f}] A={A:.1f} |score|max={smax:.1f}")
    _note("mass " + ("bf16" if q.dtype == torch.bfloat16 else "fp16" if q.dtype == torch.float16 else "fp32"), rel / bound)
    assert rel <= bound, (label, rel, bound)
    assert total <= bound, (label, total, bound)
    return ref


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", MASS_CASES, ids=_ids)
def test_key_mass_vs_float64(L, case, dtype):
    B, h, Mq, Mk, d = case
    q, k = S.mass_operands(B, h, Mq, Mk, d, dtype, seed=sum(case))
    qd, kd = q.to(DEV), k.to(DEV)
    got = L.attention_key_mass(qd, kd, h, Mq, Mk, d ** -0.5)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, Mk)
    ref = _hold_mass(got, q, k, h, Mq, Mk, d, f"{case} {dtype}")
    if Mk > 1 and Mq > 1:
        # (the head mean narrows the spread: 20 heads leave about +- 25 %)
        assert ref.max() > 1.2 * Mq / Mk and ref.min() < Mq / Mk / 1.2, "the operands do not spread the masses"
    if Mk == 1:     # every probability is exactly 1: the sum over queries and heads is an integer, 1 / h and the product round
        assert float((got.double().cpu() - Mq).abs().max()) <= 2 * 2.0 ** -24 * Mq
    assert torch.equal(got, L.attention_key_mass(qd, kd, h, Mq, Mk, d ** -0.5)), "two calls differ"
    if B == 2:      # a sample's bits are the same alone as inside B = 2
        for b in range(B):
            alone = L.attention_key_mass(qd[b:b + 1].contiguous(), kd[b:b + 1].contiguous(), h, Mq, Mk, d ** -0.5)
            assert torch.equal(alone[0], got[b]), b


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,Np", [(70, 80), (200, 208)], ids=["one tile", "two tiles"])
def test_key_mass_on_qkv_views_with_nan_pad_rows_and_sentinels(L, dtype, N, Np):
    """q and k as column ranges of one (B, Np, 3 C) q | k | v buffer (ld = 3 C) whose rows >= N and whose V columns hold NaN:
    the bits of the call on dense operands, finite; out with ldo > Mk keeps a sentinel behind column Mk."""
    B, h, d = 2, 2, 40
    C = h * d
    q, k = S.mass_operands(B, h, N, N, d, dtype, seed=5 + N)
    qkv = torch.full((B, Np, 3 * C), float("nan"), dtype=dtype)
    qkv[:, :N, :C], qkv[:, :N, C:2 * C] = q, k
    qkv = qkv.to(DEV)
    qv, kv = qkv[:, :, :C], qkv[:, :, C:2 * C]
    assert qv.stride(1) == 3 * C and kv.data_ptr() % 16 == 0
    dense = L.attention_key_mass(q.to(DEV), k.to(DEV), h, N, N, d ** -0.5)
    out = torch.full((B, N + 26), SENTINEL, dtype=torch.float32, device=DEV)
    assert L.attention_key_mass(qv, kv, h, N, N, d ** -0.5, out=out) is out
    assert bool((out[:, N:] == SENTINEL).all())
    assert torch.equal(out[:, :N], dense) and bool(torch.isfinite(dense).all())
    _hold_mass(dense, q, k, h, N, N, d, f"qkv views N={N} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [40, 160])
def test_key_mass_with_planted_keys(L, d, dtype):
    """tests/softmax_corners.py's late spike (a key in a later tile far above everything before it): the rescale branch of
    the online statistics of sweep 1 runs.  Only the scenario's q / k rows are used (its bias row, of order 1 against a spike
    of 40, has no counterpart here), and the reference is taken on exactly those rows."""
    c = SC.scenario("late_spike", "probs", d, dtype, 256)
    s = S._heads(c.q, c.Mq, SC.H) @ S._heads(c.k, c.Mk, SC.H).transpose(0, 1, 3, 2) * d ** -0.5
    late = (s[..., 64:].max(-1) > s[..., :64].max(-1) + 8.0)
    assert late.any(), "no row's maximum rises after the first tile"
    got = L.attention_key_mass(c.q.to(DEV), c.k.to(DEV), SC.H, c.Mq, c.Mk, d ** -0.5)
    _hold_mass(got, c.q, c.k, SC.H, c.Mq, c.Mk, d, f"late spike d={d} {dtype}")


def test_key_mass_bad_arguments_launch_nothing(L):
    B, h, Mq, d = 1, 2, 40, 40
    q = torch.zeros(B, Mq, h * d, dtype=torch.float16, device=DEV)
    k = torch.zeros(B, 4104, h * d, dtype=torch.float16, device=DEV)
    out = torch.full((B, 4104), SENTINEL, dtype=torch.float32, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)

    def raw(Mk=77, dd=d, code=None, scale=None, Mq_=Mq, ws_=ws, heads=h, Mqp=None):
        return L.lib().vtm_attention_key_mass(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), out.data_ptr(), 4104,
                                              L.VTM_F16 if code is None else code, B, heads, Mq_, Mq if Mqp is None else Mqp,
                                              Mk, 4104, dd, dd ** -0.5 if scale is None else scale,
                                              None if ws_ is None else ws_.data_ptr(), 0 if ws_ is None else ws_.numel(),
                                              torch.cuda.current_stream().cuda_stream)
    assert raw(Mk=4097) == EINVAL
    assert raw(dd=24, heads=3) == EINVAL
    assert raw(code=L.VTM_F32) == EINVAL
    assert raw(scale=0.0) == EINVAL
    assert raw(Mq_=65537, Mqp=65537) == EINVAL
    assert raw(Mq_=0) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert L.lib().vtm_attention_key_mass_ws_bytes(2, 128, 64) == 0
    assert L.lib().vtm_attention_key_mass_ws_bytes(2, 129, 64) == 2 * 2 * 64 * 4
    assert raw(Mk=4096) == 0                                            # the limit itself runs (zeros: uniform, Mq / Mk)
    torch.cuda.synchronize()
    assert float((out[:, :4096] - Mq / 4096).abs().max()) <= 1e-6 and bool((out[:, 4096:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------
# 2. degrade
# ---------------------------------------------------------------------------------------------------
def _f64(t):
    return t.double().cpu().numpy()


def _latents(F_, C, H, W, dtype, seed, n=None):
    g = torch.Generator().manual_seed(seed)
    n = n or F_
    x = (torch.randn(n, C, H, W, generator=g) * 1.3).to(dtype)
    m = (torch.randn(F_, C, H, W, generator=g) * 0.9).to(dtype)
    return x, m


def _mass(F_, n_cells, seed, ld=None):
    """fp32 masses around the threshold 1, some of them exactly 1 (not above: outside the mask)."""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(F_, ld or n_cells, generator=g) * 2.0
    m[:, ::7] = 1.0
    return m


def _hold(out, ref, A, dtype, label):
    got = _f64(out).reshape(ref.shape)
    tol = S.degrade_tol(ref, A, dtype)
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), label
    ratio = float((err / tol).max())
    print(f"degrade {label} max err / bound={ratio:.4f}")
    _note("degrade " + {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}[dtype], ratio)
    assert ratio <= 1.0, (label, ratio)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("case", DEGRADE_CASES, ids=_ids)
def test_degrade_vs_restatement(L, case, dtype):
    """The three prediction types on the chunk's frames as a permutation into a longer video; mass rows longer than the
    grid; the mask bit-equal; the second model_out group is the one read."""
    F_, C, H, W, h_m, w_m = case
    n = F_ + 2
    rows = [(3 * f + 1) % n for f in range(F_)] if F_ > 1 else [2]
    assert len(set(rows)) == F_
    x, m = _latents(F_, C, H, W, dtype, seed=sum(case), n=n)
    other = torch.full_like(m, float("nan"))
    mass = _mass(F_, h_m * w_m, seed=H, ld=h_m * w_m + 3)
    taps = L.gaussian_taps(4, 1.0)
    assert np.array_equal(np.asarray(taps), S.taps64(4, 1.0))
    xd, mod, md = x.to(DEV), torch.cat([other, m]).to(DEV), mass.to(DEV)
    for pred in S.PREDS:
        out, mask = L.sag_degrade(xd, mod, md, h_m, w_m, SA, SB, taps, 1.0, groups=2, group=1, frame_ids=rows,
                                  pred_type=S.PRED_CODE[pred], want_mask=True)
        assert out.dtype == dtype and tuple(out.shape) == (F_, C, H, W) and mask.dtype == torch.uint8
        ref, A, on = S.degrade64(_f64(x)[rows], _f64(m), mass.numpy(), h_m, w_m, pred, SA, SB, S.taps64(4, 1.0))
        assert 0 < on.sum() < on.size or h_m * w_m == 1
        assert np.array_equal(mask.cpu().numpy().astype(bool), on), "the mask is not bit-equal"
        _hold(out, ref, A, dtype, f"{case} {dtype} {pred}")
    # device ids: the same launch
    ids = torch.tensor(rows, dtype=torch.int32, device=DEV)
    again = L.sag_degrade(xd, mod, md, h_m, w_m, SA, SB, taps, 1.0, groups=2, group=1, frame_ids=ids,
                          pred_type=S.PRED_CODE[S.PREDS[-1]])
    assert torch.equal(again.view(torch.uint8), out.view(torch.uint8))


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_degrade_properties(L, dtype):
    F_, C, H, W, h_m, w_m = 2, 4, 64, 64, 8, 8
    x, m = _latents(F_, C, H, W, dtype, seed=11)
    xd, md = x.to(DEV), m.to(DEV)
    taps = L.gaussian_taps(4, 1.0)
    zeros, twos = torch.zeros(F_, 64, device=DEV), torch.full((F_, 64), 2.0, device=DEV)
    run = lambda mass, t=taps, pred="epsilon": L.sag_degrade(xd, md, mass, h_m, w_m, SA, SB, t, 1.0,
                                                              pred_type=S.PRED_CODE[pred], want_mask=True)
    # a mass of all 0: nothing is blurred, and for epsilon prediction sqrt_alpha x0 + sqrt_beta eps is x again
    out, mask = run(zeros)
    assert not bool(mask.any())
    ref, A, _ = S.degrade64(_f64(x), _f64(m), zeros.cpu().numpy(), h_m, w_m, "epsilon", SA, SB, S.taps64(4, 1.0))
    _hold(out, ref, A, dtype, f"mass 0 {dtype}")
    _hold(out, _f64(x), A, dtype, f"mass 0 gives x back {dtype}")
    # a mass of all 2: the full blur
    out, mask = run(twos)
    assert bool(mask.all())
    x0 = (_f64(x) - SB * _f64(m)) / SA
    a0 = (np.abs(_f64(x)) + SB * np.abs(_f64(m))) / SA
    t64 = S.taps64(4, 1.0)
    _hold(out, SA * S.blur64(x0, t64) + SB * _f64(m), SA * S.blur64(a0, t64) + SB * np.abs(_f64(m)), dtype, f"mass 2 {dtype}")
    # r = 0 is the identity blur: the mask changes no bit
    one = L.gaussian_taps(0, 1.0)
    assert one == [1.0]
    for pred in S.PREDS:
        a, b = run(zeros, one, pred)[0], run(twos, one, pred)[0]
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), pred


def test_degrade_nan_stays_where_the_blur_window_reaches(L):
    """One mass cell on (pixels 16 .. 23 of a 64 x 64 plane, cells of 8 x 8).  A NaN in x outside the mask and outside every
    masked pixel's window stays one pixel; one outside the mask but inside the window of masked pixels reaches exactly those
    pixels and itself (the mask selects: x0 outside it goes through untouched)."""
    F_, C, H, W, h_m, w_m = 1, 2, 64, 64, 8, 8
    dtype = torch.float32
    x, m = _latents(F_, C, H, W, dtype, seed=3)
    mass = torch.zeros(F_, 64)
    mass[0, 2 * 8 + 2] = 2.0
    x[0, 1, 40, 40] = float("nan")
    x[0, 1, 14, 18] = float("nan")
    out = L.sag_degrade(x.to(DEV), m.to(DEV), mass.to(DEV), h_m, w_m, SA, SB, L.gaussian_taps(4, 1.0), 1.0).cpu()
    want = torch.zeros(H, W, dtype=torch.bool)
    want[40, 40] = want[14, 18] = True
    want[16:19, 16:23] = True            # masked pixels with |y - 14| <= 4 and |x - 18| <= 4
    assert torch.equal(torch.isnan(out[0, 1]), want)
    assert bool(torch.isfinite(out[0, 0]).all())


def test_degrade_bad_arguments_launch_nothing(L):
    F_, C, H, W = 1, 1, 128, 129
    x = torch.zeros(F_, C, H, W, dtype=torch.float16, device=DEV)
    out = torch.full((F_, C, H, W), SENTINEL, dtype=torch.float16, device=DEV)
    mass = torch.zeros(F_, 256, device=DEV)
    taps = L.gaussian_taps(4, 1.0)
    arr = (L._f32 * 9)(*taps)

    def raw(H_=H, W_=W, r=4, h_m=16, w_m=16, dst=out, pred=0, code=None):
        return L.lib().vtm_sag_degrade(x.data_ptr(), F_, None, x.data_ptr(), mass.data_ptr(), 256, h_m, w_m,
                                       L.VTM_F16 if code is None else code, F_, C, H_, W_, pred, SA, SB, arr, r, 1.0,
                                       dst.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    assert raw() == EINVAL                              # H * W = 16512 > 16384
    assert b"16384" in L.lib().vtm_last_error()
    assert raw(H_=4, W_=64) == EINVAL                   # H <= r
    assert raw(H_=64, W_=64, r=5) == EINVAL
    assert raw(H_=64, W_=64, h_m=17) == EINVAL          # ld_mass = 256 < 17 * 16
    assert raw(H_=64, W_=64, pred=3) == EINVAL
    assert raw(H_=64, W_=64, code=7) == EINVAL
    assert raw(H_=64, W_=64, dst=x) == EINVAL           # out overlaps x
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    with pytest.raises(RuntimeError, match="16384"):
        L.sag_degrade(x, x.clone(), mass, 16, 16, SA, SB, taps)
    small = torch.zeros(1, 1, 64, 64, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="overlaps"):
        L.sag_degrade(small, small.clone(), mass, 8, 8, SA, SB, taps, out=small)


# ---------------------------------------------------------------------------------------------------
# 3. blocks
# ---------------------------------------------------------------------------------------------------
U16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}     # half an ulp, relative


def _spy(monkeypatch, L):
    seen = {"mass": 0}
    orig = L.attention_key_mass

    def f(q, k, *a, **kw):
        seen["mass"] += 1
        seen["q"], seen["k"] = q, k
        return orig(q, k, *a, **kw)
    monkeypatch.setattr(L, "attention_key_mass", f)
    return seen


def _forward(unet, h, cond):
    with torch.no_grad():
        torch.manual_seed(123)
        return unet.block(h, encoder_hidden_states=cond)


@pytest.fixture(scope="module")
def kernel_route(L):
    """{dtype: (h, cond, the unregistered block's output)}, computed once."""
    import vidtome_amd
    made = {}
    for dtype in DTYPES:
        h, cond = S.inputs(dtype, DEV)
        plain = S.patched(dtype, DEV)
        base = _forward(plain, h, cond)
        vidtome_amd.remove_patch(plain)
        made[dtype] = (h, cond, base)
    return made


@pytest.mark.parametrize("dtype", DTYPES)
def test_registered_mid_block_carries_the_mass_and_the_same_output(L, kernel_route, dtype, monkeypatch):
    """2 x 2 frames of 8 x 8 tokens at C = 1280 / d = 160, 64 x 64 latents: the site does not merge.  An unregistered block
    never calls attention_key_mass; the registered block's output is the bits of the unregistered run, its mass is within the
    kernel's bound of float64 on the q / k rows the core read (the spy keeps them), new on every forward."""
    import vidtome_amd
    h, cond, base = kernel_route[dtype]
    seen = _spy(monkeypatch, L)
    plain = S.patched(dtype, DEV)
    assert torch.equal(_forward(plain, h, cond), base) and seen["mass"] == 0
    assert not hasattr(plain.block, "attn1_key_mass")
    vidtome_amd.remove_patch(plain)

    unet = S.patched(dtype, DEV)
    assert vidtome_amd.register_self_attention_guidance(unet) == [S.MID_NAME]
    out = _forward(unet, h, cond)
    assert torch.equal(out, base), "the registration changed the block output"
    assert seen["mass"] == 1
    got = unet.block.attn1_key_mass
    N, C = h.shape[1], h.shape[2]
    assert tuple(got.shape) == (S.B * S.FRAMES, N) and got.dtype == torch.float32 and not got.requires_grad
    assert seen["q"].stride(1) == 3 * C and seen["k"].data_ptr() == seen["q"].data_ptr() + C * h.element_size()
    _hold_mass(got, seen["q"], seen["k"], S.HEADS, N, N, C // S.HEADS, f"registered block {dtype}")
    assert vidtome_amd.collect_from_patch(unet, "attn1_key_mass")[S.MID_NAME] is got
    _forward(unet, h, cond)
    assert unet.block.attn1_key_mass is not got and torch.equal(unet.block.attn1_key_mass, got)
    # a chunked call fills the rows of its frames
    _forward(unet, h[[3, 1]].contiguous(), cond[[3, 1]].contiguous())
    assert torch.equal(unet.block.attn1_key_mass, got[[3, 1]])
    vidtome_amd.unregister_self_attention_guidance(unet)
    assert not hasattr(unet.block, "attn1_key_mass") and not hasattr(unet.block, "vtm_sag")
    vidtome_amd.remove_patch(unet)


@pytest.mark.parametrize("route", ["fp32 block", "custom processor"])
def test_restatement_routes_agree_with_the_kernel_route(L, route, monkeypatch):
    """An fp32 block (with fp32_projections: "f32") and a block whose attn1 carries a storing processor ("module") take the
    fp32 torch restatement of to_q / to_k on norm1's output.  The check: the spy keeps the fp32 q / k rows the restatement
    read, and the stored mass is held to the kernel's bound of float64 on exactly those rows.  The sanity check beside it:
    against the fp16 kernel route of the same weights and inputs the difference is what rounding the operands to 16 bits
    moves -- a score by at most 3 u16 A per side (the weight, norm1's output and the projection each rounded once;
    A = max sum_c |q_c k_c| scale), a probability by twice the sum of both sides: 12 u16 A relative, plus the kernel's bound."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    dtype = torch.float16
    h, cond = S.inputs(dtype, DEV)
    seen = _spy(monkeypatch, L)
    ker = S.patched(dtype, DEV)
    vidtome_amd.register_self_attention_guidance(ker)
    _forward(ker, h, cond)
    mass_k = ker.block.attn1_key_mass.double().cpu().numpy()
    N, C = h.shape[1], h.shape[2]
    A, smax = S.score_bound(seen["q"], seen["k"], S.HEADS, N, N, ker.block.attn1.scale)
    vidtome_amd.remove_patch(ker)
    assert seen["mass"] == 1
    rows = {}
    orig = vpatch._key_mass_torch

    def keep_rows(q, k, heads, scale):
        rows["q"], rows["k"], rows["heads"], rows["scale"] = q, k, heads, scale
        return orig(q, k, heads, scale)
    monkeypatch.setattr(vpatch, "_key_mass_torch", keep_rows)
    if route == "fp32 block":
        unet = S.patched(torch.float32, DEV)
        # (the same 16-bit weights and inputs, held in fp32)
        unet.load_state_dict({k: v.half().float() for k, v in unet.state_dict().items()})
        vidtome_amd.update_patch(unet, fp32_projections=True, fp32_attention=True)     # attn1 on the "f32" route
        h2, cond2 = h.float(), cond.float()
    else:
        unet = S.patched(dtype, DEV, computing_self=True)
        h2, cond2 = h, cond
    vidtome_amd.register_self_attention_guidance(unet)
    _forward(unet, h2, cond2)
    assert seen["mass"] == 1, "the restatement route launched the kernel"
    got = unet.block.attn1_key_mass
    assert tuple(got.shape) == (S.B * S.FRAMES, N) and got.dtype == torch.float32 and not got.requires_grad
    assert tuple(rows["q"].shape) == (S.B * S.FRAMES, N, C) and rows["q"].dtype == torch.float32
    assert rows["heads"] == S.HEADS and rows["scale"] == unet.block.attn1.scale
    _hold_mass(got, rows["q"], rows["k"], S.HEADS, N, N, C // S.HEADS, f"{route}: restatement on its own rows")
    margin = 12 * U16[dtype] * A / S.LOG2E + S.mass_bound(N, N, C // S.HEADS, A, smax)
    rel = float((np.abs(got.double().cpu().numpy() - mass_k) / mass_k).max())
    print(f"{route}: max rel |restatement - kernel route|={rel:.3e} margin={margin:.3e} A={A:.2f}")
    assert rel <= margin, (rel, margin)
    vidtome_amd.remove_patch(unet)


def test_registered_block_raises_where_the_mass_would_be_wrong(L):
    import vidtome_amd
    dtype = torch.float16
    h, cond = S.inputs(dtype, DEV)
    unet = S.patched(dtype, DEV, latent=S.TOKENS)               # 8 x 8 latents, 64 tokens: downsample 1, the site merges
    vidtome_amd.register_self_attention_guidance(unet)
    with pytest.raises(RuntimeError, match="merges"):
        _forward(unet, h, cond)
    vidtome_amd.remove_patch(unet)
    unet = S.patched(dtype, DEV)
    vidtome_amd.register_self_attention_guidance(unet)
    vidtome_amd.register_perturbed_attention(unet, layers=("mid",), groups=2)
    with pytest.raises(RuntimeError, match="perturbed attention"):
        _forward(unet, h, cond)
    vidtome_amd.remove_perturbed_attention(unet)
    attn = unet.block.attn1
    attn.injection_schedule, attn.t, attn.vtm_num_inputs = [5], 5, 2
    with pytest.raises(RuntimeError, match="PnP"):
        _forward(unet, h, cond)
    attn.t = 7                                                   # not an injection step: the block runs
    _forward(unet, h, cond)
    assert unet.block.attn1_key_mass is not None
    vidtome_amd.remove_patch(unet)


@pytest.mark.parametrize("dtype", DTYPES)
def test_guidance_degrade_on_the_blocks_own_mass(L, dtype):
    """SelfAttentionGuidance.degrade on the registered block's mass, for a chunk of 2 frames x 2 groups into a 5-frame video,
    against the restatement fed THAT mass tensor: no threshold ambiguity, nothing excluded."""
    import vidtome_amd
    h, cond = S.inputs(dtype, DEV)
    unet = S.patched(dtype, DEV)
    vidtome_amd.register_self_attention_guidance(unet)
    _forward(unet, h, cond)
    mass = unet.block.attn1_key_mass
    Fg, (H, W) = S.FRAMES, S.LATENT
    x, m = _latents(2 * Fg, 4, H, W, dtype, seed=21, n=5)
    rows = [3, 1]
    alphas = torch.linspace(0.9991, 0.0047, 1000)
    for sampler in (vidtome_amd.GuidedDDIM(alphas, [801, 601, 401], prediction_type="v_prediction"),
                    vidtome_amd.GuidedDPMSolver(alphas, [801, 601, 401], prediction_type="epsilon")):
        sag = vidtome_amd.SelfAttentionGuidance(unet)
        assert sag.group_weights(7.5) == (1.0 - 7.5 + 0.75, 7.5, -0.75) and sag.group_weights(7.5, cfg=False) == (1.75, -0.75)
        out, mask = sag.degrade(x.to(DEV), m.to(DEV), sampler, 1, groups=2, frame_ids=rows, want_mask=True)
        a = float(alphas[601])
        ref, A, on = S.degrade64(_f64(x)[rows], _f64(m)[:Fg], mass[:Fg].cpu().numpy(), 8, 8, sampler.prediction_type,
                                 math.sqrt(a), math.sqrt(1.0 - a), S.taps64(4, 1.0))
        assert np.array_equal(mask.cpu().numpy().astype(bool), on) and 0 < on.sum() < on.size
        _hold(out, ref, A, dtype, f"guidance {type(sampler).__name__} {dtype}")
        # group 1's rows on request
        out1 = sag.degrade(x.to(DEV), m.to(DEV), sampler, 1, groups=2, group=1, frame_ids=rows)
        ref1, A1, _ = S.degrade64(_f64(x)[rows], _f64(m)[Fg:], mass[Fg:].cpu().numpy(), 8, 8, sampler.prediction_type,
                                  math.sqrt(a), math.sqrt(1.0 - a), S.taps64(4, 1.0))
        _hold(out1, ref1, A1, dtype, f"guidance group 1 {dtype}")
    big = torch.zeros(1, 4, 128, 136, dtype=dtype, device=DEV)
    with pytest.raises(RuntimeError, match="16384"):
        sag.degrade(big, big.clone(), sampler, 1, groups=1, mass=torch.zeros(1, 16 * 17, device=DEV))
    vidtome_amd.remove_patch(unet)


def test_zz_report_worst_ratios():
    print("worst error / bound:", {k: round(v, 4) for k, v in WORST.items()})
