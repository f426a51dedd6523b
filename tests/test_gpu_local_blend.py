"""GPU tests of Prompt-to-Prompt LocalBlend on the fused attn2 path (run with -m gpu on an MI355X): vtm_attention_word_map
through the C ABI and _lib.attention_word_map against a float64 numpy evaluation on the same rounded operands,
vtm_local_blend against the torch restatement of its formula, then patched blocks with register_local_blend on every
attn2 route against ``attn2_probs @ w`` of the same forward.

The bound of a word-map launch is 2 (Mk + 8) 2^-24 max|w|: two fp32 sums of Mk terms, the numerator (terms <= max|w|) and
the denominator, plus a handful of roundings on the score, with probabilities <= 1 -- derived, not measured.  A map of
vtm_attention_probs is within (Mk + 8) 2^-24 per element (tests/test_gpu_attention_maps.py), so ``map @ w`` in float64 is
within (Mk + 8) 2^-24 sum|w|; comparisons of the two kernels use the sum of both.

profiles/attention_words_resources.txt keeps the worst measured error / bound ratios of test_word_map_vs_float64."""
import numpy as np
import pytest
import torch

import attention_maps_standin as AM
import local_blend_standin as LB

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = (torch.float16, torch.bfloat16)
SENTINEL = -7.0
EINVAL = -1
U = 2.0 ** -24
# (B, h, Mq, Mk, d)
CASES = [(2, 2, 70, 77, 40),      # padded contraction, two key tiles, partial query block
         (1, 5, 33, 1, 64),       # a single key: the value is w[0]
         (2, 1, 257, 256, 160),   # the key limit, several query blocks
         (2, 8, 65, 33, 8),       # smallest head dim
         (1, 2, 40, 64, 80),      # key tile edge
         (1, 2, 40, 65, 80),      # ... one past
         (1, 41, 33, 77, 8)]      # beyond the 40 heads vtm_attention_probs takes


def bound(Mk, w):
    return 2 * (Mk + 8) * U * float(torch.as_tensor(w).abs().max())


def probs_bound(Mk, w):
    """|float64(map) @ w - exact| for a map of vtm_attention_probs: (Mk + 8) 2^-24 per element."""
    return (Mk + 8) * U * float(torch.as_tensor(w).abs().sum(-1).max())


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _operands(B, h, Mq, Mk, d, dtype, seed, Mqp=None, Mkp=None):
    g = torch.Generator().manual_seed(seed)
    Mqp, Mkp = Mqp or Mq, Mkp or Mk
    q = torch.randn(B, Mqp, h * d, generator=g).to(dtype)
    k = torch.randn(B, Mkp, h * d, generator=g).to(dtype)
    return q, k


def _weights(kind, B, Mk, seed):
    """(B, Mk) fp32 rows: "01" a 0 / 1 row per sample (at least one 1), "signed" N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "signed":
        return torch.randn(B, Mk, generator=g)
    w = (torch.rand(B, Mk, generator=g) < 0.3).float()
    w[:, 0] = 1.0
    return w


def _probs64(q, k, h, Mq, Mk, bias=None):
    """float64 per-sample mean over the heads of softmax(q k^T d^-0.5 + bias) on the same 16-bit operands."""
    B, d = q.shape[0], q.shape[2] // h
    sh = lambda t, n: t.double().numpy()[:, :n].reshape(B, n, h, d).transpose(0, 2, 1, 3)
    s = sh(q, Mq) @ sh(k, Mk).transpose(0, 1, 3, 2) * float(d) ** -0.5
    if bias is not None:
        s = s + np.asarray(bias, dtype=np.float64)[:, None, None, :]
    with np.errstate(invalid="ignore"):
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
    return p.mean(1)


def _ref(q, k, h, Mq, Mk, w, bias=None):
    """(B, Mq) float64: the head-averaged map times the sample's weights row (w: (B or 1, Mk))."""
    p = _probs64(q, k, h, Mq, Mk, bias)
    w = np.broadcast_to(w.double().numpy()[:, :Mk], (q.shape[0], Mk))
    return np.einsum("bik,bk->bi", p, w)


def _raw(L, q, k, w, out, h, Mq, Mk, d, ldo=None, bias=None, ld_bias=0, bstride=0, ld_w=None, wstride=0, rows=None, acc=0,
         code=None, scale=None, ldq=None, Mqp=None, q_ptr=None, w_ptr=None, out_ptr=None):
    return L.lib().vtm_attention_word_map(
        q.data_ptr() if q_ptr is None else q_ptr, q.stride(1) if ldq is None else ldq, k.data_ptr(), k.stride(1),
        L.dtype_code(q) if code is None else code, q.shape[0], h, Mq, q.shape[1] if Mqp is None else Mqp, Mk, k.shape[1], d,
        d ** -0.5 if scale is None else scale, None if bias is None else bias.data_ptr(), ld_bias, bstride,
        w.data_ptr() if w_ptr is None else w_ptr, w.shape[1] if ld_w is None else ld_w, wstride,
        out.data_ptr() if out_ptr is None else out_ptr, out.shape[1] if ldo is None else ldo,
        None if rows is None else rows.data_ptr(), acc, torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------
# 1. the word-map kernel
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["01", "signed"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_word_map_vs_float64(L, case, dtype, kind):
    """Every case against float64 within 2 (Mk + 8) 2^-24 max|w|; two calls bit-equal; within the sum of the two kernels'
    bounds of ``attention_probs(...) @ w`` where that kernel takes the head count.  One key: every probability is 1, and a
    0 / 1 weight comes back exactly (h * 1 * fl(1 / h) rounds to 1 for the head counts here, as the all-ones map of
    vtm_attention_probs does); a generic w[0] passes through the head sum h w[0] and the product with fl(1 / h), two
    roundings the bound covers."""
    B, h, Mq, Mk, d = case
    q, k = _operands(B, h, Mq, Mk, d, dtype, seed=sum(case))
    w = _weights(kind, B, Mk, seed=sum(case) + 1)
    qd, kd, wd = q.to(DEV), k.to(DEV), w.to(DEV)
    out = torch.full((B, Mq), SENTINEL, dtype=torch.float32, device=DEV)
    got = L.attention_word_map(qd, kd, h, Mq, Mk, d ** -0.5, wd, out, accumulate=False)
    assert got is out
    ref = _ref(q, k, h, Mq, Mk, w)
    err = float(np.abs(out.double().cpu().numpy() - ref).max())
    print(f"attention_word_map {case} {dtype} {kind} max|out-ref|={err:.3e} bound={bound(Mk, w):.3e} "
          f"ratio={err / bound(Mk, w):.3f}")
    assert err <= bound(Mk, w), (case, err)
    if Mk == 1 and kind == "01":
        assert bool((out == 1.0).all())
    again = torch.full_like(out, SENTINEL)
    L.attention_word_map(qd, kd, h, Mq, Mk, d ** -0.5, wd, again, accumulate=False)
    assert torch.equal(out, again), "two calls differ"
    if h <= L.PROBS_MAX_HEADS:
        via = np.einsum("bik,bk->bi", L.attention_probs(qd, kd, h, Mq, Mk, d ** -0.5).double().cpu().numpy(), w.double().numpy())
        both = float(np.abs(out.double().cpu().numpy() - via).max())
        assert both <= bound(Mk, w) + probs_bound(Mk, w), (case, both)


@pytest.mark.parametrize("dtype", DTYPES)
def test_accumulation_rows_and_pads(L, dtype):
    """accumulate=1 onto a prefilled out is prior + value within the bound plus one fp32 rounding of the sum; accumulate=0
    overwrites; out_rows a permutation with gaps: rows nobody names keep the sentinel; ldo > Mq: the pad columns keep it."""
    B, h, Mq, Mk, d = 3, 2, 70, 77, 40
    q, k = _operands(B, h, Mq, Mk, d, dtype, seed=21)
    w = _weights("signed", B, Mk, seed=22)
    qd, kd, wd = q.to(DEV), k.to(DEV), w.to(DEV)
    ref = _ref(q, k, h, Mq, Mk, w)
    ldo, R = 80, 7
    rows = torch.tensor([5, 0, 3], dtype=torch.int64, device=DEV)
    g = torch.Generator().manual_seed(23)
    prior = torch.randn(R, ldo, generator=g)
    out = prior.to(DEV)
    out[:, Mq:] = SENTINEL
    out[[1, 2, 4, 6]] = SENTINEL
    rc = _raw(L, qd, kd, wd, out, h, Mq, Mk, d, wstride=Mk, rows=rows, acc=1)
    assert rc == 0, L.lib().vtm_last_error()
    torch.cuda.synchronize()
    o = out.cpu()
    assert bool((o[:, Mq:] == SENTINEL).all()) and bool((o[[1, 2, 4, 6]] == SENTINEL).all())
    for b, r in enumerate([5, 0, 3]):
        want = prior[r, :Mq].double().numpy() + ref[b]
        err = np.abs(o[r, :Mq].double().numpy() - want)
        assert float((err - (bound(Mk, w) + U * np.abs(want))).max()) <= 0.0, (b, float(err.max()))
    # the same call again adds again; accumulate = 0 then overwrites with the value alone
    first = out.clone()
    assert _raw(L, qd, kd, wd, out, h, Mq, Mk, d, wstride=Mk, rows=rows, acc=1) == 0
    torch.cuda.synchronize()
    assert not torch.equal(out[rows, :Mq], first[rows, :Mq])
    assert _raw(L, qd, kd, wd, out, h, Mq, Mk, d, wstride=Mk, rows=rows, acc=0) == 0
    torch.cuda.synchronize()
    o = out.cpu()
    for b, r in enumerate([5, 0, 3]):
        assert float(np.abs(o[r, :Mq].double().numpy() - ref[b]).max()) <= bound(Mk, w)
    assert bool((o[:, Mq:] == SENTINEL).all()) and bool((o[[1, 2, 4, 6]] == SENTINEL).all())
    # the wrapper: the same bits on the same operands
    via = torch.full((R, ldo), SENTINEL, dtype=torch.float32, device=DEV)
    L.attention_word_map(qd, kd, h, Mq, Mk, d ** -0.5, wd, via, rows, accumulate=False)
    assert torch.equal(via, out)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_strided_q_pad_rows_and_weight_rows(L, dtype):
    """q as a column range of a wider buffer (ldq > h d), Mqp > Mq and Mkp > Mk with NaN in the pad rows: nothing leaks;
    per-sample weight rows (stride ld_w > Mk, NaN behind the row) and one shared row (stride 0)."""
    B, h, Mq, Mk, d = 2, 2, 70, 77, 40
    C, Mqp, Mkp, ld_w = h * d, 80, 88, 96
    q, k = _operands(B, h, Mq, Mk, d, dtype, seed=5, Mqp=Mqp, Mkp=Mkp)
    q[:, Mq:] = float("nan")
    k[:, Mk:] = float("nan")
    wide = torch.full((B, Mqp, 3 * C), float("nan"), dtype=dtype)
    wide[:, :, C:2 * C] = q
    qd = wide.to(DEV)[:, :, C:2 * C]
    assert qd.stride(1) == 3 * C
    kd = k.to(DEV)
    w = torch.full((B, ld_w), float("nan"))
    w[:, :Mk] = _weights("signed", B, Mk, seed=6)
    wd = w.to(DEV)
    out = torch.full((B + 1, Mq + 3), SENTINEL, dtype=torch.float32, device=DEV)
    assert _raw(L, qd, kd, wd, out, h, Mq, Mk, d, wstride=ld_w) == 0, L.lib().vtm_last_error()
    torch.cuda.synchronize()
    assert bool((out[B:] == SENTINEL).all()) and bool((out[:, Mq:] == SENTINEL).all())
    got = out[:B, :Mq].double().cpu().numpy()
    assert np.isfinite(got).all()
    assert float(np.abs(got - _ref(q, k, h, Mq, Mk, w[:, :Mk])).max()) <= bound(Mk, w[:, :Mk])
    # one row for every sample
    shared = torch.full_like(out, SENTINEL)
    assert _raw(L, qd, kd, wd, shared, h, Mq, Mk, d, wstride=0) == 0
    torch.cuda.synchronize()
    assert float(np.abs(shared[:B, :Mq].double().cpu().numpy() - _ref(q, k, h, Mq, Mk, w[:1, :Mk])).max()) <= bound(Mk, w[:1, :Mk])
    assert torch.equal(shared[0], out[0]) and not torch.equal(shared[1], out[1])
    # the wrapper takes the same views: (B, ld_w) rows and a (1, .) row
    via = torch.full_like(out, SENTINEL)
    L.attention_word_map(qd, kd, h, Mq, Mk, d ** -0.5, torch.nan_to_num(wd), via, accumulate=False)
    assert torch.equal(via, out)
    L.attention_word_map(qd, kd, h, Mq, Mk, d ** -0.5, torch.nan_to_num(wd[:1]), via, accumulate=False)
    assert torch.equal(via, shared)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bias(L, dtype):
    """A 0 / -10000 row per sample against float64; a -inf key contributes exactly 0 (the result is the bits of the call
    whose weight on that key is 0, whatever the weight); a sample whose keys are all -inf is NaN, its neighbour finite."""
    B, h, Mq, Mk, d = 2, 2, 70, 77, 40
    q, k = _operands(B, h, Mq, Mk, d, dtype, seed=9)
    w = _weights("signed", 1, Mk, seed=10)
    qd, kd = q.to(DEV), k.to(DEV)

    def run(bias, w_=w):
        out = torch.full((B, Mq), SENTINEL, dtype=torch.float32, device=DEV)
        return L.attention_word_map(qd, kd, h, Mq, Mk, d ** -0.5, w_.to(DEV), out, accumulate=False,
                                    bias=None if bias is None else bias.to(DEV))
    plain = run(None)
    assert torch.equal(run(torch.zeros(B, Mk)), plain), "a zero bias is not the unbiased call"
    keep = torch.arange(Mk)[None, :] < torch.tensor([20, 70])[:, None]
    b1 = (1 - keep.float()) * -10000.0
    assert float(np.abs(run(b1).double().cpu().numpy() - _ref(q, k, h, Mq, Mk, w, b1.numpy())).max()) <= bound(Mk, w)
    b2 = torch.zeros(B, Mk)
    b2[0, :66] = float("-inf")                      # among them the whole first tile
    b2[1, 3::5] = float("-inf")
    got = run(b2)
    assert float(np.abs(got.double().cpu().numpy() - _ref(q, k, h, Mq, Mk, w, b2.numpy())).max()) <= bound(Mk, w)
    w_hidden = w.clone()
    w_hidden[0, 3::5] = 1000.0                      # sample 1's hidden keys: their weight does not matter
    assert torch.equal(run(b2, w_hidden)[1], got[1]), "a key with bias -inf contributed"
    b3 = torch.zeros(B, Mk)
    b3[0] = float("-inf")
    got = run(b3)
    assert bool(torch.isnan(got[0]).all()) and torch.equal(got[1], plain[1])


def test_bad_arguments_launch_nothing(L):
    B, h, Mq, d = 1, 2, 40, 40
    q, k = _operands(B, h, Mq, 264, d, torch.float16, seed=1)
    qd, kd = q.to(DEV), k.to(DEV)
    wd = torch.ones(B, 264, device=DEV)
    out = torch.full((B, 264), SENTINEL, dtype=torch.float32, device=DEV)
    err = lambda: L.lib().vtm_last_error().decode()
    who = "vtm_attention_word_map"
    for null in ("q_ptr", "w_ptr", "out_ptr"):
        assert _raw(L, qd, kd, wd, out, h, Mq, 77, d, **{null: 0}) == EINVAL and who in err()
    assert _raw(L, qd, kd, wd, out, h, Mq, 77, d, code=L.VTM_F32) == EINVAL and "fp32" in err()
    assert _raw(L, qd, kd, wd, out, h, Mq, 257, d) == EINVAL and "257" in err()
    assert _raw(L, qd, kd, wd, out, h, Mq, 77, d, ld_w=76) == EINVAL and "ld_w" in err()
    assert _raw(L, qd, kd, wd, out, h, Mq, 77, d, ld_w=80, wstride=79) == EINVAL and "w_batch_stride" in err()
    bias = torch.zeros(B, 80, device=DEV)
    assert _raw(L, qd, kd, wd, out, h, Mq, 77, d, bias=bias, ld_bias=76) == EINVAL and "ld_bias" in err()
    assert _raw(L, qd, kd, wd, out, h, Mq, 77, d, bias=bias, ld_bias=80, bstride=8) == EINVAL and "bias_batch_stride" in err()
    assert _raw(L, qd, kd, wd, out, h, Mq, 77, d, ldq=h * d + 4) == EINVAL
    assert _raw(L, qd, kd, wd, out, h, Mq, 77, d, ldo=Mq - 1) == EINVAL and "ldo" in err()
    assert _raw(L, qd, kd, wd, out, h, Mq, 77, d, scale=0.0) == EINVAL and "scale" in err()
    assert _raw(L, qd, kd, wd, out, h, Mq, 77, d, scale=-1.0) == EINVAL
    q24 = torch.zeros(B, Mq, 48, dtype=torch.float16, device=DEV)
    assert _raw(L, q24, torch.zeros(B, 80, 48, dtype=torch.float16, device=DEV), wd, out, 2, Mq, 77, 24) == EINVAL   # d = 24
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert _raw(L, qd, kd, wd, out, h, Mq, 256, d) == 0                                   # the key limit itself runs
    torch.cuda.synchronize()
    assert float((out[:, :Mq] - 1.0).abs().max()) <= bound(256, wd) and bool((out[:, Mq:] == SENTINEL).all())   # (weights 1)
    with pytest.raises(RuntimeError, match="weights"):
        L.attention_word_map(qd, kd, h, Mq, 77, d ** -0.5, wd[:, :76].contiguous(), out)
    with pytest.raises(RuntimeError, match="out_rows"):
        L.attention_word_map(qd, kd, h, Mq, 77, d ** -0.5, wd, out, torch.zeros(B, dtype=torch.int32, device=DEV))


# ---------------------------------------------------------------------------------------------------
# 2. the blend tail
# ---------------------------------------------------------------------------------------------------
BLEND_CASES = [(2, 3, 4, 4, 8, 8, 1), (1, 2, 5, 3, 10, 9, 0), (3, 1, 16, 16, 64, 64, 3)]   # (G, F, h, w, H, W, pool)


def _blend_operands(case, dtype, seed, C=4):
    G, Fr, h, w, H, W, pool = case
    g = torch.Generator().manual_seed(seed)
    acc = torch.rand(G, Fr, h, w, generator=g) ** 32       # (peaked, like a word's map: a 7 x 7 window still leaves pixels out)
    x = torch.randn(Fr, C, H, W, generator=g).to(dtype)
    x_src = torch.randn(Fr, C, H, W, generator=g).to(dtype)
    return acc.to(DEV), x.to(DEV), x_src.to(DEV)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("case", BLEND_CASES, ids=lambda c: "x".join(map(str, c)))
def test_local_blend_vs_formula(L, case, dtype):
    """Mask and output bit-equal to the torch restatement; an all-zero map adds nothing to the mask, all maps zero give
    x_src; out may be x; without the mask pointer the same output."""
    pool, thr = case[-1], 0.55
    acc, x, x_src = _blend_operands(case, dtype, seed=sum(case))
    want, want_mask = LB.blend_formula(acc, x, x_src, pool, thr)
    out, mask = L.local_blend(acc, x, x_src, pool, thr, return_mask=True)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (x.shape[0],) + tuple(x.shape[2:])
    inside = float(want_mask.float().mean())
    print(f"local_blend {case} {dtype}: {inside:.2f} of the pixels inside the mask")
    assert 0.0 < inside < 1.0, "the case does not exercise both sides of the select"
    assert torch.equal(mask.bool(), want_mask) and bool((mask <= 1).all())
    assert torch.equal(out, want)
    assert torch.equal(L.local_blend(acc, x, x_src, pool, thr), out)                          # mask pointer NULL
    if acc.shape[0] > 1:                                                                      # one group all zero
        z = acc.clone()
        z[0] = 0
        o2, m2 = L.local_blend(z, x, x_src, pool, thr, return_mask=True)
        w2, wm2 = LB.blend_formula(z[1:], x, x_src, pool, thr)
        assert torch.equal(m2.bool(), wm2) and torch.equal(o2, w2)
    o3, m3 = L.local_blend(torch.zeros_like(acc), x, x_src, pool, thr, return_mask=True)
    assert not bool(m3.any()) and torch.equal(o3, x_src)
    alias = x.clone()
    assert L.local_blend(acc, alias, x_src, pool, thr, out=alias) is alias and torch.equal(alias, want)


def test_local_blend_bad_arguments_launch_nothing(L):
    acc, x, x_src = _blend_operands((2, 3, 4, 4, 8, 8, 1), torch.float16, seed=3)
    out = torch.full_like(x, SENTINEL)
    st = torch.cuda.current_stream().cuda_stream

    def raw(G=2, h=4, pool=1, code=L.VTM_F16, acc_ptr=acc.data_ptr(), out_ptr=out.data_ptr(), thr=0.5):
        return L.lib().vtm_local_blend(acc_ptr, G, 3, h, 4, x.data_ptr(), x_src.data_ptr(), out_ptr, code, 4, 8, 8, pool, thr,
                                       None, st)
    err = lambda: L.lib().vtm_last_error().decode()
    assert raw(acc_ptr=None) == EINVAL and "vtm_local_blend" in err()
    assert raw(G=9) == EINVAL and "groups" in err()
    assert raw(h=3) == EINVAL and "multiple" in err()
    assert raw(pool=4) == EINVAL and raw(pool=-1) == EINVAL and "pool" in err()
    assert raw(code=7) == EINVAL
    assert raw(thr=float("nan")) == EINVAL
    assert raw(out_ptr=x_src.data_ptr()) == EINVAL and "overlaps" in err()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert raw() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, LB.blend_formula(acc, x, x_src, 1, 0.5)[0])


# ---------------------------------------------------------------------------------------------------
# 3. patched blocks
# ---------------------------------------------------------------------------------------------------
def _spy(monkeypatch, L):
    seen = {"words": []}
    orig = L.attention_word_map

    def f(*a, **kw):
        seen["words"].append(a[0].shape[0])
        return orig(*a, **kw)
    monkeypatch.setattr(L, "attention_word_map", f)
    return seen


def _expected(unet_blocks, lb, Fg, K):
    """sum over the blocks of attn2_probs[group rows] @ w in float64 -> (G, Fg, N), and the bound of one launch against it
    per group: the launch's own bound plus the map's."""
    want, per = [], []
    for gi, g in enumerate(lb.groups):
        w = lb.weights[gi].double()
        want.append(sum(blk.attn2_probs[g * Fg:(g + 1) * Fg].double().cpu() @ w for blk in unet_blocks))
        per.append(bound(K, lb.weights[gi]) + probs_bound(K, lb.weights[gi]))
    return torch.stack(want), per


def _check_acc(acc, want, per, nblocks, what):
    """|acc - want| <= nblocks launches' bounds + one fp32 rounding of every addition (each <= 2^-24 of the running sum,
    itself at most nblocks max|w|... taken at the result's magnitude plus the bounds)."""
    for gi in range(want.shape[0]):
        err = (acc[gi].double().cpu() - want[gi]).abs()
        lim = nblocks * per[gi] + nblocks * U * (want[gi].abs() + nblocks * per[gi])
        print(f"{what} group slot {gi}: max|acc - maps @ w|={float(err.max()):.3e} bound={float(lim.max()):.3e}")
        assert float((err - lim).max()) <= 0.0, (what, gi, float(err.max()))


@pytest.fixture(scope="module")
def block_case():
    """{(C, dtype): (unet, h, cond, the unregistered outputs)} behind a warm-up forward (profiles/first_forward_bits.txt)."""
    import vidtome_amd
    cache = {}

    def get(C, dtype):
        key = (C, dtype)
        if key not in cache:
            unet = LB.patched(C, dtype, DEV)
            h, cond = LB.inputs(C, dtype, DEV)
            LB.forward(unet, h, cond)
            cache[key] = (unet, h, cond, LB.forward(unet, h, cond))
        return cache[key]
    yield get
    for unet, *_ in cache.values():
        vidtome_amd.remove_patch(unet)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [320, 640])
def test_registered_blocks_accumulate_their_word_maps(L, block_case, C, dtype, monkeypatch):
    """[source | uncond | cond] x 2 frames of 8 x 8 tokens, 77 text tokens, two blocks, words on groups 0 and 2: one
    launch per block and group on the group's two samples, the accumulator is sum_blocks attn2_probs[group rows] @ w, the
    outputs are the bits of the unregistered blocks', a second forward doubles the accumulator, reset zeroes it."""
    import vidtome_amd
    unet, h, cond, base = block_case(C, dtype)
    seen = _spy(monkeypatch, L)
    lb = vidtome_amd.LocalBlend(LB.words(), LB.NUM_INPUTS, LB.FRAMES)
    assert vidtome_amd.register_attention_maps(unet) == LB.BLOCKS
    assert vidtome_amd.register_local_blend(unet, lb) == LB.BLOCKS
    out = LB.forward(unet, h, cond)
    assert all(torch.equal(o, b) for o, b in zip(out, base)), "the registration changed a block output"
    assert seen["words"] == [LB.FRAMES] * 4, seen
    acc = lb.maps()
    assert tuple(acc.shape) == (2, LB.FRAMES) + LB.GRID and acc.dtype == torch.float32
    want, per = _expected(unet.blocks, lb, LB.FRAMES, LB.COND)
    first = acc.clone().view(2, LB.FRAMES, LB.TOKENS)
    _check_acc(first, want, per, 2, f"C={C} {dtype}")
    assert float(first[0].min()) > 0 and float(first[0].max()) < 2 * 3      # (a 0 / 1 row on three words: probabilities)
    LB.forward(unet, h, cond)
    second = lb.maps().view(2, LB.FRAMES, LB.TOKENS)
    # four additions of values <= max|w| each after the first forward's: every partial sum <= 4 max|w|, four roundings
    lim = 4 * U * 4 * float(lb.weights.abs().max())
    assert float((second - 2 * first).abs().max()) <= lim
    lb.reset()
    assert not bool(lb.maps().any())
    vidtome_amd.unregister_local_blend(unet)
    seen["words"].clear()
    assert all(torch.equal(o, b) for o, b in zip(LB.forward(unet, h, cond), base))
    assert seen["words"] == [] and not bool(lb.maps().any()), "an unregistered block still accumulates"
    vidtome_amd.unregister_attention_maps(unet)


def test_chunks_fill_their_frame_rows(L, block_case):
    """A video of four frames in two chunked calls, set_frames([2, 0]) and set_frames([3, 1]): every frame row holds its own
    call's map; without set_frames a two-frame call into a four-frame accumulator raises."""
    import vidtome_amd
    C, dtype = 320, torch.float16
    unet, h, cond, _ = block_case(C, dtype)
    h2, cond2 = LB.inputs(C, dtype, DEV, seed=71)
    lb = vidtome_amd.LocalBlend(LB.words(), LB.NUM_INPUTS, 4)
    vidtome_amd.register_attention_maps(unet)
    vidtome_amd.register_local_blend(unet, lb)
    with pytest.raises(RuntimeError, match="set_frames"):
        LB.forward(unet, h, cond)
    with pytest.raises(ValueError, match="distinct"):
        lb.set_frames([1, 1])
    lb.set_frames([2, 0])
    LB.forward(unet, h, cond)
    want1, per = _expected(unet.blocks, lb, LB.FRAMES, LB.COND)
    lb.set_frames([3, 1])
    LB.forward(unet, h2, cond2)
    want2, _ = _expected(unet.blocks, lb, LB.FRAMES, LB.COND)
    acc = lb.maps().view(2, 4, LB.TOKENS)
    want = torch.stack([want1[:, 1], want2[:, 1], want1[:, 0], want2[:, 0]], dim=1)          # frames 0, 1, 2, 3
    _check_acc(acc, want, per, 2, "chunks")
    assert float((want1 - want2).abs().max()) > 1e-3, "the two chunks do not differ"
    vidtome_amd.unregister_local_blend(unet)
    vidtome_amd.unregister_attention_maps(unet)


@pytest.mark.parametrize("name", ["replace", "refine+reweight"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_edited_group_accumulates_the_edited_map(L, block_case, dtype, name, monkeypatch):
    """Under register_cross_attention_control the cond group's rows are the EDITED map times w -- two launches with the
    weights M (a o w) on the source's q / k and b o w on the group's own; the source group takes the plain launch.  Against
    the float64 restatement of P2P's controller on the 16-bit q / k rows the blocks read, times w, within the two launches'
    bounds plus the fp32 rounding of the transformed weights; and against the edited ``attn2_probs @ w`` within the launches' bounds plus that map's ((K + 8) 2^-24 (1 + sum|a| + sum|b|) per
    element, tests/test_gpu_cross_control.py) plus the fp32 rounding of the transformed weights."""
    import cross_control_standin as CC
    import standin
    import vidtome_amd
    from vidtome_amd import pnp
    C = 320
    unet, h, cond, base = block_case(C, dtype)
    seen = _spy(monkeypatch, L)
    rows, orig_probs = [], L.attention_probs
    monkeypatch.setattr(L, "attention_probs", lambda *a, **kw: (rows.append((a[0], a[1])), orig_probs(*a, **kw))[1])
    spec = LB.edit_spec(name)
    e = CC.edit_of(spec)
    lb = vidtome_amd.LocalBlend(LB.words(), LB.NUM_INPUTS, LB.FRAMES)
    vidtome_amd.register_attention_maps(unet)
    vidtome_amd.register_local_blend(unet, lb)
    vidtome_amd.register_cross_attention_control(unet, [981], LB.NUM_INPUTS, {2: e})
    pnp.register_time(standin.Pipe(unet), 981)
    out = LB.forward(unet, h, cond)
    F2 = 2 * LB.FRAMES
    assert all(torch.equal(o[:F2], b[:F2]) for o, b in zip(out, base)), "source / uncond rows changed"
    assert seen["words"] == [LB.FRAMES] * 6, seen                                   # per block: source, then (a) and (b)
    want, per = _expected(unet.blocks, lb, LB.FRAMES, LB.COND)
    K = LB.COND
    w = lb.weights[1].double()
    M, a, b = e.mapper.double(), e.src_weight.double(), e.own_weight.double()
    w_src, w_own = M @ (a * w), b * w
    tight = (bound(K, w_src) + bound(K, w_own)                                      # the two launches
             + (K + 2) * U * float((M.abs() @ (a * w).abs()).max()) + U * float(w_own.abs().max()))   # fp32 weights
    per[1] = tight + (K + 8) * U * (1 + float(a.abs().sum()) + float(b.abs().sum())) * float(w.abs().sum())   # the edited map
    acc = lb.maps().view(2, LB.FRAMES, LB.TOKENS)
    _check_acc(acc, want, per, 2, f"edited {name} {dtype}")
    assert len(rows) == 2
    n = h.shape[0]
    sh = lambda t, r: t[:, :r].double().cpu().view(n, r, LB.HEADS, -1).transpose(1, 2)
    exact = torch.zeros(LB.FRAMES, LB.TOKENS, dtype=torch.float64)
    for (q, k), blk in zip(rows, unet.blocks):
        per_head = torch.softmax(sh(q, LB.TOKENS) @ sh(k, K).transpose(-1, -2) * blk.attn2.scale, dim=-1)
        for f in range(LB.FRAMES):
            exact[f] += CC.controlled_probs(spec, per_head[f], per_head[F2 + f]).mean(0) @ w
    _check_acc(acc[1:], exact[None], [tight], 2, f"edited {name} {dtype} vs float64 P2P")
    # the edit moved the cond group's accumulated map
    plain = vidtome_amd.LocalBlend(LB.words(), LB.NUM_INPUTS, LB.FRAMES)
    vidtome_amd.unregister_cross_attention_control(unet)
    vidtome_amd.register_local_blend(unet, plain)
    LB.forward(unet, h, cond)
    assert float((plain.maps()[1] - lb.maps()[1]).abs().max()) > 1e-3, "the map was not edited"
    assert torch.equal(plain.maps()[0], lb.maps()[0]), "the source group's map changed"
    vidtome_amd.unregister_local_blend(unet)
    vidtome_amd.unregister_attention_maps(unet)


def _am_case(L, monkeypatch, dtype=torch.float16, words=None, num_frames=AM.FRAMES, **patched_kw):
    """One tests/attention_maps_standin.py block (2 groups x 2 frames of 8 x 8 tokens), maps and LocalBlend registered."""
    import vidtome_amd
    C = 320
    h, cond = AM.inputs(C, dtype, DEV)
    seen = _spy(monkeypatch, L)
    unet = AM.patched(C, dtype, DEV, **patched_kw)
    g = torch.Generator().manual_seed(3)
    lb = vidtome_amd.LocalBlend(words or {0: torch.randn(AM.COND, generator=g), 1: LB.words()[0]}, AM.B, num_frames)
    vidtome_amd.register_attention_maps(unet)
    vidtome_amd.register_local_blend(unet, lb)
    return unet, h, cond, lb, seen


def _run_am(unet, h, cond, **kw):
    with torch.no_grad():
        torch.manual_seed(123)
        return unet.blocks[0](h, encoder_hidden_states=cond, **kw)


def test_masked_route(L, monkeypatch):
    """An additive (B F, 1, 77) mask of 0 / -10000 (the key-bias route): the bias rows of every group's samples go with
    its launch; hidden keys weigh nothing."""
    import vidtome_amd
    unet, h, cond, lb, seen = _am_case(L, monkeypatch)
    mask, keep = AM.prompt_mask(torch.float16, DEV)
    _run_am(unet, h, cond, encoder_attention_mask=mask)
    assert seen["words"] == [AM.FRAMES] * 2
    want, per = _expected(unet.blocks, lb, AM.FRAMES, AM.COND)
    _check_acc(lb.maps().view(2, AM.FRAMES, -1), want, per, 1, "masked")
    hidden = vidtome_amd.LocalBlend({1: (~keep[2]).float()}, AM.B, AM.FRAMES)        # only keys hidden in sample (1, 0)
    vidtome_amd.register_local_blend(unet, hidden)
    _run_am(unet, h, cond, encoder_attention_mask=mask)
    assert not bool(hidden.maps()[0, 0].any()), "hidden keys contributed"
    vidtome_amd.remove_patch(unet)


def test_ip_adapter_route(L, monkeypatch):
    """A recognised IP-Adapter call: the word map is the TEXT set's, from the text rows of the key buffer."""
    import ip_adapter_standin as IP
    import vidtome_amd
    C, dtype = 320, torch.float16
    h, cond = AM.inputs(C, dtype, DEV)
    seen = _spy(monkeypatch, L)
    unet = AM.OneBlock(C).to(device=DEV, dtype=dtype)
    procs = IP.install(unet, num_tokens=(4,), scale=(0.6,), cond_dim=AM.COND_DIM)
    torch.manual_seed(123)
    vidtome_amd.apply_patch(unet, local_merge_ratio=0.5, merge_global=True, global_merge_ratio=0.5, batch_size=AM.B)
    unet.set_size(AM.LATENT)
    lb = vidtome_amd.LocalBlend({0: LB.words()[0], 1: LB.words()[2]}, AM.B, AM.FRAMES)
    vidtome_amd.register_attention_maps(unet)
    vidtome_amd.register_local_blend(unet, lb)
    _run_am(unet, h, (cond, IP.image_states((4,), AM.B * AM.FRAMES, AM.COND_DIM, dtype, DEV)))
    assert procs[0].calls == 0 and seen["words"] == [AM.FRAMES] * 2, seen
    want, per = _expected(unet.blocks, lb, AM.FRAMES, AM.COND)
    _check_acc(lb.maps().view(2, AM.FRAMES, -1), want, per, 1, "IP-Adapter")
    vidtome_amd.remove_patch(unet)


def test_custom_processor_block_takes_the_torch_restatement(L, monkeypatch):
    """A processor the fused path does not know: the module path, no launch of the kernel, the accumulator from the torch
    restatement of the module's to_q / to_k; a module whose map cannot be read raises."""
    import vidtome_amd
    unet, h, cond, lb, seen = _am_case(L, monkeypatch, storing=True)
    _run_am(unet, h, cond)
    assert unet.blocks[0].attn2.calls == 1 and seen["words"] == []
    want, per = _expected(unet.blocks, lb, AM.FRAMES, AM.COND)
    _check_acc(lb.maps().view(2, AM.FRAMES, -1), want, per, 1, "module path")
    unet.blocks[0].attn2.norm_cross = torch.nn.Identity()                 # something between the projections and the scores
    with pytest.raises(RuntimeError, match="cannot be read"):
        _run_am(unet, h, cond)
    vidtome_amd.remove_patch(unet)


def test_fp32_block_takes_the_torch_restatement(L, monkeypatch):
    import vidtome_amd
    C, dtype = 320, torch.float32
    h, cond = AM.inputs(C, dtype, DEV)
    seen = _spy(monkeypatch, L)
    unet = AM.patched(C, dtype, DEV)
    vidtome_amd.update_patch(unet, fp32_projections=True, fp32_attention=True)
    lb = vidtome_amd.LocalBlend({0: LB.words()[0], 1: LB.words()[2]}, AM.B, AM.FRAMES)
    vidtome_amd.register_attention_maps(unet)
    vidtome_amd.register_local_blend(unet, lb)
    _run_am(unet, h, cond)
    assert seen["words"] == []
    want, per = _expected(unet.blocks, lb, AM.FRAMES, AM.COND)
    _check_acc(lb.maps().view(2, AM.FRAMES, -1), want, per, 1, "fp32 block")
    vidtome_amd.remove_patch(unet)


def test_mixed_token_counts_and_a_k_mismatch_raise(L, monkeypatch):
    import vidtome_amd
    unet, h, cond, lb, seen = _am_case(L, monkeypatch)
    _run_am(unet, h, cond)
    small = AM.patched(320, torch.float16, DEV, latent=(6, 6))
    vidtome_amd.register_local_blend(small, lb)
    h36, _ = AM.inputs(320, torch.float16, DEV, tokens=36)
    with pytest.raises(RuntimeError, match=r"36 tokens per frame, the accumulator 64"):
        _run_am(small, h36, cond)
    short = vidtome_amd.LocalBlend({0: torch.ones(AM.COND - 1)}, AM.B, AM.FRAMES)
    vidtome_amd.register_local_blend(unet, short)
    with pytest.raises(RuntimeError, match=r"K = 77 tokens, the word weights are for K = 76"):
        _run_am(unet, h, cond)
    vidtome_amd.remove_patch(unet)
    vidtome_amd.remove_patch(small)


def test_blend_on_accumulated_maps(L, monkeypatch):
    """lb.blend after a registered forward: the formula on lb.maps(), and the mask when asked for."""
    import vidtome_amd
    unet, h, cond, lb, seen = _am_case(L, monkeypatch, words={0: LB.words()[0], 1: LB.words()[0]})
    _run_am(unet, h, cond)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(AM.FRAMES, 4, 32, 32, generator=g).to(device=DEV, dtype=torch.float16)
    x_src = torch.randn(AM.FRAMES, 4, 32, 32, generator=g).to(device=DEV, dtype=torch.float16)
    # (random weights give flat maps: the threshold is put at the median of the pooled, normalised map, so that both sides
    # of the select are exercised)
    acc = lb.maps()
    ratio = torch.nn.functional.max_pool2d(acc, 3, stride=1, padding=1) / acc.amax(dim=(2, 3), keepdim=True)
    lb.threshold = float(ratio.amax(dim=0).median())
    out, mask = lb.blend(x, x_src, return_mask=True)
    want, want_mask = LB.blend_formula(lb.maps(), x, x_src, lb.pool, lb.threshold)
    assert torch.equal(out, want) and torch.equal(mask.bool(), want_mask) and 0 < int(mask.sum()) < mask.numel()
    assert torch.equal(lb.blend(x, x_src), want)
    vidtome_amd.remove_patch(unet)
