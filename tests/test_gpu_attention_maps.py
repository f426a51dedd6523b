"""GPU tests of the head-averaged cross-attention maps (run with -m gpu on an MI355X): vtm_attention_probs through the C ABI
and through _lib.attention_probs against a float64 numpy evaluation on the same rounded operands, then the patched block
with register_attention_maps on every attn2 route against a float64 restatement of the module's own to_q / to_k.

The bound of every comparison is (Mk + 8) * 2^-24: the rounding of an fp32 evaluation of probabilities <= 1 (Mk terms in
the denominator, a handful of roundings on the score), not a model tolerance."""
import numpy as np
import pytest
import torch

import attention_maps_standin as AM

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = (torch.float16, torch.bfloat16)
SENTINEL = -7.0
# (B, h, Mq, Mk, d)
CASES = [(2, 2, 70, 77, 40),      # padded contraction, two key tiles, partial query block
         (1, 5, 33, 1, 64),       # a single key: every probability exactly 1
         (2, 1, 257, 256, 160),   # the key limit, several query blocks
         (2, 8, 65, 33, 8),       # smallest head dim
         (1, 2, 40, 64, 80),      # key tile edge
         (1, 2, 40, 65, 80)]      # ... one past


def bound(Mk):
    return (Mk + 8) * 2.0 ** -24


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


def _ref(q, k, h, Mq, Mk, bias=None):
    """float64 mean over the heads of softmax(q k^T d^-0.5 + bias) on the same 16-bit operands; bias (B or 1, Mk)."""
    B, d = q.shape[0], q.shape[2] // h
    sh = lambda t, n: t.double().numpy()[:, :n].reshape(B, n, h, d).transpose(0, 2, 1, 3)
    s = sh(q, Mq) @ sh(k, Mk).transpose(0, 1, 3, 2) * float(d) ** -0.5
    if bias is not None:
        s = s + np.asarray(bias, dtype=np.float64)[:, None, None, :]
    with np.errstate(invalid="ignore"):
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
    return p.mean(1)


def _raw(L, q, k, out, ldo, h, Mq, Mk, d, bias=None, ld_bias=0, stride=0, code=None, scale=None, ldq=None, Mqp=None):
    return L.lib().vtm_attention_probs(q.data_ptr(), q.stride(1) if ldq is None else ldq, k.data_ptr(), k.stride(1),
                                       out.data_ptr(), ldo, L.dtype_code(q) if code is None else code, q.shape[0], h, Mq,
                                       q.shape[1] if Mqp is None else Mqp, Mk, k.shape[1], d,
                                       d ** -0.5 if scale is None else scale, None if bias is None else bias.data_ptr(),
                                       ld_bias, stride, torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernel_vs_float64(L, case, dtype):
    B, h, Mq, Mk, d = case
    q, k = _operands(B, h, Mq, Mk, d, dtype, seed=sum(case))
    got = L.attention_probs(q.to(DEV), k.to(DEV), h, Mq, Mk, d ** -0.5)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, Mq, Mk)
    g = got.double().cpu().numpy()
    ref = _ref(q, k, h, Mq, Mk)
    err, rows = float(np.abs(g - ref).max()), float(np.abs(g.sum(-1) - 1.0).max())
    print(f"attention_probs {case} {dtype} max|out-ref|={err:.3e} max|rowsum-1|={rows:.3e} bound={bound(Mk):.3e}")
    assert err <= bound(Mk), (case, err)
    assert rows <= bound(Mk), (case, rows)
    if Mk == 1:
        assert bool((got == 1.0).all())
    again = L.attention_probs(q.to(DEV), k.to(DEV), h, Mq, Mk, d ** -0.5)
    assert torch.equal(got, again), "two calls differ"


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_strided_q_pad_rows_and_sentinels(L, dtype):
    """q as a column range of a wider buffer (ldq > h d), Mqp > Mq and Mkp > Mk with NaN in the pad rows, out rows >= Mq and
    columns [Mk, ldo) keep a sentinel."""
    B, h, Mq, Mk, d = 2, 2, 70, 77, 40
    C, Mqp, Mkp, ldo = h * d, 80, 88, 96
    q, k = _operands(B, h, Mq, Mk, d, dtype, seed=5, Mqp=Mqp, Mkp=Mkp)
    q[:, Mq:] = float("nan")
    k[:, Mk:] = float("nan")
    wide = torch.full((B, Mqp, 3 * C), float("nan"), dtype=dtype)
    wide[:, :, C:2 * C] = q
    qd = wide.to(DEV)[:, :, C:2 * C]
    assert qd.stride(1) == 3 * C
    kd = k.to(DEV)
    out = torch.full((B * Mq + 3, ldo), SENTINEL, dtype=torch.float32, device=DEV)
    rc = _raw(L, qd, kd, out, ldo, h, Mq, Mk, d)
    assert rc == 0, L.lib().vtm_last_error()
    torch.cuda.synchronize()
    assert bool((out[B * Mq:] == SENTINEL).all()) and bool((out[:, Mk:] == SENTINEL).all())
    g = out[:B * Mq, :Mk].view(B, Mq, Mk).double().cpu().numpy()
    err = float(np.abs(g - _ref(q, k, h, Mq, Mk)).max())
    assert err <= bound(Mk), err
    assert torch.equal(L.attention_probs(qd, kd, h, Mq, Mk, d ** -0.5), out[:B * Mq, :Mk].view(B, Mq, Mk))


@pytest.mark.parametrize("dtype", DTYPES)
def test_bias(L, dtype):
    B, h, Mq, Mk, d = 2, 2, 70, 77, 40
    q, k = _operands(B, h, Mq, Mk, d, dtype, seed=9)
    qd, kd = q.to(DEV), k.to(DEV)
    run = lambda bias: L.attention_probs(qd, kd, h, Mq, Mk, d ** -0.5, None if bias is None else bias.to(DEV))
    plain = run(None)
    assert torch.equal(run(torch.zeros(B, Mk)), plain), "a zero bias is not the unbiased call"
    # a 0 / -10000 row per sample (another prompt length in each)
    keep = torch.arange(Mk)[None, :] < torch.tensor([20, 70])[:, None]
    b1 = (1 - keep.float()) * -10000.0
    got = run(b1)
    assert float(np.abs(got.double().cpu().numpy() - _ref(q, k, h, Mq, Mk, b1.numpy())).max()) <= bound(Mk)
    assert bool((got.cpu()[~keep[:, None, :].expand(B, Mq, Mk)] == 0.0).all())          # exp(-10000) underflows
    # one row for every sample: bias_batch_stride = 0
    shared = run(b1[:1])
    assert float(np.abs(shared.double().cpu().numpy() - _ref(q, k, h, Mq, Mk, b1[:1].numpy())).max()) <= bound(Mk)
    assert torch.equal(shared[0], got[0]) and not torch.equal(shared[1], got[1])
    # -inf keys, among them the whole first tile: exactly 0, the rest against float64
    b2 = torch.zeros(B, Mk)
    b2[0, :66] = float("-inf")
    b2[1, 3::5] = float("-inf")
    got = run(b2)
    assert bool((got.cpu()[(b2 == float("-inf"))[:, None, :].expand(B, Mq, Mk)] == 0.0).all())
    assert float(np.abs(got.double().cpu().numpy() - _ref(q, k, h, Mq, Mk, b2.numpy())).max()) <= bound(Mk)
    # every key of sample 0 hidden: NaN there, sample 1 untouched
    b3 = torch.zeros(B, Mk)
    b3[0] = float("-inf")
    got = run(b3)
    assert bool(torch.isnan(got[0]).all()) and torch.equal(got[1], plain[1])


def test_bad_arguments_launch_nothing(L):
    B, h, Mq, d = 1, 2, 40, 40
    q, k = _operands(B, h, Mq, 264, d, torch.float16, seed=1)
    qd, kd = q.to(DEV), k.to(DEV)
    out = torch.full((B * Mq, 264), SENTINEL, dtype=torch.float32, device=DEV)
    EINVAL = -1
    assert _raw(L, qd, kd, out, 264, h, Mq, 257, d) == EINVAL                                     # Mk = 257
    q24 = torch.zeros(B, Mq, 48, dtype=torch.float16, device=DEV)
    assert _raw(L, q24, torch.zeros(B, 80, 48, dtype=torch.float16, device=DEV), out, 264, 2, Mq, 77, 24) == EINVAL   # d = 24
    assert _raw(L, qd, kd, out, 264, h, Mq, 77, d, code=L.VTM_F32) == EINVAL                      # VTM_F32
    assert _raw(L, qd, kd, out, 264, h, Mq, 77, d, scale=0.0) == EINVAL                           # scale = 0
    q41 = torch.zeros(B, Mq, 41 * 8, dtype=torch.float16, device=DEV)                             # 41 heads: one past the limit
    assert _raw(L, q41, torch.zeros(B, 80, 41 * 8, dtype=torch.float16, device=DEV), out, 264, 41, Mq, 77, 8) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    q40 = torch.zeros(B, Mq, 40 * 8, dtype=torch.float16, device=DEV)                             # the limit itself runs
    assert _raw(L, q40, torch.zeros(B, 80, 40 * 8, dtype=torch.float16, device=DEV), out, 264, 40, Mq, 77, 8) == 0
    torch.cuda.synchronize()
    assert float((out[:, :77] - 1.0 / 77).abs().max()) <= bound(77) and bool((out[:, 77:] == SENTINEL).all())   # (uniform)
    out.fill_(SENTINEL)
    assert _raw(L, qd, kd, out, 264, h, Mq, 256, d) == 0
    torch.cuda.synchronize()
    assert not bool((out[:, :256] == SENTINEL).any())


@pytest.mark.parametrize("h,Mk", [(2, 264), (41, 77)], ids=["Mk=264", "41 heads"])
def test_rows_beyond_the_kernels_limits_take_the_torch_restatement(L, h, Mk, monkeypatch):
    """patch._probs_rows on 16-bit rows the kernel refuses (Mk > 256, more than 40 heads): no launch, the fp32 torch
    restatement on the same rows, within the bound of float64."""
    from vidtome_amd import patch as vpatch
    monkeypatch.setattr(L, "attention_probs", lambda *a, **kw: pytest.fail("the kernel does not take this call"))
    B, Mq, d = 2, 40, 8
    q, k = _operands(B, h, Mq, Mk, d, torch.float16, seed=h + Mk, Mqp=48, Mkp=(Mk + 7) // 8 * 8)
    bias = torch.zeros(B, Mk)
    bias[1, 5:30] = float("-inf")
    got = vpatch._probs_rows(q.to(DEV), k.to(DEV), h, Mq, Mk, d ** -0.5, bias.to(DEV))
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, Mq, Mk)
    err = float(np.abs(got.double().cpu().numpy() - _ref(q, k, h, Mq, Mk, bias.numpy())).max())
    print(f"torch restatement h={h} Mk={Mk} max|out-ref|={err:.3e}")
    assert err <= bound(Mk) and bool((got[1, :, 5:30] == 0).all())


# ---------------------------------------------------------------------------------------------------
# 2. the patched block
# ---------------------------------------------------------------------------------------------------
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}     # half an ulp, relative


def _spies(monkeypatch, L):
    """Counts the attn2 core launches (attention_kv over the 77 keys, attention_kv_bias, attention_kv_sets) and the new
    wrapper's, and keeps the q / k rows and the bias the core was launched on."""
    seen = {"probs": 0, "kv": 0, "bias": 0, "sets": 0}

    def spy(name, key, keep):
        orig = getattr(L, name)

        def f(*a, **kw):
            if keep(a):
                seen[key] += 1
                seen["q"], seen["k"] = a[0], a[1]
                seen["b"] = a[7] if name == "attention_kv_bias" else None
            return orig(*a, **kw)
        monkeypatch.setattr(L, name, f)
    spy("attention_kv", "kv", lambda a: a[5] == AM.COND)            # (attn1's launches have other key counts)
    spy("attention_kv_bias", "bias", lambda a: True)
    spy("attention_kv_sets", "sets", lambda a: True)
    orig = L.attention_probs

    def probs(*a, **kw):
        seen["probs"] += 1
        return orig(*a, **kw)
    monkeypatch.setattr(L, "attention_probs", probs)
    orig_ln = L.layernorm_panels

    def ln(x, w, *a, **kw):
        seen.setdefault("ln", []).append((x, w))
        return orig_ln(x, w, *a, **kw)
    monkeypatch.setattr(L, "layernorm_panels", ln)
    return seen


def _forward(unet, h, cond, **kw):
    with torch.no_grad():
        torch.manual_seed(123)
        return unet.blocks[0](h, encoder_hidden_states=cond, **kw)


def _rows_are_the_modules_projections(blk, seen, cond, dtype):
    """The q / k rows the core (and the map) read ARE attn2's to_q(norm2(h)) / to_k(cond): against the float64 restatement,
    within what rounding the operands and the result to the model's dtype can move -- u (|y| + |x| |W|^T) elementwise, u
    half an ulp of the dtype (the fp32 accumulation adds 2^-24 of the same sum per term; 10 % of head-room covers it)."""
    hs = next(x for x, w in seen["ln"] if w is blk.norm2.weight)
    x2 = torch.nn.functional.layer_norm(hs.double().cpu(), hs.shape[-1:], blk.norm2.weight.detach().double().cpu(),
                                        blk.norm2.bias.detach().double().cpu(), blk.norm2.eps)
    for got, (y, mag) in ((seen["q"][:, :hs.shape[1]], AM.projection64(blk.attn2.to_q, x2)),
                          (seen["k"][:, :AM.COND], AM.projection64(blk.attn2.to_k, cond))):
        over = (got.double().cpu() - y).abs() - 1.1 * UNIT[dtype] * (y.abs() + mag)
        assert float(over.max()) <= 0.0, float(over.max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [320, 640])
def test_registered_block_carries_the_map_and_the_same_output(L, C, dtype, monkeypatch):
    """2 x 2 frames of 8 x 8 tokens, 77 text tokens, C = 320 / d = 40 and C = 640 / d = 80.  The registered block's output
    is the bits of the unregistered run; attn2 stays on the fused route (one attention_kv launch over the 77 keys, one
    attention_probs launch beside it); an unregistered block has no attribute.  The map is held to (Mk + 8) 2^-24 against
    the float64 restatement of the module's own to_q / to_k AS THE MODEL'S DTYPE HOLDS THEM: the restatement's q / k are
    the 16-bit rows the block's core read -- the same reading as the kernel test's "float64 on the same rounded q / k"; a
    restatement whose q / k are not rounded differs from ANY 16-bit evaluation by the rounding of q and k, ~1e-4 -- and
    those rows are checked to be to_q(norm2(h)) / to_k(cond) of the module's weights within operand rounding."""
    import vidtome_amd
    h, cond = AM.inputs(C, dtype, DEV)
    seen = _spies(monkeypatch, L)
    plain = AM.patched(C, dtype, DEV)
    base = _forward(plain, h, cond)
    assert not hasattr(plain.blocks[0], "attn2_probs") and not hasattr(plain.blocks[0], "vtm_attention_maps")
    assert (seen["probs"], seen["kv"]) == (0, 1)
    vidtome_amd.remove_patch(plain)

    unet = AM.patched(C, dtype, DEV)
    blk = unet.blocks[0]
    assert vidtome_amd.register_attention_maps(unet) == ["blocks.0"]
    seen.update(probs=0, kv=0, bias=0, sets=0, ln=[])
    out = _forward(unet, h, cond)
    assert torch.equal(out, base), "the switch changed the block output"
    assert (seen["probs"], seen["kv"], seen["bias"], seen["sets"]) == (1, 1, 0, 0), seen
    got = blk.attn2_probs
    N = AM.LATENT[0] * AM.LATENT[1]
    assert tuple(got.shape) == (AM.B * AM.FRAMES, N, AM.COND) and got.dtype == torch.float32 and not got.requires_grad
    ref = AM.probs64(seen["q"][:, :N], seen["k"][:, :AM.COND], AM.HEADS, blk.attn2.scale)
    err = float((got.double().cpu() - ref).abs().max())
    print(f"registered block C={C} {dtype} max|map - float64|={err:.3e} bound={bound(AM.COND):.3e}")
    assert err <= bound(AM.COND), err
    _rows_are_the_modules_projections(blk, seen, cond, dtype)
    assert vidtome_amd.collect_from_patch(unet, "attn2_probs")["blocks.0"] is got
    _forward(unet, h, cond)
    assert blk.attn2_probs is not got and tuple(blk.attn2_probs.shape) == tuple(got.shape)   # replaced, not accumulated
    assert float((blk.attn2_probs.sum(-1) - 1).abs().max()) <= bound(AM.COND)
    vidtome_amd.unregister_attention_maps(unet)
    assert not hasattr(blk, "attn2_probs") and not hasattr(blk, "vtm_attention_maps")
    vidtome_amd.remove_patch(unet)


def test_masked_block_hides_the_masked_keys(L, monkeypatch):
    """An additive (B F, 1, 77) mask of 0 / -10000: the key-bias route (one attention_kv_bias launch, one attention_probs
    launch), probability 0 on the hidden keys, the rest within the bound."""
    import vidtome_amd
    C, dtype = 320, torch.float16
    h, cond = AM.inputs(C, dtype, DEV)
    mask, keep = AM.prompt_mask(dtype, DEV)
    seen = _spies(monkeypatch, L)
    unet = AM.patched(C, dtype, DEV)
    vidtome_amd.register_attention_maps(unet)
    _forward(unet, h, cond, encoder_attention_mask=mask)
    assert (seen["probs"], seen["kv"], seen["bias"]) == (1, 0, 1), seen
    got = unet.blocks[0].attn2_probs
    N = h.shape[1]
    assert bool((got.cpu()[~keep[:, None, :].expand(-1, N, -1)] == 0.0).all())
    ref = AM.probs64(seen["q"][:, :N], seen["k"][:, :AM.COND], AM.HEADS, unet.blocks[0].attn2.scale, mask[:, 0])
    err = float((got.double().cpu() - ref).abs().max())
    print(f"masked block max|map - float64|={err:.3e}")
    assert err <= bound(AM.COND), err
    vidtome_amd.remove_patch(unet)


def test_odd_token_count_on_the_library_gemm_route(L, monkeypatch):
    """6 x 6 tokens (N % 8 != 0) through cross_attention() (VIDTOME_FF=blas): q is padded to 40 rows, the map has 36."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    monkeypatch.setattr(vpatch, "FF_MODE", "blas")
    C, dtype, N = 320, torch.float16, 36
    h, cond = AM.inputs(C, dtype, DEV, tokens=N)
    seen = _spies(monkeypatch, L)
    unet = AM.patched(C, dtype, DEV, latent=(6, 6))
    vidtome_amd.register_attention_maps(unet)
    _forward(unet, h, cond)
    assert (seen["probs"], seen["kv"]) == (1, 1) and seen["q"].shape[1] == 40, seen
    got = unet.blocks[0].attn2_probs
    assert tuple(got.shape) == (AM.B * AM.FRAMES, N, AM.COND)
    ref = AM.probs64(seen["q"][:, :N], seen["k"][:, :AM.COND], AM.HEADS, unet.blocks[0].attn2.scale)
    err = float((got.double().cpu() - ref).abs().max())
    print(f"6 x 6 tokens max|map - float64|={err:.3e}")
    assert err <= bound(AM.COND), err
    vidtome_amd.remove_patch(unet)


def test_custom_processor_block_gets_the_torch_fallback(L, monkeypatch):
    """A block whose attn2 carries a processor the fused path does not know takes the module path; its map comes from the
    torch restatement, within 1e-5 of the kernel's map on the same to_q / to_k rows (two fp32 evaluations that differ by the
    base of the exponential and the order of the sums) and within the kernel's bound of float64."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    C, dtype = 320, torch.float16
    h, cond = AM.inputs(C, dtype, DEV)
    seen = _spies(monkeypatch, L)
    rows = {}
    orig = vpatch._probs_torch

    def keep_rows(q, k, heads, scale, bias):
        rows["q"], rows["k"] = q, k
        return orig(q, k, heads, scale, bias)
    monkeypatch.setattr(vpatch, "_probs_torch", keep_rows)
    unet = AM.patched(C, dtype, DEV, storing=True)
    vidtome_amd.register_attention_maps(unet)
    blk = unet.blocks[0]
    _forward(unet, h, cond)
    assert blk.attn2.calls == 1 and (seen["probs"], seen["kv"], seen["bias"], seen["sets"]) == (0, 0, 0, 0), seen
    got = blk.attn2_probs
    assert tuple(got.shape) == (AM.B * AM.FRAMES, h.shape[1], AM.COND) and got.dtype == torch.float32
    assert tuple(rows["q"].shape) == tuple(h.shape) and rows["q"].dtype == dtype
    kernel = L.attention_probs(rows["q"].contiguous(), rows["k"].contiguous(), AM.HEADS, h.shape[1], AM.COND, blk.attn2.scale)
    d_kernel = float((got - kernel).abs().max())
    d_ref = float((got.double().cpu() - AM.probs64(rows["q"], rows["k"], AM.HEADS, blk.attn2.scale)).abs().max())
    print(f"module path max|fallback - kernel|={d_kernel:.3e} max|fallback - float64|={d_ref:.3e}")
    assert d_kernel <= 1e-5 and d_ref <= bound(AM.COND), (d_kernel, d_ref)
    vidtome_amd.remove_patch(unet)


def test_ip_adapter_block_gives_the_map_of_the_text_set(L, monkeypatch):
    """A recognised IP-Adapter call (tests/ip_adapter_standin.py): the core is one attention_kv_sets launch over text and
    image keys, the map is the text set's own softmax -- 77 columns that sum to 1."""
    import ip_adapter_standin as IP
    import vidtome_amd
    C, dtype = 320, torch.float16
    h, cond = AM.inputs(C, dtype, DEV)
    seen = _spies(monkeypatch, L)
    unet = AM.OneBlock(C).to(device=DEV, dtype=dtype)
    procs = IP.install(unet, num_tokens=(4,), scale=(0.6,), cond_dim=AM.COND_DIM)
    torch.manual_seed(123)
    vidtome_amd.apply_patch(unet, local_merge_ratio=0.5, merge_global=True, global_merge_ratio=0.5, batch_size=AM.B)
    unet.set_size(AM.LATENT)
    vidtome_amd.register_attention_maps(unet)
    images = IP.image_states((4,), AM.B * AM.FRAMES, AM.COND_DIM, dtype, DEV)
    _forward(unet, h, (cond, images))
    assert procs[0].calls == 0 and (seen["probs"], seen["sets"], seen["kv"]) == (1, 1, 0), seen
    got = unet.blocks[0].attn2_probs
    N = h.shape[1]
    assert tuple(got.shape) == (AM.B * AM.FRAMES, N, AM.COND)
    assert seen["k"].shape[1] > 80                                                  # (the buffer holds the image keys too)
    ref = AM.probs64(seen["q"][:, :N], seen["k"][:, :AM.COND], AM.HEADS, unet.blocks[0].attn2.scale)
    err = float((got.double().cpu() - ref).abs().max())
    print(f"IP-Adapter block max|map - float64 (text set)|={err:.3e}")
    assert err <= bound(AM.COND), err
    vidtome_amd.remove_patch(unet)


def test_fp32_block_with_fp32_projections_gets_the_map_from_its_fp32_rows(L, monkeypatch):
    """An fp32 block with ``fp32_projections``: attn2 runs on the fp32 GEMMs and the fp32 core (norm_cross_attention_f32);
    the kernel takes 16-bit rows only, so the map is the torch restatement on the segment's fp32 q / k rows."""
    import vidtome_amd
    C, dtype = 320, torch.float32
    h, cond = AM.inputs(C, dtype, DEV)
    seen = _spies(monkeypatch, L)
    unet = AM.patched(C, dtype, DEV)
    vidtome_amd.update_patch(unet, fp32_projections=True, fp32_attention=True)
    vidtome_amd.register_attention_maps(unet)
    _forward(unet, h, cond)
    assert (seen["probs"], seen["kv"], seen["bias"]) == (0, 1, 0) and seen["q"].dtype == torch.float32, seen
    got = unet.blocks[0].attn2_probs
    N = h.shape[1]
    assert tuple(got.shape) == (AM.B * AM.FRAMES, N, AM.COND) and got.dtype == torch.float32
    ref = AM.probs64(seen["q"][:, :N], seen["k"][:, :AM.COND], AM.HEADS, unet.blocks[0].attn2.scale)
    err = float((got.double().cpu() - ref).abs().max())
    print(f"fp32 block max|map - float64|={err:.3e}")
    assert err <= bound(AM.COND), err
    vidtome_amd.remove_patch(unet)


def test_ada_layer_norm_block_with_a_mask_gets_the_module_path_map(L, monkeypatch):
    """An AdaLayerNorm block handed a mask calls attn2's own forward (whatever the mask's form); the map comes from the
    torch restatement on the module's to_q / to_k, with 0 on the hidden keys."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    C, dtype = 320, torch.float16
    h, cond = AM.inputs(C, dtype, DEV)
    mask, keep = AM.prompt_mask(dtype, DEV)
    seen = _spies(monkeypatch, L)
    rows = {}
    orig = vpatch._probs_torch

    def keep_rows(q, k, heads, scale, bias):
        rows["q"], rows["k"], rows["b"] = q, k, bias
        return orig(q, k, heads, scale, bias)
    monkeypatch.setattr(vpatch, "_probs_torch", keep_rows)
    unet = AM.patched(C, dtype, DEV, storing=True, computing_self=True)
    blk = unet.blocks[0]
    blk.use_ada_layer_norm = True
    blk.norm1, blk.norm2 = AM.AdaNorm(blk.norm1), AM.AdaNorm(blk.norm2)
    vidtome_amd.register_attention_maps(unet)
    _forward(unet, h, cond, encoder_attention_mask=mask, timestep=torch.zeros(AM.B * AM.FRAMES, dtype=torch.long, device=DEV))
    assert blk.attn2.calls == 1 and (seen["probs"], seen["kv"], seen["bias"]) == (0, 0, 0), seen
    got = blk.attn2_probs
    N = h.shape[1]
    assert tuple(got.shape) == (AM.B * AM.FRAMES, N, AM.COND)
    assert bool((got.cpu()[~keep[:, None, :].expand(-1, N, -1)] == 0.0).all())
    ref = AM.probs64(rows["q"], rows["k"], AM.HEADS, blk.attn2.scale, rows["b"])
    err = float((got.double().cpu() - ref).abs().max())
    print(f"AdaLayerNorm block max|map - float64|={err:.3e}")
    assert err <= bound(AM.COND), err
    vidtome_amd.remove_patch(unet)
