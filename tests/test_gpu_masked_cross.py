"""GPU tests of masked cross-attention on the HIP path (run with -m gpu on an MI355X): vtm_attention_kv_bias through the C
ABI and through _lib.attention_kv_bias against a float64 numpy softmax on the same rounded operands, then the patched block
with an `encoder_attention_mask` against a float64 restatement of the block, where it ran, and what keeps the module path.

Shapes of the kernel tests (the smallest that reach every edge): B = 2, 2 heads, Mq = 72 in a buffer of Mqp = 80 rows (a partial
query block; rows 72 .. 79 of the output hold a sentinel), Mk = 8 / 77 / 130 keys (one short tile; a second tile of 13 keys
with Mkp = 80; three tiles), every head dim the block sites use plus d = 8.  Tolerance: the attention core's stated figures
(INTEGRATION.md section 1), 1e-3 of the output scale for fp16 and 8e-3 for bf16."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import standin
from test_gpu_lora import _capture_plans, _oracle_rows, _patch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}            # the attention core's figures
BLOCK_TOL = {torch.float16: 2e-3, torch.bfloat16: 8e-3}      # the whole block's
B, H, MQ, MQP = 2, 2, 72, 80
KEYS = (8, 77, 130)
HEAD_DIMS = (8, 40, 64, 80, 160)
DTYPES = (torch.float16, torch.bfloat16)
SENTINEL = 5.0


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


# ---------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------
def _operands(d, Mk, dtype, seed):
    """q (B, Mqp, C), k / v (B, Mkp, C) on the host, different data per sample; the padding keys behind Mk hold large finite
    values (nothing may read them as keys)."""
    g = torch.Generator().manual_seed(seed)
    C, Mkp = H * d, (Mk + 7) // 8 * 8
    q = torch.randn(B, MQP, C, generator=g).to(dtype)
    k = torch.full((B, Mkp, C), 3.0e4).to(dtype)
    v = torch.full((B, Mkp, C), 3.0e4).to(dtype)
    k[:, :Mk] = torch.randn(B, Mk, C, generator=g).to(dtype)
    v[:, :Mk] = torch.randn(B, Mk, C, generator=g).to(dtype)
    return q, k, v


def _ref(q, k, v, bias, Mk, d):
    """float64 numpy softmax(q k^T scale + bias) v on the same 16-bit operands; bias (B, Mk) float64 (may hold -inf)."""
    sh = lambda t, n: t.double().numpy()[:, :n].reshape(B, n, H, d).transpose(0, 2, 1, 3)
    s = sh(q, MQ) @ sh(k, Mk).transpose(0, 1, 3, 2) * d ** -0.5 + np.asarray(bias, dtype=np.float64)[:, None, None, :]
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return (p @ sh(v, Mk)).transpose(0, 2, 1, 3).reshape(B, MQ, H * d)


def _dev(q, k, v):
    return q.to(DEV), k.to(DEV), v.transpose(1, 2).contiguous().to(DEV)


def _raw(L, qd, kd, vtd, out, Mk, d, bias_ptr, ld, stride, code=None):
    C = H * d
    return L.lib().vtm_attention_kv_bias(qd.data_ptr(), C, kd.data_ptr(), C, vtd.data_ptr(), vtd.shape[2], out.data_ptr(), C,
                                         L.dtype_code(qd) if code is None else code, B, H, MQ, MQP, Mk, kd.shape[1], d,
                                         d ** -0.5, bias_ptr, ld, stride, torch.cuda.current_stream().cuda_stream)


def _run(L, qd, kd, vtd, Mk, d, bias, stride=None):
    """One C-ABI call on a sentinel-filled output: the device result (B, Mqp, C); rows >= Mq must still hold the sentinel."""
    out = torch.full((B, MQP, H * d), SENTINEL, dtype=qd.dtype, device=DEV)
    ld = bias.shape[1]
    rc = _raw(L, qd, kd, vtd, out, Mk, d, bias.data_ptr(), ld, bias.stride(0) if stride is None else stride)
    assert rc == 0, L.lib().vtm_last_error()
    torch.cuda.synchronize()
    assert bool((out[:, MQ:] == SENTINEL).all()), "rows >= Mq were written"
    return out


def _ratio(got, ref):
    """max |got - ref| over the output scale; got: the device result, ref: (B, Mq, C) float64."""
    g = got[:, :MQ].double().cpu().numpy()
    assert np.isfinite(g).all()
    return float(np.abs(g - ref).max()) / max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_zero_bias_is_the_plain_core(L, d, dtype):
    """A bias of zeros: within the tolerance of the float64 reference and of vtm_attention_kv on the same operands (another
    kernel: bit equality is not asked)."""
    for Mk in KEYS:
        q, k, v = _operands(d, Mk, dtype, seed=1000 * d + Mk)
        qd, kd, vtd = _dev(q, k, v)
        ref = _ref(q, k, v, np.zeros((B, Mk)), Mk, d)
        got = _run(L, qd, kd, vtd, Mk, d, torch.zeros(B, Mk, device=DEV))
        plain = L.attention_kv(qd, kd, vtd, H, MQ, Mk, d ** -0.5)
        e_ref, e_plain = _ratio(got, ref), _ratio(got, plain[:, :MQ].double().cpu().numpy())
        print(f"attention_kv_bias zero d={d} {dtype} Mk={Mk} err/scale={e_ref:.3e} vs attention_kv={e_plain:.3e}")
        assert e_ref < TOL[dtype] and e_plain < TOL[dtype], (Mk, e_ref, e_plain)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_random_bias_rows_and_batch_indexing(L, d, dtype):
    """Finite bias in [-4, 4], another row per sample, in rows longer than Mk whose tails hold NaN (never read).  Then the
    same call with bias_batch_stride = 0: sample 1 must equal the reference computed with sample 0's row.  The wrapper gives
    the bits of the C-ABI call for (B, ld), (1, ld) and a row stride above ld."""
    for Mk in KEYS:
        q, k, v = _operands(d, Mk, dtype, seed=2000 * d + Mk)
        qd, kd, vtd = _dev(q, k, v)
        g = torch.Generator().manual_seed(Mk)
        ld = Mk + 5
        bias = torch.full((B, ld), float("nan"))
        bias[:, :Mk] = torch.rand(B, Mk, generator=g) * 8 - 4
        bd = bias.to(DEV)
        got = _run(L, qd, kd, vtd, Mk, d, bd)
        err = _ratio(got, _ref(q, k, v, bias[:, :Mk].double().numpy(), Mk, d))
        print(f"attention_kv_bias random d={d} {dtype} Mk={Mk} err/scale={err:.3e}")
        assert err < TOL[dtype], (Mk, err)
        shared = _run(L, qd, kd, vtd, Mk, d, bd, stride=0)
        err0 = _ratio(shared, _ref(q, k, v, bias[:1, :Mk].expand(B, Mk).double().numpy(), Mk, d))
        assert err0 < TOL[dtype], (Mk, err0)
        assert torch.equal(shared[0], got[0]) and not torch.equal(shared[1], got[1])
        scale = d ** -0.5
        assert torch.equal(L.attention_kv_bias(qd, kd, vtd, H, MQ, Mk, scale, bd)[:, :MQ], got[:, :MQ])
        assert torch.equal(L.attention_kv_bias(qd, kd, vtd, H, MQ, Mk, scale, bd[:1])[:, :MQ], shared[:, :MQ])
        wide = torch.full((B, 2 * ld), float("nan"), device=DEV)
        wide[:, :ld] = bd
        assert torch.equal(L.attention_kv_bias(qd, kd, vtd, H, MQ, Mk, scale, wide[:, :ld])[:, :MQ], got[:, :MQ])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_minus_10000_on_the_last_keys(L, d, dtype):
    """What Diffusers gives for a padded prompt: 0 on the prompt's keys, -10000 behind them, another length per sample.
    Within the tolerance of the reference over the unmasked prefix."""
    hidden = {8: (3, 5), 77: (20, 47), 130: (10, 70)}
    for Mk in KEYS:
        q, k, v = _operands(d, Mk, dtype, seed=3000 * d + Mk)
        keep = torch.arange(Mk)[None, :] < (Mk - torch.tensor(hidden[Mk]))[:, None]
        bias = (1 - keep.to(dtype)) * -10000.0                       # as the UNet builds it, in the model's dtype
        prefix = np.where(keep.numpy(), 0.0, -np.inf)
        got = _run(L, *_dev(q, k, v), Mk, d, bias.float().to(DEV))
        err = _ratio(got, _ref(q, k, v, prefix, Mk, d))
        print(f"attention_kv_bias -10000 d={d} {dtype} Mk={Mk} err/scale={err:.3e}")
        assert err < TOL[dtype], (Mk, err)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_minus_inf_on_interior_keys_is_probability_zero(L, d, dtype):
    """-inf on one interior key of every tile (other keys per sample) whose k rows are scaled to dominate unmasked: within the
    tolerance; with those keys' k and v rows replaced by other finite values the output is bit-identical (p is exactly 0)."""
    for Mk in KEYS:
        q, k, v = _operands(d, Mk, dtype, seed=4000 * d + Mk)
        g = torch.Generator().manual_seed(Mk)
        bias = torch.rand(B, Mk, generator=g) * 2 - 1
        masked = [[t * 64 + min(5 + 3 * b, Mk - t * 64 - 1) for t in range((Mk + 63) // 64)] for b in range(B)]
        for b in range(B):
            bias[b, masked[b]] = float("-inf")
            k[b, masked[b]] = (k[b, masked[b]].float() * 16).to(dtype)
        qd, kd, vtd = _dev(q, k, v)
        got = _run(L, qd, kd, vtd, Mk, d, bias.to(DEV))
        err = _ratio(got, _ref(q, k, v, bias.double().numpy(), Mk, d))
        leak = _ratio(got, _ref(q, k, v, np.where(np.isinf(bias.numpy()), 0.0, bias.double().numpy()), Mk, d))
        print(f"attention_kv_bias -inf d={d} {dtype} Mk={Mk} err/scale={err:.3e} (unmasked it would be {leak:.3e})")
        assert err < TOL[dtype], (Mk, err)
        assert leak > 10 * TOL[dtype], "the masked keys would not have mattered"
        k2, v2 = k.clone(), v.clone()
        for b in range(B):
            k2[b, masked[b]] = (torch.randn(len(masked[b]), H * d, generator=g) * 4).to(dtype)
            v2[b, masked[b]] = (torch.randn(len(masked[b]), H * d, generator=g) * 100).to(dtype)
        again = _run(L, *_dev(q, k2, v2), Mk, d, bias.to(DEV))
        assert torch.equal(again, got), Mk


def test_kernel_rejects_bad_arguments(L):
    """A null bias, ld_bias < Mk, a batch stride inside a row, fp32 operands: an error code, nothing launched (out untouched);
    the wrapper raises on fp32 tensors."""
    d, Mk = 40, 77
    lib = L.lib()
    for dtype in (torch.float16, torch.float32):
        q = torch.zeros(B, MQP, H * d, dtype=dtype, device=DEV)
        k = torch.zeros(B, 80, H * d, dtype=dtype, device=DEV)
        vt = torch.zeros(B, H * d, 80, dtype=dtype, device=DEV)
        bias = torch.zeros(B, 80, device=DEV)
        out = torch.full((B, MQP, H * d), SENTINEL, dtype=dtype, device=DEV)
        if dtype == torch.float32:
            assert _raw(L, q, k, vt, out, Mk, d, bias.data_ptr(), 80, 80) == -1
            assert b"fp32" in lib.vtm_last_error()
        else:
            assert _raw(L, q, k, vt, out, Mk, d, None, 80, 80) == -1
            assert b"bias" in lib.vtm_last_error()
            assert _raw(L, q, k, vt, out, Mk, d, bias.data_ptr(), Mk - 1, 80) == -1
            for stride in (1, 40, 79):
                assert _raw(L, q, k, vt, out, Mk, d, bias.data_ptr(), 80, stride) == -1
            assert _raw(L, q, k, vt, out, Mk, 24, bias.data_ptr(), 80, 80) == -1        # a head dim without a kernel
            assert _raw(L, q, k, vt, out, 81, d, bias.data_ptr(), 81, 81) == -1         # Mk beyond Mkp
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())
    with pytest.raises(RuntimeError):
        L.attention_kv_bias(q, k, vt, H, MQ, Mk, d ** -0.5, bias)                        # fp32 through the wrapper


# ---------------------------------------------------------------------------------------------------
# 2. the block
# ---------------------------------------------------------------------------------------------------
FRAMES, LATENT, COND = 4, (16, 16), 77


class _TorchAttention(torch.nn.Module):
    """A computing, counting forward for a stand-in Attention: the module path."""
    calls = 0

    def forward(self, x, encoder_hidden_states=None, attention_mask=None, **kw):
        self.calls += 1
        ctx = x if encoder_hidden_states is None else encoder_hidden_states
        n, N, _ = x.shape
        sh = lambda t: t.view(n, t.shape[1], self.heads, -1).transpose(1, 2)
        mask = attention_mask
        if mask is not None and mask.dim() == 3:
            mask = mask[:, None]
        o = F.scaled_dot_product_attention(sh(self.to_q(x)), sh(self.to_k(ctx)), sh(self.to_v(ctx)), attn_mask=mask,
                                           scale=self.scale)
        return self.to_out[0](o.transpose(1, 2).reshape(n, N, -1))


class _TorchSelf(_TorchAttention, standin.Attention):
    pass


class _TorchCross(_TorchAttention, standin.CrossAttention):
    pass


class _AdaNorm(torch.nn.Module):
    """AdaLayerNorm's call form (x, timestep) around a LayerNorm."""

    def __init__(self, ln):
        super().__init__()
        self.ln = ln

    def forward(self, x, timestep=None):
        return self.ln(x)


class _OneBlock(standin.ModelMixin):
    """One full tests/standin.py block (its Attention.forward raises) at downsample 1, weights drawn like sites.SiteUNet's;
    ``computing``: attn1 / attn2 are the counting torch implementations instead."""

    def __init__(self, C, heads, computing=False, seed=0):
        super().__init__()
        blk = standin.BasicTransformerBlock(C, heads, True, 768)
        if computing:
            blk.attn1, blk.attn2 = _TorchSelf(C, heads), _TorchCross(C, heads, 768)
        self.blocks = torch.nn.ModuleList([blk])
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in self.parameters():
                if p.ndim == 2:
                    p.copy_(torch.randn(p.shape, generator=g) * p.shape[-1] ** -0.5)

    def set_size(self, latent_hw):
        self._tome_info["size"] = latent_hw


def _inputs(C, dtype, ck):
    from vidtome_amd import sites as S
    site = S.Site("site", 1, C, 8)
    h = S.synthetic_hidden(site, B, FRAMES, LATENT, dtype, DEV, seed=70 + 10 * ck, clip_seed=7, regime="corr01")
    cond = torch.randn(B * FRAMES, COND, 768, generator=torch.Generator().manual_seed(3)).to(device=DEV, dtype=dtype)
    return h, cond


def _prompt_mask(dtype):
    """Diffusers' additive form of an encoder_attention_mask, (B F, 1, 77) of 0 / -10000: another prompt length in every row."""
    lengths = torch.tensor([20 + 7 * i for i in range(B * FRAMES)])
    keep = torch.arange(COND)[None, :] < lengths[:, None]
    return ((1 - keep.to(dtype)) * -10000.0).unsqueeze(1).to(DEV)


def _masked_oracle_rows(blk, plan, hidden, cond, mask, idx):
    """float64 block output at the joined-chunk positions idx: the self-attention segment from the merge plan
    (test_gpu_lora._oracle_rows), then norm2 / attn2 over the conditioning with ``mask`` (n, 1, 77; None: no mask) ADDED TO
    THE SCORES / norm3 / GEGLU feed-forward."""
    fold = lambda m: (m.weight.detach().double().cpu(), None if m.bias is None else m.bias.detach().double().cpu())
    lin = lambda m, x: x @ fold(m)[0].T + (0 if fold(m)[1] is None else fold(m)[1])
    ln = lambda n, x: F.layer_norm(x, x.shape[-1:], n.weight.double().cpu(), n.bias.double().cpu(), n.eps)
    h = _oracle_rows(blk, plan, hidden, None, FRAMES, idx, fold, False)
    N = hidden.shape[1]
    c = cond.double().cpu().view(B, FRAMES, COND, -1)
    add = torch.zeros(B, FRAMES, COND, dtype=torch.float64) if mask is None else mask.double().cpu().view(B, FRAMES, COND)
    frame = torch.as_tensor(idx) // N
    a2 = blk.attn2
    sh = lambda t: t.view(t.shape[0], a2.heads, -1).transpose(0, 1)
    x2 = ln(blk.norm2, h)
    o2 = torch.empty_like(h)
    for b in range(B):
        for f in frame.unique().tolist():
            sel = (frame == f).nonzero().flatten()
            q, kf, vf = lin(a2.to_q, x2[b, sel]), lin(a2.to_k, c[b, f]), lin(a2.to_v, c[b, f])
            p = torch.softmax(sh(q) @ sh(kf).transpose(-1, -2) * a2.scale + add[b, f], dim=-1)
            o2[b, sel] = (p @ sh(vf)).transpose(0, 1).reshape(len(sel), -1)
    h2 = lin(a2.to_out[0], o2) + h
    p = lin(blk.ff.net[0].proj, ln(blk.norm3, h2))
    D = p.shape[-1] // 2
    return lin(blk.ff.net[2], p[..., :D] * F.gelu(p[..., D:])) + h2


def _spies(monkeypatch, L):
    """Counts the new wrapper's calls and records the key count of every _lib.attention_kv call."""
    seen = {"bias": 0, "kv_keys": []}
    orig_b, orig_kv = L.attention_kv_bias, L.attention_kv

    def bias(*a, **kw):
        seen["bias"] += 1
        return orig_b(*a, **kw)

    def kv(*a, **kw):
        seen["kv_keys"].append(a[5])
        return orig_kv(*a, **kw)
    monkeypatch.setattr(L, "attention_kv_bias", bias)
    monkeypatch.setattr(L, "attention_kv", kv)
    return seen


@pytest.mark.parametrize("mode", ["panels", "blas"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [320, 640])
def test_masked_block_vs_float64_oracle(L, C, dtype, mode, monkeypatch):
    """A full stand-in block (attn1's and attn2's module forward raise) at C = 320 / d = 40 and C = 640 / d = 80, 4 frames of
    16 x 16 tokens, 77 conditioning tokens, through apply_patch with an encoder_attention_mask (n, 1, 77) of 0 / -10000 and
    another prompt length in every row: the block output on sampled rows against the block's own modules in float64 with the
    mask added to the attn2 scores, 2e-3 (fp16) / 8e-3 (bf16) of the output scale; exactly one _lib.attention_kv_bias call
    per block forward and no _lib.attention_kv call over the 77 keys; the oracle without the mask misses.  ``blas``: the
    library-GEMM dispatch (VIDTOME_FF=blas) reaches the wrapper too.  At the parent commit the mask sent attn2 to the
    module, whose forward raises."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    from vidtome_amd.utils import join_frame
    if mode == "blas":
        monkeypatch.setattr(vpatch, "FF_MODE", "blas")
    unet = _OneBlock(C, 8).to(device=DEV, dtype=dtype)
    plans = _capture_plans(monkeypatch)
    seen = _spies(monkeypatch, L)
    _patch(unet, B, LATENT)
    torch.manual_seed(123)
    blk = unet.blocks[0]
    mask = _prompt_mask(dtype)
    g = np.random.default_rng(0)
    with torch.no_grad():
        for ck in range(2):
            unet._tome_info["args"]["global_rand"] = [0.5, 0.0][ck]
            h, cond = _inputs(C, dtype, ck)
            seen["bias"], seen["kv_keys"] = 0, []
            out = blk(h, encoder_hidden_states=cond, encoder_attention_mask=mask)
            assert seen["bias"] == 1 and COND not in seen["kv_keys"], seen
    plan = plans[id(blk)]
    Lj = plan.L
    idx = np.unique(np.concatenate([np.arange(8), np.arange(Lj - 8, Lj), g.integers(0, Lj, 160)]))
    ref = _masked_oracle_rows(blk, plan, h, cond, mask, idx)
    got = join_frame(out, FRAMES).double().cpu()[:, idx]
    osc = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max()) / osc
    drop = float((got - _masked_oracle_rows(blk, plan, h, cond, None, idx)).abs().max()) / osc
    print(f"masked block C={C} {dtype} {mode} err/scale={err:.3e} (without the mask {drop:.3e})")
    assert err < BLOCK_TOL[dtype], (C, err)
    assert drop > 2 * BLOCK_TOL[dtype], "the mask is not noise"
    vidtome_amd.remove_patch(unet)


@pytest.mark.parametrize("case", ["bool", "per-query", "ada"])
def test_other_mask_forms_keep_the_module_path(L, case, monkeypatch):
    """A bool mask, a per-query mask (n, N, 77), and the published form on an AdaLayerNorm block, on a block whose attn2 is a
    counting torch implementation: the module is called once per forward, the new wrapper never, nothing raises."""
    import vidtome_amd
    C, dtype = 320, torch.float16
    unet = _OneBlock(C, 8, computing=True).to(device=DEV, dtype=dtype)
    seen = _spies(monkeypatch, L)
    _patch(unet, B, LATENT)
    torch.manual_seed(123)
    blk = unet.blocks[0]
    h, cond = _inputs(C, dtype, 0)
    mask = _prompt_mask(dtype)
    kw = {}
    if case == "bool":
        mask = mask == 0
    elif case == "per-query":
        mask = mask.expand(-1, h.shape[1], -1).contiguous()
    else:
        blk.use_ada_layer_norm = True
        blk.norm1, blk.norm2 = _AdaNorm(blk.norm1), _AdaNorm(blk.norm2)
        kw = {"timestep": torch.zeros(B * FRAMES, dtype=torch.long, device=DEV)}
    with torch.no_grad():
        out = blk(h, encoder_hidden_states=cond, encoder_attention_mask=mask, **kw)
    assert bool(torch.isfinite(out).all())
    assert blk.attn2.calls == 1 and seen["bias"] == 0 and COND not in seen["kv_keys"], (case, seen)
    vidtome_amd.remove_patch(unet)
