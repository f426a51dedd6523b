"""GPU tests of IP-Adapter region masks on the HIP path (run with -m gpu on an MI355X): vtm_attention_kv_sets_masked against
the unmasked kernel (bit for bit where the weights are 0 / 1), against the float64 expression (fractional weights, a table per
sample), its argument checks, and the patched block with ``ip_adapter_masks`` against a float64 oracle of its own modules."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ip_adapter_mask_standin as mstand
from test_gpu_ip_adapter import BLOCK_TOL, TOL, _capture_plans, _operands
from test_gpu_lora import _StandInSites, _cond, _hidden, _oracle_rows, _patch, _site_list

pytestmark = pytest.mark.gpu
DEV = "cuda"
# B = 2 with different data per sample, 2 heads; 300 queries in a buffer of 304 rows: not a multiple of the 32-query wave nor
# of the 256 / 128-query workgroup (a ragged last wave, a partial workgroup).  Text 77, then 4, 4 and 100 keys at 80, 88, 96:
# the 4-key sets on 8-aligned starts with 3e4 padding between them, the 100-key set crosses a 64-key tile.
B, HEADS, MQ = 2, 2, 300
LENS, WEIGHTS = (77, 4, 4, 100), (1.0, 0.6, -0.5, 1.25)
DIMS = [40, 64, 160]                   # 8 waves / DV = 2, 8 waves / DV = 2, 4 waves / DV = 5
DTYPES = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


@functools.lru_cache(maxsize=None)
def _case(d, dtype):
    """Operands on the host and on the device, the sets, and the unmasked result (computed once, never written)."""
    from vidtome_amd import _lib
    q, k, v, sets = _operands(LENS, WEIGHTS, B, MQ, HEADS, d, dtype, seed=7 * d)
    assert q.shape[1] == 304 and [s for s, _, _ in sets] == [0, 80, 88, 96]
    dev = (q.to(DEV), k.to(DEV), v.transpose(1, 2).contiguous().to(DEV))
    plain = _lib.attention_kv_sets(*dev, HEADS, MQ, sets, d ** -0.5)
    return q, k, v, sets, dev, plain


def _raw(L, dev, sets, d, rows, table, ld=None, stride=None, out=None, null_table=False):
    """vtm_attention_kv_sets_masked through the C ABI -> (status, out)."""
    q, k, vt = dev
    n, C = len(sets), q.shape[2]
    out = torch.zeros_like(q) if out is None else out
    ld = (table.shape[-1] if table is not None else MQ) if ld is None else ld
    stride = (table.shape[-2] * table.shape[-1] if table is not None and table.dim() == 3 else 0) if stride is None else stride
    st = L.lib().vtm_attention_kv_sets_masked(
        q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), vt.data_ptr(), vt.stride(1), out.data_ptr(), C, L.dtype_code(q),
        q.shape[0], HEADS, MQ, q.shape[1], k.shape[1], d, d ** -0.5, n, (ctypes.c_int64 * n)(*[s for s, _, _ in sets]),
        (ctypes.c_int64 * n)(*[m for _, m, _ in sets]), (ctypes.c_float * n)(*[w for _, _, w in sets]),
        (ctypes.c_int * n)(*rows), None if table is None or null_table else table.data_ptr(), ld, stride,
        torch.cuda.current_stream().cuda_stream)
    return st, out


def _ref(q, k, v, sets, rows, table, scale):
    """float64: sum_s w_s m_s[b, i] softmax_s(q K_s^T scale) V_s on the same 16-bit operands; table (R, Mqp) or (B, R, Mqp)."""
    Bq, Mqp, C = q.shape
    sh = lambda t: t.double().view(Bq, t.shape[1], HEADS, C // HEADS).transpose(1, 2)
    out = torch.zeros(Bq, HEADS, Mqp, C // HEADS, dtype=torch.float64)
    tab = table.double().cpu()
    for (s, n, w), r in zip(sets, rows):
        p = torch.softmax(sh(q) @ sh(k[:, s:s + n]).transpose(-1, -2) * scale, dim=-1)
        term = w * (p @ sh(v[:, s:s + n]))
        if r >= 0:
            m = tab[r].expand(Bq, Mqp) if tab.dim() == 2 else tab[:, r]
            term = term * m[:, None, :, None]
        out += term
    return out.transpose(1, 2).reshape(Bq, Mqp, C)


def _soft_rectangles(n_tokens, pad_to, boxes, res=64):
    """Rows of the stand-in's bicubic downsample of soft-edged rectangles (ones inside, a half-valued rim, zeros outside) to
    n_tokens tokens, in a table padded with zeros to pad_to columns: fractional values, some below 0 and some above 1."""
    rows = []
    for (y0, y1, x0, x1) in boxes:
        m = torch.zeros(1, res, res)
        m[:, y0 - 1:y1 + 1, x0 - 1:x1 + 1] = 0.5
        m[:, y0:y1, x0:x1] = 1.0
        rows.append(mstand.IPAdapterMaskProcessor.downsample(m, 1, n_tokens, 1).reshape(n_tokens).float())
    t = torch.zeros(len(rows), pad_to)
    t[:, :n_tokens] = torch.stack(rows)
    assert float(t.min()) < -1e-3 and float(t.max()) > 1 + 1e-3 and bool(((t > 0.05) & (t < 0.95)).any())
    return t


# ---------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", DIMS)
def test_no_mask_and_all_ones_are_the_unmasked_kernel_bitwise(L, d, dtype):
    """Every set_mask -1: the bits of vtm_attention_kv_sets (the same kernel).  A table of ones on every adapter set: the same
    bits again -- the fold factor is (w * 1) / l -- through the C ABI and through the wrapper."""
    q, k, v, sets, dev, plain = _case(d, dtype)
    st, got = _raw(L, dev, sets, d, [-1] * 4, None)
    assert st == 0 and torch.equal(got[:, :MQ], plain[:, :MQ])
    ones = torch.ones(3, 304, device=DEV)
    st, got = _raw(L, dev, sets, d, [-1, 0, 1, 2], ones)
    assert st == 0 and torch.equal(got[:, :MQ], plain[:, :MQ])
    assert bool((got[:, MQ:] == 0).all())                        # rows >= Mq are not written
    assert torch.equal(L.attention_kv_sets_masked(*dev, HEADS, MQ, sets, d ** -0.5, [-1, 0, 1, 2], ones), plain)
    assert torch.equal(L.attention_kv_sets_masked(*dev, HEADS, MQ, sets, d ** -0.5, [-1] * 4, None), plain)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", DIMS)
def test_binary_masks_select_sets_per_row_bitwise(L, d, dtype):
    """0 / 1 masks that split the queries between the adapter sets -- set 1 on rows 0-149, set 2 on rows 150-299 (the flip
    sits inside a wave), set 3 on rows 100-199: every output row is, bit for bit, the unmasked launch over exactly the sets
    whose mask is 1 at that row (a weight of 0 adds o * 0 to the fp32 sum)."""
    q, k, v, sets, dev, _ = _case(d, dtype)
    table = torch.zeros(3, 304)
    table[0, :150] = 1
    table[1, 150:300] = 1
    table[2, 100:200] = 1
    got = L.attention_kv_sets_masked(*dev, HEADS, MQ, sets, d ** -0.5, [-1, 0, 1, 2], table.to(DEV))
    assert bool(torch.isfinite(got).all())
    for lo, hi, active in ((0, 100, (1,)), (100, 150, (1, 3)), (150, 200, (2, 3)), (200, 300, (2,))):
        assert all(bool((table[a - 1, lo:hi] == 1).all()) for a in active)
        want = L.attention_kv_sets(*dev, HEADS, MQ, [sets[0]] + [sets[a] for a in active], d ** -0.5)
        assert torch.equal(got[:, lo:hi], want[:, lo:hi]), (lo, hi)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", DIMS)
def test_fractional_masks_vs_float64(L, d, dtype):
    """Weights from the bicubic downsample of soft-edged rectangles (fractional, slightly below 0 and above 1), one table for
    both samples and then a table per sample with different masks: every element within 1e-3 (fp16) / 8e-3 (bf16) of the
    output scale of the float64 expression -- the attention core's figures."""
    q, k, v, sets, dev, _ = _case(d, dtype)
    rows = [-1, 0, 1, 2]
    shared = _soft_rectangles(MQ, 304, [(8, 40, 4, 30), (20, 60, 30, 62), (2, 20, 10, 50)])
    other = _soft_rectangles(MQ, 304, [(30, 62, 2, 40), (4, 24, 6, 28), (40, 60, 20, 60)])
    for what, table in (("shared", shared), ("per sample", torch.stack([shared, other]))):
        ref = _ref(q, k, v, sets, rows, table, d ** -0.5)[:, :MQ]
        got = L.attention_kv_sets_masked(*dev, HEADS, MQ, sets, d ** -0.5, rows, table.to(DEV))[:, :MQ].double().cpu()
        assert bool(torch.isfinite(got).all())
        err = float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))
        print(f"attention_kv_sets_masked d={d} {dtype} {what} table err/scale={err:.3e}")
        assert err < TOL[dtype], (what, err)
    # the two tables differ where it matters: sample 1 of the per-sample call is not sample 1 of the shared one
    a = L.attention_kv_sets_masked(*dev, HEADS, MQ, sets, d ** -0.5, rows, shared.to(DEV))
    b = L.attention_kv_sets_masked(*dev, HEADS, MQ, sets, d ** -0.5, rows, torch.stack([shared, other]).to(DEV))
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])


def test_bad_arguments_are_refused_without_a_launch(L):
    """A row outside the table's range, a masked set without a table, rows shorter than Mq, overlapping per-sample tables:
    VTM_EINVAL, nothing launched (out untouched)."""
    d = 40
    q, k, v, sets, dev, _ = _case(d, torch.float16)
    table = torch.ones(3, 304, device=DEV)
    out = torch.full_like(dev[0], 5.0)
    assert _raw(L, dev, sets, d, [-1, 0, 1, 4], table, out=out)[0] == -1            # rows are 0 .. n_sets - 1
    assert b"row" in L.lib().vtm_last_error()
    assert _raw(L, dev, sets, d, [-1, 0, -2, 1], table, out=out)[0] == -1
    assert _raw(L, dev, sets, d, [-1, 0, 1, 2], table, out=out, null_table=True)[0] == -1
    assert b"null" in L.lib().vtm_last_error()
    assert _raw(L, dev, sets, d, [-1, 0, 1, 2], table, ld=MQ - 4, out=out)[0] == -1
    assert b"ld_mask" in L.lib().vtm_last_error()
    assert _raw(L, dev, sets, d, [-1, 0, 1, 2], table, stride=2 * 304, out=out)[0] == -1
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    with pytest.raises(RuntimeError):                            # the wrapper: a row the table does not have, a short table
        L.attention_kv_sets_masked(*dev, HEADS, MQ, sets, d ** -0.5, [-1, 0, 1, 3], table)
    with pytest.raises(RuntimeError):
        L.attention_kv_sets_masked(*dev, HEADS, MQ, sets, d ** -0.5, [-1, 0, 1, 2], table[:, :296].contiguous())
    with pytest.raises(RuntimeError):
        L.attention_kv_sets_masked(*dev, HEADS, MQ, sets, d ** -0.5, [-1, 0, 1, 2], table.double())


# ---------------------------------------------------------------------------------------------------
# 2. the patched block
# ---------------------------------------------------------------------------------------------------
def _masked_oracle_rows(blk, plan, hidden, text, ims, scales, weights, fsize, idx):
    """float64 block output at the joined-chunk positions idx: attn1 from test_gpu_lora._oracle_rows (``plan`` None, the site
    that does not merge: attn1 per frame), then norm2 / the decoupled cross-attention of attn2's own modules with the term
    of adapter a times ``weights[a]`` ((N,) per-token weights, None: everywhere) / norm3 / GEGLU feed-forward."""
    fold = lambda m: (m.weight.detach().double().cpu(), None if m.bias is None else m.bias.detach().double().cpu())
    lin = lambda m, x: x @ fold(m)[0].T + (0 if fold(m)[1] is None else fold(m)[1])
    ln = lambda n, x: torch.nn.functional.layer_norm(x, x.shape[-1:], n.weight.double().cpu(), n.bias.double().cpu(), n.eps)
    N = hidden.shape[1]
    pos = torch.as_tensor(idx)
    if plan is not None:
        h = _oracle_rows(blk, plan, hidden, None, fsize, idx, fold, False)
    else:
        a1 = blk.attn1
        X = hidden.double().cpu().view(-1, fsize, N, hidden.shape[-1])
        sh1 = lambda t: t.view(t.shape[0], a1.heads, -1).transpose(0, 1)
        h = torch.empty(X.shape[0], len(idx), X.shape[-1], dtype=torch.float64)
        for b in range(X.shape[0]):
            for f in (pos // N).unique().tolist():
                sel = (pos // N == f).nonzero().flatten()
                x1 = ln(blk.norm1, X[b, f])
                q, k, v = lin(a1.to_q, x1[pos[sel] % N]), lin(a1.to_k, x1), lin(a1.to_v, x1)
                o = (torch.softmax(sh1(q) @ sh1(k).transpose(-1, -2) * a1.scale, dim=-1) @ sh1(v)).transpose(0, 1)
                h[b, sel] = lin(a1.to_out[0], o.reshape(len(sel), -1)) + X[b, f, pos[sel] % N]
    Bn = h.shape[0]
    per_frame = lambda t: t.double().cpu().reshape(Bn, fsize, -1, t.shape[-1])
    c, im = per_frame(text), [per_frame(t) for t in ims]
    a2, proc = blk.attn2, blk.attn2.processor
    heads, d = a2.heads, h.shape[-1] // a2.heads
    sh = lambda t: t.view(t.shape[0], heads, d).transpose(0, 1)
    att = lambda q, k, v: (torch.softmax(sh(q) @ sh(k).transpose(-1, -2) * a2.scale, dim=-1) @ sh(v)).transpose(0, 1).reshape(
        q.shape[0], -1)
    x2 = ln(blk.norm2, h)
    o2 = torch.empty_like(h)
    for b in range(Bn):
        for f in (pos // N).unique().tolist():
            sel = (pos // N == f).nonzero().flatten()
            q = lin(a2.to_q, x2[b, sel])
            o = att(q, lin(a2.to_k, c[b, f]), lin(a2.to_v, c[b, f]))
            for a, s in enumerate(scales):
                term = s * att(q, lin(proc.to_k_ip[a], im[a][b, f]), lin(proc.to_v_ip[a], im[a][b, f]))
                o = o + (term if weights[a] is None else term * weights[a].double()[pos[sel] % N, None])
            o2[b, sel] = o
    h2 = lin(a2.to_out[0], o2) + h
    p = lin(blk.ff.net[0].proj, ln(blk.norm3, h2))
    D = p.shape[-1] // 2
    return lin(blk.ff.net[2], p[..., :D] * torch.nn.functional.gelu(p[..., D:])) + h2


@pytest.mark.parametrize("case,dtype", [("both masked", torch.float16), ("both masked", torch.bfloat16),
                                        ("one entry None", torch.float16), ("blas", torch.float16)])
def test_masked_ip_adapter_block_vs_float64_oracle(L, case, dtype, monkeypatch):
    """Stand-in sites (the module forward of attn1 raises) -- the merged top and mid sites and the site that does not merge
    -- latent 32 x 32, B = 2, F = 4, two chunks, two adapters of (16, 4) tokens and scales (1.0, 0.6), one image each with a
    half-frame mask: the first the left half at the latent's resolution, the second the top half as (1, 1, 64, 64), so that
    the downsample resamples at every site.  Sampled rows against the block's own modules in float64 on the same merge plan
    within 2e-3 (fp16) / 8e-3 (bf16) of the output scale; one vtm_attention_kv_sets_masked launch per site per forward and no
    call of the processor; the oracle without the masks is more than twice the tolerance away (on the masked-out rows a whole
    adapter term is gone).  ``one entry None``: the first adapter unmasked.  ``blas``: the VIDTOME_FF=blas dispatch."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    from vidtome_amd import sites as S
    from vidtome_amd.utils import join_frame
    sl = _site_list("up3.0", "up2.0", "up1.0")
    Bv, F, latent = 2, 4, (32, 32)
    num_tokens, scales = (16, 4), (1.0, 0.6)
    unet = _StandInSites(sl, True).to(device=DEV, dtype=dtype)
    procs = mstand.install(unet, num_tokens, scales)
    if case == "blas":
        monkeypatch.setattr(vpatch, "FF_MODE", "blas")
    seen = _capture_plans(monkeypatch)
    calls, orig = [], L.attention_kv_sets_masked
    monkeypatch.setattr(L, "attention_kv_sets_masked", lambda *a, **kw: (calls.append((a[5], a[7])), orig(*a, **kw))[1])
    _patch(unet, Bv, latent)
    text = _cond(Bv, F, dtype)
    g = torch.Generator().manual_seed(5)
    ims = [torch.randn(Bv * F, 1, t, 768, generator=g).to(device=DEV, dtype=dtype) for t in num_tokens]
    left = torch.zeros(1, 1, 32, 32, device=DEV)
    left[..., :16] = 1
    top = torch.zeros(1, 1, 64, 64, device=DEV)
    top[:, :, :32] = 1
    masks = [None if case == "one entry None" else left, top]
    kw = {"ip_adapter_masks": masks}
    rng = np.random.default_rng(0)
    tol = BLOCK_TOL[dtype]
    with torch.no_grad():
        for ck in range(2):
            unet._tome_info["args"]["global_rand"] = [0.5, 0.0][ck]
            hs = _hidden(sl, Bv, F, latent, dtype, ck, seed0=60)
            calls.clear()
            outs = [blk(h, encoder_hidden_states=(text, ims), cross_attention_kwargs=kw) for blk, h in zip(unet.blocks, hs)]
            n_sets = 3
            assert len(calls) == len(sl) and all(len(s) == n_sets for s, _ in calls), calls
            assert all(r == ([-1, -1, 0] if masks[0] is None else [-1, 0, 1]) for _, r in calls), calls
            if ck != 1:
                continue
            for blk, h, o in zip(unet.blocks, hs, outs):
                plan = seen.get(id(blk))                           # (None at the site that does not merge: attn1 per frame)
                N = h.shape[1]
                Lj = F * N if plan is None else plan.L
                idx = np.unique(np.concatenate([np.arange(8), np.arange(Lj - 8, Lj), rng.integers(0, Lj, 96)]))
                weights = [None if m is None else
                           mstand.IPAdapterMaskProcessor.downsample(m[:, 0].cpu(), 1, N, 1).reshape(N) for m in masks]
                ref = _masked_oracle_rows(blk, plan, h, text, ims, scales, weights, F, idx)
                got = join_frame(o, F).double().cpu()[:, idx]
                osc = max(1.0, float(ref.abs().max()))
                err = float((got - ref).abs().max()) / osc
                print(f"masked ip block [{case}] C={h.shape[-1]} {dtype} err/scale={err:.3e}")
                assert err < tol, (h.shape[-1], err)
                drop = _masked_oracle_rows(blk, plan, h, text, ims, scales, [None, None], F, idx)
                assert float((got - drop).abs().max()) / osc > 2 * tol, "the masks are not noise"
    assert all(p.calls == 0 for p in procs)
    vidtome_amd.remove_patch(unet)
