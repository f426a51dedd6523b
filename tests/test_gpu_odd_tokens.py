"""GPU tests of frames whose token count per sample is no multiple of 8 (run with -m gpu on an MI355X): attn2's fused segment
and the un-merged attn1 segment at N = 12, 20, 100 (N % 8 = 4), 405 (5) and 1590 (6).

DESIGN.md 4.4 records what the kernels need: every attention core addresses query, key and output rows as (sample * rows +
row) * ld with ld % 8 == 0, the panel GEMM's row epilogue and vtm_to_panels address rows the same way, so all of them take a
DENSE (B, N, C) tensor at any N; only V^T needs a padded row (ldvt = N rounded up to 8), which vtm_transpose_cols writes,
zeros in the key columns past N.  So no segmented (pitch Np) form of vtm_linear_panels / vtm_to_panels was built, and the
bit-for-bit check the issue asks of those exports is asked here of what the routing relies on instead: the dense layout with
sample starts on unaligned rows against the same rows laid out with every sample on a pitch of Np rows (the layout of
the N % 8 == 0 path), through the panel GEMM, through vtm_to_panels and through every attention core.

B = 3 samples of different data everywhere, so a wrong sample start shows in samples 1 and 2.  Tolerances of the float64
checks: the project's stated figures, 1e-3 of the output scale in fp16 and 8e-3 in bf16; the
routing test: the whole block's 2e-3 (fp16) / 8e-3 (bf16)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import standin

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}
BLOCK_TOL = {torch.float16: 2e-3, torch.bfloat16: 8e-3}
DTYPES = (torch.float16, torch.bfloat16)
B, COND, COND_DIM = 3, 77, 768
SENTINEL = 5.0
# (C, heads, N): d = 40 / 80 / 64 / 160; N % 8 = 4, 5, 6; one and several 256-row GEMM tiles, one and several key tiles
SHAPES = [(320, 8, 12), (320, 8, 100), (640, 8, 20), (640, 10, 405), (640, 8, 1590), (1280, 8, 405)]
IDS = [f"C{c}-h{h}-N{n}" for c, h, n in SHAPES]


def _np(N):
    return (N + 7) // 8 * 8


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rand(shape, dtype, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _pitched(x, N, fill):
    """(B, N, ...) -> (B, Np, ...) with rows N .. Np - 1 of every sample holding ``fill``."""
    out = torch.full((x.shape[0], _np(N)) + tuple(x.shape[2:]), fill, dtype=x.dtype, device=x.device)
    out[:, :N] = x
    return out


# ---------------------------------------------------------------------------------------------------
# 1. dense rows at unaligned sample starts against the pitch-Np layout, bit for bit; stores outside the rows
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,heads,N", SHAPES, ids=IDS)
def test_panel_gemm_rows_do_not_depend_on_where_they_are_stored(L, C, heads, N, dtype):
    """vtm_to_panels + vtm_linear_panels (bias, with and without the residual) on the dense B * N rows and on the rows on a
    pitch of Np (NaN in the rows between the samples): every logical row bit-equal -- a row's accumulation order does not
    depend on its position -- and the panels are the rows' own 8-channel groups.  The dense output sits inside a
    sentinel-filled buffer with 8 guard rows behind it: the whole buffer is compared, so a store past row B * N is seen."""
    x = _rand((B, N, C), dtype, 11).to(DEV)
    w = _rand((C, C), dtype, 12, C ** -0.5).to(DEV)
    bias = _rand((C,), torch.float32, 13).to(DEV)
    resid = _rand((B, N, C), dtype, 14).to(DEV)
    n, Np = B * N, _np(N)
    wp = L.to_panels(w)
    xp = L.to_panels(x.view(n, C))
    rows_pad = xp.shape[1]
    assert tuple(xp.shape) == (C // 8, L.panel_rows(n), 8)
    assert torch.equal(xp[:, :n], x.view(n, C // 8, 8).transpose(0, 1))
    assert not bool(xp[:, n:].any()), "panel rows past n must be zero"
    xq = L.to_panels(_pitched(x, N, float("nan")).view(B * Np, C))
    assert rows_pad % 256 == 0
    for r in (None, resid):
        buf = torch.full((n + 8, C), SENTINEL, dtype=dtype, device=DEV)
        L.linear_panels(xp, n, wp, C, bias, resid=None if r is None else r.view(n, C), out=buf[:n])
        rp = None if r is None else _pitched(r, N, 0.0).view(B * Np, C)
        pitched = L.linear_panels(xq, B * Np, wp, C, bias, resid=rp).view(B, Np, C)
        torch.cuda.synchronize()
        assert bool((buf[n:] == SENTINEL).all()), "a store past the last row"
        assert torch.equal(buf[:n].view(B, N, C), pitched[:, :N])
        assert bool(torch.isfinite(buf[:n].float()).all())


def _raw_kv(L, q, Mqp, k, Mkp, vt, out, heads, Mq, Mk, bias=None):
    """vtm_attention_kv (or _bias) through the C ABI on caller-owned buffers; q / k may be row ranges of wider rows."""
    C = vt.shape[1]
    d = C // heads
    if bias is None:
        ws, nb = L._attention_ws(q.shape[0], heads, Mq, Mk, d, q.device)
        rc = L.lib().vtm_attention_kv(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), vt.data_ptr(), vt.stride(1),
                                      out.data_ptr(), C, L.dtype_code(q), q.shape[0], heads, Mq, Mqp, Mk, Mkp, d, d ** -0.5, 1,
                                      None if ws is None else ws.data_ptr(), nb, _stream())
    else:
        rc = L.lib().vtm_attention_kv_bias(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), vt.data_ptr(), vt.stride(1),
                                           out.data_ptr(), C, L.dtype_code(q), q.shape[0], heads, Mq, Mqp, Mk, Mkp, d, d ** -0.5,
                                           bias.data_ptr(), bias.shape[1], bias.stride(0), _stream())
    assert rc == 0, L.lib().vtm_last_error()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,heads,N", SHAPES, ids=IDS)
def test_cross_core_takes_dense_queries(L, C, heads, N, dtype):
    """attn2's cores (vtm_attention_kv and vtm_attention_kv_bias, 77 keys) with Mqp = N on dense (B, N, C) queries against
    Mqp = Np with NaN in the query rows N .. Np - 1: rows < N bit-equal; the dense output has 8 sentinel guard rows behind it
    and the pitched output keeps its sentinel in rows N .. Np - 1 (whole buffers are compared)."""
    Np, Mk, Mkp = _np(N), COND, _np(COND)
    q = _rand((B, N, C), dtype, 21).to(DEV)
    k = _pitched(_rand((B, Mk, C), dtype, 22), Mk, float("nan")).to(DEV)
    vt = _pitched(_rand((B, Mk, C), dtype, 23), Mk, float("nan")).transpose(1, 2).contiguous().to(DEV)
    bias = torch.zeros(B, Mk)
    bias[:, 50:] = -10000.0
    bias[0, 60:] = 0.0
    bias[:, 7] = float("-inf")
    for bd in (None, bias.to(DEV)):
        dense = torch.full((B * N + 8, C), SENTINEL, dtype=dtype, device=DEV)
        _raw_kv(L, q, N, k, Mkp, vt, dense, heads, N, Mk, bd)
        pitched = torch.full((B, Np, C), SENTINEL, dtype=dtype, device=DEV)
        _raw_kv(L, _pitched(q, N, float("nan")), Np, k, Mkp, vt, pitched, heads, N, Mk, bd)
        assert bool((dense[B * N:] == SENTINEL).all()) and bool((pitched[:, N:] == SENTINEL).all())
        got = dense[:B * N].view(B, N, C)
        assert bool(torch.isfinite(got.float()).all())
        assert torch.equal(got, pitched[:, :N])
        # the wrapper makes the same launch on a dense (B, N, C) tensor
        wrapped = (L.attention_kv(q, k, vt, heads, N, Mk, (C // heads) ** -0.5) if bd is None
                   else L.attention_kv_bias(q, k, vt, heads, N, Mk, (C // heads) ** -0.5, bd))
        assert tuple(wrapped.shape) == (B, N, C) and torch.equal(wrapped, got)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,heads,N", SHAPES, ids=IDS)
def test_self_core_and_transpose_cols_at_an_odd_key_count(L, C, heads, N, dtype):
    """The un-merged attn1 operands: q | k | v as column ranges of a dense (B, N, 3C) projection, V^T from vtm_transpose_cols
    into a sentinel-filled (B, C, Np) buffer -- the V columns transposed, zeros in the key columns N .. Np - 1, nothing else
    written.  vtm_attention with M = Mp = N on them against M = N, Mp = Np on pitched q / k whose rows N .. Np - 1 hold NaN and
    a V^T whose columns N .. Np - 1 hold NaN: rows < N finite and bit-equal to the run with zeros there and to the dense run."""
    Np, d = _np(N), C // heads
    qkv = _rand((B, N, 3 * C), dtype, 31).to(DEV)
    vt = torch.full((B, C, Np), SENTINEL, dtype=dtype, device=DEV)
    rc = L.lib().vtm_transpose_cols(qkv.data_ptr() + 2 * C * qkv.element_size(), 3 * C, L.dtype_code(qkv), B, N, C,
                                    vt.data_ptr(), Np, _stream())
    assert rc == 0, L.lib().vtm_last_error()
    torch.cuda.synchronize()
    want = torch.zeros((B, C, Np), dtype=dtype, device=DEV)
    want[:, :, :N] = qkv[:, :, 2 * C:].transpose(1, 2)
    assert torch.equal(vt, want)
    assert torch.equal(L.transpose_cols(qkv, 2 * C, C), want)

    def run(q, k, vt_, Mp):
        out = torch.full((B * Mp + 8, C), SENTINEL, dtype=dtype, device=DEV)
        ws, nb = L._attention_ws(B, heads, N, N, d, q.device)
        rc = L.lib().vtm_attention(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), vt_.data_ptr(), vt_.stride(1),
                                   out.data_ptr(), C, L.dtype_code(q), B, heads, N, Mp, d, d ** -0.5, 1,
                                   None if ws is None else ws.data_ptr(), nb, _stream())
        assert rc == 0, L.lib().vtm_last_error()
        torch.cuda.synchronize()
        assert bool((out[B * Mp:] == SENTINEL).all())
        out = out[:B * Mp].view(B, Mp, C)
        assert bool((out[:, N:] == SENTINEL).all())
        return out[:, :N]
    dense = run(qkv[:, :, :C], qkv[:, :, C:2 * C], vt, N)
    assert bool(torch.isfinite(dense.float()).all())
    res = {}
    for fill in (0.0, float("nan")):
        qk = _pitched(qkv[:, :, :2 * C].contiguous(), N, fill)
        vtf = vt.clone()
        vtf[:, :, N:] = fill
        res[fill != 0.0] = run(qk[:, :, :C], qk[:, :, C:], vtf, Np)
    assert bool(torch.isfinite(res[True].float()).all())
    assert torch.equal(res[True], res[False]) and torch.equal(res[False], dense)


# ---------------------------------------------------------------------------------------------------
# 2. the segments against float64
# ---------------------------------------------------------------------------------------------------
class _Block(standin.ModelMixin):
    """One full stand-in block (attn1 / attn2 module forwards raise) with non-trivial norms and biases."""

    def __init__(self, C, heads, seed=0):
        super().__init__()
        self.blocks = torch.nn.ModuleList([standin.BasicTransformerBlock(C, heads, True, COND_DIM)])
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if p.ndim == 2:
                    p.copy_(torch.randn(p.shape, generator=g) * p.shape[-1] ** -0.5)
                else:                                    # LayerNorm weights around 1, every bias around 0
                    p.copy_(torch.randn(p.shape, generator=g) * 0.1 + (1.0 if name.endswith("weight") else 0.0))

    def set_size(self, latent_hw):
        self._tome_info["size"] = latent_hw


@functools.lru_cache(maxsize=None)
def _case(C, heads, N, dtype):
    """Block, tokens, conditioning and mask of one shape (built once, shared by the tests and left unchanged)."""
    blk = _Block(C, heads).to(device=DEV, dtype=dtype).blocks[0]
    h = _rand((B, N, C), dtype, 41).to(DEV)
    enc = _rand((B, COND, COND_DIM), dtype, 42).to(DEV)
    lengths = torch.tensor([40, 77, 55])
    keep = torch.arange(COND)[None, :] < lengths[:, None]
    mask = ((1 - keep.to(dtype)) * -10000.0).unsqueeze(1)
    mask[:, 0, 9] = float("-inf")
    return blk, h, enc, mask.to(DEV)


def _f64(dtype):
    """The float64 restatement's tools: every operand as the device holds it, every intermediate rounded where the module
    path rounds it (a 16-bit tensor between two modules)."""
    rd = lambda t: t.to(dtype).double()
    w = lambda m: m.weight.detach().double().cpu()
    lin = lambda m, x: rd(x @ w(m).T + (0 if m.bias is None else m.bias.detach().double().cpu()))
    ln = lambda n, x: rd(F.layer_norm(x, x.shape[-1:], n.weight.double().cpu(), n.bias.double().cpu(), n.eps))
    return rd, lin, ln


def _att64(a, q, k, v, add=None):
    sh = lambda t: t.view(t.shape[0], t.shape[1], a.heads, -1).transpose(1, 2)
    s = sh(q) @ sh(k).transpose(-1, -2) * a.scale
    if add is not None:
        s = s + add[:, None]
    return (torch.softmax(s, dim=-1) @ sh(v)).transpose(1, 2).reshape(q.shape)


@functools.lru_cache(maxsize=None)
def _cross_ref(C, heads, N, dtype, masked):
    blk, h, enc, mask = _case(C, heads, N, dtype)
    rd, lin, ln = _f64(dtype)
    a, x, c = blk.attn2, h.double().cpu(), enc.double().cpu()
    o = rd(_att64(a, lin(a.to_q, ln(blk.norm2, x)), lin(a.to_k, c), lin(a.to_v, c), mask.double().cpu() if masked else None))
    return lin(a.to_out[0], o) + x


@functools.lru_cache(maxsize=None)
def _self_ref(C, heads, N, dtype):
    blk, h, _, _ = _case(C, heads, N, dtype)
    rd, lin, ln = _f64(dtype)
    a, x = blk.attn1, h.double().cpu()
    x1 = ln(blk.norm1, x)
    return lin(a.to_out[0], rd(_att64(a, lin(a.to_q, x1), lin(a.to_k, x1), lin(a.to_v, x1)))) + x


def _ratio(got, ref):
    g, ref = got.detach().double().cpu(), ref.detach()
    assert bool(torch.isfinite(g).all())
    return float((g - ref).abs().max()) / max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,heads,N", SHAPES, ids=IDS)
def test_cross_segment_vs_float64(L, C, heads, N, dtype, masked):
    """``attn2(norm2(h), enc) + h`` through norm_cross_attention_residual at an odd N, plain and with a per-key mask of
    0 / -10000 (another prompt length per sample) and one -inf key: within 1e-3 (fp16) / 8e-3 (bf16) of the output scale of
    the float64 restatement.  The same segment on tokens extended to Np rows per sample -- the N % 8 == 0 path of the parent
    commit -- gives the same bits in the rows < N (queries are independent)."""
    from vidtome_amd import patch as vpatch
    blk, h, enc, mask = _case(C, heads, N, dtype)
    m = mask if masked else None
    assert vpatch.fused_cross_ok(blk.norm2, blk.attn2, h, enc, m, {})
    with torch.no_grad():
        got = vpatch.norm_cross_attention_residual(blk.norm2, blk.attn2, h, enc, attention_mask=m)
        ext = _pitched(h, N, 0.0)
        ext[:, N:] = _rand((B, _np(N) - N, C), dtype, 43).to(DEV)
        wide = vpatch.norm_cross_attention_residual(blk.norm2, blk.attn2, ext, enc, attention_mask=m)
    assert tuple(got.shape) == (B, N, C)
    err = _ratio(got, _cross_ref(C, heads, N, dtype, masked))
    print(f"odd-N attn2 segment C={C} d={C // heads} N={N} {dtype} masked={masked} err/scale={err:.3e}")
    assert err < TOL[dtype], err
    assert torch.equal(got, wide[:, :N])
    if masked:      # the mask is not noise
        assert _ratio(got, _cross_ref(C, heads, N, dtype, False)) > 2 * TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,heads,N", SHAPES, ids=IDS)
def test_unmerged_self_segment_vs_float64(L, C, heads, N, dtype):
    """``attn1(norm1(h)) + h`` per frame through unmerged_self_attention_residual at an odd N: within 1e-3 (fp16) / 8e-3
    (bf16) of the output scale of the float64 restatement (extra rows would be keys here: the reference alone decides)."""
    from vidtome_amd import patch as vpatch
    blk, h, _, _ = _case(C, heads, N, dtype)
    with torch.no_grad():
        got = vpatch.unmerged_self_attention_residual(blk, h)
    assert tuple(got.shape) == (B, N, C)
    err = _ratio(got, _self_ref(C, heads, N, dtype))
    print(f"odd-N un-merged attn1 segment C={C} d={C // heads} N={N} {dtype} err/scale={err:.3e}")
    assert err < TOL[dtype], err


# ---------------------------------------------------------------------------------------------------
# 3. routing: a patched UNet at 480 x 848 (latent 60 x 106)
# ---------------------------------------------------------------------------------------------------
BATCH, FRAMES, LATENT = 2, 4, (60, 106)
SITES = {"un-merged": ("up1.0", 4, 1280, (15, 27)), "merged": ("up2.0", 2, 640, (30, 53))}


def _run_block(site_key, dtype, monkeypatch, module_path):
    """One forward of one patched full block on seeded inputs -> (output, F.linear input row counts, attention_kv calls,
    linear_panels calls).  ``module_path``: VIDTOME_FF=blas / VIDTOME_PROJ=blas semantics -- the parent commit's routing at
    these sizes (cross_attention(), patched_self_attention_segment over library GEMMs)."""
    import vidtome_amd
    from vidtome_amd import _lib, patch as vpatch, sites as S
    name, ds, C, (gh, gw) = SITES[site_key]
    N = gh * gw
    if module_path:
        monkeypatch.setattr(vpatch, "FF_MODE", "blas")
        monkeypatch.setattr(vpatch, "PROJ_MODE", "blas")
        monkeypatch.setattr(vpatch, "FUSED_PROJ", False)
    seen = {"linear_rows": [], "kv": [], "panels": 0}
    orig_lin, orig_kv, orig_pan = F.linear, _lib.attention_kv, _lib.linear_panels

    def lin(x, *a, **kw):
        seen["linear_rows"].append(x.numel() // x.shape[-1])
        return orig_lin(x, *a, **kw)

    def kv(q, k, vt, heads, Mq, Mk, *a, **kw):
        seen["kv"].append((tuple(q.shape), Mq, Mk))
        return orig_kv(q, k, vt, heads, Mq, Mk, *a, **kw)

    def pan(*a, **kw):
        seen["panels"] += 1
        return orig_pan(*a, **kw)
    monkeypatch.setattr(F, "linear", lin)
    monkeypatch.setattr(_lib, "attention_kv", kv)
    monkeypatch.setattr(_lib, "linear_panels", pan)
    unet = S.SiteUNet([S.Site(name, ds, C, 8)], seed=0, full=True).to(device=DEV, dtype=dtype)
    vidtome_amd.apply_patch(unet, local_merge_ratio=0.5, merge_global=True, global_merge_ratio=0.5, batch_size=BATCH)
    unet.set_size(LATENT)
    torch.manual_seed(123)
    g = torch.Generator().manual_seed(5)
    h = S.regime_tokens("corr01", BATCH, FRAMES, N, C, g).reshape(BATCH * FRAMES, N, C).to(device=DEV, dtype=dtype)
    cond = _rand((BATCH * FRAMES, COND, COND_DIM), dtype, 6).to(DEV)
    with torch.no_grad():
        out = unet.blocks[0](h, encoder_hidden_states=cond)
    torch.cuda.synchronize()
    vidtome_amd.remove_patch(unet)
    monkeypatch.undo()
    return out, seen, N


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("site", sorted(SITES))
def test_patched_block_stays_on_the_panel_path_at_odd_sizes(L, site, dtype, monkeypatch):
    """480 x 848 video, 4 frames, batch 2: the C = 1280 site holds 15 x 27 = 405 tokens per frame and does not merge, the
    C = 640 site 30 x 53 = 1590 and merges.  One block forward issues no F.linear over the B F N (or B F Np) token rows,
    hands vtm_attention_kv the DENSE (B F, N, C) queries with Mq = N over the 77 conditioning keys, runs panel GEMMs, and ends
    within the whole block's bound of the same block on the library-GEMM routing (what these sizes took before)."""
    out, seen, N = _run_block(site, dtype, monkeypatch, module_path=False)
    n, C = BATCH * FRAMES, out.shape[-1]
    assert N % 8 and tuple(out.shape) == (n, N, C)
    token_rows = {n * N, n * _np(N)}
    assert not token_rows & set(seen["linear_rows"]), seen["linear_rows"]
    assert ((n, N, C), N, COND) in seen["kv"], seen["kv"]
    assert seen["panels"] >= (5 if site == "un-merged" else 3), seen
    ref, seen_ref, _ = _run_block(site, dtype, monkeypatch, module_path=True)
    assert token_rows & set(seen_ref["linear_rows"]), "the library-GEMM routing did not run in the reference"
    assert bool(torch.isfinite(out.float()).all())
    err = float((out.double() - ref.double()).abs().max()) / max(1.0, float(ref.double().abs().max()))
    print(f"odd-N patched block {site} N={N} {dtype} vs library-GEMM routing err/scale={err:.3e}")
    assert err < BLOCK_TOL[dtype], err
