"""GPU tests of IP-Adapter cross-attention on the HIP path (run with -m gpu on an MI355X): vtm_attention_kv_sets against the
float64 expression, the one-set call against vtm_attention_kv, the patched block with an IP-Adapter processor against a
float64 oracle of its own modules, where it ran (fused path / module path), and adapter-state changes."""
import ctypes

import numpy as np
import pytest
import torch

from ip_adapter_standin import image_states, install
from lora_standin import SDPAAttention
from test_gpu_lora import CFG2, _StandInSites, _cond, _hidden, _oracle_rows, _patch, _site_list

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}            # the attention core's figures
BLOCK_TOL = {torch.float16: 2e-3, torch.bfloat16: 8e-3}      # the whole block's


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


# ---------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------
LAYOUTS = [((77, 4), (1.0, 0.6)), ((77, 16), (1.0, -0.5)), ((77, 257), (1.0, 1.5)), ((154, 4, 16), (1.0, 0.7, 0.3)),
           ((77, 4, 16, 257), (0.8, -0.4, 1.25, 2.0))]


def _operands(lens, weights, B, Mq, heads, d, dtype, seed, pad_value=3.0e4):
    """q (B, Mq8, C), k (B, Mkp, C), vt (B, C, Mkp) with set s at the next multiple of 8 keys; the padding keys between the
    sets hold large finite values.  Different data per sample."""
    g = torch.Generator().manual_seed(seed)
    C = heads * d
    sets, end = [], 0
    for n, w in zip(lens, weights):
        sets.append((end, n, w))
        end = (end + n + 7) // 8 * 8
    Mqp = (Mq + 7) // 8 * 8
    q = torch.randn(B, Mqp, C, generator=g).to(dtype)
    k = torch.full((B, end, C), pad_value).to(dtype)
    v = torch.full((B, end, C), pad_value).to(dtype)
    for s, n, _ in sets:
        k[:, s:s + n] = torch.randn(B, n, C, generator=g).to(dtype)
        v[:, s:s + n] = torch.randn(B, n, C, generator=g).to(dtype)
    return q, k, v, sets


def _ref_sets(q, k, v, sets, heads, scale):
    """The float64 expression on the same 16-bit operands."""
    B, Mqp, C = q.shape
    sh = lambda t: t.double().view(B, t.shape[1], heads, C // heads).transpose(1, 2)
    out = torch.zeros(B, heads, Mqp, C // heads, dtype=torch.float64)
    for s, n, w in sets:
        p = torch.softmax(sh(q) @ sh(k[:, s:s + n]).transpose(-1, -2) * scale, dim=-1)
        out += w * (p @ sh(v[:, s:s + n]))
    return out.transpose(1, 2).reshape(B, Mqp, C)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("d", [40, 64, 80, 160])
def test_kernel_vs_float64(L, d, dtype):
    """sum_s w_s softmax_s(q K_s^T scale) V_s for every layout, negative weights and weights above 1, Mq not a multiple of the
    query block, B = 2 with different data per sample: every element within 1e-3 (fp16) / 8e-3 (bf16) of the output scale;
    the padding keys between the sets are large and finite; a second call gives the same bits."""
    heads, B, Mq = 2, 2, 1001              # (not a multiple of the query block, nor of 8: the buffers hold 1008 rows)
    scale = d ** -0.5
    worst = 0.0
    for i, (lens, weights) in enumerate(LAYOUTS):
        q, k, v, sets = _operands(lens, weights, B, Mq, heads, d, dtype, seed=100 * d + i)
        ref = _ref_sets(q, k, v, sets, heads, scale)[:, :Mq]
        qd, kd, vtd = q.to(DEV), k.to(DEV), v.transpose(1, 2).contiguous().to(DEV)
        got = L.attention_kv_sets(qd, kd, vtd, heads, Mq, sets, scale)
        again = L.attention_kv_sets(qd, kd, vtd, heads, Mq, sets, scale)
        assert torch.equal(got, again)
        got = got[:, :Mq].double().cpu()
        assert bool(torch.isfinite(got).all()), (lens, "padding keys were read")
        osc = max(1.0, float(ref.abs().max()))
        err = float((got - ref).abs().max()) / osc
        worst = max(worst, err)
        print(f"attention_kv_sets d={d} {dtype} sets={lens} err/scale={err:.3e}")
        assert err < TOL[dtype], (lens, err)
    print(f"attention_kv_sets d={d} {dtype} worst err/scale={worst:.3e}")


def test_kernel_uses_strided_views_and_other_head_dims(L):
    """q as a column window of a wider buffer (row stride 2C), heads = 8 at d = 40 (SD-1.5's top block), and d = 8 .. 128."""
    for d, heads in ((40, 8), (8, 2), (16, 2), (32, 2), (96, 2), (128, 2)):
        B, Mq, dtype = 2, 300, torch.float16
        q, k, v, sets = _operands((77, 16), (1.0, 0.5), B, Mq, heads, d, dtype, seed=d)
        ref = _ref_sets(q, k, v, sets, heads, d ** -0.5)[:, :Mq]
        wide = torch.cat([q, torch.full_like(q, 7.0)], dim=2).to(DEV)
        got = L.attention_kv_sets(wide[:, :, :heads * d], k.to(DEV), v.transpose(1, 2).contiguous().to(DEV), heads, Mq, sets,
                                  d ** -0.5)[:, :Mq].double().cpu()
        assert float((got - ref).abs().max()) < 1e-3 * max(1.0, float(ref.abs().max())), d


def test_kernel_rejects_bad_arguments(L):
    """n_sets 0 or 9, a misaligned start, an end beyond Mkp, fp32 operands: an error code, nothing launched (out untouched)."""
    lib, s = L.lib(), torch.cuda.current_stream().cuda_stream
    B, Mq, heads, d = 1, 64, 2, 40
    C = heads * d
    for dtype in (torch.float16, torch.float32):
        q = torch.zeros(B, Mq, C, dtype=dtype, device=DEV)
        k = torch.zeros(B, 96, C, dtype=dtype, device=DEV)
        vt = torch.zeros(B, C, 96, dtype=dtype, device=DEV)
        out = torch.full((B, Mq, C), 5.0, dtype=dtype, device=DEV)

        def call(starts, lens, ws, n=None):
            n = len(starts) if n is None else n
            m = max(len(starts), 1)
            return lib.vtm_attention_kv_sets(q.data_ptr(), C, k.data_ptr(), C, vt.data_ptr(), 96, out.data_ptr(), C,
                                             L.dtype_code(q), B, heads, Mq, Mq, 96, d, d ** -0.5, n,
                                             (ctypes.c_int64 * m)(*starts), (ctypes.c_int64 * m)(*lens),
                                             (ctypes.c_float * m)(*ws), s)
        if dtype == torch.float32:
            assert call([0, 80], [77, 4], [1.0, 0.5]) == -1
            assert b"fp32" in lib.vtm_last_error()
        else:
            assert call([0], [77], [1.0], n=0) == -1
            assert call([0] * 9, [8] * 9, [1.0] * 9) == -1
            assert call([0, 78], [77, 4], [1.0, 0.5]) == -1          # misaligned start
            assert call([0, 80], [77, 17], [1.0, 0.5]) == -1         # the end lies beyond Mkp = 96
            assert call([0, 80], [77, 0], [1.0, 0.5]) == -1          # an empty set
            assert call([0, 80], [77, 4], [1.0, float("nan")]) == -1
        torch.cuda.synchronize()
        assert bool((out == 5.0).all())
    with pytest.raises(RuntimeError):
        L.attention_kv_sets(q, k, vt, heads, Mq, [(0, 77, 1.0), (80, 4, 0.5)], d ** -0.5)     # fp32 through the wrapper
    with pytest.raises(RuntimeError):
        L.attention_kv_sets(q.half(), k.half(), vt.half(), heads, Mq, [], d ** -0.5)


# ---------------------------------------------------------------------------------------------------
# 2. one set of weight 1 is attention_kv
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_one_set_of_weight_one_is_attention_kv_bitwise(L, dtype, monkeypatch):
    for d in (40, 80):
        q, k, v, sets = _operands((77, 16), (1.0, 0.5), 2, 520, 8, d, dtype, seed=d)
        qd, kd, vtd = q.to(DEV), k.to(DEV), v.transpose(1, 2).contiguous().to(DEV)
        want = L.attention_kv(qd, kd, vtd, 8, 520, 77, d ** -0.5)
        seen = []
        orig = L.attention_kv
        monkeypatch.setattr(L, "attention_kv", lambda *a, **kw: (seen.append(1), orig(*a, **kw))[1])
        got = L.attention_kv_sets(qd, kd, vtd, 8, 520, [(0, 77, 1.0)], d ** -0.5)
        monkeypatch.setattr(L, "attention_kv", orig)
        assert seen == [1] and torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------
# helpers of the whole-block tests
# ---------------------------------------------------------------------------------------------------
def _conditioning(num_tokens, B, F, dtype, legacy, images=1, seed=5):
    text = _cond(B, F, dtype)
    ims = image_states(num_tokens, B * F, 768, dtype, DEV, seed=seed, images=images)
    return (torch.cat([text, ims[0]], dim=1) if legacy else (text, ims)), text, ims


def _capture_plans(monkeypatch):
    """{id(block): its merge plan of the last forward, None for a block that does not merge}."""
    from vidtome_amd import patch as vpatch
    seen, orig = {}, vpatch.compute_merge

    def rec(module, x, info, **kw):
        res = orig(module, x, info, **kw)
        seen[id(module)] = getattr(res[0], "plan", None)
        return res
    monkeypatch.setattr(vpatch, "compute_merge", rec)
    return seen


def _spy(monkeypatch, L):
    calls = []
    orig = L.attention_kv_sets
    monkeypatch.setattr(L, "attention_kv_sets", lambda *a, **kw: (calls.append(a[5]), orig(*a, **kw))[1])
    return calls


def _ip_oracle_rows(blk, plan, hidden, text, ims, scales, fsize, idx):
    """float64 block output at the joined-chunk positions idx: the segment from test_gpu_lora._oracle_rows (``plan`` None, a
    site that does not merge: attn1 per frame), then norm2 / the decoupled cross-attention of attn2's own modules / norm3 /
    GEGLU feed-forward."""
    fold = lambda m: (m.weight.detach().double().cpu(), None if m.bias is None else m.bias.detach().double().cpu())
    lin = lambda m, x: x @ fold(m)[0].T + (0 if fold(m)[1] is None else fold(m)[1])
    ln = lambda n, x: torch.nn.functional.layer_norm(x, x.shape[-1:], n.weight.double().cpu(), n.bias.double().cpu(), n.eps)
    N = hidden.shape[1]
    if plan is not None:
        h = _oracle_rows(blk, plan, hidden, None, fsize, idx, fold, False)
    else:
        a1 = blk.attn1
        X = hidden.double().cpu().view(-1, fsize, N, hidden.shape[-1])
        sh1 = lambda t: t.view(t.shape[0], a1.heads, -1).transpose(0, 1)
        pos = torch.as_tensor(idx)
        h = torch.empty(X.shape[0], len(idx), X.shape[-1], dtype=torch.float64)
        for b in range(X.shape[0]):
            for f in (pos // N).unique().tolist():
                sel = (pos // N == f).nonzero().flatten()
                x1 = ln(blk.norm1, X[b, f])
                q, k, v = lin(a1.to_q, x1[pos[sel] % N]), lin(a1.to_k, x1), lin(a1.to_v, x1)
                o = (torch.softmax(sh1(q) @ sh1(k).transpose(-1, -2) * a1.scale, dim=-1) @ sh1(v)).transpose(0, 1)
                h[b, sel] = lin(a1.to_out[0], o.reshape(len(sel), -1)) + X[b, f, pos[sel] % N]
    Bn = h.shape[0]
    per_frame = lambda t: t.double().cpu().view(Bn, fsize, -1, t.shape[-1])
    c, im = per_frame(text), [per_frame(t) for t in ims]
    frame = torch.as_tensor(idx) // N
    a2, proc = blk.attn2, blk.attn2.processor
    heads, d = a2.heads, h.shape[-1] // a2.heads
    sh = lambda t: t.view(t.shape[0], heads, d).transpose(0, 1)
    att = lambda q, k, v: (torch.softmax(sh(q) @ sh(k).transpose(-1, -2) * a2.scale, dim=-1) @ sh(v)).transpose(0, 1).reshape(
        q.shape[0], -1)
    x2 = ln(blk.norm2, h)
    o2 = torch.empty_like(h)
    for b in range(Bn):
        for f in frame.unique().tolist():
            sel = (frame == f).nonzero().flatten()
            q = lin(a2.to_q, x2[b, sel])
            o = att(q, lin(a2.to_k, c[b, f]), lin(a2.to_v, c[b, f]))
            for a, s in enumerate(scales):
                if s != 0:
                    o = o + s * att(q, lin(proc.to_k_ip[a], im[a][b, f]), lin(proc.to_v_ip[a], im[a][b, f]))
            o2[b, sel] = o
    h2 = lin(a2.to_out[0], o2) + h
    p = lin(blk.ff.net[0].proj, ln(blk.norm3, h2))
    D = p.shape[-1] // 2
    return lin(blk.ff.net[2], p[..., :D] * torch.nn.functional.gelu(p[..., D:])) + h2


# ---------------------------------------------------------------------------------------------------
# 3. the whole block against float64, and 4a. that it ran on the fused path
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("num_tokens,scales,legacy", [((4,), (0.6,), False), ((4,), (0.6,), True), ((16,), (1.0,), False),
                                                       ((16,), (1.0,), True), ((4, 16), (0.7, 0.3), False)])
def test_ip_adapter_block_vs_float64_oracle(L, dtype, num_tokens, scales, legacy, monkeypatch):
    """Stand-in sites (attn1's module forward raises) at the cfg-2 geometry -- a merged top site, a merged mid site, an
    un-merged site -- with an IP-Adapter processor on attn2, through apply_patch for three chunks: the block output on
    sampled rows against the block's own modules in float64 on the same merge plan, 2e-3 (fp16) / 8e-3 (bf16) of the output
    scale; one vtm_attention_kv_sets launch per block per forward and no call of the processor; the oracle without the
    adapter term misses.  At the parent commit the tuple raised AttributeError in attn2 and the legacy form ran the module."""
    import vidtome_amd
    from vidtome_amd import sites as S
    from vidtome_amd.utils import join_frame
    sl = _site_list("up3.0", "up2.0", "up1.0")
    B, F, latent = CFG2["B"], CFG2["F"], CFG2["latent"]
    unet = _StandInSites(sl, True).to(device=DEV, dtype=dtype)
    procs = install(unet, num_tokens, scales)
    seen = _capture_plans(monkeypatch)
    calls = _spy(monkeypatch, L)
    _patch(unet, B, latent)
    torch.manual_seed(123)
    cond, text, ims = _conditioning(num_tokens, B, F, dtype, legacy)
    g = np.random.default_rng(0)
    tol = BLOCK_TOL[dtype]
    with torch.no_grad():
        for ck in range(3):
            unet._tome_info["args"]["global_rand"] = [0.5, 0.0, 1.0][ck]
            hs = _hidden(sl, B, F, latent, dtype, ck, seed0=60)
            calls.clear()
            outs = S.run_block_pass(unet, hs, cond)
            assert len(calls) == len(sl) and all(len(c) == 1 + len(num_tokens) for c in calls), calls
            if ck != 1:
                continue
            for blk, h, o in zip(unet.blocks, hs, outs):
                plan = seen.get(id(blk))
                assert (plan is None) == (h.shape[-1] == 1280)     # the C = 1280 site does not merge: attn1 per frame
                Lj = F * h.shape[1] if plan is None else plan.L
                idx = np.unique(np.concatenate([np.arange(8), np.arange(Lj - 8, Lj), g.integers(0, Lj, 96)]))
                ref = _ip_oracle_rows(blk, plan, h, text, ims, scales, F, idx)
                got = join_frame(o, F).double().cpu()[:, idx]
                osc = max(1.0, float(ref.abs().max()))
                err = float((got - ref).abs().max()) / osc
                print(f"ip block C={h.shape[-1]} {dtype} tokens={num_tokens} legacy={legacy} err/scale={err:.3e}")
                assert err < tol, (h.shape[-1], err)
                drop = _ip_oracle_rows(blk, plan, h, text, ims, [0.0] * len(scales), F, idx)
                assert float((got - drop).abs().max()) / osc > 2 * tol, "the adapter term is not noise"
    assert all(p.calls == 0 for p in procs)
    vidtome_amd.remove_patch(unet)


def test_unmerged_site_vs_float64_oracle(L, monkeypatch):
    """The un-merged C = 1280 site has no merge plan to take rows from: its block output against float64 on all rows of a
    few frames (attn1 per frame, then the IP-Adapter attn2 and the feed-forward)."""
    import vidtome_amd
    from vidtome_amd import sites as S
    sl = _site_list("up1.0")
    B, F, latent = CFG2["B"], CFG2["F"], CFG2["latent"]
    for dtype in (torch.float16, torch.bfloat16):
        unet = _StandInSites(sl, True).to(device=DEV, dtype=dtype)
        install(unet, (4, 16), (0.7, 0.3))
        _patch(unet, B, latent)
        cond, text, ims = _conditioning((4, 16), B, F, dtype, False)
        hs = _hidden(sl, B, F, latent, dtype, 0, seed0=70)
        with torch.no_grad():
            out = S.run_block_pass(unet, hs, cond)[0]
        blk = unet.blocks[0]
        fold = lambda m: (m.weight.detach().double().cpu(), None if m.bias is None else m.bias.detach().double().cpu())
        lin = lambda m, x: x @ fold(m)[0].T + (0 if fold(m)[1] is None else fold(m)[1])
        ln = lambda n, x: torch.nn.functional.layer_norm(x, x.shape[-1:], n.weight.double().cpu(), n.bias.double().cpu(), n.eps)
        heads = blk.attn1.heads

        def att(a, q, k, v):
            sh = lambda t: t.view(t.shape[0], heads, -1).transpose(0, 1)
            return (torch.softmax(sh(q) @ sh(k).transpose(-1, -2) * a.scale, dim=-1) @ sh(v)).transpose(0, 1).reshape(q.shape[0], -1)
        for fr in (0, F - 1, B * F - 1):
            x = hs[0][fr].double().cpu()
            x1 = ln(blk.norm1, x)
            h = lin(blk.attn1.to_out[0], att(blk.attn1, lin(blk.attn1.to_q, x1), lin(blk.attn1.to_k, x1), lin(blk.attn1.to_v, x1))) + x
            a2, proc = blk.attn2, blk.attn2.processor
            q = lin(a2.to_q, ln(blk.norm2, h))
            c = text[fr].double().cpu()
            o = att(a2, q, lin(a2.to_k, c), lin(a2.to_v, c))
            for a, s in enumerate((0.7, 0.3)):
                i = ims[a][fr].double().cpu()
                o = o + s * att(a2, q, lin(proc.to_k_ip[a], i), lin(proc.to_v_ip[a], i))
            h2 = lin(a2.to_out[0], o) + h
            p = lin(blk.ff.net[0].proj, ln(blk.norm3, h2))
            D = p.shape[-1] // 2
            ref = lin(blk.ff.net[2], p[..., :D] * torch.nn.functional.gelu(p[..., D:])) + h2
            err = float((out[fr].double().cpu() - ref).abs().max()) / max(1.0, float(ref.abs().max()))
            print(f"ip un-merged block {dtype} frame={fr} err/scale={err:.3e}")
            assert err < BLOCK_TOL[dtype], (dtype, fr, err)
        vidtome_amd.remove_patch(unet)


# ---------------------------------------------------------------------------------------------------
# 4b. what keeps the module path, keeps it: no launch of the new core, the processor runs, nothing raises
# ---------------------------------------------------------------------------------------------------
def _computing_sites(sl, dtype, num_tokens, scales, name="IPAdapterAttnProcessor2_0"):
    from vidtome_amd import sites as S
    unet = S.SiteUNet(sl, seed=0, full=True).to(device=DEV, dtype=dtype)
    for blk in unet.blocks:
        blk.attn1 = SDPAAttention(blk.attn1)       # (processor kwargs send attn1 to its module forward too)
    return unet, install(unet, num_tokens, scales, name=name)


@pytest.mark.parametrize("case", ["masks", "list scales", "fp32", "fp32 projections", "unknown name", "blas"])
def test_what_is_not_understood_keeps_the_module_path(L, case, monkeypatch):
    """Masks, per-image scale lists, fp32 models, an unknown processor name: no launch of the new core, the processor is
    called, nothing raises; attn2 through the patched block's dispatch is the module's forward bit for bit, and the whole
    patched block at the site that does not merge equals the block evaluated by its own modules (attn1 and the feed-forward
    run on the library either way: within 2e-3 of the output scale, the project's whole-block figure).  ``blas``: the
    non-panel dispatch recognises the processor too and runs the new core between library GEMMs."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    sl = _site_list("up3.0", "up2.0", "up1.0")
    B, F, latent = 2, 4, (32, 32)
    dtype = torch.float32 if case.startswith("fp32") else torch.float16
    images = 2 if case == "list scales" else 1
    scales = ([0.5, 0.2],) if case == "list scales" else (0.6,)
    unet, procs = _computing_sites(sl, dtype, (4,), (0.6,), "UnknownIPProcessor" if case == "unknown name"
                                   else "IPAdapterAttnProcessor2_0")
    for p in procs:
        p.scale = list(scales)
    if case == "blas":
        monkeypatch.setattr(vpatch, "FF_MODE", "blas")
    calls = _spy(monkeypatch, L)
    _patch(unet, B, latent)
    if case == "fp32 projections":
        vidtome_amd.update_patch(unet, fp32_projections=True)
    cond, text, ims = _conditioning((4,), B, F, dtype, False, images=images)
    kw = {}
    with torch.no_grad():
        for ck in range(2):
            hs = _hidden(sl, B, F, latent, dtype, ck, seed0=80)
            for blk, h in zip(unet.blocks, hs):
                if case == "masks":
                    kw = {"ip_adapter_masks": [torch.ones(1, h.shape[1], 1, device=DEV, dtype=dtype)]}
                if h.shape[-1] == 1280:             # the site that does not merge: the UNPATCHED block is its own modules
                    h1 = blk.attn1(blk.norm1(h)) + h
                    h2 = blk.attn2(blk.norm2(h1), encoder_hidden_states=cond, **kw) + h1
                    want = blk.ff(blk.norm3(h2)) + h2
                    blk.attn2.processor.calls -= 1
                out = blk(h, encoder_hidden_states=cond, cross_attention_kwargs=kw)
                assert bool(torch.isfinite(out).all())
                if h.shape[-1] == 1280:
                    err = float((out.float() - want.float()).abs().max()) / max(1.0, float(want.abs().max()))
                    print(f"module-path block [{case}] vs its own modules err/scale={err:.3e}")
                    assert err < 2e-3, (case, err)
    if case == "blas":                              # VIDTOME_FF=blas: the same recognition, library GEMMs around the new core
        assert len(calls) == 2 * len(sl) and all(p.calls == 0 for p in procs)
    else:
        assert calls == [] and all(p.calls == 2 for p in procs)
    # attn2 itself: the patched block's cross-attention IS the module's forward, bit for bit (blas: within the core's bound)
    a2 = next(b.attn2 for b in unet.blocks if b.attn2.to_q.in_features == 320)
    x = torch.randn(B * F, 1024, 320, generator=torch.Generator().manual_seed(1)).to(device=DEV, dtype=dtype)
    if case == "masks":
        kw = {"ip_adapter_masks": [torch.ones(1, 1024, 1, device=DEV, dtype=dtype)]}
    with torch.no_grad():
        got = vpatch.cross_attention(a2, x, cond, None, **kw)
        want = a2(x, encoder_hidden_states=cond, **kw)
    if case == "blas":
        assert float((got.float() - want.float()).abs().max()) < 2e-3 * max(1.0, float(want.abs().max()))
    else:
        assert torch.equal(got, want)
    vidtome_amd.remove_patch(unet)


def test_fused_block_agrees_with_the_module_path(L, monkeypatch):
    """Computing modules, 4 frames: the fused IP-Adapter block against the same block with the recogniser forced to refuse
    (the processor's own arithmetic: every term rounded to fp16 and added in fp16) within 2e-3 of the output scale; the
    block without the adapter is far outside."""
    import vidtome_amd
    from vidtome_amd import ip_adapter
    sl = _site_list("up3.0", "up2.0")
    B, F, latent = 2, 4, (32, 32)
    cond, _, _ = _conditioning((4, 16), B, F, torch.float16, False)
    res = {}
    for path in ("fused", "module", "base"):
        unet, procs = _computing_sites(sl, torch.float16, (4, 16), (0.7, 0.3) if path != "base" else (0.0, 0.0))
        if path == "module":
            monkeypatch.setattr(ip_adapter, "is_ip_processor", lambda attn: False)
        _patch(unet, B, latent)
        with torch.no_grad():
            res[path] = [blk(h, encoder_hidden_states=cond) for blk, h in
                         zip(unet.blocks, _hidden(sl, B, F, latent, torch.float16, 0, seed0=90))]
        assert all(p.calls == (1 if path == "module" else 0) for p in procs)
        monkeypatch.undo()
        vidtome_amd.remove_patch(unet)
    for a, b, c in zip(res["fused"], res["module"], res["base"]):
        osc = max(1.0, float(b.abs().max()))
        assert float((a.float() - b.float()).abs().max()) < 2e-3 * osc
        assert float((c.float() - b.float()).abs().max()) > 2 * 2e-3 * osc


# ---------------------------------------------------------------------------------------------------
# 5. state changes
# ---------------------------------------------------------------------------------------------------
def test_scale_changes_zero_scales_nan_tokens_and_remove_patch(L, monkeypatch):
    import vidtome_amd
    from vidtome_amd import sites as S
    sl = _site_list("up3.0", "up2.0")
    B, F, latent, dtype = 2, 4, (32, 32), torch.float16

    def model(num_tokens, scales, ip=True):
        unet = _StandInSites(sl, True).to(device=DEV, dtype=dtype)
        procs = install(unet, num_tokens, scales) if ip else []
        return _patch(unet, B, latent), procs

    def run(unet, cond):
        torch.manual_seed(123)
        for blk in unet.blocks:
            blk.__dict__.pop("generator", None)
            blk.global_tokens = None
        with torch.no_grad():
            return [[o.clone() for o in S.run_block_pass(unet, _hidden(sl, B, F, latent, dtype, ck, seed0=95), cond)]
                    for ck in range(2)]
    eq = lambda x, y: all(torch.equal(a, b) for ca, cb in zip(x, y) for a, b in zip(ca, cb))
    cond2, text, ims = _conditioning((4, 16), B, F, dtype, False)
    two, procs = model((4, 16), (0.7, 0.3))
    first = run(two, cond2)
    # a scale changed between two forwards takes effect on the next one (and back)
    for p in procs:
        p.scale = [0.7, 1.1]
    changed = run(two, cond2)
    assert not eq(changed, first)
    for p in procs:
        p.scale = [0.7, 0.3]
    assert eq(run(two, cond2), first)
    # one of two scales 0 = the one-adapter block (same projections: install draws adapter 0's weights first)
    one, procs1 = model((4,), (0.7,))
    same_weights = lambda dst: [db.load_state_dict({k: v for k, v in tb.state_dict().items() if ".processor." not in k},
                                                   strict=False) for db, tb in zip(dst.blocks, two.blocks)]
    same_weights(one)                              # (the stand-in's biases are drawn from the global generator)
    for p2, p1 in zip(procs, procs1):
        p1.to_k_ip[0].load_state_dict(p2.to_k_ip[0].state_dict())
        p1.to_v_ip[0].load_state_dict(p2.to_v_ip[0].state_dict())
        p2.scale = [0.7, 0.0]
    want_one = run(one, (text, ims[:1]))
    assert eq(run(two, cond2), want_one) and not eq(want_one, first)
    # NaN in the image tokens of a zero-scale adapter never reaches the output
    nan_ims = [ims[0], torch.full_like(ims[1], float("nan"))]
    assert eq(run(two, (text, nan_ims)), want_one)
    # all scales 0 = the block without an adapter, bit for bit, without a launch of the new core
    plain, _ = model((), (), ip=False)
    same_weights(plain)
    for p in procs:
        p.scale = [0.0, 0.0]
    calls = _spy(monkeypatch, L)
    got_zero = run(two, (text, nan_ims))
    assert len(calls) == 2 * len(sl)               # the wrapper was asked ...
    monkeypatch.undo()
    assert eq(got_zero, run(plain, text))          # ... and routed the single set to attention_kv
    # remove_patch restores the class and drops every cache on the processor's projections
    for p in procs:
        p.scale = [0.7, 0.3]
    run(two, cond2)
    cached = [m for p in procs for m in list(p.to_k_ip) + list(p.to_v_ip)]
    assert all("_vtm_packed" in m.__dict__ for m in cached)
    for m in (two, one, plain):
        vidtome_amd.remove_patch(m)
    assert all("_vtm_packed" not in m.__dict__ and "_vtm_lora" not in m.__dict__ for m in cached)
    assert all(type(b).__name__ == "BasicTransformerBlock" for b in two.blocks)
