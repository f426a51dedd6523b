"""The fp32 attention core (csrc/attention_f32.hip) on the GPU: kernel launches against the oracle (double accumulation),
patched fp32 blocks with `update_patch(unet, fp32_attention=True)` against a double restatement, and the paths that
must not change (fp32 models without the switch, 16-bit models with it, folded keys).

Bar: 2e-5 of the output scale.  For a head the fp32 core accumulates scores over d channels and O^T / the denominator
over up to Mk = 90 319 keys in fp32 MFMA chains; the rounding of a chain of n terms grows like sqrt(n) * 2^-24 of the
partial sums for data without a bias, i.e. ~2e-5 relative at n = 90 319 in the worst of the sums, which is the
denominator (all terms positive).  A relative error r of the denominator moves an output by r * |output|, within the
bar for |output| <= the scale.  The fp16 core misses the same bar by an order of magnitude (asserted per head dim)."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 2e-5
HEAD_DIMS = (8, 16, 32, 40, 64, 80, 96, 128, 160)


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _pad8(n):
    return (n + 7) // 8 * 8


def _inputs(B, h, d, Mq, Mk, seed, qs=1.5):
    """fp32 q (B, Mqp, C), k (B, Mkp, C), vt (B, C, Mkp) on the device, moderately peaked softmax rows."""
    C = h * d
    g = torch.Generator(device=DEV).manual_seed(seed)
    base = torch.randn(B, 1, C, generator=g, device=DEV)
    q = torch.zeros(B, _pad8(Mq), C, device=DEV)
    k = torch.zeros(B, _pad8(Mk), C, device=DEV)
    q[:, :Mq] = qs * torch.randn(B, Mq, C, generator=g, device=DEV)
    k[:, :Mk] = 0.3 * base + torch.randn(B, Mk, C, generator=g, device=DEV)
    vt = torch.zeros(B, C, _pad8(Mk), device=DEV)
    vt[:, :, :Mk] = torch.randn(B, C, Mk, generator=g, device=DEV)
    return q, k, vt


def _ref(oracle, q, k, vt, h, d, Mk, rows, share=1):
    """oracle.attention_qkv on the query rows `rows` (share > 1: q / k of the source samples for every group)."""
    B = q.shape[0]
    src = B // share
    qn = q[:, rows].cpu().numpy()
    kn = k[:, :Mk].cpu().numpy()
    vn = vt[:, :, :Mk].transpose(1, 2).contiguous().cpu().numpy()
    if share > 1:
        qn = np.concatenate([qn[:src]] * share)
        kn = np.concatenate([kn[:src]] * share)
    return oracle.attention_qkv(np.ascontiguousarray(qn), np.ascontiguousarray(kn), vn, h, d ** -0.5)


def _err(got, ref):
    scale = float(np.abs(ref).max())
    assert scale > 0.05, "the comparison should not be about zeros"
    return float(np.abs(got - ref).max()) / scale


@pytest.mark.parametrize("d", HEAD_DIMS)
@pytest.mark.parametrize("share", [1, 2, 3])
def test_self_attention_every_head_dim(L, oracle, d, share):
    """vtm_attention (fp32): odd M, a ragged last key tile, PnP sharing over 1 / 2 / 3 groups.  On the unshared launch
    the fp16 core on the same inputs misses the bar: the bar discriminates."""
    h, M = 2, 1001
    B = 2 * share if share > 1 else 2
    q, k, vt = _inputs(B, h, d, M, M, seed=d * 10 + share)
    o = L.attention(q, k, vt, h, M, d ** -0.5, share)
    assert o.dtype == torch.float32
    rows = np.arange(M)
    ref = _ref(oracle, q, k, vt, h, d, M, rows, share)
    got = o[:, :M].cpu().numpy()
    assert np.isfinite(got).all()
    assert _err(got, ref) <= BAR, (d, share, _err(got, ref))
    if share == 1:
        o16 = L.attention(q.half(), k.half(), vt.half(), h, M, d ** -0.5, 1)
        assert _err(o16[:, :M].float().cpu().numpy(), ref) > BAR, d


@pytest.mark.parametrize("d,Mq,Mk", [(40, 333, 77), (64, 1000, 77), (80, 515, 2053), (160, 200, 4097), (8, 77, 1999),
                                     (128, 4099, 513)])
def test_attention_kv_mq_ne_mk(L, oracle, d, Mq, Mk):
    """vtm_attention_kv (fp32) with Mq != Mk, Mk = 77 padded to 80 included."""
    h, B = 3, 2
    q, k, vt = _inputs(B, h, d, Mq, Mk, seed=Mq + Mk + d)
    o = L.attention_kv(q, k, vt, h, Mq, Mk, d ** -0.5)
    ref = _ref(oracle, q, k, vt, h, d, Mk, np.arange(Mq))
    assert _err(o[:, :Mq].cpu().numpy(), ref) <= BAR, d


@pytest.mark.parametrize("d", [40, 64, 80, 160])
@pytest.mark.parametrize("frac", [0.15, 0.55, 0.97])
@pytest.mark.parametrize("share", [1, 3])
def test_bounded_launches(L, oracle, d, frac, share):
    """vtm_attention_kv_bounded / _shared_bounded (fp32): only the first q_count[b] rows are live, from a fraction of a
    round to nearly all.  The launches are sized for at least two rounds and the binding's workspace holds a device
    plan, so they are planned on the device -- asserted through the restated selection of test_gpu_attention_plans.py,
    which pins that plan's tiers and records on shapes of its own."""
    from test_gpu_attention_plans import Selection, _binding_ws, cus
    h = 8
    B = 3 if share == 3 else 2
    Mq, Mk = 9000, 6000
    q, k, vt = _inputs(B, h, d, Mq, Mk, seed=int(frac * 100) + d + share)
    cnt = [max(1, int(frac * Mq) - 37 * b) for b in range(B)]
    if share > 1:
        cnt = [cnt[0]] * B                   # align_batch: every sample of a group has the same live rows
    q_count = torch.tensor(cnt, dtype=torch.int32, device=DEV)
    sel = Selection("shared_bounded" if share > 1 else "bounded", d, B, h, Mq, Mk, share, vt.shape[2],
                    _binding_ws(L, torch.float32, B, h, Mq, Mk, d, True), cnt, cus(), f32=True)
    assert (sel.kind, sel.plan) == ("f32", "device"), ("the shape does not select the plan it names", sel.kind, sel.plan)
    o = L.attention_kv(q, k, vt, h, Mq, Mk, d ** -0.5, q_count=q_count, share_groups=share)
    rs = np.random.default_rng(d)
    lo = min(cnt)
    rows = np.unique(np.concatenate([np.arange(min(64, lo)), np.arange(max(0, lo - 64), lo), rs.integers(0, lo, 128)]))
    ref = _ref(oracle, q, k, vt, h, d, Mk, rows, share)
    got = o[:, rows].cpu().numpy()
    assert _err(got, ref) <= BAR, (d, frac, share)


@pytest.mark.parametrize("name,B,h,d,Mq,Mk", [
    ("cfg-2 top block", 2, 8, 40, 34816, 52224),
    ("cfg-2 mid block", 2, 8, 80, 8704, 13056),
    ("cfg-5 top block", 2, 5, 64, 64513, 90319),
])
def test_full_size_vs_oracle(L, oracle, name, B, h, d, Mq, Mk):
    """The full-size launches on sampled query rows (first and last blocks, rows spread over the rest), under whichever
    plan the shape takes on this device (the plans themselves are pinned in test_gpu_attention_plans.py)."""
    q, k, vt = _inputs(B, h, d, Mq, Mk, seed=Mq + Mk)
    o = L.attention_kv(q, k, vt, h, Mq, Mk, d ** -0.5)
    rs = np.random.default_rng(Mq)
    rows = np.unique(np.concatenate([np.arange(0, 64), np.arange(Mq - 96, Mq), rs.choice(Mq, 384, replace=False)]))
    ref = _ref(oracle, q, k, vt, h, d, Mk, rows)
    got = o[:, torch.from_numpy(rows).to(DEV)].cpu().numpy()
    assert _err(got, ref) <= BAR, (name, _err(got, ref))


@pytest.mark.parametrize("d", [40, 64, 160])
@pytest.mark.parametrize("case", ["spike_late", "spike_every_tile", "all_very_negative", "wide_range"])
def test_attention_rescale_paths_fp32(L, oracle, d, case):
    """The online-softmax corner cases of test_attention_rescale_paths (test_gpu_parity.py) on attention_f32_kernel: the
    running maximum jumps late (the deferred-rescale branch, taken by both query halves of a wave under one __all),
    grows in every 32-key tile, sits far below zero, or the logits span +-40.  d = 40 ends its contraction on the half
    chunk, d = 160 has one query half per wave.  M = 700 is not a multiple of 32: the last live wave's second half
    (rows 688 .. 703) is partly past M.  The bar is BAR in all four cases: a plain float32 CPU restatement of wide_range
    (numpy float32 matmul and softmax on the same inputs) is within 2.0e-6 / 2.8e-6 / 2.4e-6 of the float64 oracle at
    d = 40 / 64 / 160, so fp32 score rounding does meet BAR there and no allowance is made."""
    B, h, M = 1, 2, 700          # 22 key tiles of 32
    C = h * d
    g = torch.Generator().manual_seed(77 + d)
    q = torch.randn(B, M, C, generator=g)
    k = torch.randn(B, M, C, generator=g)
    v = torch.randn(B, M, C, generator=g)
    if case == "spike_late":
        k[:, 600] = 6.0 * q[:, 17]                     # one key dominates query 17 from tile 18 on
        k[:, 333, :d] = 5.0 * q[:, 400, :d]
    elif case == "spike_every_tile":
        for t in range(22):
            k[:, min(32 * t + 5, M - 1)] = (0.5 + 0.225 * t) * q[:, 3]
    elif case == "all_very_negative":
        k = -3.0 * q[:, :1].expand(B, M, C).clone() + 0.05 * k   # every score of query 0 ~ -3 |q|^2 / sqrt(d)
        q[:, 1:] = 3.0 * q[:, :1] + 0.05 * q[:, 1:]
    else:
        q, k = 3.0 * q, 3.0 * k
    Mp = _pad8(M)
    pad = lambda t: torch.nn.functional.pad(t, (0, 0, 0, Mp - M))
    o = L.attention(pad(q).to(DEV), pad(k).to(DEV), pad(v).to(DEV).transpose(1, 2).contiguous(), h, M, d ** -0.5, 1)
    assert o.dtype == torch.float32
    got = o[:, :M].cpu().numpy()
    ref = oracle.attention_qkv(q.numpy(), k.numpy(), v.numpy(), h, d ** -0.5)
    assert np.isfinite(got).all()
    print(f"fp32 rescale paths d={d} {case}: {_err(got, ref):.3g} of max|ref|")
    assert _err(got, ref) <= BAR, (d, case, _err(got, ref))


def test_folded_keys_reject_fp32(L):
    """The fp32 path never folds keys: the export returns an error (no launch), the binding raises before the call."""
    B, h, d, M = 1, 1, 40, 64
    q = torch.zeros(B, M, h * d, device=DEV)
    vt = torch.zeros(B, h * d, M, device=DEV)
    cnt = torch.full((B,), M, dtype=torch.int32, device=DEV)
    bias = torch.zeros(B, M, dtype=torch.int32, device=DEV)
    out = torch.full_like(q, 7.0)
    rc = L.lib().vtm_attention_kv_folded(q.data_ptr(), h * d, q.data_ptr(), h * d, vt.data_ptr(), M, out.data_ptr(), h * d,
                                         L.VTM_F32, B, h, M, M, M, M, d, 0.1, None, cnt.data_ptr(), bias.data_ptr(), M,
                                         None, 0, None)
    assert rc < 0
    assert b"never folded" in L.lib().vtm_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(RuntimeError, match="never folded"):
        L.attention_kv(q, q, vt, h, M, M, 0.1, k_fold=(cnt, bias))


# ---------------------------------------------------------------------------------------------------
# patched fp32 blocks
# ---------------------------------------------------------------------------------------------------
def _run(unet, hiddens):
    """One pass; returns (outs, plans) with the merge plan every block used (None: un-merged)."""
    from vidtome_amd import patch as vpatch
    from vidtome_amd import sites as S
    seen = {}
    orig = vpatch.compute_merge

    def rec(module, x, info, **kw):
        res = orig(module, x, info, **kw)
        seen[id(module)] = getattr(res[0], "plan", None)
        return res

    vpatch.compute_merge = rec
    try:
        with torch.no_grad():
            outs = S.run_segment_pass(unet, hiddens)
    finally:
        vpatch.compute_merge = orig
    return outs, [seen.get(id(b)) for b in unet.blocks]


def _rows_vs_double(blk, plan, hidden, out, fsize, share=1, n_rows=160, seed=0):
    """to_out(softmax(q K^T) V)[inv] + hidden on sampled positions, in float64 from the plan's merged rows (q / k of the
    source sample for every group when share > 1).  Returns the error relative to max(1, |ref|)."""
    from vidtome_amd.utils import join_frame
    a = blk.attn1
    f64 = lambda t: t.detach().double().cpu()
    wq, wk, wv, wo, bo = (f64(a.to_q.weight), f64(a.to_k.weight), f64(a.to_v.weight), f64(a.to_out[0].weight),
                          f64(a.to_out[0].bias))
    merged = f64(plan.merged[:, :plan.M])
    Bn, Lt = plan.inv.shape
    g = np.random.default_rng(seed)
    idx = torch.from_numpy(np.unique(np.concatenate([np.arange(8), np.arange(Lt - 8, Lt), g.integers(0, Lt, n_rows)])))
    m = plan.inv.cpu()[:, idx]
    src = (lambda t: t[:1].expand_as(t)) if share > 1 else (lambda t: t)
    k, v = src(merged) @ wk.T, merged @ wv.T
    q = torch.stack([src(merged)[b, m[b]] for b in range(Bn)]) @ wq.T
    h, C = a.heads, q.shape[-1]
    d = C // h
    sh = lambda t: t.view(t.shape[0], t.shape[1], h, d).transpose(1, 2)
    p = torch.softmax(sh(q) @ sh(k).transpose(-1, -2) * a.scale, dim=-1)
    o = (p @ sh(v)).transpose(1, 2).reshape(Bn, -1, C)
    ref = o @ wo.T + bo + f64(join_frame(hidden, fsize))[:, idx]
    got = f64(join_frame(out, fsize))[:, idx]
    return float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def _unmerged_vs_double(blk, hidden, out):
    """attn1(norm1(h)) + h per frame in float64 (the site does not merge)."""
    a, n = blk.attn1, blk.norm1
    f64 = lambda t: t.detach().double().cpu()
    x = f64(hidden)
    xn = torch.nn.functional.layer_norm(x, n.normalized_shape, f64(n.weight), f64(n.bias), n.eps)
    q, k, v = xn @ f64(a.to_q.weight).T, xn @ f64(a.to_k.weight).T, xn @ f64(a.to_v.weight).T
    h, C = a.heads, q.shape[-1]
    d = C // h
    sh = lambda t: t.view(t.shape[0], t.shape[1], h, d).transpose(1, 2)
    o = (torch.softmax(sh(q) @ sh(k).transpose(-1, -2) * a.scale, dim=-1) @ sh(v)).transpose(1, 2).reshape(x.shape)
    ref = o @ f64(a.to_out[0].weight).T + f64(a.to_out[0].bias) + x
    return float((f64(out) - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def test_fp32_blocks_at_cfg2_sizes(L):
    """An fp32 SD-1.5 stand-in at cfg-2 sizes (2 x 16 frames 512x512, global merging) with fp32_attention: top (d = 40),
    mid (d = 80) and an un-merged site (d = 160), three chunks so the global level is in steady state."""
    import vidtome_amd
    from vidtome_amd import sites as S
    B, F, latent = 2, 16, (64, 64)
    sl = [s for s in S.sd15_sites() if s.name in ("down0.0", "down1.0", "down2.0")]
    unet = S.SiteUNet(sl, seed=3).to(device=DEV, dtype=torch.float32)
    vidtome_amd.apply_patch(unet, local_merge_ratio=0.9, merge_global=True, global_merge_ratio=0.8, batch_size=B)
    vidtome_amd.update_patch(unet, fp32_attention=True)
    unet.set_size(latent)
    torch.manual_seed(123)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for chunk in range(3):
            hiddens = [S.synthetic_hidden(s, B, F, latent, torch.float32, DEV, seed=90 + 10 * chunk + i) for i, s in enumerate(sl)]
            outs, plans = _run(unet, hiddens)
    assert not any("fp32 model --" in str(x.message) for x in w)          # the fp16-core warning is not given
    assert plans[0] is not None and plans[1] is not None and plans[2] is None
    for i in (0, 1):
        e = _rows_vs_double(unet.blocks[i], plans[i], hiddens[i], outs[i], F, seed=i)
        assert e <= BAR, (sl[i].name, e)
    e = _unmerged_vs_double(unet.blocks[2], hiddens[2], outs[2])
    assert e <= BAR, e
    vidtome_amd.remove_patch(unet)


def test_fp32_blocks_pnp_shared(L):
    """The same with PnP sharing: batch 3 (source | uncond | cond), align_batch, shared probabilities (q / k of the source
    sample for every group, live-query launches included)."""
    import vidtome_amd
    from vidtome_amd import sites as S
    B, F, latent = 3, 16, (64, 64)
    sl = [s for s in S.sd15_sites() if s.name in ("up3.0", "up2.0")]
    unet = S.SiteUNet(sl, seed=2).to(device=DEV, dtype=torch.float32)
    for blk in unet.blocks:
        blk.attn1.injection_schedule, blk.attn1.t, blk.attn1.vtm_num_inputs = [981], 981, B
    vidtome_amd.apply_patch(unet, local_merge_ratio=0.5, merge_global=True, global_merge_ratio=0.5, batch_size=B,
                            align_batch=True)
    vidtome_amd.update_patch(unet, fp32_attention=True)
    unet.set_size(latent)
    torch.manual_seed(123)
    for chunk in range(2):
        hiddens = [S.synthetic_hidden(s, B, F, latent, torch.float32, DEV, seed=70 + 10 * chunk + i) for i, s in enumerate(sl)]
        outs, plans = _run(unet, hiddens)
    for i in range(len(sl)):
        assert plans[i] is not None
        e = _rows_vs_double(unet.blocks[i], plans[i], hiddens[i], outs[i], F, share=B, seed=i)
        assert e <= BAR, (sl[i].name, e)
    vidtome_amd.remove_patch(unet)


def _pass(dtype, flag, seed=5):
    import vidtome_amd
    from vidtome_amd import sites as S
    B, F, latent = 2, 8, (32, 32)
    sl = [s for s in S.sd15_sites() if s.name in ("down0.0", "down1.0", "down2.0")]
    unet = S.SiteUNet(sl, seed=4).to(device=DEV, dtype=dtype)
    vidtome_amd.apply_patch(unet, merge_global=True, batch_size=B)
    if flag is not None:
        vidtome_amd.update_patch(unet, fp32_attention=flag)
    unet.set_size(latent)
    torch.manual_seed(seed)
    res = []
    for chunk in range(2):
        hiddens = [S.synthetic_hidden(s, B, F, latent, dtype, DEV, seed=30 + 10 * chunk + i) for i, s in enumerate(sl)]
        with torch.no_grad():
            res += [o.clone() for o in S.run_segment_pass(unet, hiddens)]
    vidtome_amd.remove_patch(unet)
    return res


def test_fp32_model_without_the_switch_is_unchanged(L):
    """Without the switch an fp32 model runs today's fp16 core: bit-identical to an explicit restatement of that path
    (fp32 projections, q / k / v^T rounded to fp16, vtm_attention, fp32 output projection), to an explicit
    fp32_attention=False, and the warning still comes once."""
    from vidtome_amd import patch as vpatch
    from vidtome_amd import sites as S
    vpatch._warned.discard("fp32-core")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        a = _pass(torch.float32, None)
    assert sum("fp32 model --" in str(x.message) for x in w) == 1
    b = _pass(torch.float32, False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = _pass(torch.float32, True)
    assert any(not torch.equal(x, y) for x, y in zip(a, c))             # the switch does change the arithmetic
    # explicit restatement of the fp16-core path on one module
    blk = S.SiteUNet([s for s in S.sd15_sites() if s.name == "down0.0"], seed=4).to(device=DEV).blocks[0]
    x = torch.randn(2, 1024, 320, device=DEV)
    with torch.no_grad():
        y = vpatch.self_attention(blk.attn1, x)
        at = blk.attn1
        wqk = torch.cat([at.to_q.weight, at.to_k.weight])
        qk = torch.nn.functional.linear(x, wqk).half()
        vt = torch.empty(2, 320, 1024, device=DEV)
        for i in range(2):
            torch.mm(at.to_v.weight, x[i].t(), out=vt[i])
        o = L.attention(qk[:, :, :320], qk[:, :, 320:], vt.half(), at.heads, 1024, at.scale, 1).float()
        y2 = torch.nn.functional.linear(o, at.to_out[0].weight, at.to_out[0].bias)
        y3 = vpatch.self_attention(blk.attn1, x, fp32_core=True)
    assert torch.equal(y, y2)
    assert not torch.equal(y, y3)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_16bit_models_ignore_the_switch(L, dtype):
    a = _pass(dtype, None)
    b = _pass(dtype, True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
