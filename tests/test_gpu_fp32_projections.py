"""The fp32 projection GEMMs (csrc/linear_f32.hip, `update_patch(model, fp32_projections=True)`) on the GPU: the kernel
against float64 for every epilogue / orientation / output type, a whole fp32 block with no library GEMM and no torch
attention, accuracy against a float64 restatement at cfg-2 sizes and against the reference's recorded blocks, and the paths
that must not change.

Kernel bar, per element: |y - y64| <= 1e-6 * sum_k |a_k w_k| (+ 1e-7 |b|): a k-ordered fp32 fmaf chain of K <= 5120 terms
rounds each partial sum once, 2^-24 relative, so its error is at most K 2^-24 sum|a_k w_k| in the worst case and about
sqrt(K) 2^-24 of it in practice (4e-6 .. 3e-7); the bar sits between the two."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 12345.0


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _pad8(n):
    return (n + 7) // 8 * 8


def _gelu64(g):
    return 0.5 * g * (1.0 + torch.erf(g / np.sqrt(2.0)))


# (K, N, epilogue, transposed, B, n, P0, P1, maps: "" / "rows" / "rows2" / "both", bias)
CASES = [
    (320, 640, "none", False, 2, 1001, 900, 300, "both", True),      # q | k of the cfg-2 top block through the map
    (320, 320, "none", True, 3, 777, 800, 0, "rows", False),          # V^T (256 x 64 tile), B = 3
    (640, 640, "resid", False, 1, 1234, 1234, 0, "", True),           # attn2 / FF output, identity rows
    (1280, 1280, "resid", True, 2, 333, 400, 50, "rows2", True),      # live-query rows only, channel-major residual
    (320, 2560, "geglu", False, 1, 999, 999, 0, "", True),            # FF GEGLU, C = 320
    (128, 1024, "geglu", True, 2, 301, 200, 120, "both", True),       # test-fixture K, channel-major GEGLU
    (768, 320, "none", False, 2, 77, 77, 0, "", False),               # attn2 k of the conditioning (K = 768)
    (1024, 1024, "none", False, 3, 129, 129, 0, "", True),            # SD-2.1 conditioning width
    (5120, 1280, "resid", False, 1, 250, 250, 0, "", True),           # FF output of the C = 1280 blocks
    (2560, 640, "none", True, 1, 515, 515, 0, "", True),              # FF output K of the C = 640 blocks
    (136, 72, "none", False, 2, 50, 60, 0, "rows", True),             # K and N tails (K % 32 = 8, N % 64 = 8)
    (136, 48, "geglu", False, 1, 37, 37, 0, "", False),               # GEGLU with D = 24 (a ragged channel tile)
]


def _case_inputs(K, N, B, n, P0, P1, maps, bias, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x0 = torch.randn(B, P0, K, generator=g, device=DEV)
    x1 = torch.randn(B, P1, K, generator=g, device=DEV) if P1 else None
    W = torch.randn(N, K, generator=g, device=DEV) * K ** -0.5
    b = torch.randn(N, generator=g, device=DEV) if bias else None
    P = P0 + P1
    M = max(n, 64) + 17
    rows = torch.randint(0, P, (B, M), generator=g, device=DEV, dtype=torch.int32) if maps in ("rows", "both") else None
    hi = M if rows is not None else P
    rows2 = torch.randint(0, hi, (B, n), generator=g, device=DEV, dtype=torch.int32) if maps in ("rows2", "both") else None
    if rows is not None and rows2 is None:
        rows = rows[:, :n].contiguous() if M >= n else rows
    return x0, x1, W, b, rows, rows2


def _gathered(x0, x1, rows, rows2, n):
    pool = x0 if x1 is None else torch.cat([x0, x1], dim=1)
    B = pool.shape[0]
    idx = torch.arange(n, device=DEV).expand(B, n)
    if rows2 is not None:
        idx = rows2.long()
    if rows is not None:
        idx = torch.gather(rows.long(), 1, idx)
    return torch.stack([pool[b, idx[b]] for b in range(B)])                     # (B, n, K)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"K{c[0]}-N{c[1]}-{c[2]}-{'T' if c[3] else 'R'}-B{c[4]}-n{c[5]}-{c[8] or 'id'}")
def test_kernel_vs_float64(L, case):
    K, N, epi, tr, B, n, P0, P1, maps, bias = case
    x0, x1, W, b, rows, rows2 = _case_inputs(K, N, B, n, P0, P1, maps, bias, seed=K + N + n)
    Nout = N // 2 if epi == "geglu" else N
    # sentinel-filled result buffers: rows >= n (channels >= Nout when channel-major) and the ldo padding must stay untouched
    shape = (B, Nout + 3, _pad8(n) + 8) if tr else (B, n + 5, Nout + 8)
    resid = torch.randn(shape, device=DEV) if epi == "resid" else None
    outs = {}
    for dt in (torch.float32, torch.float16):
        buf = torch.full(shape, SENT, dtype=dt, device=DEV)
        y = L.linear_f32(x0, x1, rows, rows2, n, W, b, epilogue=epi, resid=resid, out_dtype=dt, transposed=tr, out=buf)
        assert y.data_ptr() == buf.data_ptr()
        outs[dt] = buf
    torch.cuda.synchronize()
    for dt, buf in outs.items():
        valid = buf[:, :Nout, :n] if tr else buf[:, :n, :Nout]
        pad = torch.ones(shape, dtype=torch.bool, device=DEV)
        (pad[:, :Nout, :n] if tr else pad[:, :n, :Nout]).fill_(False)
        assert bool((buf[pad] == SENT).all()), ("padding written", dt)
        assert bool(torch.isfinite(valid).all())
    y32 = outs[torch.float32][:, :Nout, :n] if tr else outs[torch.float32][:, :n, :Nout]
    y16 = outs[torch.float16][:, :Nout, :n] if tr else outs[torch.float16][:, :n, :Nout]
    assert torch.equal(y16, y32.half())                                          # one rounding of the fp32 value

    a = _gathered(x0, x1, rows, rows2, n).double()
    Wd = W.double()
    bd = b.double() if b is not None else torch.zeros(N, dtype=torch.float64, device=DEV)
    z = a @ Wd.T + bd                                                            # (B, n, N)
    S = a.abs() @ Wd.abs().T
    tol = 1e-6 * S + 1e-7 * bd.abs()
    if epi == "geglu":
        D = Nout
        v, gt, tv, tg = z[..., :D], z[..., D:], tol[..., :D], tol[..., D:]
        ref = v * _gelu64(gt)
        dgelu = (_gelu64(gt + 1e-4) - _gelu64(gt - 1e-4)).abs() / 2e-4
        tol = tv * _gelu64(gt).abs() + v.abs() * dgelu * tg + v.abs() * 2e-7 * (1 + gt.abs()) + 2e-7 * ref.abs()
    else:
        ref = z
        if epi == "resid":
            r = resid[:, :Nout, :n].transpose(1, 2) if tr else resid[:, :n, :Nout]
            ref = ref + r.double()
            tol = tol + 1.2e-7 * ref.abs()
    got = (y32.transpose(1, 2) if tr else y32).double()
    err = (got - ref).abs()
    bad = err > tol
    assert not bool(bad.any()), (case, float(err.max()), float((err / tol.clamp_min(1e-30)).max()))


def test_linear_rows_f32_is_the_plain_epilogue(L):
    """vtm_linear_rows with VTM_F32 = vtm_linear_f32 NONE / VTM_F32, bit for bit."""
    x0, x1, W, b, rows, rows2 = _case_inputs(320, 640, 2, 500, 400, 100, "both", True, seed=7)
    a = L.linear_rows(x0, x1, rows, rows2, 500, W, b)
    c = L.linear_f32(x0, x1, rows, rows2, 500, W, b)
    assert a.dtype == torch.float32 and torch.equal(a, c)


# ---------------------------------------------------------------------------------------------------
# patched fp32 blocks
# ---------------------------------------------------------------------------------------------------
def _full_unet(names, dtype, seed, B, latent, flags, **patch_kw):
    import vidtome_amd
    from vidtome_amd import sites as S
    sl = [s for s in S.sd15_sites() if s.name in names]
    unet = S.SiteUNet(sl, seed=seed, full=True).to(device=DEV, dtype=dtype)
    vidtome_amd.apply_patch(unet, batch_size=B, **patch_kw)
    if flags:
        vidtome_amd.update_patch(unet, **flags)
    unet.set_size(latent)
    return unet, sl


def _cond(B, F, seed, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    c = torch.randn(B, 1, 77, 768, generator=g, device=DEV).expand(B, F, 77, 768)
    return c.reshape(B * F, 77, 768).to(dtype).contiguous()


def _block_passes(unet, sl, B, F, latent, dtype, chunks, seed):
    from vidtome_amd import sites as S
    torch.manual_seed(seed)
    res = []
    for ck in range(chunks):
        hiddens = [S.synthetic_hidden(s, B, F, latent, dtype, DEV, seed=seed + 10 * ck + i) for i, s in enumerate(sl)]
        with torch.no_grad():
            res.append((hiddens, [o.clone() for o in S.run_block_pass(unet, hiddens, _cond(B, F, seed + ck, dtype))]))
    return res


def test_library_free_fp32_block(L, monkeypatch):
    """An fp32 full-block pass with both flags runs on libvidtome_hip.so alone: every torch GEMM and torch's attention raise
    during the pass.  Merged top (d = 40) and mid (d = 80) sites and an un-merged one (d = 160), 2 chunks, global merging."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    B, F, latent = 2, 4, (32, 32)
    unet, sl = _full_unet(("down0.0", "down1.0", "down2.0"), torch.float32, 3, B, latent,
                          dict(fp32_projections=True, fp32_attention=True), merge_global=True)
    calls = {"linear_f32": 0}
    orig = L.linear_f32

    def counted(*a, **k):
        calls["linear_f32"] += 1
        return orig(*a, **k)

    def banned(name):
        def f(*a, **k):
            raise AssertionError(f"{name} called inside the fp32 block")
        return f
    monkeypatch.setattr(L, "linear_f32", counted)
    for mod, name in ((torch.nn.functional, "linear"), (torch, "mm"), (torch, "matmul"), (torch, "bmm"), (torch, "baddbmm"),
                      (torch, "einsum"), (torch.nn.functional, "scaled_dot_product_attention")):
        monkeypatch.setattr(mod, name, banned(name))
    plans = []
    orig_cm = vpatch.compute_merge

    def rec(module, x, info, **kw):
        res = orig_cm(module, x, info, **kw)
        plans.append(getattr(res[0], "plan", None))
        return res
    monkeypatch.setattr(vpatch, "compute_merge", rec)
    res = _block_passes(unet, sl, B, F, latent, torch.float32, 2, seed=40)
    monkeypatch.undo()
    assert plans[-3] is not None and plans[-2] is not None and plans[-3].gather_map is not None and plans[-1] is None
    assert calls["linear_f32"] >= 2 * 3 * 7
    for _, outs in res:
        assert all(o.dtype == torch.float32 and bool(torch.isfinite(o).all()) for o in outs)
    vidtome_amd.remove_patch(unet)


def _block_rows_vs_double(blk, plan, hidden, seg, out, cond, fsize, n_rows=96, seed=0):
    """(segment error, block error) on sampled positions, relative to the output scale: the segment
    to_out(softmax(q K^T) V)[inv] + hidden from the plan's merged rows (plan None: per frame from norm1), then
    norm2 -> attn2 over the conditioning -> + and norm3 -> GEGLU feed-forward -> + on those rows, all in float64."""
    from vidtome_amd.utils import join_frame
    F_ = torch.nn.functional
    f64 = lambda t: t.detach().double()
    a = blk.attn1
    h, C = a.heads, hidden.shape[-1]
    d = C // h
    sh = lambda t: t.reshape(t.shape[0], t.shape[1], h, d).transpose(1, 2)
    core = lambda q, k, v, s: (torch.softmax(sh(q) @ sh(k).transpose(-1, -2) * s, dim=-1) @ sh(v)).transpose(1, 2).reshape(
        q.shape[0], q.shape[1], C)
    wq, wk, wv, wo, bo = (f64(a.to_q.weight), f64(a.to_k.weight), f64(a.to_v.weight), f64(a.to_out[0].weight),
                          f64(a.to_out[0].bias))
    g = np.random.default_rng(seed)
    if plan is not None:
        merged = f64(plan.merged[:, :plan.M])
        Bn, Lt = plan.inv.shape
        idx = torch.from_numpy(np.unique(np.concatenate([np.arange(8), np.arange(Lt - 8, Lt), g.integers(0, Lt, n_rows)])))
        m = plan.inv[:, idx.to(DEV)].long()
        k, v = merged @ wk.T, merged @ wv.T
        q = torch.stack([merged[b, m[b]] for b in range(Bn)]) @ wq.T
        x = f64(join_frame(hidden, fsize))[:, idx]
        y_seg = core(q, k, v, a.scale) @ wo.T + bo + x
        pick = lambda t: f64(join_frame(t, fsize))[:, idx]
        cnd = f64(cond.view(-1, fsize, *cond.shape[1:])[:, 0])
    else:
        n1 = blk.norm1
        x_all = f64(hidden)
        xn = F_.layer_norm(x_all, n1.normalized_shape, f64(n1.weight), f64(n1.bias), n1.eps)
        N = hidden.shape[1]
        idx = torch.from_numpy(np.unique(np.concatenate([np.arange(8), g.integers(0, N, n_rows)])))
        y_seg = (core(xn[:, idx.to(DEV)] @ wq.T, xn @ wk.T, xn @ wv.T, a.scale) @ wo.T + bo + x_all[:, idx.to(DEV)])
        pick = lambda t: f64(t)[:, idx.to(DEV)]
        cnd = f64(cond)
    # attn2 and the feed-forward are row-wise: apply them to the double segment rows
    a2, n2, n3 = blk.attn2, blk.norm2, blk.norm3
    yn = F_.layer_norm(y_seg, n2.normalized_shape, f64(n2.weight), f64(n2.bias), n2.eps)
    o2 = core(yn @ f64(a2.to_q.weight).T, cnd @ f64(a2.to_k.weight).T, cnd @ f64(a2.to_v.weight).T, a2.scale)
    y2 = o2 @ f64(a2.to_out[0].weight).T + f64(a2.to_out[0].bias) + y_seg
    yn3 = F_.layer_norm(y2, n3.normalized_shape, f64(n3.weight), f64(n3.bias), n3.eps)
    proj, lin = blk.ff.net[0].proj, blk.ff.net[2]
    z = yn3 @ f64(proj.weight).T + f64(proj.bias)
    D = z.shape[-1] // 2
    y3 = (z[..., :D] * _gelu64(z[..., D:])) @ f64(lin.weight).T + f64(lin.bias) + y2
    e_seg = float((pick(seg) - y_seg).abs().max()) / max(1.0, float(y_seg.abs().max()))
    e_blk = float((pick(out) - y3).abs().max()) / max(1.0, float(y3.abs().max()))
    return e_seg, e_blk


def _cfg2_run(flags, chunks=3):
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    from vidtome_amd import sites as S
    B, F, latent = 2, 16, (64, 64)
    unet, sl = _full_unet(("down0.0", "down1.0", "down2.0"), torch.float32, 3, B, latent, flags, local_merge_ratio=0.9,
                          merge_global=True, global_merge_ratio=0.8)
    segs, plans = {}, {}
    orig_seg, orig_cm = vpatch.self_attention_segment, vpatch.compute_merge

    def seg(block, h, *a, **k):
        segs[id(block)] = r = orig_seg(block, h, *a, **k)
        return r

    def cm(module, x, info, **kw):
        res = orig_cm(module, x, info, **kw)
        plans[id(module)] = getattr(res[0], "plan", None)
        return res
    vpatch.self_attention_segment, vpatch.compute_merge = seg, cm
    try:
        torch.manual_seed(123)
        for ck in range(chunks):
            hiddens = [S.synthetic_hidden(s, B, F, latent, torch.float32, DEV, seed=90 + 10 * ck + i) for i, s in enumerate(sl)]
            cond = _cond(B, F, 500 + ck)
            with torch.no_grad():
                outs = S.run_block_pass(unet, hiddens, cond)
    finally:
        vpatch.self_attention_segment, vpatch.compute_merge = orig_seg, orig_cm
    errs = []
    for i, blk in enumerate(unet.blocks):
        errs.append(_block_rows_vs_double(blk, plans[id(blk)], hiddens[i], segs[id(blk)], outs[i], cond, F, seed=i))
    kinds = [plans[id(b)] is not None for b in unet.blocks]
    vidtome_amd.remove_patch(unet)
    return errs, kinds


def test_cfg2_blocks_with_both_flags_vs_double(L):
    """2 x 16 frames, 64 x 64 latent, three chunks with global merging: top (d = 40), mid (d = 80), un-merged (d = 160)."""
    errs, kinds = _cfg2_run(dict(fp32_projections=True, fp32_attention=True))
    assert kinds == [True, True, False]
    print("segment / block error, both flags:", errs)
    for e_seg, e_blk in errs:
        assert e_seg <= 2e-5 and e_blk <= 5e-5, errs


def test_cfg2_blocks_with_fp32_projections_alone(L):
    """The fp16-core class: q / k / V^T rounded once to fp16 at the GEMM's store."""
    errs, _ = _cfg2_run(dict(fp32_projections=True), chunks=2)
    print("segment / block error, fp32_projections alone:", errs)
    for e_seg, e_blk in errs:
        assert e_seg <= 2e-3 and e_blk <= 2e-3, errs


@pytest.mark.parametrize("name", ["fullblock16_cfg_f4_d40", "fullblock16_pnp_f4_d64"])
def test_full_block_vs_reference_chain_fp32(L, name, monkeypatch):
    """The whole patched block of an fp32 model with both flags against the reference's recorded blocks (CPU fp32 run on an
    fp16-grid model whose norm1 output was rounded to the fp16 grid, tests/golden/make_golden_fullblock.py): block outputs
    within 1e-4 of the scale (the fp16 model's bar is 2e-3), anchors within one fp16 ulp.  PnP with aligned matching and shared
    probabilities included."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    from vidtome_amd import pnp
    from helpers import load_chain
    from inputs import portable_weight
    from standin import Pipe, StandInUNet, load_block_weights

    cfg, z = load_chain(name)
    keep = cfg["keep_blocks"]
    unet = load_block_weights(StandInUNet(cfg["C"], cfg["heads"], True, cfg["cond_dim"]), z, DEV, torch.float32,
                              portable=portable_weight)
    pipe = Pipe(unet)
    if cfg["injection"] is not None:
        pnp.register_attention_control(pipe, cfg["injection"], cfg["B"])
        pnp.register_time(pipe, cfg["t"])
    vidtome_amd.apply_patch(unet, local_merge_ratio=cfg["local_ratio"], merge_global=cfg["merge_global"],
                            global_merge_ratio=cfg["global_ratio"], batch_size=cfg["B"], align_batch=cfg["align"],
                            target_stride=4, global_rand=0.5)
    vidtome_amd.update_patch(unet, fp32_projections=True, fp32_attention=True)
    norm1s = {id(m.norm1) for m in unet.modules() if m.__class__.__name__ == "ToMeBlock"}
    orig_ln = vpatch.layer_norm
    monkeypatch.setattr(vpatch, "layer_norm", lambda norm, x: orig_ln(norm, x).half().float() if id(norm) in norm1s
                        else orig_ln(norm, x))
    calls = {"n": 0}
    orig_f32 = L.linear_f32

    def counted(*a, **k):
        calls["n"] += 1
        return orig_f32(*a, **k)
    monkeypatch.setattr(L, "linear_f32", counted)
    torch.set_rng_state(torch.from_numpy(z["rng_state"]))
    names = [str(s) for s in z["block_names"]]
    worst = 0.0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV).float()
    for ck, F in enumerate(cfg["chunk_frames"]):
        if ck in cfg.get("reset_before", []):
            vidtome_amd.update_patch(unet, global_tokens=None)
        hiddens = [(t(z[f"c{ck}/b{bi}/hidden"]) if bi in keep else None) for bi in range(9)]
        cond = t(z[f"c{ck}/cond"])
        cond = cond[:, None].expand(-1, F, -1, -1).reshape(cfg["B"] * F, cond.shape[1], cond.shape[2]).contiguous()
        latent = torch.zeros(tuple(int(v) for v in z[f"c{ck}/latent_shape"]), device=DEV, dtype=torch.float32)
        with torch.no_grad():
            outs = unet(latent, hiddens, encoder_hidden_states=cond, timestep=cfg["t"])
        for bi in keep:
            ref_out = z[f"c{ck}/b{bi}/out"]
            err = np.abs(outs[bi].cpu().numpy() - ref_out).max() / max(1.0, np.abs(ref_out).max())
            worst = max(worst, err)
            assert err < 1e-4, (name, ck, bi, err)
        gts = vidtome_amd.collect_from_patch(unet, attr="global_tokens")
        for nme in names:
            key = f"c{ck}/gt/{nme}"
            if key in z.files and gts.get(nme) is not None:
                # anchors are row copies of norm1's output on the fp16 grid: an fp32 LayerNorm value within rounding of a
                # grid midpoint lands one fp16 ulp (2^-11 relative) away from the recorded one, as the fixture notes
                err = np.abs(gts[nme].float().cpu().numpy() - z[key]).max() / max(1.0, np.abs(z[key]).max())
                assert err < 1e-3, (name, ck, nme, err)
    print(name, "worst block-output error / scale (fp32, both flags):", worst)
    assert calls["n"] > 0
    monkeypatch.undo()
    vidtome_amd.remove_patch(unet)


# ---------------------------------------------------------------------------------------------------
# invariance
# ---------------------------------------------------------------------------------------------------
def _torch_cross_forward(self, x, encoder_hidden_states=None, attention_mask=None):
    """What Diffusers' Attention computes for the stand-in's attn2 (which has no forward of its own): the path an fp32 block
    without ``fp32_projections`` takes through the module."""
    F_ = torch.nn.functional
    B, N, C = x.shape
    h = self.heads
    ctx = x if encoder_hidden_states is None else encoder_hidden_states
    sh = lambda t: t.reshape(B, -1, h, C // h).transpose(1, 2)
    o = F_.scaled_dot_product_attention(sh(self.to_q(x)), sh(self.to_k(ctx)), sh(self.to_v(ctx)), scale=self.scale)
    return self.to_out[0](o.transpose(1, 2).reshape(B, N, C))


@pytest.fixture
def cross_forward(monkeypatch):
    from vidtome_amd import sites as S
    monkeypatch.setattr(S.CrossAttention, "forward", _torch_cross_forward, raising=False)


def _small_pass(dtype, flags, seed=5):
    import vidtome_amd
    B, F, latent = 2, 4, (32, 32)
    unet, sl = _full_unet(("down0.0", "down1.0", "down2.0"), dtype, 4, B, latent, flags, merge_global=True)
    res = [o for _, outs in _block_passes(unet, sl, B, F, latent, dtype, 2, seed) for o in outs]
    vidtome_amd.remove_patch(unet)
    return res


def test_fp32_model_with_the_flag_off_is_unchanged(L, cross_forward):
    a = _small_pass(torch.float32, None)
    b = _small_pass(torch.float32, dict(fp32_projections=False))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = _small_pass(torch.float32, dict(fp32_projections=True))
    assert any(not torch.equal(x, y) for x, y in zip(a, c))               # the flag does change the arithmetic


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_16bit_models_ignore_the_flag(L, dtype, cross_forward):
    a = _small_pass(dtype, None)
    b = _small_pass(dtype, dict(fp32_projections=True, fp32_attention=True))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_run_step_with_streams_equals_the_sequential_loop(L):
    """With the flag, chunks issued on alternating HIP streams give the sequential loop's outputs and anchors bit for bit."""
    import vidtome_amd
    from vidtome_amd import scheduler as sch
    from vidtome_amd import sites as S
    B, latent, n_frames = 2, (32, 32), 10
    res = {}
    for use_streams in (False, True):
        unet, sl = _full_unet(("up3.0", "up2.0"), torch.float32, 6, B, latent,
                              dict(fp32_projections=True, fp32_attention=True), local_merge_ratio=0.5, merge_global=True,
                              global_merge_ratio=0.5)
        np.random.seed(3)
        torch.manual_seed(3)
        sc = sch.ChunkScheduler(chunk_size=4, merge_global=True, chunk_ord="seq")
        outs, anchors = {}, {}

        def process(chunk):
            F, f0 = len(chunk), int(chunk[0])
            hs = [S.synthetic_hidden(s_, B, F, latent, torch.float32, DEV, seed=500 + f0 + 31 * i, clip_seed=9 + i,
                                     regime="corr01") for i, s_ in enumerate(sl)]
            with torch.no_grad():
                outs[f0] = S.run_block_pass(unet, hs, _cond(B, F, 77))
            anchors[f0] = [b.global_tokens for b in unet.blocks]

        streams = [torch.cuda.Stream(), torch.cuda.Stream()] if use_streams else None
        sch.run_step(unet, sc, n_frames, process, streams=streams)
        torch.cuda.synchronize()
        res[use_streams] = (outs, anchors)
        vidtome_amd.remove_patch(unet)
    (oa, aa), (ob, ab) = res[False], res[True]
    assert sorted(oa) == sorted(ob) and len(oa) > 1
    for f0 in oa:
        assert all(torch.equal(x, y) for x, y in zip(oa[f0], ob[f0]))
        assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(aa[f0], ab[f0]))


def test_lora_fp32_block_matches_its_folded_restatement(L):
    """A LoRA-adapted fp32 block with the flag takes its folded fp32 weights (lora.linear_params): its outputs equal, bit for
    bit, those of the twin whose Linears hold vtm_lora_fold's outputs as plain weights (the same fp32 GEMMs read the same
    values), and dropping the adapters is far outside the bar."""
    import vidtome_amd
    from lora_standin import folded_twin, wrap_lora
    from vidtome_amd import sites as S
    B, F, latent = 2, 4, (32, 32)
    sl = [s for s in S.sd15_sites() if s.name in ("down0.0", "down1.0")]
    base = S.SiteUNet(sl, seed=8, full=True).to(device=DEV, dtype=torch.float32)
    unet = S.SiteUNet(sl, seed=8, full=True).to(device=DEV, dtype=torch.float32)
    wrapped = wrap_lora(unet, ranks=(16,), seed=11)
    assert len(wrapped) == len(sl) * 10
    twin = folded_twin(unet)
    res = []
    for model in (unet, twin, base):
        vidtome_amd.apply_patch(model, batch_size=B, merge_global=True)
        vidtome_amd.update_patch(model, fp32_projections=True, fp32_attention=True)
        model.set_size(latent)
        res.append(_block_passes(model, sl, B, F, latent, torch.float32, 2, seed=21))
        vidtome_amd.remove_patch(model)
    for (_, oa), (_, ob), (_, oc) in zip(*res):
        for x, y, z in zip(oa, ob, oc):
            assert torch.equal(x, y)
            assert float((x - z).abs().max()) > 1e-3 * max(1.0, float(z.abs().max()))
