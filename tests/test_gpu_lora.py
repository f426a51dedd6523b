"""GPU tests of LoRA-adapted blocks on the HIP path (run with -m gpu on an MI355X): vtm_lora_fold against a float64 host
fold, the patched block with LoRA layers against its folded twin (bit for bit, every projection path), against a float64
oracle built from host-folded weights, against the module path, across adapter-state changes, streams and PnP."""
import functools

import numpy as np
import pytest
import torch

import standin
from lora_standin import (PeftLinear, SDPAAttention, folded_twin, host_fold, refold_twin, wrap_lora)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG2 = dict(B=2, F=16, latent=(64, 64))          # SD-1.5, 16 frames at 512 x 512


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


# ---------------------------------------------------------------------------------------------------
# 1. the fold kernel
# ---------------------------------------------------------------------------------------------------
def _ulp(x: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of `dtype` at the float64 values x."""
    p, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}[dtype]
    _, e = torch.frexp(x)
    e = torch.where(x == 0, torch.full_like(e, emin), (e - 1).clamp_min(emin))
    return torch.ldexp(torch.ones_like(x), (e - p).to(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_fold_kernel_vs_float64_host_fold(L, dtype):
    """out = round(W + up @ down) at the projection shapes of SD-1.5 (320^2, 640^2, 1280^2, the GEGLU projection
    10 240 x 1280, attn2's k / v 320 x 768 and 1280 x 1024), r = 4, 12, 64 and 256 (two adapters of 128) against the float64
    fold: fp32 within the a-priori bound of an (r + 1)-term fp32 sum, (r + 1) 2^-24 of the element's magnitude bound
    |W| + |up| @ |down| (2^-22 flat was measured to be exceeded by 0.3 % at r = 12 and 4 % at r = 256); fp16 / bf16 within one
    ulp of the output dtype on top of that (elements that cancel to almost nothing carry the fp32 sum's error, not a 16-bit
    one)."""
    g = torch.Generator().manual_seed(0)
    for co, ci in ((320, 320), (640, 640), (1280, 1280), (10240, 1280), (320, 768), (1280, 1024)):
        for r in (4, 12, 64, 256):
            W = (torch.randn(co, ci, generator=g) * ci ** -0.5).to(dtype).to(DEV)
            ups, downs = [], []
            for rr in ((128, 128) if r == 256 else (r,)):
                A = (torch.randn(rr, ci, generator=g) * ci ** -0.5).to(dtype)
                B = (torch.randn(co, rr, generator=g) * rr ** -0.5 * 0.4).to(dtype)
                ups.append(B.float() * 0.75)
                downs.append(A.float())
            up, down = torch.cat(ups, 1).contiguous().to(DEV), torch.cat(downs, 0).contiguous().to(DEV)
            got = L.lora_fold(W, up, down)
            assert got.dtype == dtype and got.shape == W.shape
            ref = W.double() + up.double() @ down.double()
            err = (got.double() - ref).abs()
            bound = (r + 1) * 2.0 ** -24 * (W.double().abs() + up.double().abs() @ down.double().abs())
            if dtype != torch.float32:
                bound = bound + _ulp(ref, dtype)
            assert bool((err <= bound).all()), (co, ci, r, float((err / bound).max()))
    lib, s = L.lib(), torch.cuda.current_stream().cuda_stream
    W = torch.zeros(64, 64, dtype=dtype, device=DEV)
    up, down, out = torch.zeros(64, 4, device=DEV), torch.zeros(4, 64, device=DEV), torch.empty_like(W)
    p = lambda t: t.data_ptr()
    code = L.dtype_code(W)
    assert lib.vtm_lora_fold(p(W), code, p(up), p(down), 64, 64, 4, p(out), s) == 0
    for args in ((0, 64, 4), (64, 0, 4), (64, 64, 0), (-1, 64, 4), (64, 64, -4), (64 * 70000, 64, 4)):
        assert lib.vtm_lora_fold(p(W), code, p(up), p(down), *args, p(out), s) == -1, args
    assert lib.vtm_lora_fold(p(W), 7, p(up), p(down), 64, 64, 4, p(out), s) == -1
    assert lib.vtm_lora_fold(p(W), code, p(up), None, 64, 64, 4, p(out), s) == -1
    assert lib.vtm_lora_fold(p(W), code, p(up), p(down), 64, 64, 4, None, s) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------
def _hidden(sl, B, F, latent, dtype, ck, seed0=0):
    from vidtome_amd import sites as S
    return [S.synthetic_hidden(s, B, F, latent, dtype, DEV, seed=seed0 + 10 * ck + i, clip_seed=7 + i, regime="corr01")
            for i, s in enumerate(sl)]


def _cond(B, F, dtype):
    return torch.randn(B * F, 77, 768, generator=torch.Generator().manual_seed(3)).to(device=DEV, dtype=dtype)


def _run(unet, sl, B, F, latent, dtype, full, n_chunks=3, seed0=0):
    """Chunks of one clip through the patched sites; chunk 1 has the local chunk on the src side of the global level
    (live / compacted queries, anchors with content ids), chunk 2 on the dst side (duplicate-key folding at d = 40)."""
    from vidtome_amd import sites as S
    torch.manual_seed(123)
    for blk in unet.blocks:                  # a fresh run: generators forked again from the seed, no anchors
        blk.__dict__.pop("generator", None)
        blk.global_tokens = None
    cond = _cond(B, F, dtype) if full else None
    outs = []
    with torch.no_grad():
        for ck in range(n_chunks):
            unet._tome_info["args"]["global_rand"] = [0.5, 0.0, 1.0][ck % 3]
            hs = _hidden(sl, B, F, latent, dtype, ck, seed0)
            outs.append([o.clone() for o in (S.run_block_pass(unet, hs, cond) if full else S.run_segment_pass(unet, hs))])
    return outs


def _patch(unet, B, latent, **kw):
    import vidtome_amd
    vidtome_amd.apply_patch(unet, local_merge_ratio=0.5, merge_global=True, global_merge_ratio=0.5, batch_size=B, **kw)
    unet.set_size(latent)
    return unet


def _site_list(*names):
    from vidtome_amd import sites as S
    return [s for s in S.sd15_sites() if s.name in names]


# ---------------------------------------------------------------------------------------------------
# 2. plumbing: a LoRA block equals its folded twin bit for bit on every path
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,dtype", [("default", torch.float16), ("blas", torch.float16), ("default", torch.bfloat16),
                                        ("default", torch.float32)])
def test_lora_block_equals_its_folded_twin_bitwise(L, mode, dtype, monkeypatch):
    """Full cfg-2 sizes, top (C = 320: vtm_linear_rows, live queries, key folding), mid (C = 640: panels) and the un-merged
    C = 1280 site, whole blocks (fused attn2, panel feed-forward); "blas" = VIDTOME_PROJ=blas / VIDTOME_FF=blas; fp32
    models (segment only: their attn2 is the module's own business either way).  Three chunks, every output bit-equal to
    the plain model whose Linears hold vtm_lora_fold's outputs -- except under "blas", whose library GEMMs did not reproduce
    their own last bits from one run of the same model to the next (a different site differed in each of two GPU runs):
    there the LoRA block must stay within twice the spread of two runs of the twin itself, or 2e-3 of the output scale."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    from vidtome_amd import sites as S
    if mode == "blas":
        monkeypatch.setattr(vpatch, "PROJ_MODE", "blas")
        monkeypatch.setattr(vpatch, "FUSED_PROJ", False)
        monkeypatch.setattr(vpatch, "FF_MODE", "blas")
    full = dtype != torch.float32
    sl = _site_list("up3.0", "up2.0", "up1.0") if full else _site_list("up3.0", "up2.0")
    B, F, latent = CFG2["B"], CFG2["F"], CFG2["latent"]
    base = S.SiteUNet(sl, seed=0, full=full).to(device=DEV, dtype=dtype)
    unet = S.SiteUNet(sl, seed=0, full=full).to(device=DEV, dtype=dtype)
    wrapped = wrap_lora(unet, ranks=(64,), seed=1)
    assert len(wrapped) == len(sl) * (10 if full else 4)
    twin = folded_twin(unet)
    res = {}
    for name, model in (("lora", unet), ("twin", twin)) + ((("base", base),) if mode == "default" and dtype == torch.float16
                                                           else ()):
        _patch(model, B, latent)
        res[name] = _run(model, sl, B, F, latent, dtype, full)
        if name == "twin" and mode == "blas":
            res["twin2"] = _run(model, sl, B, F, latent, dtype, full)
        vidtome_amd.remove_patch(model)
    for ck in range(3):
        for i, (a, b) in enumerate(zip(res["lora"][ck], res["twin"][ck])):
            assert bool(torch.isfinite(a).all()), (ck, sl[i].name)
            if mode == "blas":
                spread = float((res["twin2"][ck][i].float() - b.float()).abs().max())
                assert float((a.float() - b.float()).abs().max()) <= max(2 * spread, 2e-3 * float(b.abs().max())), ck
            else:
                assert torch.equal(a, b), (ck, sl[i].name)
    if "base" in res:                       # the adapters are not noise: dropping them is far outside any tolerance
        for a, b in zip(res["lora"][2], res["base"][2]):
            assert (a.float() - b.float()).abs().max() > 10 * 2e-3 * max(1.0, float(b.abs().max()))
    assert all("_vtm_lora" not in m.__dict__ for m in wrapped)      # remove_patch dropped the folded copies


# ---------------------------------------------------------------------------------------------------
# 3. the fused path runs for LoRA blocks (the module forward raises) and matches a float64 oracle
# ---------------------------------------------------------------------------------------------------
class _StandInSites(standin.ModelMixin):
    """Sites of tests/standin.py blocks (whose Attention.forward raises), initialised like sites.SiteUNet."""

    def __init__(self, sl, full, seed=0):
        super().__init__()
        self.blocks = torch.nn.ModuleList([standin.BasicTransformerBlock(s.channels, s.heads, full, 768) for s in sl])
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in self.parameters():
                if p.ndim == 2:
                    p.copy_(torch.randn(p.shape, generator=g) * p.shape[-1] ** -0.5)

    def set_size(self, latent_hw):
        self._tome_info["size"] = latent_hw


def _attn_rows(q, k, v, heads, scale):
    B, S, C = q.shape
    d = C // heads
    sh = lambda t: t.view(B, t.shape[1], heads, d).transpose(1, 2)
    p = torch.softmax(sh(q) @ sh(k).transpose(-1, -2) * scale, dim=-1)
    return (p @ sh(v)).transpose(1, 2).reshape(B, S, C)


def _oracle_rows(blk, plan, hidden, cond, fsize, idx, fold, full):
    """float64 block outputs at the joined-chunk positions idx from host-folded weights (`fold(module)` -> (W, b)):
    to_out(softmax(q K^T) V)[inv[i]] + hidden[i] from the merged tokens the plan selects (our norm1 output), then for a
    whole block norm2 / attn2 over the conditioning / norm3 / GEGLU feed-forward."""
    from vidtome_amd.utils import join_frame
    a = blk.attn1
    fold = functools.lru_cache(maxsize=None)(fold)
    lin = lambda m, x: x @ fold(m)[0].T + (0 if fold(m)[1] is None else fold(m)[1])
    merged = plan.merged[:, :plan.M].double().cpu()
    m = plan.inv.cpu()[:, idx]
    xq = torch.stack([merged[b, m[b]] for b in range(merged.shape[0])])
    o = _attn_rows(lin(a.to_q, xq), lin(a.to_k, merged), lin(a.to_v, merged), a.heads, a.scale)
    h = lin(a.to_out[0], o) + join_frame(hidden, fsize).double().cpu()[:, idx]
    if not full:
        return h
    ln = lambda n, x: torch.nn.functional.layer_norm(x, x.shape[-1:], n.weight.double().cpu(), n.bias.double().cpu(), n.eps)
    N = hidden.shape[1]
    Bn = h.shape[0]
    c = cond.double().cpu().view(Bn, fsize, cond.shape[1], cond.shape[2])
    frame = torch.as_tensor(idx) // N
    a2 = blk.attn2
    x2 = ln(blk.norm2, h)
    o2 = torch.empty_like(h)
    for b in range(Bn):                                 # every sampled row attends to the conditioning of its own frame
        for f in frame.unique().tolist():
            sel = (frame == f).nonzero().flatten()
            kf, vf = lin(a2.to_k, c[b, f]), lin(a2.to_v, c[b, f])
            o2[b, sel] = _attn_rows(lin(a2.to_q, x2[b, sel])[None], kf[None], vf[None], a2.heads, a2.scale)[0]
    h2 = lin(a2.to_out[0], o2) + h
    p = lin(blk.ff.net[0].proj, ln(blk.norm3, h2))
    D = p.shape[-1] // 2
    return lin(blk.ff.net[2], p[..., :D] * torch.nn.functional.gelu(p[..., D:])) + h2


def _capture_plans(monkeypatch):
    from vidtome_amd import patch as vpatch
    seen, orig = {}, vpatch.compute_merge

    def rec(module, x, info, **kw):
        res = orig(module, x, info, **kw)
        seen[id(module)] = res[0].plan
        return res
    monkeypatch.setattr(vpatch, "compute_merge", rec)
    return seen


@pytest.mark.parametrize("full,dtype,tol", [(False, torch.float16, 1e-3), (True, torch.float16, 2e-3),
                                            (True, torch.bfloat16, 8e-3)])
def test_fused_lora_block_vs_float64_oracle(L, full, dtype, tol, monkeypatch):
    """LoRA on every projection of blocks whose Attention.forward raises: apply_patch + a 3-chunk steady state runs on the
    fused path (at the parent commit the wrapped projections sent the block to the module) and matches a float64 oracle
    built from weights folded on the host, on sampled rows: 1e-3 of the output scale for the segment, 2e-3 for the whole
    block, 8e-3 for bf16.  The oracle with the adapters dropped misses the same bound by more than 10x."""
    import vidtome_amd
    from vidtome_amd import sites as S
    from vidtome_amd.utils import join_frame
    sl = _site_list("up3.0", "up2.0")
    B, F, latent = 2, 4, (32, 32)
    unet = _StandInSites(sl, full).to(device=DEV, dtype=dtype)
    assert len(wrap_lora(unet, ranks=(64,), seed=2)) == len(sl) * (10 if full else 4)
    seen = _capture_plans(monkeypatch)
    _patch(unet, B, latent)
    torch.manual_seed(123)
    cond = _cond(B, F, dtype) if full else None
    g = np.random.default_rng(0)
    base_fold = lambda m: (lambda bl: (bl.weight.detach().double().cpu(),
                                       None if bl.bias is None else bl.bias.detach().double().cpu()))(
        m.base_layer if isinstance(m, PeftLinear) else m)
    with torch.no_grad():
        for ck in range(3):
            unet._tome_info["args"]["global_rand"] = [0.5, 0.0, 1.0][ck]
            hs = _hidden(sl, B, F, latent, dtype, ck, seed0=40)
            outs = S.run_block_pass(unet, hs, cond) if full else S.run_segment_pass(unet, hs)
            if ck == 0:
                continue
            for blk, h, o in zip(unet.blocks, hs, outs):
                plan = seen[id(blk)]
                assert plan.global_level is not None
                Lj = plan.L
                idx = np.unique(np.concatenate([np.arange(8), np.arange(Lj - 8, Lj), g.integers(0, Lj, 160)]))
                ref = _oracle_rows(blk, plan, h, cond, F, idx, host_fold, full)
                got = join_frame(o, F).double().cpu()[:, idx]
                scale = max(1.0, float(ref.abs().max()))
                err = float((got - ref).abs().max())
                assert err < tol * scale, (ck, err / scale)
                drop = float((got - _oracle_rows(blk, plan, h, cond, F, idx, base_fold, full)).abs().max())
                assert drop > 10 * tol * scale, (ck, drop / scale)
    vidtome_amd.remove_patch(unet)


# ---------------------------------------------------------------------------------------------------
# 4. semantics: the fused LoRA block agrees with the module path (PEFT with two adapters, legacy layers)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["peft", "legacy"])
def test_fused_lora_block_agrees_with_the_module_path(L, kind, monkeypatch):
    """4 frames, C = 320 and 640, whole blocks with computing (SDPA) attention modules: the fused path with folded weights
    against the module path (the recogniser forced to refuse the LoRA layers: the modules' own forwards, adapters applied
    by the layers themselves), within 2e-3 of the output scale; the unadapted block is > 10x further away."""
    import vidtome_amd
    from vidtome_amd import lora
    from vidtome_amd import sites as S
    sl = _site_list("up3.0", "up2.0")
    B, F, latent = 2, 4, (32, 32)
    res = {}
    for path in ("fused", "module", "base"):
        unet = S.SiteUNet(sl, seed=0, full=True).to(device=DEV, dtype=torch.float16)
        for blk in unet.blocks:
            blk.attn1, blk.attn2 = SDPAAttention(blk.attn1), SDPAAttention(blk.attn2)
        if path != "base":
            wrap_lora(unet, kind=kind, ranks=(32, 16) if kind == "peft" else (48,), seed=3)
        orig = lora.recognise
        if path == "module":
            monkeypatch.setattr(lora, "recognise", lambda m: orig(m) if orig(m) == lora.PLAIN else None)
        res[path] = _run(_patch(unet, B, latent), sl, B, F, latent, torch.float16, True)
        monkeypatch.setattr(lora, "recognise", orig)
        vidtome_amd.remove_patch(unet)
    for ck in range(3):
        for a, b, c in zip(res["fused"][ck], res["module"][ck], res["base"][ck]):
            scale = max(1.0, float(b.abs().max()))
            assert float((a.float() - b.float()).abs().max()) < 2e-3 * scale, ck
            assert float((c.float() - b.float()).abs().max()) > 10 * 2e-3 * scale, ck


# ---------------------------------------------------------------------------------------------------
# 5. adapter-state changes
# ---------------------------------------------------------------------------------------------------
def test_adapter_state_changes_rebuild_the_fold(L):
    """scaling = 0 and disable_adapters equal the unadapted block bit for bit; after merge() the block equals the twin
    holding the merged weight (the adapter counted once) and after unmerge() the twin of the restored fold; a scaling
    change between two forwards gives the new fold's output; remove_patch drops the folded weights."""
    import vidtome_amd
    from vidtome_amd import sites as S
    sl = _site_list("up3.0", "up2.0")
    B, F, latent = 2, 4, (32, 32)
    base = _patch(S.SiteUNet(sl, seed=0, full=True).to(device=DEV, dtype=torch.float16), B, latent)
    unet = S.SiteUNet(sl, seed=0, full=True).to(device=DEV, dtype=torch.float16)
    wrapped = wrap_lora(unet, ranks=(32, 16), seed=4)
    twin = _patch(folded_twin(unet), B, latent)
    _patch(unet, B, latent)
    run = lambda model: _run(model, sl, B, F, latent, torch.float16, True, n_chunks=2)
    eq = lambda x, y: all(torch.equal(a, b) for ca, cb in zip(x, y) for a, b in zip(ca, cb))
    want_base = run(base)
    first = run(unet)
    assert eq(first, run(twin)) and not eq(first, want_base)
    assert all("_vtm_lora" in m.__dict__ for m in wrapped)
    for m in wrapped:
        m.scaling["a0"], m.scaling["a1"] = 0.0, 0.0
    assert eq(run(unet), want_base)
    for m in wrapped:
        m.scaling["a0"], m.scaling["a1"] = 0.5, 0.5
        m.enable_adapters(False)
    assert eq(run(unet), want_base)
    for m in wrapped:
        m.enable_adapters(True)
    assert eq(run(unet), first)
    for m in wrapped:
        m.merge()
    refold_twin(twin, unet)                  # the twin now holds the merged base weights
    merged = run(unet)
    assert eq(merged, run(twin))
    for m in wrapped:
        m.unmerge()
    refold_twin(twin, unet)
    assert eq(run(unet), run(twin))
    for m in wrapped:
        m.scaling["a1"] = 1.25
    refold_twin(twin, unet)
    changed = run(unet)
    assert eq(changed, run(twin)) and not eq(changed, first)
    for model in (base, twin, unet):
        vidtome_amd.remove_patch(model)
    assert all("_vtm_lora" not in m.__dict__ for m in wrapped)


# ---------------------------------------------------------------------------------------------------
# 6. streams and PnP
# ---------------------------------------------------------------------------------------------------
def test_lora_run_step_with_streams_equals_the_sequential_loop(L):
    """scheduler.run_step(streams=[s0, s1]) with LoRA layers and COLD caches (the first chunk folds on s0, the next chunk's
    stream waits for the fold on the device): outputs, anchors and generator states bit-equal to the sequential loop."""
    import vidtome_amd
    from vidtome_amd import scheduler as sch
    from vidtome_amd import sites as S
    B, latent, n_frames = 2, (32, 32), 14
    sl = [S.Site("up3.0", 1, 320, 8), S.Site("up2.0", 2, 640, 8)]
    res = {}
    for use_streams in (False, True):
        unet = S.SiteUNet(sl, seed=6).to(device=DEV, dtype=torch.float16)
        wrap_lora(unet, ranks=(64,), seed=5)
        _patch(unet, B, latent)
        np.random.seed(3)
        torch.manual_seed(3)
        sc = sch.ChunkScheduler(chunk_size=4, merge_global=True, chunk_ord="seq")
        outs, anchors = {}, {}

        def process(chunk):
            F, f0 = len(chunk), int(chunk[0])
            hs = [S.synthetic_hidden(s_, B, F, latent, torch.float16, DEV, seed=500 + f0 + 31 * i, clip_seed=9 + i,
                                     regime="corr01") for i, s_ in enumerate(sl)]
            with torch.no_grad():
                outs[f0] = S.run_segment_pass(unet, hs)
            anchors[f0] = [b.global_tokens for b in unet.blocks]

        streams = [torch.cuda.Stream(), torch.cuda.Stream()] if use_streams else None
        for _ in range(2):
            sch.run_step(unet, sc, n_frames, process, streams=streams)
        torch.cuda.synchronize()
        res[use_streams] = ({k: [o.float().cpu() for o in v] for k, v in outs.items()},
                            {k: [a.float().cpu() for a in v] for k, v in anchors.items()},
                            [b.generator.get_state() for b in unet.blocks])
        vidtome_amd.remove_patch(unet)
    assert res[False][0].keys() == res[True][0].keys()
    for k in res[False][0]:
        for a, b in zip(res[False][0][k] + res[False][1][k], res[True][0][k] + res[True][1][k]):
            assert torch.equal(a, b), k
    for a, b in zip(res[False][2], res[True][2]):
        assert torch.equal(a, b)


def test_lora_pnp_top_block_takes_the_shared_probability_kernel(L, monkeypatch):
    """A cfg-3-shaped PnP top block (batch 3 [source | uncond | cond], align_batch, 16 frames at 512 x 512) with LoRA
    layers runs the shared-probability attention on the fused path and equals its folded twin bit for bit."""
    import vidtome_amd
    from vidtome_amd import _lib
    from vidtome_amd import sites as S
    B, F, latent = 3, 16, (64, 64)
    sl = _site_list("up3.0")
    unet = S.SiteUNet(sl, seed=2).to(device=DEV, dtype=torch.float16)
    wrap_lora(unet, ranks=(64,), seed=6)
    twin = folded_twin(unet)
    shared = []
    orig_kv, orig_att = _lib.attention_kv, _lib.attention

    def spy_kv(*a, **kw):
        shared.append(kw.get("share_groups", 1))
        return orig_kv(*a, **kw)

    def spy_att(q, k, vt, heads, M, scale, share=1, *a, **kw):
        shared.append(share)
        return orig_att(q, k, vt, heads, M, scale, share, *a, **kw)
    monkeypatch.setattr(_lib, "attention_kv", spy_kv)
    monkeypatch.setattr(_lib, "attention", spy_att)
    res = {}
    for name, model in (("lora", unet), ("twin", twin)):
        for blk in model.blocks:
            blk.attn1.injection_schedule, blk.attn1.t, blk.attn1.vtm_num_inputs = [981], 981, B
        shared.clear()
        res[name] = _run(_patch(model, B, latent, align_batch=True), sl, B, F, latent, torch.float16, False, n_chunks=2)
        assert shared and all(s == B for s in shared), shared
        vidtome_amd.remove_patch(model)
    for ca, cb in zip(res["lora"], res["twin"]):
        for a, b in zip(ca, cb):
            assert torch.equal(a, b)
