"""GPU tests of DoRA-adapted blocks on the HIP path (run with -m gpu on an MI355X): vtm_dora_norms / vtm_dora_fold against
float64, the patched block with DoRA layers (a first DoRA adapter, optionally a plain one after it) on the fused path
against a float64 oracle, against its folded twin bit for bit, against the module path, and across adapter-state changes."""
import numpy as np
import pytest
import torch

from dora_standin import folded_twin_dora, host_fold_dora, refold_twin_dora, wrap_dora
from lora_standin import SDPAAttention
from test_gpu_lora import CFG2, _capture_plans, _cond, _hidden, _oracle_rows, _patch, _run, _site_list, _StandInSites, _ulp

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24                           # fp32 unit roundoff


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


# ---------------------------------------------------------------------------------------------------
# 1. the norm and fold kernels
# ---------------------------------------------------------------------------------------------------
def _operands(co, ci, kd, kp, dtype, g):
    """W (co, ci) in dtype, up / down with the DoRA adapter's kd columns / rows first and kp plain ones after, the magnitudes
    ||W||_row perturbed by 5 %."""
    W = (torch.randn(co, ci, generator=g) * ci ** -0.5).to(dtype)
    ups, downs = [], []
    for rr, s in ((kd, 0.5), (kp, 0.75)):
        if rr:
            downs.append((torch.randn(rr, ci, generator=g) * ci ** -0.5).to(dtype).float())
            ups.append((torch.randn(co, rr, generator=g) * rr ** -0.5 * 0.4).to(dtype).float() * s)
    mag = (W.float().norm(dim=1) * (1 + 0.05 * torch.randn(co, generator=g))).to(dtype).float()
    return (W.to(DEV), torch.cat(ups, 1).contiguous().to(DEV), torch.cat(downs, 0).contiguous().to(DEV), mag.to(DEV))


def _bounds(W, up, down, mag, kd):
    """float64 (norms, fold) and their a-priori fp32 error bounds (see the test's docstring)."""
    W, up, down, mag = W.double(), up.double(), down.double(), mag.double()
    c_in, r = W.shape[1], up.shape[1]
    v = W + up[:, :kd] @ down[:kd]
    Ev = (kd + 1) * U * (W.abs() + up[:, :kd].abs() @ down[:kd].abs())
    S = (v * v).sum(1)
    dS = c_in * U * ((v.abs() + Ev) ** 2).sum(1) * 1.001 + (2 * v.abs() * Ev + Ev * Ev).sum(1)
    n = S.sqrt()
    rho_n = dS / S + 2 * U
    rho_r = (rho_n * 1.01 + U)[:, None]
    rr = (mag / n)[:, None]
    p = up[:, kd:] @ down[kd:] if r > kd else torch.zeros_like(W)
    Ep = (r - kd) * U * (up[:, kd:].abs() @ down[kd:].abs()) if r > kd else torch.zeros_like(W)
    t = rr.abs() * (1 + rho_r) * (v.abs() + Ev)
    bound = rr.abs() * (rho_r * (v.abs() + Ev) + Ev) + U * t + Ep + U * (t * (1 + U) + p.abs() + Ep)
    return n, rho_n * n, rr * v + p, bound


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_dora_kernels_vs_float64(L, dtype):
    """vtm_dora_norms and vtm_dora_fold at the projection shapes of SD-1.5 (320^2, 640^2, 1280^2, the GEGLU projection
    10 240 x 1280, attn2's k / v 320 x 768 and 1280 x 1024) and two shapes that are not multiples of 64, DoRA ranks 4, 64
    and 128, alone and with a trailing plain adapter of rank 16, against float64.  A-priori bounds, u = 2^-24: an element
    v = w + s_d B_d A_d carries Ev = (k_dora + 1) u (|w| + |up| |down|) (the fold kernel's bound); the sum of squares
    c_in u sum (|v| + Ev)^2 + sum (2 |v| Ev + Ev^2); the norm that relative error + 2u; r = m / n that + u; the output
    |r| (rho_r (|v| + Ev) + Ev), one rounding of the product and one of the sum, the plain chain (r - k_dora) u |up||down|;
    16-bit outputs one ulp of the output dtype on top.  A second call gives the same bits; bad arguments return -1."""
    g = torch.Generator().manual_seed(0)
    shapes = ((320, 320), (640, 640), (1280, 1280), (10240, 1280), (320, 768), (1280, 1024), (200, 333), (77, 1000))
    for co, ci in shapes:
        for kd in (4, 64, 128):
            for kp in (0, 16):
                W, up, down, mag = _operands(co, ci, kd, kp, dtype, g)
                norms = L.dora_norms(W, up, down, kd)
                got = L.dora_fold(W, up, down, mag, kd, norms=norms)
                assert got.dtype == dtype and got.shape == W.shape and norms.shape == (co,)
                n, n_bound, ref, bound = _bounds(W, up, down, mag, kd)
                err_n = (norms.double() - n).abs()
                assert bool((err_n <= n_bound).all()), (co, ci, kd, kp, float((err_n / n_bound).max()))
                if dtype != torch.float32:
                    bound = bound + _ulp(ref, dtype)
                err = (got.double() - ref).abs()
                assert bool((err <= bound).all()), (co, ci, kd, kp, float((err / bound).max()))
                assert torch.equal(L.dora_norms(W, up, down, kd), norms)
                assert torch.equal(L.dora_fold(W, up, down, mag, kd), got)
    lib, s = L.lib(), torch.cuda.current_stream().cuda_stream
    W = torch.zeros(64, 64, dtype=dtype, device=DEV)
    up, down, out = torch.zeros(64, 4, device=DEV), torch.zeros(4, 64, device=DEV), torch.empty_like(W)
    mag, nrm = torch.ones(64, device=DEV), torch.ones(64, device=DEV)
    p = lambda t: t.data_ptr()
    code = L.dtype_code(W)
    assert lib.vtm_dora_norms(p(W), code, p(up), p(down), 64, 64, 4, 2, p(nrm), s) == 0
    assert lib.vtm_dora_fold(p(W), code, p(up), p(down), p(mag), p(nrm), 64, 64, 4, 2, p(out), s) == 0
    for args in ((0, 64, 4, 2), (64, 0, 4, 2), (64, 64, 0, 0), (-1, 64, 4, 2), (64, 64, -4, 2), (64, 64, 4, 0),
                 (64, 64, 4, 5), (64, 64, 4, -1), (64 * 70000, 64, 4, 2)):
        assert lib.vtm_dora_norms(p(W), code, p(up), p(down), *args, p(nrm), s) == -1, args
        assert lib.vtm_dora_fold(p(W), code, p(up), p(down), p(mag), p(nrm), *args, p(out), s) == -1, args
    assert lib.vtm_dora_norms(p(W), 7, p(up), p(down), 64, 64, 4, 2, p(nrm), s) == -1
    assert lib.vtm_dora_fold(p(W), 7, p(up), p(down), p(mag), p(nrm), 64, 64, 4, 2, p(out), s) == -1
    assert lib.vtm_dora_norms(p(W), code, p(up), p(down), 64, 64, 4, 2, None, s) == -1
    assert lib.vtm_dora_norms(p(W), code, None, p(down), 64, 64, 4, 2, p(nrm), s) == -1
    for i in range(6):
        ptrs = [p(W), p(up), p(down), p(mag), p(nrm), p(out)]
        ptrs[i] = None
        assert lib.vtm_dora_fold(ptrs[0], code, ptrs[1], ptrs[2], ptrs[3], ptrs[4], 64, 64, 4, 2, ptrs[5], s) == -1, i
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# 2. the fused path runs for DoRA blocks (the module forward raises) and matches a float64 oracle
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full,dtype,tol", [(False, torch.float16, 1e-3), (True, torch.float16, 2e-3),
                                            (True, torch.bfloat16, 8e-3)])
@pytest.mark.parametrize("trailing", [None, 16])
def test_fused_dora_block_vs_float64_oracle(L, full, dtype, tol, trailing, monkeypatch):
    """DoRA on every projection of blocks whose Attention.forward raises: apply_patch + a 3-chunk steady state runs on the
    fused path (at the parent commit a DoRA layer sent the block to the module, which raises here) and matches a float64
    oracle built from host_fold_dora weights on sampled rows: 1e-3 of the output scale for the segment, 2e-3 for the whole
    block, 8e-3 for bf16.  The same oracle with the magnitudes ignored (r = 1) misses the bound by more than 5x."""
    import vidtome_amd
    from vidtome_amd import sites as S
    from vidtome_amd.utils import join_frame
    sl = _site_list("up3.0", "up2.0")
    B, F, latent = 2, 4, (32, 32)
    unet = _StandInSites(sl, full).to(device=DEV, dtype=dtype)
    assert len(wrap_dora(unet, rank=64, trailing=trailing, seed=2)) == len(sl) * (10 if full else 4)
    seen = _capture_plans(monkeypatch)
    _patch(unet, B, latent)
    torch.manual_seed(123)
    cond = _cond(B, F, dtype) if full else None
    g = np.random.default_rng(0)
    no_mag = lambda m: host_fold_dora(m, magnitude=False)
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
                ref = _oracle_rows(blk, plan, h, cond, F, idx, host_fold_dora, full)
                got = join_frame(o, F).double().cpu()[:, idx]
                scale = max(1.0, float(ref.abs().max()))
                err = float((got - ref).abs().max())
                assert err < tol * scale, (ck, err / scale)
                miss = float((got - _oracle_rows(blk, plan, h, cond, F, idx, no_mag, full)).abs().max())
                assert miss > 5 * tol * scale, (ck, miss / scale)
    vidtome_amd.remove_patch(unet)


# ---------------------------------------------------------------------------------------------------
# 3. plumbing: a DoRA block equals its folded twin bit for bit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,container,trailing", [(torch.float16, "module", None), (torch.float16, "param", 16),
                                                      (torch.bfloat16, "module", 16), (torch.float32, "param", None)])
def test_dora_block_equals_its_folded_twin_bitwise(L, dtype, container, trailing):
    """Full cfg-2 sizes, top (C = 320), mid (C = 640) and the un-merged C = 1280 site as whole blocks (fp32 models: the
    segment), three chunks: every output bit-equal to the plain model whose Linears hold vtm_dora_fold's outputs."""
    import vidtome_amd
    from vidtome_amd import sites as S
    full = dtype != torch.float32
    sl = _site_list("up3.0", "up2.0", "up1.0") if full else _site_list("up3.0", "up2.0")
    B, F, latent = CFG2["B"], CFG2["F"], CFG2["latent"]
    unet = S.SiteUNet(sl, seed=0, full=full).to(device=DEV, dtype=dtype)
    wrapped = wrap_dora(unet, rank=64, trailing=trailing, container=container, seed=1)
    twin = folded_twin_dora(unet)
    res = {}
    for name, model in (("dora", unet), ("twin", twin)):
        _patch(model, B, latent)
        res[name] = _run(model, sl, B, F, latent, dtype, full)
        vidtome_amd.remove_patch(model)
    for ck in range(3):
        for i, (a, b) in enumerate(zip(res["dora"][ck], res["twin"][ck])):
            assert bool(torch.isfinite(a).all()), (ck, sl[i].name)
            assert torch.equal(a, b), (ck, sl[i].name)
    assert all("_vtm_lora" not in m.__dict__ for m in wrapped)      # remove_patch dropped the folded copies


# ---------------------------------------------------------------------------------------------------
# 4. semantics: the fused DoRA block agrees with the module path (PEFT's DoRA forward)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol", [(torch.float16, 2e-3), (torch.bfloat16, 1.6e-2)])
def test_fused_dora_block_agrees_with_the_module_path(L, dtype, tol, monkeypatch):
    """4 frames, C = 320 and 640, whole blocks with computing (SDPA) attention modules, a DoRA adapter and a plain one
    after it: the fused path with folded weights against the module path (the recogniser forced to refuse the adapted
    layers: the stand-in's DoRA forward in the model dtype), within 2e-3 of the output scale -- the LoRA agreement bar --
    and, for bf16, that bar scaled by the 8x larger unit roundoff (1.6e-2: the bf16 module path alone, PEFT's row norms
    and m / n rounded to bf16, was measured 6.7e-3 ... 8.3e-3 of the scale away from float64 on the host); the unadapted
    block is > 4x further away."""
    import vidtome_amd
    from vidtome_amd import lora
    from vidtome_amd import sites as S
    sl = _site_list("up3.0", "up2.0")
    B, F, latent = 2, 4, (32, 32)
    res = {}
    for path in ("fused", "module", "base"):
        unet = S.SiteUNet(sl, seed=0, full=True).to(device=DEV, dtype=dtype)
        for blk in unet.blocks:
            blk.attn1, blk.attn2 = SDPAAttention(blk.attn1), SDPAAttention(blk.attn2)
        if path != "base":
            wrap_dora(unet, rank=32, trailing=16, seed=3)
        orig = lora.recognise
        if path == "module":
            monkeypatch.setattr(lora, "recognise", lambda m: orig(m) if orig(m) == lora.PLAIN else None)
        res[path] = _run(_patch(unet, B, latent), sl, B, F, latent, dtype, True)
        monkeypatch.setattr(lora, "recognise", orig)
        vidtome_amd.remove_patch(unet)
    for ck in range(3):
        for a, b, c in zip(res["fused"][ck], res["module"][ck], res["base"][ck]):
            scale = max(1.0, float(b.abs().max()))
            err = float((a.float() - b.float()).abs().max())
            assert err < tol * scale, (ck, err / scale)
            assert float((c.float() - b.float()).abs().max()) > 4 * tol * scale, ck


# ---------------------------------------------------------------------------------------------------
# 5. adapter-state changes
# ---------------------------------------------------------------------------------------------------
def test_dora_state_changes_rebuild_the_fold(L):
    """After each change the patched DoRA block equals the twin refolded from the new state, bit for bit: an in-place edit
    of the magnitudes, a DoRA scaling change, set_adapters to the plain adapter alone and back, disable (= the unadapted
    block), merge (the twin of the merged base weights) and unmerge, twice; remove_patch drops the folded weights."""
    import vidtome_amd
    from vidtome_amd import sites as S
    sl = _site_list("up3.0", "up2.0")
    B, F, latent = 2, 4, (32, 32)
    base = _patch(S.SiteUNet(sl, seed=0, full=True).to(device=DEV, dtype=torch.float16), B, latent)
    unet = S.SiteUNet(sl, seed=0, full=True).to(device=DEV, dtype=torch.float16)
    wrapped = wrap_dora(unet, rank=32, trailing=16, seed=4)
    twin = _patch(folded_twin_dora(unet), B, latent)
    _patch(unet, B, latent)
    run = lambda model: _run(model, sl, B, F, latent, torch.float16, True, n_chunks=2)
    eq = lambda x, y: all(torch.equal(a, b) for ca, cb in zip(x, y) for a, b in zip(ca, cb))
    want_base = run(base)
    first = run(unet)
    assert eq(first, run(twin)) and not eq(first, want_base)
    assert all("_vtm_lora" in m.__dict__ for m in wrapped)
    outs = [first]

    def follows(what, changes=True):
        refold_twin_dora(twin, unet)
        got = run(unet)
        assert eq(got, run(twin)), what
        assert not changes or not eq(got, outs[-1]), what
        outs.append(got)

    with torch.no_grad():
        for m in wrapped:
            m.magnitude("d0").mul_(1.03)
    follows("in-place magnitude edit")
    for m in wrapped:
        m.scaling["d0"] = 0.3
    follows("DoRA scaling")
    for m in wrapped:
        m.set_adapter("a1")
    follows("plain adapter alone")
    for m in wrapped:
        m.set_adapter(["d0", "a1"])
    follows("both again")
    assert eq(outs[-1], outs[-3])
    for m in wrapped:
        m.enable_adapters(False)
    assert eq(run(unet), want_base)
    for m in wrapped:
        m.enable_adapters(True)
    assert eq(run(unet), outs[-1])
    for _ in range(2):
        for m in wrapped:
            m.merge()
        follows("merge", changes=False)                 # the same Linear, rounded differently (or not)
        for m in wrapped:
            m.unmerge()
        follows("unmerge", changes=False)
    for model in (base, twin, unet):
        vidtome_amd.remove_patch(model)
    assert all("_vtm_lora" not in m.__dict__ for m in wrapped)
