"""GPU tests of LoHa / LoKr (LyCORIS) adapted blocks on the HIP path (run with -m gpu on an MI355X): vtm_loha_delta /
vtm_lokr_delta / vtm_delta_fold against float64, the patched block with LyCORIS layers on the fused path against a float64
oracle, against its folded twin bit for bit, against the module path, and across adapter-state changes."""
import itertools

import numpy as np
import pytest
import torch

from lora_standin import SDPAAttention
from lycoris_standin import (LycorisLinear, folded_twin_lycoris, host_fold_lycoris, refold_twin_lycoris, wrap_lycoris)
from test_gpu_lora import CFG2, _capture_plans, _cond, _hidden, _oracle_rows, _patch, _run, _site_list, _StandInSites, _ulp

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24                           # fp32 unit roundoff
KINDS = {"loha": dict(kind="loha", rank=64), "lokr": dict(kind="lokr", rank=8, forms=("full", "lowrank"))}


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


# ---------------------------------------------------------------------------------------------------
# 1. the delta and fold kernels
# ---------------------------------------------------------------------------------------------------
def _gamma(r):
    """Relative bound of a k-ascending chain of r fmafs from +0: r u / (1 - r u) <= 1.001 r u for r <= 2^13."""
    return 1.001 * r * U


def _rand(g, rows, cols, std, dtype):
    """A factor as a 16-bit (or fp32) model holds it, passed to the kernels as fp32 on the device."""
    return (torch.randn(rows, cols, generator=g) * std).to(dtype).float().to(DEV)


def _chain(a, b):
    """float64 (product, bound of its fp32 chain) of two fp32 matrices."""
    a, b = a.double(), b.double()
    return a @ b, _gamma(a.shape[1]) * (a.abs() @ b.abs())


def _product_bound(c1, e1, c2, e2, mul):
    """float64 (product, error bound) of one fp32 product `mul` of two computed operands c +- e."""
    a1, a2 = c1.abs(), c2.abs()
    return mul(c1, c2), mul(a1, e2) + mul(e1, a2) + mul(e1, e2) + U * mul(a1 + e1, a2 + e2)


def _check_fold(L, W, deltas, refs, what):
    """`deltas()` builds the fp32 delta with the kernels; refs = [(float64 delta_a, its bound)] per adapter, in order."""
    dtype = W.dtype
    got = L.delta_fold(W, deltas())
    assert got.dtype == dtype and got.shape == W.shape
    D, E = refs[0]
    for p, ep in refs[1:]:              # one fp32 addition per further adapter
        D, E = D + p, E + ep + U * (D.abs() + E + p.abs() + ep)
    ref = W.double() + D
    bound = E + U * (W.double().abs() + D.abs() + E)
    if dtype != torch.float32:
        bound = bound + _ulp(ref, dtype)
    err = (got.double() - ref).abs()
    assert bool((err <= bound).all()), (what, float((err / bound).max()))
    assert float(D.abs().max()) > 0 and float((got.double() - W.double()).abs().max()) > 0, what
    assert torch.equal(L.delta_fold(W, deltas()), got), what           # the same bits on a second call
    return float((err / bound).max())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_lycoris_kernels_vs_float64(L, dtype):
    """vtm_loha_delta, vtm_lokr_delta and vtm_delta_fold against float64.  LoHa at (320, 320), (320, 1280), (2560, 320),
    (320, 768), (200, 333) and (77, 1000) with ranks 1, 33 and 64; LoKr as W1 (x) W2 at 16 x 20 (x) 20 x 16 and 16 x 16 (x)
    20 x 20 (320^2), 20 x 32 (x) 32 x 20 (640^2), 16 x 24 (x) 20 x 32 (attn2's k / v, 320 x 768: 768 = 24 x 32) and
    5 x 7 (x) 8 x 9, each factor full or low-rank (rank 4, multiplied out by vtm_lora_fold from a zero fp32 base); one and
    two adapters.  A-priori bounds, u = 2^-24: a chain of r fmafs from +0 carries E = gamma_r |A| |B|, gamma_r = r u /
    (1 - r u) <= 1.001 r u; one product of two computed operands c1 +- E1, c2 +- E2 carries |c1| E2 + |c2| E1 + E1 E2 and
    its own rounding u (|c1| + E1) (|c2| + E2); the sum of two adapters' deltas adds their bounds and one rounding of the
    sum; the fold adds u (|W| + |delta| + E) for its one fp32 addition; 16-bit outputs one ulp of the output dtype on top.
    A second call gives the same bits; bad arguments return -1."""
    g = torch.Generator().manual_seed(0)
    worst = 0.0
    for (co, ci), r, n in itertools.product(((320, 320), (320, 1280), (2560, 320), (320, 768), (200, 333), (77, 1000)),
                                            (1, 33, 64), (1, 2)):
        W = (torch.randn(co, ci, generator=g) * ci ** -0.5).to(dtype).to(DEV)
        ads = [(_rand(g, co, r, 0.3 * r ** -0.5, dtype) * s, _rand(g, r, ci, 1.0, dtype), _rand(g, co, r, 0.3 * r ** -0.5, dtype),
                _rand(g, r, ci, 1.0, dtype)) for s in (0.5, 0.75)[:n]]

        def deltas():
            d = None
            for w1a, w1b, w2a, w2b in ads:
                d = L.loha_delta(w1a, w1b, w2a, w2b, out=d, accumulate=d is not None)
            return d
        refs = [_product_bound(*_chain(w1a, w1b), *_chain(w2a, w2b), torch.mul) for w1a, w1b, w2a, w2b in ads]
        worst = max(worst, _check_fold(L, W, deltas, refs, ("loha", co, ci, r, n)))
    shapes = (((16, 20), (20, 16)), ((16, 16), (20, 20)), ((20, 32), (32, 20)), ((16, 24), (20, 32)), ((5, 7), (8, 9)))
    for (s1, s2), forms, n in itertools.product(shapes, itertools.product(("full", "lowrank"), repeat=2), (1, 2)):
        co, ci = s1[0] * s2[0], s1[1] * s2[1]
        W = (torch.randn(co, ci, generator=g) * ci ** -0.5).to(dtype).to(DEV)
        ads = []
        for s in (0.5, 0.75)[:n]:
            fs = []
            for form, (rows, cols), sc in zip(forms, (s1, s2), (s, 1.0)):
                fs.append((_rand(g, rows, cols, 0.3, dtype) * sc,) if form == "full" else
                          (_rand(g, rows, 4, 0.15, dtype) * sc, _rand(g, 4, cols, 1.0, dtype)))
            ads.append(fs)

        def full(f):
            if len(f) == 1:
                return f[0]
            return L.lora_fold(torch.zeros(f[0].shape[0], f[1].shape[1], device=DEV), f[0], f[1])

        def deltas():
            d = None
            for f1, f2 in ads:
                d = L.lokr_delta(full(f1), full(f2), out=d, accumulate=d is not None)
            return d
        op = lambda f: (f[0].double(), torch.zeros_like(f[0], dtype=torch.float64)) if len(f) == 1 else _chain(*f)
        refs = [_product_bound(*op(f1), *op(f2), torch.kron) for f1, f2 in ads]
        assert deltas().shape == (co, ci)
        worst = max(worst, _check_fold(L, W, deltas, refs, ("lokr", s1, s2, forms, n)))
    print(f"lycoris kernels {dtype}: worst error / bound {worst:.3f}")
    # accumulate adds to what the delta holds; out= is written in place
    w1, w2 = _rand(g, 5, 7, 0.3, dtype), _rand(g, 8, 9, 0.3, dtype)
    d = L.lokr_delta(w1, w2)
    d2 = L.lokr_delta(w1, w2, out=d.clone(), accumulate=True)
    assert torch.equal(d2, d + d) and torch.equal(d, torch.kron(w1, w2))
    lib, s = L.lib(), torch.cuda.current_stream().cuda_stream
    W = torch.zeros(64, 64, dtype=dtype, device=DEV)
    a, b, dl, out = torch.zeros(64, 4, device=DEV), torch.zeros(4, 64, device=DEV), torch.zeros(64, 64, device=DEV), torch.empty_like(W)
    k1, k2 = torch.zeros(8, 8, device=DEV), torch.zeros(8, 8, device=DEV)
    p = lambda t: t.data_ptr()
    code = L.dtype_code(W)
    assert lib.vtm_loha_delta(p(a), p(b), p(a), p(b), 64, 64, 4, 0, p(dl), s) == 0
    assert lib.vtm_lokr_delta(p(k1), p(k2), 8, 8, 8, 8, 64, 64, 1, p(dl), s) == 0
    assert lib.vtm_delta_fold(p(W), code, p(dl), 64, 64, p(out), s) == 0
    for args in ((0, 64, 4), (64, 0, 4), (64, 64, 0), (-1, 64, 4), (64 * 70000, 64, 4)):
        assert lib.vtm_loha_delta(p(a), p(b), p(a), p(b), *args, 0, p(dl), s) == -1, args
    assert lib.vtm_loha_delta(p(a), p(b), p(a), p(b), 64, 64, 4, 0, None, s) == -1
    for args in ((8, 8, 8, 8, 64, 65), (8, 8, 8, 9, 64, 64), (0, 8, 8, 8, 64, 64), (8, 8, 8, 8, -64, 64)):
        assert lib.vtm_lokr_delta(p(k1), p(k2), *args, 0, p(dl), s) == -1, args
    assert lib.vtm_lokr_delta(p(k1), None, 8, 8, 8, 8, 64, 64, 0, p(dl), s) == -1
    assert lib.vtm_delta_fold(p(W), 7, p(dl), 64, 64, p(out), s) == -1
    assert lib.vtm_delta_fold(p(W), code, p(dl), 64, 0, p(out), s) == -1
    assert lib.vtm_delta_fold(p(W), code, None, 64, 64, p(out), s) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# 2. the fused path runs for LyCORIS blocks (the module forward raises) and matches a float64 oracle
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full,dtype,tol", [(False, torch.float16, 1e-3), (True, torch.float16, 2e-3),
                                            (True, torch.bfloat16, 8e-3)])
@pytest.mark.parametrize("kind", ["loha", "lokr"])
def test_fused_lycoris_block_vs_float64_oracle(L, kind, full, dtype, tol, monkeypatch):
    """LoHa (rank 64) / LoKr (w1 full, w2 of rank 8) on every projection of blocks whose Attention.forward raises:
    apply_patch + a 3-chunk steady state runs on the fused path (at the parent commit a LyCORIS layer sent the block to the
    module, which raises here) and matches a float64 oracle built from host_fold_lycoris weights on sampled rows: 1e-3 of the
    output scale for the segment, 2e-3 for the whole block, 8e-3 for bf16.  The same oracle with the adapters left out
    misses the bound by more than 4x."""
    import vidtome_amd
    from vidtome_amd import sites as S
    from vidtome_amd.utils import join_frame
    sl = _site_list("up3.0", "up2.0")
    B, F, latent = 2, 4, (32, 32)
    unet = _StandInSites(sl, full).to(device=DEV, dtype=dtype)
    assert len(wrap_lycoris(unet, seed=2, **KINDS[kind])) == len(sl) * (10 if full else 4)
    seen = _capture_plans(monkeypatch)
    _patch(unet, B, latent)
    torch.manual_seed(123)
    cond = _cond(B, F, dtype) if full else None
    g = np.random.default_rng(0)
    no_adapters = lambda m: host_fold_lycoris(m, adapters=False)
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
                ref = _oracle_rows(blk, plan, h, cond, F, idx, host_fold_lycoris, full)
                got = join_frame(o, F).double().cpu()[:, idx]
                scale = max(1.0, float(ref.abs().max()))
                err = float((got - ref).abs().max())
                miss = float((got - _oracle_rows(blk, plan, h, cond, F, idx, no_adapters, full)).abs().max())
                print(f"{kind} {dtype} full={full} chunk {ck}: err {err / scale:.2e} miss {miss / scale:.2e} of the scale")
                assert err < tol * scale, (ck, err / scale)
                assert miss > 4 * tol * scale, (ck, miss / scale)
    vidtome_amd.remove_patch(unet)


# ---------------------------------------------------------------------------------------------------
# 3. plumbing: a LyCORIS block equals its folded twin bit for bit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,kind,opts", [
    (torch.float16, "loha", dict(rank=32, n_adapters=2)),
    (torch.float16, "lokr", dict(rank=8, forms=("full", "lowrank"))),
    (torch.bfloat16, "loha", dict(rank=64)),
    (torch.bfloat16, "lokr", dict(rank=8, forms=("lowrank", "full"), n_adapters=2)),
    (torch.float32, "loha", dict(rank=64)),
    (torch.float32, "lokr", dict(rank=8, forms=("lowrank", "lowrank")))])
def test_lycoris_block_equals_its_folded_twin_bitwise(L, dtype, kind, opts):
    """Full cfg-2 sizes, top (C = 320: the rows path), mid (C = 640: the panel path) and the un-merged C = 1280 site (the
    stacked q | k | v pack) as whole blocks (fp32 models: the segment), three chunks: every output bit-equal to the plain
    model whose Linears hold the fold kernels' outputs."""
    import vidtome_amd
    from vidtome_amd import sites as S
    full = dtype != torch.float32
    sl = _site_list("up3.0", "up2.0", "up1.0") if full else _site_list("up3.0", "up2.0")
    B, F, latent = CFG2["B"], CFG2["F"], CFG2["latent"]
    unet = S.SiteUNet(sl, seed=0, full=full).to(device=DEV, dtype=dtype)
    wrapped = wrap_lycoris(unet, kind, seed=1, **opts)
    assert len(wrapped) == len(sl) * (10 if full else 4)
    twin = folded_twin_lycoris(unet)
    assert not any(isinstance(m, LycorisLinear) for m in twin.modules())
    res = {}
    for name, model in (("lycoris", unet), ("twin", twin)):
        _patch(model, B, latent)
        res[name] = _run(model, sl, B, F, latent, dtype, full)
        if name == "lycoris":
            assert all("_vtm_lora" in m.__dict__ for m in wrapped)  # every projection was read through the fold
        vidtome_amd.remove_patch(model)
    for ck in range(3):
        for i, (a, b) in enumerate(zip(res["lycoris"][ck], res["twin"][ck])):
            assert bool(torch.isfinite(a).all()), (ck, sl[i].name)
            assert torch.equal(a, b), (ck, sl[i].name)
    assert all("_vtm_lora" not in m.__dict__ for m in wrapped)      # remove_patch dropped the folded copies


# ---------------------------------------------------------------------------------------------------
# 4. semantics: the fused LyCORIS block agrees with the module path (the layers' own forward)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol", [(torch.float16, 2e-3), (torch.bfloat16, 1.61e-2)])
@pytest.mark.parametrize("kind", ["loha", "lokr"])
def test_fused_lycoris_block_agrees_with_the_module_path(L, kind, dtype, tol, monkeypatch):
    """4 frames, C = 320 and 640, whole blocks with computing (SDPA) attention modules and two LoHa (rank 64) / LoKr (w1
    full, w2 of rank 8) adapters on every projection: the fused path with folded weights against the module path (the
    recogniser forced to refuse the adapted layers: the stand-in's forward, each delta built and applied in the model
    dtype).  The bars start from the LoRA / DoRA agreement bars, 2e-3 of the output scale for fp16 and 1.6e-2 for bf16,
    and widen to twice the module path's own distance from float64 where that exceeds half the bar.  Measured on the host
    at these shapes (the blocks' forward in the model dtype against a float64 copy, three chunks, both sites): fp16
    8.7e-4 ... 9.2e-4 (LoHa) and 8.3e-4 ... 9.4e-4 (LoKr) of the scale, under half of 2e-3: the bar stays; bf16
    7.0e-3 ... 8.05e-3 (LoHa) and 6.9e-3 ... 7.9e-3 (LoKr), the largest just over half of 1.6e-2: the bf16 bar is
    2 x 8.05e-3 = 1.61e-2.  The unadapted block is > 4x further away."""
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
            wrap_lycoris(unet, seed=3, n_adapters=2, **KINDS[kind])
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
            away = float((c.float() - b.float()).abs().max())
            print(f"{kind} {dtype} chunk {ck}: fused vs module {err / scale:.2e}, unadapted vs module {away / scale:.2e}")
            assert err < tol * scale, (ck, err / scale)
            assert away > 4 * tol * scale, ck


# ---------------------------------------------------------------------------------------------------
# 5. adapter-state changes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["loha", "lokr"])
def test_lycoris_state_changes_rebuild_the_fold(L, kind):
    """After each change the patched block equals the twin refolded from the new state, bit for bit: an in-place edit of a
    factor, a scaling change, set_adapter to one adapter and back, disable (= the unadapted block) and enable, merge (the
    twin of the merged base weights) and unmerge, twice; remove_patch drops the folded weights."""
    import vidtome_amd
    from vidtome_amd import sites as S
    sl = _site_list("up3.0", "up2.0")
    B, F, latent = 2, 4, (32, 32)
    base = _patch(S.SiteUNet(sl, seed=0, full=True).to(device=DEV, dtype=torch.float16), B, latent)
    unet = S.SiteUNet(sl, seed=0, full=True).to(device=DEV, dtype=torch.float16)
    wrapped = wrap_lycoris(unet, seed=4, n_adapters=2, **KINDS[kind])
    twin = _patch(folded_twin_lycoris(unet), B, latent)
    _patch(unet, B, latent)
    run = lambda model: _run(model, sl, B, F, latent, torch.float16, True, n_chunks=2)
    eq = lambda x, y: all(torch.equal(a, b) for ca, cb in zip(x, y) for a, b in zip(ca, cb))
    want_base = run(base)
    first = run(unet)
    assert eq(first, run(twin)) and not eq(first, want_base)
    assert all("_vtm_lora" in m.__dict__ for m in wrapped)
    outs = [first]

    def follows(what, changes=True):
        refold_twin_lycoris(twin, unet)
        got = run(unet)
        assert eq(got, run(twin)), what
        assert not changes or not eq(got, outs[-1]), what
        outs.append(got)

    factor = "hada_w2_b" if kind == "loha" else "lokr_w2_a"
    with torch.no_grad():
        for m in wrapped:
            getattr(m, factor)["a0"].mul_(1.05)
    follows("in-place factor edit")
    for m in wrapped:
        m.scaling["a1"] = 0.3
    follows("scaling")
    for m in wrapped:
        m.set_adapter("a1")
    follows("one adapter alone")
    for m in wrapped:
        m.set_adapter(["a0", "a1"])
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
