"""GPU tests of merge_mlp, the feed-forward on the merged local tokens (run with -m gpu on an MI355X):

1. vtm_layernorm_gather bit for bit against the rows of vtm_layernorm_panels / vtm_layernorm, both output layouts, both
   kernel families, with guards around the output;
2. the "merged-panels" segment bit for bit against the existing primitives run over ALL L rows (a panel GEMM's row does not
   depend on where it is stored or on how many rows there are: tests/test_gpu_odd_tokens.py holds the kernels to the first,
   and the K loop of csrc/ff.hip is split over weight rows only, never over K), on real plans of compute_merge;
3. both merged routes against a float64 restatement of ``u(ff(norm3(m(h)))) + h``;
4. the whole block through apply_patch / update_patch(merge_mlp=True).

B = 3 samples of different data everywhere.  Tolerances: the project's stated figures, 1e-3 of the
output scale in fp16 and 8e-3 in bf16 for a segment, 2e-3 / 8e-3 for the whole block; fp32 on the "merged" route 2e-6."""
import copy
import functools

import pytest
import torch

import standin

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3, torch.float32: 2e-6}
BLOCK_TOL = {torch.float16: 2e-3, torch.bfloat16: 8e-3}
DTYPES = (torch.float16, torch.bfloat16)
B = 3
SENTINEL = 5.0


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rand(shape, dtype, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _double(norm, ff, make_ff):
    """The block's own norm3 / feed-forward classes in float64 on the device, with its parameters (fresh modules: the
    originals carry the fused path's packed-weight caches)."""
    C = norm.normalized_shape[0]
    n64, f64 = torch.nn.LayerNorm(C, eps=norm.eps), make_ff(C)
    n64.load_state_dict(norm.state_dict())
    f64.load_state_dict(ff.state_dict())
    return n64.to(DEV).double(), f64.to(DEV).double()


def _name(dtype):
    return str(dtype).replace("torch.", "")


# ---------------------------------------------------------------------------------------------------
# 1. the kernel, bit for bit
# ---------------------------------------------------------------------------------------------------
LROWS = 100
WIDTHS = (64, 128, 320, 640, 1280)       # generic kernel (1 chunk per lane), then one per layernorm_rows_kernel width
COUNTS = (1, 7, 37, 100, 300)            # fewer rows than a wave holds, no multiple of R or 8, all of L, more rows than L


def _maps(n, rows_per_sample, seed=3):
    """(B, n) int32: sample 0 runs descending (wrapping), sample 1 is random with repeats, sample 2 repeats every row three
    times from the middle on -- three different maps."""
    i = torch.arange(n)
    m0 = (rows_per_sample - 1 - i) % rows_per_sample
    m1 = torch.randint(0, rows_per_sample, (n,), generator=torch.Generator().manual_seed(seed))
    m2 = (rows_per_sample // 2 + i // 3) % rows_per_sample
    return torch.stack([m0, m1, m2]).to(torch.int32).to(DEV)


def _raw_gather(L, x, gamma, beta, rows, out, panel_rows, eps=1e-5):
    Bx, Lx, C = x.shape
    rc = L.lib().vtm_layernorm_gather(x.data_ptr(), None if gamma is None else gamma.data_ptr(),
                                      None if beta is None else beta.data_ptr(), L.dtype_code(x), Bx, Lx, C, rows.data_ptr(),
                                      rows.shape[1], eps, out.data_ptr(), panel_rows, _stream())
    assert rc == 0, L.lib().vtm_last_error()
    torch.cuda.synchronize()


def _check_gather(L, x, gamma, beta, rows, panels):
    """Both layouts inside sentinel-filled buffers; the reference rows are picked with torch indexing."""
    Bx, Lx, C = x.shape
    n = rows.shape[1]
    pick = (torch.arange(Bx, device=DEV)[:, None] * Lx + rows.long()).reshape(-1)             # row of x behind output row b n + i
    assert int(rows.min()) >= 0 and int(rows.max()) < Lx
    dense_ref = L.layernorm(x, gamma, beta, 1e-5).view(Bx * Lx, C)[pick]
    buf = torch.full((Bx * n + 8, C), SENTINEL, dtype=x.dtype, device=DEV)
    _raw_gather(L, x, gamma, beta, rows, buf, 0)
    assert bool((buf[Bx * n:] == SENTINEL).all()), "a store past the last row"
    assert torch.equal(buf[:Bx * n], dense_ref)
    assert torch.equal(L.layernorm_gather(x, rows, gamma, beta, 1e-5, panels=False).view(Bx * n, C), dense_ref)
    if not panels:
        return
    panel_ref = L.layernorm_panels(x, gamma, beta, 1e-5)[:, pick]                              # (C / 8, B n, 8)
    assert torch.equal(panel_ref, dense_ref.view(Bx * n, C // 8, 8).transpose(0, 1))          # (the two references agree)
    pr = L.panel_rows(Bx * n)
    pbuf = torch.full((C // 8 + 1, pr, 8), SENTINEL, dtype=x.dtype, device=DEV)               # one guard panel behind
    _raw_gather(L, x, gamma, beta, rows, pbuf, pr)
    assert torch.equal(pbuf[:-1, :Bx * n], panel_ref)
    assert bool((pbuf[:-1, Bx * n:] == SENTINEL).all()), "a store into the panels' padding rows"
    assert bool((pbuf[-1] == SENTINEL).all()), "a store past the last panel"
    got = L.layernorm_gather(x, rows, gamma, beta, 1e-5)
    assert tuple(got.shape) == (C // 8, pr, 8) and torch.equal(got[:, :Bx * n], panel_ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("C", WIDTHS)
def test_layernorm_gather_rows_are_the_layernorms_rows(L, C, n, dtype):
    x = _rand((B, LROWS, C), dtype, 100 + C, 2.0).to(DEV) + 0.5
    gamma, beta = _rand((C,), dtype, 1).to(DEV), _rand((C,), dtype, 2).to(DEV)
    _check_gather(L, x, gamma, beta, _maps(n, LROWS), panels=True)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("C", WIDTHS)
def test_layernorm_gather_fp32_token_rows(L, C, n):
    x = _rand((B, LROWS, C), torch.float32, 200 + C, 2.0).to(DEV) + 0.5
    gamma, beta = _rand((C,), torch.float32, 1).to(DEV), _rand((C,), torch.float32, 2).to(DEV)
    _check_gather(L, x, gamma, beta, _maps(n, LROWS), panels=False)


@pytest.mark.parametrize("affine", ["none", "gamma", "beta"])
def test_layernorm_gather_without_an_affine_part(L, affine):
    x = _rand((B, LROWS, 320), torch.float16, 31, 2.0).to(DEV)
    gamma = _rand((320,), torch.float16, 1).to(DEV) if affine == "gamma" else None
    beta = _rand((320,), torch.float16, 2).to(DEV) if affine == "beta" else None
    _check_gather(L, x, gamma, beta, _maps(37, LROWS), panels=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_layernorm_gather_takes_the_kernel_the_layernorm_of_x_takes(L, dtype):
    """C = 1280 runs on layernorm_rows_kernel from 32768 rows of x on (a wave per row below): B L = 3 * 11000 rows select it
    for vtm_layernorm, so the gathered rows must come from it too -- the two kernels sum in different orders.  (The other
    generic shapes, C = 1024 and 2048 with 2 and 4 chunks per lane, ride along at L = 100.)"""
    Lbig = 11000
    assert B * Lbig >= 32768
    x = _rand((B, Lbig, 1280), dtype, 41, 2.0).to(DEV)
    gamma, beta = _rand((1280,), dtype, 1).to(DEV), _rand((1280,), dtype, 2).to(DEV)
    _check_gather(L, x, gamma, beta, _maps(37, Lbig), panels=True)
    for C in (1024, 2048):          # 2 and 4 chunks per lane (C = 1280 at L = 100 above is 3)
        x = _rand((B, LROWS, C), dtype, 42, 2.0).to(DEV)
        gamma, beta = _rand((C,), dtype, 1).to(DEV), _rand((C,), dtype, 2).to(DEV)
        _check_gather(L, x, gamma, beta, _maps(37, LROWS), panels=True)


# ---------------------------------------------------------------------------------------------------
# real plans: compute_merge on seeded corr01 tokens
# ---------------------------------------------------------------------------------------------------
GLOBALS = {"local": None, "global-src": 0.0, "global-dst": 1.0}      # global_rand: coin > 0.0 -> local chunk is src; 1.0 -> dst
CASES = [(F, N, C, ratio, glob) for F in (4, 8) for N in (64, 100) for C in (320, 640) for ratio in (0.5, 0.9)
         for glob in GLOBALS]
CASE_IDS = [f"F{F}-N{N}-C{C}-r{ratio}-{glob}" for F, N, C, ratio, glob in CASES]


@functools.lru_cache(maxsize=None)
def _unet(C, dtype):
    """One full SD block of width C with every parameter random (LayerNorm affine parts and biases included)."""
    from vidtome_amd import sites as S
    unet = S.SiteUNet([S.Site("up3.0", 1, C, 8)], seed=C, full=True)
    g = torch.Generator().manual_seed(C + 1)
    with torch.no_grad():
        for p in unet.parameters():
            if p.ndim == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.3 + (1.0 if p is unet.blocks[0].norm3.weight else 0.0))
    return unet.to(device=DEV, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _hidden(F, N, C, dtype):
    """The hidden states in front of the feed-forward (B F, N, C): shared by every plan of the shape, left unchanged."""
    return _rand((B * F, N, C), dtype, 7 * F + N + C, 1.5).to(DEV)


@functools.lru_cache(maxsize=None)
def _plan(F, N, C, ratio, glob, dtype):
    """The plan compute_merge makes for the second chunk of a step (so that anchors exist when the global level is on)."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch, sites as S
    unet = _unet(C, dtype)
    side = int(round(N ** 0.5))
    vidtome_amd.apply_patch(unet, local_merge_ratio=ratio, merge_global=glob != "local", global_merge_ratio=0.5, batch_size=B,
                            global_rand=GLOBALS[glob] if glob != "local" else 0.5)
    unet.set_size((side, side))
    blk = unet.blocks[0]
    blk.generator = torch.Generator().manual_seed(1000 + F + N)
    blk.__dict__.pop("global_tokens", None)              # (the block is shared: no anchors of another case)
    gb = lambda: torch.Generator().manual_seed(77)
    plan = None
    with torch.no_grad():
        for chunk in range(2):
            x = S.regime_tokens("corr01", B, F, N, C, torch.Generator().manual_seed(50 + chunk), gb())
            m, _, _ = vpatch.compute_merge(blk, x.reshape(B * F, N, C).to(device=DEV, dtype=dtype), blk._tome_info,
                                           materialize=False)
            plan = m.plan
    torch.cuda.synchronize()
    assert (plan.global_level is not None) == (glob != "local")
    if glob != "local":
        assert plan.local_chunk == (0 if glob == "global-src" else 1)
    assert len(plan.levels) == (1 if F == 4 else 2)
    vidtome_amd.remove_patch(unet)
    return plan


def _block(C, dtype, flag=True):
    """The block of ``_unet`` as a patched block would look to ff_route (apply_patch's two attributes and the opt-in)."""
    blk = _unet(C, dtype).blocks[0]
    blk.use_ada_layer_norm = blk.use_ada_layer_norm_zero = False
    blk.__dict__.pop("merge_mlp", None)
    if flag:
        blk.merge_mlp = True
    return blk


def _check_maps(plan, F, N):
    Lj = F * N
    keep, inv = plan.keep, plan.inv_local
    Ml = keep.shape[1]
    assert tuple(keep.shape) == (B, Ml) and tuple(inv.shape) == (B, Lj) and keep.dtype == inv.dtype == torch.int32
    assert Ml < Lj
    assert int(keep.min()) >= 0 and int(keep.max()) < Lj, "a local level referenced an anchor row"
    assert int(inv.min()) >= 0 and int(inv.max()) < Ml
    # every kept token is restored from its own merged row
    back = torch.gather(keep.long(), 1, torch.gather(inv.long(), 1, keep.long()))
    assert torch.equal(back, keep.long())
    kept = torch.zeros(B, Lj, dtype=torch.bool, device=DEV).scatter_(1, keep.long(), True)
    own = torch.gather(keep.long(), 1, inv.long()) == torch.arange(Lj, device=DEV)[None, :]
    assert bool((own == kept).all()), "keep[inv_local[i]] == i must hold for exactly the kept i"
    return Ml


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("F,N,C,ratio,glob", CASES, ids=CASE_IDS)
def test_merged_panels_segment_is_the_plain_chain_through_the_maps(L, F, N, C, ratio, glob, dtype):
    """out[b, i] == Y[b, keep[b, inv_local[b, i]]] + h[b, i] exactly, Y = layernorm_panels -> ff_geglu -> linear_panels
    without residual over all L rows -- the flag-off chain."""
    from vidtome_amd import patch as vpatch
    from vidtome_amd.utils import join_frame
    plan, h, blk = _plan(F, N, C, ratio, glob, dtype), _hidden(F, N, C, dtype), _block(C, dtype)
    Ml = _check_maps(plan, F, N)
    assert vpatch.ff_route(blk, h, plan) == "merged-panels"
    calls = []
    orig = {n: getattr(L, n) for n in ("layernorm_gather", "ff_geglu", "linear_panels", "unmerge_add")}

    def counted(n):
        def f(*a, **k):
            calls.append(n)
            return orig[n](*a, **k)
        return f
    try:
        for n in orig:
            setattr(L, n, counted(n))
        with torch.no_grad():
            vpatch.merged_feed_forward_residual(blk, h, plan, "merged-panels")       # (packs the weights)
            del calls[:]
            got = vpatch.merged_feed_forward_residual(blk, h, plan, "merged-panels")
    finally:
        for n in orig:
            setattr(L, n, orig[n])
    assert calls == ["layernorm_gather", "ff_geglu", "linear_panels", "unmerge_add"], calls
    hj = join_frame(h, F)
    Lj = F * N
    w1, b1, D, w2, b2 = vpatch._ff_panel_weights(blk.ff)
    xp = L.layernorm_panels(hj, blk.norm3.weight, blk.norm3.bias, blk.norm3.eps)
    Y = L.linear_panels(L.ff_geglu(xp, B * Lj, w1, D, b1), B * Lj, w2, C, b2).view(B, Lj, C)
    src = torch.gather(plan.keep.long(), 1, plan.inv_local.long())
    want = torch.gather(Y, 1, src[:, :, None].expand(-1, -1, C)) + hj
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B * F, N, C) and bool(torch.isfinite(got.float()).all())
    assert torch.equal(join_frame(got, F), want), f"M_l / L = {Ml} / {Lj}"
    # ... and the flag changes the result: a merged-away token carries its partner's feed-forward output
    plain = vpatch.norm_feed_forward_residual(blk.norm3, blk.ff, h)
    assert not torch.equal(plain, got)


@functools.lru_cache(maxsize=None)
def _ff64(F, N, C, dtype):
    """ff(norm3(h)) of EVERY row of the joined hidden states in float64, with the block's own modules in double (a row of
    LayerNorm / GEGLU / Linear depends on that row alone, so ff(norm3(m(h))) is a row selection of it)."""
    from vidtome_amd.utils import join_frame
    from vidtome_amd import sites as S
    blk = _unet(C, dtype).blocks[0]
    norm, ff = _double(blk.norm3, blk.ff, S.FeedForward)
    with torch.no_grad():
        return ff(norm(join_frame(_hidden(F, N, C, dtype), F).double()))


def _restated(plan, F, N, C, dtype):
    """u(ff(norm3(m(h)))) + h in float64."""
    from vidtome_amd.utils import join_frame
    y = torch.gather(_ff64(F, N, C, dtype), 1, plan.keep.long()[:, :, None].expand(-1, -1, C))          # ff(norm3(m(h)))
    u = torch.gather(y, 1, plan.inv_local.long()[:, :, None].expand(-1, -1, C))
    return u + join_frame(_hidden(F, N, C, dtype), F).double()


def _ratio(got, ref):
    g = got.detach().double()
    assert bool(torch.isfinite(g).all())
    return float((g - ref).abs().max()) / max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("F,N,C,ratio,glob", CASES, ids=CASE_IDS)
def test_merged_panels_segment_vs_float64(L, F, N, C, ratio, glob, dtype):
    from vidtome_amd import patch as vpatch
    from vidtome_amd.utils import join_frame
    plan, h, blk = _plan(F, N, C, ratio, glob, dtype), _hidden(F, N, C, dtype), _block(C, dtype)
    assert vpatch.ff_route(blk, h, plan) == "merged-panels"
    with torch.no_grad():
        got = vpatch.merged_feed_forward_residual(blk, h, plan, "merged-panels")
    err = _ratio(join_frame(got, F), _restated(plan, F, N, C, dtype))
    print(f"merge_mlp merged-panels {CASE_IDS[CASES.index((F, N, C, ratio, glob))]} {_name(dtype)} err/scale={err:.3e}")
    assert err < TOL[dtype], err


@pytest.mark.parametrize("dtype", DTYPES + (torch.float32,), ids=_name)
@pytest.mark.parametrize("F,N,C,ratio,glob", CASES, ids=CASE_IDS)
def test_merged_route_vs_float64(L, F, N, C, ratio, glob, dtype, monkeypatch):
    """The "merged" route -- VIDTOME_FF=blas on a 16-bit block, and an fp32 block -- against the same restatement; its
    LayerNorm is the gathered one with token rows out."""
    from vidtome_amd import patch as vpatch
    from vidtome_amd.utils import join_frame
    plan, h, blk = _plan(F, N, C, ratio, glob, dtype), _hidden(F, N, C, dtype), _block(C, dtype)
    if dtype != torch.float32:
        monkeypatch.setattr(vpatch, "FF_MODE", "blas")
    assert vpatch.ff_route(blk, h, plan) == "merged"
    calls = []
    orig = L.layernorm_gather
    monkeypatch.setattr(L, "layernorm_gather", lambda *a, **k: calls.append(k.get("panels")) or orig(*a, **k))
    with torch.no_grad():
        got = vpatch.merged_feed_forward_residual(blk, h, plan, "merged")
    assert calls == [False], calls
    err = _ratio(join_frame(got, F), _restated(plan, F, N, C, dtype))
    print(f"merge_mlp merged {CASE_IDS[CASES.index((F, N, C, ratio, glob))]} {_name(dtype)} err/scale={err:.3e}")
    assert err < TOL[dtype], err


def test_merged_route_with_a_norm_the_library_does_not_take(L, monkeypatch):
    """A norm3 that is not the plain LayerNorm: vtm_gather_rows + the module, same restatement."""
    from vidtome_amd import patch as vpatch
    from vidtome_amd.utils import join_frame

    class OtherNorm(torch.nn.LayerNorm):
        pass
    F, N, C, ratio, glob, dtype = 4, 100, 320, 0.5, "local", torch.float16
    plan, h = _plan(F, N, C, ratio, glob, dtype), _hidden(F, N, C, dtype)
    blk = copy.copy(_block(C, dtype))
    blk._modules = dict(blk._modules)
    other = OtherNorm(C).to(device=DEV, dtype=dtype)
    other.load_state_dict(blk.norm3.state_dict())
    blk._modules["norm3"] = other
    assert vpatch.ff_route(blk, h, plan) == "merged"
    monkeypatch.setattr(L, "layernorm_gather", lambda *a, **k: pytest.fail("the gathered LayerNorm ran for a foreign norm"))
    with torch.no_grad():
        got = vpatch.merged_feed_forward_residual(blk, h, plan, "merged")
    err = _ratio(join_frame(got, F), _restated(plan, F, N, C, dtype))
    assert err < TOL[dtype], err


# ---------------------------------------------------------------------------------------------------
# 4. the whole block through the public API
# ---------------------------------------------------------------------------------------------------
WC, WHEADS, WF, LATENT, COND, COND_DIM = 320, 8, 4, (16, 16), 77, 768
MERGING, UNMERGED = 6, 3          # blocks of the stand-in UNet: up_blocks[3] (downsample 1, 256 tokens), up_blocks[2] (2, 64)


def _standin(dtype):
    torch.manual_seed(5)
    unet = standin.StandInUNet(WC, WHEADS, full=True, cond_dim=COND_DIM)
    with torch.no_grad():
        for p in unet.parameters():
            if p.ndim == 1:
                p.add_(torch.randn(p.shape) * 0.2)
    return unet.to(device=DEV, dtype=dtype)


def _forward(unet, index, hiddens, cond, record=None):
    """The chunks ``hiddens`` in turn through block ``index`` from the same generator state and without anchors; the last
    chunk's output, and the generator state behind it."""
    from vidtome_amd import patch as vpatch
    blk = list(unet.blocks())[index]
    blk.generator = torch.Generator().manual_seed(11)
    blk.__dict__.pop("global_tokens", None)
    orig = vpatch.compute_merge

    def rec(*a, **k):
        res = orig(*a, **k)
        record.append(getattr(res[0], "plan", None))
        return res
    if record is not None:
        vpatch.compute_merge = rec
    try:
        latent = torch.zeros(1, 4, *LATENT, device=DEV)
        with torch.no_grad():
            for h in hiddens:
                feed = [None] * 9
                feed[index] = h
                out = unet(latent, feed, encoder_hidden_states=cond[:h.shape[0]])[index]
    finally:
        vpatch.compute_merge = orig
    torch.cuda.synchronize()
    return out, blk.generator.get_state()


@pytest.mark.parametrize("merge_global", [False, True], ids=["local", "global"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_whole_block_through_the_public_api(L, dtype, merge_global):
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    from vidtome_amd.utils import join_frame
    unet = _standin(dtype)
    vidtome_amd.apply_patch(unet, local_merge_ratio=0.5, merge_global=merge_global, global_merge_ratio=0.5, max_downsample=1,
                            batch_size=B)
    N = LATENT[0] * LATENT[1]
    chunks = [_rand((B * WF, N, WC), dtype, 60 + c).to(DEV) for c in range(2 if merge_global else 1)]
    cond = _rand((B * WF, COND, COND_DIM), dtype, 6).to(DEV)
    small = [_rand((B * WF, N // 4, WC), dtype, 70).to(DEV)]         # the downsample-2 site: does not merge at max_downsample 1
    single = [_rand((B, N, WC), dtype, 71).to(DEV)]                   # F = 1
    try:
        off, state_off = _forward(unet, MERGING, chunks, cond)
        off_small, _ = _forward(unet, UNMERGED, small, cond)
        off_single, _ = _forward(unet, MERGING, single, cond)
        assert vidtome_amd.update_patch(unet, merge_mlp=True) is unet
        routes = []
        orig_route = vpatch.ff_route
        vpatch.ff_route = lambda *a: routes.append(orig_route(*a)) or routes[-1]
        try:
            on, state_on = _forward(unet, MERGING, chunks, cond)
            assert routes == ["merged-panels"] * len(chunks), routes
            on_small, _ = _forward(unet, UNMERGED, small, cond)
            on_single, _ = _forward(unet, MERGING, single, cond)
            assert routes[len(chunks):] == ["panels", "panels"], routes
        finally:
            vpatch.ff_route = orig_route
        assert torch.equal(state_on, state_off), "the flag moved the generator"
        assert torch.equal(on_small, off_small) and torch.equal(on_single, off_single)
        assert not torch.equal(on, off)
        # the restatement: the flag-off block with a zero feed-forward gives the hidden states in front of the feed-forward
        # and, from the same generator state, the plan
        blk = list(unet.blocks())[MERGING]
        vidtome_amd.update_patch(unet, merge_mlp=False)
        ff = blk.ff
        blk.ff = standin.Zero()
        plans = []
        try:
            pre, _ = _forward(unet, MERGING, chunks, cond, record=plans)
        finally:
            blk.ff = ff
        plan = plans[-1]
        assert len(plans) == len(chunks) and (plan.global_level is not None) == merge_global
        norm64, ff64 = _double(blk.norm3, ff, standin.FeedForward)
        hj = join_frame(pre, WF).double()
        pick = lambda t, idx: torch.gather(t, 1, idx.long()[:, :, None].expand(-1, -1, WC))
        with torch.no_grad():
            ref = pick(ff64(norm64(pick(hj, plan.keep))), plan.inv_local) + hj
        err = _ratio(join_frame(on, WF), ref)
        diff = _ratio(join_frame(off, WF), ref)
        print(f"merge_mlp whole block {_name(dtype)} global={merge_global} err/scale={err:.3e} (flag off vs restatement {diff:.3e})")
        assert err < BLOCK_TOL[dtype], err
        # after remove_patch + apply_patch the flag is gone
        vidtome_amd.update_patch(unet, merge_mlp=True)
        vidtome_amd.remove_patch(unet)
        vidtome_amd.apply_patch(unet, local_merge_ratio=0.5, merge_global=merge_global, global_merge_ratio=0.5, max_downsample=1,
                                batch_size=B)
        assert not any(hasattr(b, "merge_mlp") for b in unet.blocks())
        again, _ = _forward(unet, MERGING, chunks, cond)
        assert torch.equal(again, off)
    finally:
        vidtome_amd.remove_patch(unet)
