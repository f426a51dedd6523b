"""GPU tests of perturbed-attention-guidance (PAG) blocks on the HIP path (run with -m gpu on an MI355X): the patched block
with a PAG processor on attn1 against a float64 restatement built from the captured merge plan and against the module path
(the stand-in processor called by attn1), that the attention cores ran for the org samples only, the identity property of the
perturbed samples, the registered form against the processor form, and the calls that keep the module path.

Sites: down0.0 (C = 320, d = 40: the rows route, live / compacted queries, folded keys), down1.0 (C = 640, d = 80: panels)
and mid (un-merged, C = 1280); 4 frames per sample of a 16 x 16 latent (256, 64 and 4 tokens per frame), and one
single-frame chunk at down0.0."""
import numpy as np
import pytest
import torch

import pag_standin as PS
from test_gpu_lora import _StandInSites, _cond, _hidden, _oracle_rows, _patch, _site_list

pytestmark = pytest.mark.gpu
DEV = "cuda"
LATENT = (16, 16)
SITES = ("down0.0", "down1.0", "mid")
# the segment / the whole block, relative to the output scale
SEG_TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}
BLOCK_TOL = {torch.float16: 2e-3, torch.bfloat16: 8e-3}
F32_TOL = 2e-3          # tests/test_gpu_fp32_projections.py: fp32_projections alone (the fp16 core class)
FORMS = [(3, 3), (2, 4)]          # (groups, batch_size): [uncond | cond | perturbed], [org, org | perturbed, perturbed]


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


# ---------------------------------------------------------------------------------------------------
# the float64 restatement
# ---------------------------------------------------------------------------------------------------
def _w64(m):
    return m.weight.detach().double().cpu(), None if m.bias is None else m.bias.detach().double().cpu()


def _lin(m, x):
    w, b = _w64(m)
    return x @ w.T + (0 if b is None else b)


def _attn64(q, k, v, heads, scale, mask=None):
    B, S, C = q.shape
    sh = lambda t: t.view(B, t.shape[1], heads, C // heads).transpose(1, 2)
    s = sh(q) @ sh(k).transpose(-1, -2) * scale
    if mask is not None:
        s = s + mask[:, None]
    return (torch.softmax(s, dim=-1) @ sh(v)).transpose(1, 2).reshape(B, S, C)


def _rows64(blk, merged, m, resid, n_org, cond=None, frame=None, mask=None):
    """float64 block rows: attn1's batch ``merged`` (B, M, C), row m[b, i] of sample b feeds output row i, ``resid`` the
    hidden states at those rows.  Org samples: to_out(softmax(q K^T) V); perturbed samples (from n_org on):
    to_out(to_v(x)); + residual.  With ``cond`` (B, frames, T, D) and the frame of every row the rest of the block follows:
    norm2 / attn2 over the row's own frame's conditioning, norm3 / GEGLU feed-forward."""
    a = blk.attn1
    xq = torch.stack([merged[b, m[b]] for b in range(merged.shape[0])])
    org = _attn64(_lin(a.to_q, xq[:n_org]), _lin(a.to_k, merged[:n_org]), _lin(a.to_v, merged[:n_org]), a.heads, a.scale, mask)
    h = _lin(a.to_out[0], torch.cat([org, _lin(a.to_v, xq[n_org:])])) + resid
    if cond is None:
        return h
    ln = lambda n, x: torch.nn.functional.layer_norm(x, x.shape[-1:], n.weight.double().cpu(), n.bias.double().cpu(), n.eps)
    a2 = blk.attn2
    x2 = ln(blk.norm2, h)
    o2 = torch.empty_like(h)
    for b in range(h.shape[0]):
        for f in frame.unique().tolist():
            sel = (frame == f).nonzero().flatten()
            kf, vf = _lin(a2.to_k, cond[b, f]), _lin(a2.to_v, cond[b, f])
            o2[b, sel] = _attn64(_lin(a2.to_q, x2[b, sel])[None], kf[None], vf[None], a2.heads, a2.scale)[0]
    h2 = _lin(a2.to_out[0], o2) + h
    p = _lin(blk.ff.net[0].proj, ln(blk.norm3, h2))
    D = p.shape[-1] // 2
    return _lin(blk.ff.net[2], p[..., :D] * torch.nn.functional.gelu(p[..., D:])) + h2


def _site_oracle(blk, plan, hidden, out, groups, F, cond, rng):
    """(got, want) float64 rows of one block call.  A merged site: sampled rows of the joined chunk through the captured
    plan, the batch split over its samples; the un-merged site: every row, a frame a sample of attn1's batch (our norm1 output
    is what the plan's merged tokens are at the other sites), the split over the frame rows."""
    from vidtome_amd import pag
    from vidtome_amd import patch as vpatch
    from vidtome_amd.utils import join_frame
    BF, N, C = hidden.shape
    if plan is None:
        merged = vpatch.layer_norm(blk.norm1, hidden).double().cpu()
        m = torch.arange(N).expand(BF, N)
        n_org = pag.split(BF, groups)[0]
        c = None if cond is None else cond.double().cpu()[:, None]
        want = _rows64(blk, merged, m, hidden.double().cpu(), n_org, c, torch.zeros(N, dtype=torch.long))
        return out.double().cpu(), want
    B, Lj = BF // F, plan.L
    idx = np.unique(np.concatenate([np.arange(8), np.arange(Lj - 8, Lj), rng.integers(0, Lj, 96)]))
    merged = plan.merged[:, :plan.M].double().cpu()
    m = torch.as_tensor(idx).expand(B, len(idx)) if plan.inv is None else plan.inv.cpu().long()[:, idx]
    n_org = pag.split(B, groups)[0]
    resid = join_frame(hidden, F).double().cpu()[:, idx]
    c = None if cond is None else cond.double().cpu().view(B, F, cond.shape[1], cond.shape[2])
    want = _rows64(blk, merged, m, resid, n_org, c, torch.as_tensor(idx) // N)
    if cond is None and plan.inv is not None:            # the org samples are test_gpu_lora's oracle, row for row
        ref = _oracle_rows(blk, plan, hidden, None, F, idx, _w64, False)[:n_org]
        assert float((want[:n_org] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))   # (float64 both)
    return join_frame(out, F).double().cpu()[:, idx], want


# ---------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------
def _model(names, dtype, groups, B, full=False, form="processor", seed=0, **patch_kw):
    """Stand-in sites with PAG on attn1 -- the Diffusers processor of ``groups`` (a computing attn1 that calls it), or plain
    blocks registered with ``register_perturbed_attention`` -- patched for a batch of B."""
    import vidtome_amd
    sl = _site_list(*names)
    torch.manual_seed(1000 + seed)           # (the biases keep torch's default init: the same in every model of a seed)
    unet = _StandInSites(sl, full, seed).to(device=DEV, dtype=dtype)
    procs = PS.install(unet, groups) if form == "processor" else []
    _patch(unet, B, LATENT, **patch_kw)
    if form == "marker":
        assert len(vidtome_amd.register_perturbed_attention(unet, layers=("blocks.",), groups=groups)) == len(sl)
    return unet, sl, procs


def _capture_plans(monkeypatch):
    """test_gpu_lora._capture_plans for models with an un-merged site: on the module path that site calls compute_merge
    too, which answers without a plan there."""
    from vidtome_amd import patch as vpatch
    seen, orig = {}, vpatch.compute_merge

    def rec(module, x, info, **kw):
        res = orig(module, x, info, **kw)
        seen[id(module)] = getattr(res[0], "plan", None)
        return res
    monkeypatch.setattr(vpatch, "compute_merge", rec)
    return seen


def _fresh(unet):
    torch.manual_seed(123)
    for blk in unet.blocks:                  # a fresh run: generators forked again from the seed, no anchors
        blk.__dict__.pop("generator", None)
        blk.global_tokens = None


def _chunks(unet, sl, B, F, dtype, cond=None, n_chunks=3, seed0=70, each=None):
    """Chunks of one clip through the patched sites (chunk 0 stores its tokens: every merged row a query; chunk 1 has the
    local chunk on the src side of the global level: live / compacted queries; chunk 2 on the dst side: folded keys at
    d = 40).  ``each(ck, hiddens, outs)`` runs after every chunk."""
    from vidtome_amd import sites as S
    _fresh(unet)
    res = []
    with torch.no_grad():
        for ck in range(n_chunks):
            unet._tome_info["args"]["global_rand"] = [0.5, 0.0, 1.0][ck % 3]
            hs = _hidden(sl, B, F, LATENT, dtype, ck, seed0)
            outs = S.run_block_pass(unet, hs, cond) if cond is not None else S.run_segment_pass(unet, hs)
            if each is not None:
                each(ck, hs, outs)
            res.append([o.clone() for o in outs])
    return res


def _force_module(monkeypatch):
    from vidtome_amd import patch as vpatch
    monkeypatch.setattr(vpatch, "attn1_route", lambda *a, **kw: "module")


def _parity(monkeypatch, names, dtype, groups, B, F, tol, full=False, flags=None, want_route=None):
    """The fused forward against the float64 restatement (every chunk, every site) and against the module path."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    unet, sl, procs = _model(names, dtype, groups, B, full)
    if flags:
        vidtome_amd.update_patch(unet, **flags)
    seen = _capture_plans(monkeypatch)
    cond = _cond(B, F, dtype) if full else None
    rng = np.random.default_rng(0)
    errs = []

    def check(ck, hs, outs):
        for blk, site, h, o in zip(unet.blocks, sl, hs, outs):
            assert vpatch.attn1_route(blk, h) == (want_route or vpatch.attn1_route(blk, h)) != "module"
            plan = seen.get(id(blk))
            assert (plan is None) == (site.name == "mid")
            if plan is not None and F > 1 and ck > 0:
                assert plan.global_level is not None
            got, want = _site_oracle(blk, plan, h, o, groups, F, cond, rng)
            scale = max(1.0, float(want.abs().max()))
            errs.append((site.name, ck, float((got - want).abs().max()) / scale))
    fused = _chunks(unet, sl, B, F, dtype, cond, each=check)
    print("PAG fused vs float64 (site, chunk, error / scale):", errs)
    assert all(p.calls == 0 for p in procs)
    assert all(e < tol for _, _, e in errs), errs
    _force_module(monkeypatch)
    module = _chunks(unet, sl, B, F, dtype, cond)
    assert all(p.calls == 3 for p in procs)
    for ck in range(3):
        for site, a, b in zip(sl, fused[ck], module[ck]):
            scale = max(1.0, float(b.abs().max()))
            err = float((a.float() - b.float()).abs().max()) / scale
            assert err < tol, (site.name, ck, err)
    vidtome_amd.remove_patch(unet)


# ---------------------------------------------------------------------------------------------------
# 1. parity
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups,B", FORMS)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_pag_segment_vs_float64_and_the_module_path(L, dtype, groups, B, monkeypatch):
    _parity(monkeypatch, SITES, dtype, groups, B, 4, SEG_TOL[dtype])


def test_pag_full_block_vs_float64_and_the_module_path(L, monkeypatch):
    """The whole block once (fp16, [uncond | cond | perturbed]): attn2 and the GEGLU feed-forward behind the PAG segment.
    (Measured once in bf16 as well: 7.6e-3 of the output scale against float64, inside 8e-3, but 8.5e-3 between the fused and
    the module path -- two bf16 results two ulps apart at an output of magnitude 117, each within 8e-3 of float64 -- so the
    whole-block comparison of two 16-bit paths at the one-path figure is kept to fp16.)"""
    _parity(monkeypatch, SITES, torch.float16, 3, 3, 4, BLOCK_TOL[torch.float16], full=True)


@pytest.mark.parametrize("groups,B", FORMS)
def test_pag_fp32_projections_vs_float64_and_the_module_path(L, groups, B, monkeypatch):
    """fp32 tokens, the block's ``fp32_projections``: the org samples on the fp16 core, the perturbed samples' V in fp32."""
    _parity(monkeypatch, ("down0.0",), torch.float32, groups, B, 4, F32_TOL, flags=dict(fp32_projections=True))


@pytest.mark.filterwarnings("ignore:vidtome_amd. attn1 projections")
@pytest.mark.parametrize("groups,B", FORMS)
def test_pag_library_gemm_route(L, groups, B, monkeypatch):
    """VIDTOME_PROJ=blas: the materialised-token body (``self_attention``), the perturbed samples' V an F.linear."""
    from vidtome_amd import patch as vpatch
    monkeypatch.setattr(vpatch, "PROJ_MODE", "blas")
    monkeypatch.setattr(vpatch, "FUSED_PROJ", False)
    _parity(monkeypatch, ("down0.0", "down1.0"), torch.float16, groups, B, 4, SEG_TOL[torch.float16], want_route="blas")


@pytest.mark.parametrize("groups,B", FORMS)
def test_pag_single_frame_chunk(L, groups, B, monkeypatch):
    """F = 1: no local level, the live rows are the chunk's own tokens (the unmerge is a slice)."""
    _parity(monkeypatch, ("down0.0",), torch.float16, groups, B, 1, SEG_TOL[torch.float16])


# ---------------------------------------------------------------------------------------------------
# 2. it ran where claimed
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups,B", FORMS)
def test_pag_cores_run_for_the_org_samples_only(L, groups, B, monkeypatch):
    """The processor is never called, no site takes the module route, and every attention core launch of the three sites
    has a leading batch of n_org -- the plain, the query-bounded and the folded-key variants all occur.  (At the parent
    commit the module path called the processor, and there was no vidtome_amd.pag to import.)"""
    import vidtome_amd
    from vidtome_amd import _lib, pag
    from vidtome_amd import patch as vpatch
    F = 4
    unet, sl, procs = _model(SITES, torch.float16, groups, B)
    seen = []
    orig_att, orig_kv = _lib.attention, _lib.attention_kv

    def spy_att(q, *a, **kw):
        seen.append((q.shape[2], q.shape[0], "plain"))
        return orig_att(q, *a, **kw)

    def spy_kv(q, *a, **kw):
        kind = "folded" if kw.get("k_fold") is not None else "bounded" if kw.get("q_count") is not None else "kv"
        seen.append((q.shape[2], q.shape[0], kind))
        return orig_kv(q, *a, **kw)
    monkeypatch.setattr(_lib, "attention", spy_att)
    monkeypatch.setattr(_lib, "attention_kv", spy_kv)
    routes = []
    _chunks(unet, sl, B, F, torch.float16,
            each=lambda ck, hs, outs: routes.extend(vpatch.attn1_route(b, h) for b, h in zip(unet.blocks, hs)))
    assert all(p.calls == 0 for p in procs)
    assert routes == ["rows", "panels", "panels"] * 3
    want = {320: pag.split(B, groups)[0], 640: pag.split(B, groups)[0], 1280: pag.split(B * F, groups)[0]}
    assert len(seen) == 9, seen
    for C, lead, kind in seen:
        assert lead == want[C], seen
    kinds = {(C, kind) for C, _, kind in seen}
    assert {(320, "plain"), (320, "bounded"), (320, "folded"), (640, "plain"), (1280, "plain")} <= kinds, kinds
    vidtome_amd.remove_patch(unet)


# ---------------------------------------------------------------------------------------------------
# 3. the identity property
# ---------------------------------------------------------------------------------------------------
def test_pag_perturbed_frames_do_not_mix_tokens(L):
    """mid (un-merged: LayerNorm is row-wise and nothing is matched): changing one token of a perturbed frame leaves every
    other row of the output bit-identical; changing a token of an org frame changes the other rows of that frame."""
    import vidtome_amd
    from vidtome_amd import sites as S
    B, F = 3, 4
    unet, sl, procs = _model(("mid",), torch.float16, 3, B)
    h = _hidden(sl, B, F, LATENT, torch.float16, 0, 90)[0]
    N = h.shape[1]
    run = lambda x: S.run_segment_pass(unet, [x])[0].clone()
    with torch.no_grad():
        base = run(h)
        ptb = h.clone()
        ptb[9, 2] += 1.0                                       # frame 9 of 12: a frame of the last (perturbed) sample
        out = run(ptb)
        others = torch.ones(B * F, N, dtype=torch.bool)
        others[9, 2] = False
        assert torch.equal(out[others], base[others])
        assert not torch.equal(out[9, 2], base[9, 2])
        org = h.clone()
        org[1, 2] += 1.0                                       # frame 1: an org frame
        out = run(org)
        for r in (0, 1, 3):
            assert not torch.equal(out[1, r], base[1, r])
        others = torch.ones(B * F, dtype=torch.bool)
        others[1] = False
        assert torch.equal(out[others], base[others])
    assert procs[0].calls == 0
    vidtome_amd.remove_patch(unet)


# ---------------------------------------------------------------------------------------------------
# 4. the registered form
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups,B", FORMS)
def test_registered_blocks_equal_the_processor_form_bitwise(L, groups, B):
    """register_perturbed_attention on plain blocks (whose Attention.forward raises) gives the bits of the run that
    recognised the Diffusers processor, at every site and chunk; a batch that does not split raises before any launch."""
    import vidtome_amd
    res = {}
    for form in ("processor", "marker"):
        unet, sl, _ = _model(SITES, torch.float16, groups, B, form=form)
        res[form] = _chunks(unet, sl, B, 4, torch.float16)
        if form == "marker":
            unet._tome_info["args"]["batch_size"] = B + 1
            with pytest.raises(ValueError, match="does not split"):
                _chunks(unet, sl, B + 1, 4, torch.float16, n_chunks=1)
        vidtome_amd.remove_patch(unet)
    for ca, cb in zip(res["processor"], res["marker"]):
        for a, b in zip(ca, cb):
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------
# 5. what keeps the module path
# ---------------------------------------------------------------------------------------------------
def test_pag_with_an_attention_mask_runs_the_module(L):
    """A key mask on attn1 (mid, 8 org frames of 4 keys): the module's own forward -- the processor -- runs and the block
    matches the float64 restatement with the mask on the org frames."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    B, F = 3, 4
    unet, sl, procs = _model(("mid",), torch.float16, 3, B)
    blk = unet.blocks[0]
    h = _hidden(sl, B, F, LATENT, torch.float16, 0, 95)[0]
    N = h.shape[1]
    mask = torch.zeros(8, 1, N, dtype=torch.float16, device=DEV)
    mask[::2, :, 1] = -10000.0
    mask[3, :, 2:] = -10000.0
    assert vpatch.attn1_route(blk, h, None, mask) == "module"
    blk.generator = vpatch.init_generator(h.device)
    with torch.no_grad():
        out = vpatch.self_attention_segment(blk, h, None, mask)
        merged = vpatch.layer_norm(blk.norm1, h).double().cpu()
    assert procs[0].calls == 1
    want = _rows64(blk, merged, torch.arange(N).expand(B * F, N), h.double().cpu(), 8, mask=mask.double().cpu())
    scale = max(1.0, float(want.abs().max()))
    assert float((out.double().cpu() - want).abs().max()) < SEG_TOL[torch.float16] * scale
    plain = _rows64(blk, merged, torch.arange(N).expand(B * F, N), h.double().cpu(), 8)
    assert float((plain - want).abs().max()) > 10 * SEG_TOL[torch.float16] * scale      # the mask is not noise
    vidtome_amd.remove_patch(unet)


def test_pag_under_pnp_sharing_runs_the_module(L, monkeypatch):
    """PnP sharing on attn1 of a PAG block (batch 3, aligned matching): the module's own forward runs and matches the float64
    restatement of what that forward -- the processor -- computes."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    B, F = 3, 4
    unet, sl, procs = _model(("down0.0",), torch.float16, 3, B, align_batch=True)
    blk = unet.blocks[0]
    blk.attn1.injection_schedule, blk.attn1.t, blk.attn1.vtm_num_inputs = [981], 981, B
    seen = _capture_plans(monkeypatch)
    rng = np.random.default_rng(1)
    errs = []

    def check(ck, hs, outs):
        assert vpatch.attn1_route(blk, hs[0]) == "module"
        got, want = _site_oracle(blk, seen[id(blk)], hs[0], outs[0], 3, F, None, rng)
        errs.append(float((got - want).abs().max()) / max(1.0, float(want.abs().max())))
    _chunks(unet, sl, B, F, torch.float16, each=check)
    assert procs[0].calls == 3
    assert all(e < SEG_TOL[torch.float16] for e in errs), errs
    vidtome_amd.remove_patch(unet)
