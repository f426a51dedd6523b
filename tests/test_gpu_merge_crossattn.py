"""GPU tests of merge_crossattn, attn2 on the merged local tokens with keys routed per frame (run with -m gpu on an MI355X):

1. vtm_frame_order exactly against numpy (argsort, searchsorted), with sentinel guards behind every output;
2. vtm_attention_kv_segments against a float64 restatement: empty segments, segment ends inside and on the edge of a wave
   and of a workgroup, a segment over several query blocks, a tight and a loose bound, guard rows, ldq > h d, the peaked
   rows of tests/softmax_corners.py through one segment per sample, argument errors;
3. ``merged_cross_attention_residual`` on real plans of compute_merge against the float64 restatement of
       y[b, j]   = attn2(norm2(h[b, keep[b, j]]), encoder_hidden_states[b F + keep[b, j] // N])
       out[b, i] = y[b, inv_local[b, i]] + h[b, i]
   and the row-wise identity against the existing fused attn2;
4. the whole block through apply_patch / update_patch(merge_crossattn=True), alone and with merge_mlp=True;
5. every "plain" condition of ``cross_merge_route``: the flag changes no bit.

B = 3 samples of different data everywhere, and the conditioning differs per frame row wherever there are frames.
Tolerances: the project's stated figures, 1e-3 of the output scale in fp16 and 8e-3 in bf16 for a
kernel or a segment, 2e-3 / 8e-3 for the whole block."""
import functools

import numpy as np
import pytest
import torch

import softmax_corners as SC
import standin

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}
BLOCK_TOL = {torch.float16: 2e-3, torch.bfloat16: 8e-3}
DTYPES = (torch.float16, torch.bfloat16)
B = 3
EINVAL = -1
GUARD = -77


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _rand(shape, dtype, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _ratio(got, ref):
    g = got.detach().double()
    assert bool(torch.isfinite(g).all())
    return float((g - ref).abs().max()) / max(1.0, float(ref.abs().max()))


# ---------------------------------------------------------------------------------------------------
# 1. vtm_frame_order
# ---------------------------------------------------------------------------------------------------
FO_F, FO_N = 4, 24
FO_L = FO_F * FO_N


def _keeps(Ml, F=FO_F, N=FO_N):
    """(3, Ml) int32, distinct rows of [0, F N) per sample: sample 0 descending, sample 1 random, sample 2 fills frame 2
    first, then frames 0 and 3, frame 1 last, and is shuffled -- at Ml = 37 frame 2 keeps all N rows and frames 1 and 3 keep
    none; at Ml = L every frame keeps all; at Ml = 1 three frames keep none."""
    g = torch.Generator().manual_seed(100 + Ml)
    Lj = F * N
    desc = torch.arange(Lj - 1, -1, -1)[:Ml]
    rand = torch.randperm(Lj, generator=g)[:Ml]
    fill = torch.cat([torch.arange(2 * N, 3 * N), torch.arange(0, N), torch.arange(3 * N, Lj), torch.arange(N, 2 * N)])
    special = fill[:Ml][torch.randperm(Ml, generator=g)]
    return torch.stack([desc, rand, special]).to(torch.int32)


def _frame_order_ref(keep, inv, F, N):
    Bk, Ml = keep.shape
    ks = np.take_along_axis(keep, np.argsort(keep, axis=1, kind="stable"), 1)
    inv_s = np.stack([np.searchsorted(ks[b], keep[b][inv[b]]) for b in range(Bk)])
    seg = [b * Ml + int(np.searchsorted(ks[b], f * N)) for b in range(Bk) for f in range(F)] + [Bk * Ml]
    return ks.astype(np.int32), inv_s.astype(np.int32), np.asarray(seg, dtype=np.int32)


def _raw_frame_order(L, keep, inv, F, N):
    """The raw entry inside guarded buffers -> (keep_sorted, inv_sorted, seg_off) as numpy."""
    Bk, Ml = keep.shape
    Lj = F * N
    outs = [torch.full((n + 8,), GUARD, dtype=torch.int32, device=DEV) for n in (Bk * Ml, Bk * Lj, Bk * F + 1)]
    nbytes = L.lib().vtm_frame_order_ws_bytes(Bk, F, N)
    assert nbytes >= Bk * Lj * 4
    ws = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    rc = L.lib().vtm_frame_order(keep.data_ptr(), Ml, inv.data_ptr(), Bk, F, N, ws.data_ptr(), nbytes, outs[0].data_ptr(),
                                 outs[1].data_ptr(), outs[2].data_ptr(), _stream())
    assert rc == 0, L.lib().vtm_last_error()
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0x5A).all()), "a store past the workspace"
    res = []
    for o, n in zip(outs, (Bk * Ml, Bk * Lj, Bk * F + 1)):
        assert bool((o[n:] == GUARD).all()), "a store past an output"
        res.append(o[:n].cpu().numpy())
    return res[0].reshape(Bk, Ml), res[1].reshape(Bk, Lj), res[2]


def _check_frame_order(L, keep, inv, F, N):
    ks, inv_s, seg = _raw_frame_order(L, keep.to(DEV), inv.to(DEV), F, N)
    rks, rinv, rseg = _frame_order_ref(keep.numpy(), inv.numpy().astype(np.int64), F, N)
    assert np.array_equal(ks, rks)
    assert np.array_equal(inv_s, rinv)
    assert np.array_equal(seg, rseg), (seg, rseg)
    Bk, Ml = keep.shape
    assert seg[0] == 0 and seg[-1] == Bk * Ml and bool((np.diff(seg) >= 0).all()) and int(np.diff(seg).max()) <= N
    # the frame of every sorted row is its segment's
    for s in range(Bk * F):
        rows = ks.reshape(-1)[seg[s]:seg[s + 1]]
        assert bool((rows // N == s % F).all())
    w = L.frame_order(keep.to(DEV), inv.to(DEV), F, N)
    torch.cuda.synchronize()
    for got, want in zip(w, (rks, rinv, rseg)):
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    return seg


@pytest.mark.parametrize("Ml", [1, 37, FO_L])
def test_frame_order_is_argsort_and_searchsorted(L, Ml):
    keep = _keeps(Ml)
    inv = torch.randint(0, Ml, (B, FO_L), generator=torch.Generator().manual_seed(5 + Ml)).to(torch.int32)
    if Ml > 1:
        assert all(len(set(inv[b].tolist())) < FO_L for b in range(B)), "inv_local must repeat entries"
    seg = _check_frame_order(L, keep, inv, FO_F, FO_N)
    lens = np.diff(seg).reshape(B, FO_F)
    if Ml == 37:
        assert lens[2].tolist() == [13, 0, 24, 0]          # one frame keeps all N rows, two keep none
    if Ml == FO_L:
        assert bool((lens == FO_N).all())


@pytest.mark.parametrize("F,N,Ml", [(3, 2500, 4001), (2, 9000, 10001)], ids=["N2500", "N9000"])
def test_frame_order_frames_longer_than_a_scan_tile(L, F, N, Ml):
    """N = 2500 rows per frame: the rank kernel scans a frame's table in three tiles of 1024 slots, the last one partial.
    N = 9000: more rows than the table of 8192 holds, the frame takes it twice."""
    g = torch.Generator().manual_seed(9)
    keep = torch.stack([torch.randperm(F * N, generator=g)[:Ml] for _ in range(B)]).to(torch.int32)
    inv = torch.randint(0, Ml, (B, F * N), generator=g).to(torch.int32)
    _check_frame_order(L, keep, inv, F, N)


def test_frame_order_bad_arguments_launch_nothing(L):
    keep = _keeps(37).to(DEV)
    inv = torch.zeros(B, FO_L, dtype=torch.int32, device=DEV)
    nbytes = L.lib().vtm_frame_order_ws_bytes(B, FO_F, FO_N)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    outs = [torch.full((n,), GUARD, dtype=torch.int32, device=DEV) for n in (B * 37, B * FO_L, B * FO_F + 1)]
    ok = dict(keep=keep.data_ptr(), Ml=37, inv=inv.data_ptr(), B=B, F=FO_F, N=FO_N, ws=ws.data_ptr(), nbytes=nbytes,
              ks=outs[0].data_ptr(), inv_s=outs[1].data_ptr(), seg=outs[2].data_ptr())
    bad = [dict(keep=None), dict(inv=None), dict(ws=None), dict(ks=None), dict(inv_s=None), dict(seg=None), dict(Ml=0),
           dict(Ml=FO_L + 1), dict(B=0), dict(F=0), dict(N=-1), dict(F=1 << 20, N=1 << 20)]
    for change in bad:
        a = dict(ok, **change)
        rc = L.lib().vtm_frame_order(a["keep"], a["Ml"], a["inv"], a["B"], a["F"], a["N"], a["ws"], a["nbytes"], a["ks"],
                                     a["inv_s"], a["seg"], _stream())
        assert rc == EINVAL, (change, rc)
        assert L.lib().vtm_last_error().decode().startswith("vtm_frame_order:")
    rc = L.lib().vtm_frame_order(ok["keep"], 37, ok["inv"], B, FO_F, FO_N, ok["ws"], nbytes - 1, ok["ks"], ok["inv_s"],
                                 ok["seg"], _stream())
    assert rc not in (0, EINVAL)                               # VTM_EWORKSPACE
    torch.cuda.synchronize()
    assert all(bool((o == GUARD).all()) for o in outs)


# ---------------------------------------------------------------------------------------------------
# 2. vtm_attention_kv_segments
# ---------------------------------------------------------------------------------------------------
SEG_LENS = [0, 1, 31, 32, 33, 0, 127, 128, 129, 255, 256, 257, 515, 0]
SEG_H = 2
SENTINEL = -7.0
PAD = 3.0e4                    # key rows / V^T columns behind Mk: never read as keys


def _attend64(q, k, v, heads, scale):
    """softmax(q k^T scale) v per head in float64: q (n, C), k / v (Mk, C) -> (n, C)."""
    n, C = q.shape
    d = C // heads
    sh = lambda t: t.double().view(t.shape[0], heads, d).transpose(0, 1)
    p = torch.softmax(sh(q) @ sh(k).transpose(1, 2) * scale, dim=-1)
    return (p @ sh(v)).transpose(0, 1).reshape(n, C)


@functools.lru_cache(maxsize=None)
def _seg_operands(d, Mk, dtype):
    """q (rows, C), k / v (n_seg, Mkp, C) with PAD behind Mk, the offsets and the float64 result: made once per shape, shared
    by the tests and left unchanged.  Every segment has keys of its own."""
    g = torch.Generator().manual_seed(1000 + 7 * d + Mk)
    C, rows, n_seg, Mkp = SEG_H * d, sum(SEG_LENS), len(SEG_LENS), (Mk + 7) // 8 * 8
    q = torch.randn(rows, C, generator=g).to(dtype).to(DEV)
    k = torch.randn(n_seg, Mkp, C, generator=g).to(dtype).to(DEV)
    v = torch.randn(n_seg, Mkp, C, generator=g).to(dtype).to(DEV)
    k[:, Mk:] = PAD
    v[:, Mk:] = PAD
    off = np.concatenate([[0], np.cumsum(SEG_LENS)]).astype(np.int32)
    ref = torch.zeros(rows, C, dtype=torch.float64, device=DEV)
    for s in range(n_seg):
        if off[s + 1] > off[s]:
            ref[off[s]:off[s + 1]] = _attend64(q[off[s]:off[s + 1]], k[s, :Mk], v[s, :Mk], SEG_H, d ** -0.5)
    return q, k, v.transpose(1, 2).contiguous(), torch.from_numpy(off).to(DEV), ref


def _run_segments(L, q, k, vt, off, bound, Mk, d):
    """The wrapper on a query view with ldq = C + 8 and an output with 8 guard rows -> the (rows, C) result."""
    rows, C = q.shape
    qbuf = torch.full((rows + 8, C + 8), SENTINEL, dtype=q.dtype, device=DEV)
    qbuf[:rows, :C] = q
    obuf = torch.full((rows + 8, C), SENTINEL, dtype=q.dtype, device=DEV)
    qv = qbuf[:rows, :C]
    assert qv.stride(0) == C + 8 > SEG_H * d
    got = L.attention_kv_segments(qv, k, vt, SEG_H, off, bound, Mk, d ** -0.5, out=obuf[:rows])
    torch.cuda.synchronize()
    assert got.data_ptr() == obuf.data_ptr()
    assert bool((obuf[rows:] == SENTINEL).all()), "rows behind rows_total were written"
    return obuf[:rows]


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("Mk", [77, 8, 154])
@pytest.mark.parametrize("d", [40, 64, 80, 160])
def test_segments_vs_float64(L, d, Mk, dtype):
    q, k, vt, off, ref = _seg_operands(d, Mk, dtype)
    bar = TOL[dtype] * max(1.0, float(ref.abs().max()))
    results = []
    for bound in (515, 4096):                        # tight and loose
        got = _run_segments(L, q, k, vt, off, bound, Mk, d)
        g = got.double()
        assert bool(torch.isfinite(g).all())
        rows_err = (g - ref).abs().amax(-1)
        err = float(rows_err.max())
        print(f"segments d={d} Mk={Mk} {_name(dtype)} bound={bound} err={err:.3e} bar={bar:.3e} ratio={err / bar:.3f}")
        assert err < bar, (bound, err, bar, int((rows_err >= bar).sum()), "rows miss")
        results.append(got.clone())
    assert torch.equal(results[0], results[1]), "the bound changed a result"


def test_segment_longer_than_the_bound_keeps_its_first_rows(L):
    """The stated contract: with max_seg_rows = 256 the segments of 257 and 515 rows get their first 256 rows, the rest of
    their rows are not written; every other segment is whole."""
    d, Mk, dtype = 40, 77, torch.float16
    q, k, vt, off, ref = _seg_operands(d, Mk, dtype)
    got = _run_segments(L, q, k, vt, off, 256, Mk, d)
    o = off.cpu().numpy()
    bar = TOL[dtype] * max(1.0, float(ref.abs().max()))
    for s, n in enumerate(SEG_LENS):
        a, b_, cut = int(o[s]), int(o[s + 1]), int(o[s]) + min(n, 256)
        if cut > a:
            assert float((got[a:cut].double() - ref[a:cut]).abs().max()) < bar, s
        assert bool((got[cut:b_] == SENTINEL).all()), (s, "rows behind the bound were written")


def test_offsets_outside_the_rows_address_nothing(L):
    """Offsets that break the contract (negative, beyond rows_total, decreasing) are clamped on the device: nothing outside
    the rows is written and the call ends clean."""
    d, Mk, dtype = 40, 77, torch.float16
    q, k, vt, off, ref = _seg_operands(d, Mk, dtype)
    rows = q.shape[0]
    bad = off.clone()
    bad[0] = -40
    bad[5] = 50                       # decreasing: behind offset 97
    bad[-1] = rows + 1000
    got = _run_segments(L, q, k, vt, bad, 4096, Mk, d)
    g = got.double()
    written = ~(got == SENTINEL).all(-1)
    assert bool(torch.isfinite(g[written]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("d", SC.DIMS)
@pytest.mark.parametrize("name", ["late_spike", "staircase_over", "staircase_under", "first_key_dominant", "wide_range",
                                  "all_very_negative"])
def test_segments_softmax_corners(L, name, d, dtype):
    """The peaked rows of tests/softmax_corners.py (the per-key-bias kernel's operands, their bias dropped): the two samples
    of a case are two segments of 300 rows with keys of their own, against the float64 expression on the same operands."""
    c = SC.scenario(name, "bias", d, dtype, 200).replace(bias=None)
    if name in ("late_spike", "staircase_over"):
        assert any(SC.case_census(c, b, h, 0).rescales > 0 for b in range(SC.B) for h in range(SC.H)), "no rescale reached"
    ref = SC.reference(c)
    bar = SC.bar(c, ref)
    q = c.q[:, :c.Mq].reshape(SC.B * c.Mq, SC.H * d).contiguous().to(DEV)
    off = torch.tensor([0, c.Mq, 2 * c.Mq], dtype=torch.int32, device=DEV)
    got = L.attention_kv_segments(q, c.k.to(DEV), c.v.transpose(1, 2).contiguous().to(DEV), SC.H, off, c.Mq, c.Mk, d ** -0.5)
    torch.cuda.synchronize()
    g = got.double().cpu().numpy().reshape(SC.B, c.Mq, -1)
    assert bool(np.isfinite(g).all())
    err = float(np.abs(g - ref).max())
    print(f"segments corner {name} d={d} {_name(dtype)} err={err:.3e} bar={bar:.3e} ratio={err / bar:.3f}")
    assert err <= bar, (err, bar)


def test_segments_bad_arguments_leave_out_untouched(L):
    d, Mk, dtype = 40, 77, torch.float16
    q, k, vt, off, _ = _seg_operands(d, Mk, dtype)
    rows, C = q.shape
    out = torch.full((rows, C), SENTINEL, dtype=dtype, device=DEV)
    ok = dict(q=q.data_ptr(), ldq=C, k=k.data_ptr(), ldk=C, vt=vt.data_ptr(), ldvt=vt.stride(1), out=out.data_ptr(), ldo=C,
              dtype=L.VTM_F16, rows=rows, off=off.data_ptr(), n_seg=len(SEG_LENS), bound=515, h=SEG_H, Mk=Mk, Mkp=k.shape[1],
              d=d, scale=d ** -0.5)
    bad = [dict(dtype=L.VTM_F32), dict(dtype=7), dict(q=None), dict(k=None), dict(vt=None), dict(out=None), dict(off=None),
           dict(rows=0), dict(n_seg=0), dict(bound=0), dict(h=0), dict(Mk=0), dict(Mkp=Mk), dict(Mkp=72), dict(d=48),
           dict(scale=0.0), dict(scale=float("inf")), dict(ldq=C + 4), dict(ldq=C - 8), dict(ldk=C + 4), dict(ldvt=Mk),
           dict(ldvt=72), dict(ldo=C + 2), dict(ldo=C - 4), dict(rows=1 << 31)]
    for change in bad:
        a = dict(ok, **change)
        rc = L.lib().vtm_attention_kv_segments(a["q"], a["ldq"], a["k"], a["ldk"], a["vt"], a["ldvt"], a["out"], a["ldo"],
                                               a["dtype"], a["rows"], a["off"], a["n_seg"], a["bound"], a["h"], a["Mk"],
                                               a["Mkp"], a["d"], a["scale"], _stream())
        assert rc == EINVAL, (change, rc)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    with pytest.raises(RuntimeError, match="fp16 / bf16"):
        L.attention_kv_segments(q.float(), k.float(), vt.float(), SEG_H, off, 515, Mk, d ** -0.5)


# ---------------------------------------------------------------------------------------------------
# a full SD block of the package's stand-in UNet, and real plans of compute_merge
# ---------------------------------------------------------------------------------------------------
F, SIDE, COND, COND_DIM, HEADS = 4, 24, 77, 768, 8
N = SIDE * SIDE                    # 576 tokens per frame: a segment spans more than one query block of 256 (or 128) rows


@functools.lru_cache(maxsize=None)
def _unet(C, dtype):
    """One full SD block of width C with every parameter random (LayerNorm affine parts and biases included)."""
    from vidtome_amd import sites as S
    unet = S.SiteUNet([S.Site("up3.0", 1, C, HEADS)], seed=C, full=True)
    g = torch.Generator().manual_seed(C + 1)
    blk = unet.blocks[0]
    with torch.no_grad():
        for p in unet.parameters():
            if p.ndim == 1:
                norm_w = any(p is n.weight for n in (blk.norm1, blk.norm2, blk.norm3))
                p.copy_(torch.randn(p.shape, generator=g) * 0.2 + (1.0 if norm_w else 0.0))
    return unet.to(device=DEV, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _tokens(C, dtype, chunk):
    """corr01 hidden states (B F, N, C) of one chunk of a clip: the frames of a position are near copies, so the matching
    merges across frames."""
    from vidtome_amd import sites as S
    x = S.regime_tokens("corr01", B, F, N, C, torch.Generator().manual_seed(50 + chunk), torch.Generator().manual_seed(77))
    return x.reshape(B * F, N, C).to(device=DEV, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _cond(dtype):
    """(B F, 77, 768): another conditioning for every frame row (1.5 N(0, 1): scores of about 1.5 units, so that the attn2
    output of two frames differs by a good part of the output scale)."""
    return _rand((B * F, COND, COND_DIM), dtype, 6, 1.5).to(DEV)


def _apply(unet, merge_global, **kw):
    import vidtome_amd
    opts = dict(local_merge_ratio=0.5, merge_global=merge_global, global_merge_ratio=0.5, batch_size=B, target_stride=2)
    opts.update(kw)
    vidtome_amd.apply_patch(unet, **opts)
    unet.set_size((SIDE, SIDE))
    return unet.blocks[0]


def _fresh(blk):
    blk.generator = torch.Generator().manual_seed(11)
    blk.__dict__.pop("global_tokens", None)


@functools.lru_cache(maxsize=None)
def _plan(C, merge_global, dtype):
    """The plan compute_merge makes for the last chunk (the second one with a global level, so that anchors exist): two local
    levels (4 frames at target_stride 2)."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    unet = _unet(C, dtype)
    blk = _apply(unet, merge_global)
    _fresh(blk)
    plan = None
    with torch.no_grad():
        for chunk in range(2 if merge_global else 1):
            m, _, _ = vpatch.compute_merge(blk, _tokens(C, dtype, chunk), blk._tome_info, materialize=False)
            plan = m.plan
    torch.cuda.synchronize()
    assert len(plan.levels) == 2 and (plan.global_level is not None) == merge_global
    assert plan.fsize == F and plan.L == F * N
    vidtome_amd.remove_patch(unet)
    return plan


def _block(C, dtype):
    blk = _unet(C, dtype).blocks[0]
    blk.use_ada_layer_norm = blk.use_ada_layer_norm_zero = False
    blk.merge_crossattn = True
    return blk


def _attn2_64(blk, h, cond):
    """attn2(norm2(h), cond) of EVERY row in float64, frame row by frame row: h (B F, N, C), cond (B F, K, D) -> (B F, N, C)."""
    a, n2 = blk.attn2, blk.norm2
    C = h.shape[-1]
    w = lambda lin: lin.weight.detach().double()
    xn = torch.nn.functional.layer_norm(h.double(), (C,), n2.weight.detach().double(), n2.bias.detach().double(), n2.eps)
    q, k, v = xn @ w(a.to_q).T, cond.double() @ w(a.to_k).T, cond.double() @ w(a.to_v).T
    o = torch.stack([_attend64(q[i], k[i], v[i], a.heads, (C // a.heads) ** -0.5) for i in range(h.shape[0])])
    return o @ w(a.to_out[0]).T + a.to_out[0].bias.detach().double()


def _pick(t, idx):
    return torch.gather(t, 1, idx.long()[:, :, None].expand(-1, -1, t.shape[-1]))


def _merged_attn2_64(blk, h, cond, plan):
    """(the merged result, the plain one).  The two formulas of the contract in float64: a row of attn2 depends on that row and on its frame's conditioning alone,
    so y is a row selection of attn2 over every row -- row keep[b, j] of sample b lies in frame keep[b, j] // N, whose
    conditioning is encoder_hidden_states[b F + keep[b, j] // N]."""
    from vidtome_amd.utils import join_frame
    hj = join_frame(h, F).double()
    A = join_frame(_attn2_64(blk, h, cond), F)
    return _pick(_pick(A, plan.keep), plan.inv_local) + hj, A + hj


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("merge_global", [False, True], ids=["local", "global"])
@pytest.mark.parametrize("C", [320, 640])
def test_merged_segment_on_real_plans(L, C, merge_global, dtype):
    from vidtome_amd import patch as vpatch
    from vidtome_amd.utils import join_frame
    plan, blk = _plan(C, merge_global, dtype), _block(C, dtype)
    h, cond = _rand((B * F, N, C), dtype, 7 + C).to(DEV), _cond(dtype)
    Ml = plan.keep.shape[1]
    assert Ml < F * N and int(plan.keep.max()) < F * N
    route = vpatch.attn2_route(blk, h, cond, None, {})
    assert route.frame == "panels" and vpatch.cross_merge_route(blk, h, plan, route, cond, None) == "merged-panels"
    calls = []
    orig = L.attention_kv_segments
    L.attention_kv_segments = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        with torch.no_grad():
            got = vpatch.merged_cross_attention_residual(blk, h, cond, plan)
            plain = vpatch.norm_cross_attention_residual(blk.norm2, blk.attn2, h, cond)
    finally:
        L.attention_kv_segments = orig
    torch.cuda.synchronize()
    assert calls == [1] and tuple(got.shape) == (B * F, N, C) and got.dtype == dtype
    # the frame order is cached on the plan and leaves the maps alone
    ks, inv_s, seg = plan.frame_order()
    assert plan.frame_order()[0] is ks and torch.equal(_pick(ks[:, :, None], inv_s)[:, :, 0], _pick(plan.keep[:, :, None],
                                                                                                   plan.inv_local)[:, :, 0])
    lens = (seg[1:] - seg[:-1]).cpu()
    assert int(lens.max()) <= N and int(lens.max()) > 256, "a segment must span more than one query block"
    with torch.no_grad():
        ref, ref_plain = _merged_attn2_64(blk, h, cond, plan)
    gj = join_frame(got, F)
    err = _ratio(gj, ref)
    # the row-wise identity against the existing path: A = today's fused attn2 output minus its residual
    hj = join_frame(h, F).double()
    A = join_frame(plain, F).double() - hj
    ident = _ratio(gj, hj + _pick(A, _pick(plan.keep[:, :, None], plan.inv_local)[:, :, 0]))
    apart = float((ref - ref_plain).abs().max()) / max(1.0, float(ref.abs().max()))
    print(f"merge_crossattn segment C={C} global={merge_global} {_name(dtype)} M_l/L={Ml}/{F * N} err/scale={err:.3e} "
          f"identity={ident:.3e} merged-vs-plain={apart:.3e}")
    assert apart > 10 * TOL[dtype], "the merged and the plain restatement must differ far beyond the tolerance"
    assert err < TOL[dtype], err
    assert ident < TOL[dtype], ident


# ---------------------------------------------------------------------------------------------------
# 4. the whole block through the public API
# ---------------------------------------------------------------------------------------------------
WC = 320


def _forward(blk, chunks, cond, **kw):
    """The chunks in turn through the block from the same generator state and without anchors: the last output, and the
    generator state behind it."""
    _fresh(blk)
    with torch.no_grad():
        for h in chunks:
            out = blk(h, encoder_hidden_states=cond, **kw)
    torch.cuda.synchronize()
    return out, blk.generator.get_state()


@pytest.mark.parametrize("with_mlp", [False, True], ids=["alone", "with-merge_mlp"])
@pytest.mark.parametrize("merge_global", [False, True], ids=["local", "global"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_whole_block_through_the_public_api(L, dtype, merge_global, with_mlp):
    import vidtome_amd
    from vidtome_amd import patch as vpatch, sites as S
    from vidtome_amd.utils import join_frame
    unet = _unet(WC, dtype)
    blk = _apply(unet, merge_global)
    chunks = [_tokens(WC, dtype, c) for c in range(2 if merge_global else 1)]
    cond = _cond(dtype)
    flags = dict(merge_crossattn=True, **({"merge_mlp": True} if with_mlp else {}))
    try:
        off, state_off = _forward(blk, chunks, cond)
        assert vidtome_amd.update_patch(unet, **flags) is unet
        calls = []
        orig = L.attention_kv_segments
        L.attention_kv_segments = lambda *a, **k: calls.append(1) or orig(*a, **k)
        try:
            on, state_on = _forward(blk, chunks, cond)
        finally:
            L.attention_kv_segments = orig
        assert len(calls) == len(chunks), "the segments kernel did not run once per chunk"
        assert torch.equal(state_on, state_off), "the flag moved the generator"
        assert not torch.equal(on, off)
        # the restatement.  The flag-off block without attn2 and with a zero feed-forward gives the hidden states in front of
        # attn2 and, from the same generator state, the plan.
        vidtome_amd.update_patch(unet, merge_crossattn=False, merge_mlp=False)
        attn2, ff = blk.attn2, blk.ff
        plans = []
        real = vpatch.compute_merge

        def rec(*a, **k):
            res = real(*a, **k)
            plans.append(getattr(res[0], "plan", None))
            return res
        vpatch.compute_merge = rec
        blk.attn2, blk.ff = None, standin.Zero()
        try:
            pre, _ = _forward(blk, chunks, cond)
        finally:
            blk.attn2, blk.ff = attn2, ff
            vpatch.compute_merge = real
        plan = plans[-1]
        assert len(plans) == len(chunks) and (plan.global_level is not None) == merge_global and len(plan.levels) == 2
        n64, f64 = torch.nn.LayerNorm(WC, eps=blk.norm3.eps), S.FeedForward(WC)
        n64.load_state_dict(blk.norm3.state_dict())
        f64.load_state_dict(ff.state_dict())
        n64, f64 = n64.to(DEV).double(), f64.to(DEV).double()
        with torch.no_grad():
            h2, h2_plain = _merged_attn2_64(blk, pre, cond, plan)
            if with_mlp:
                ref = _pick(f64(n64(_pick(h2, plan.keep))), plan.inv_local) + h2
            else:
                ref = f64(n64(h2)) + h2
            ref_plain = f64(n64(h2_plain)) + h2_plain
        err = _ratio(join_frame(on, F), ref)
        apart = float((ref - ref_plain).abs().max()) / max(1.0, float(ref.abs().max()))
        print(f"merge_crossattn whole block {_name(dtype)} global={merge_global} mlp={with_mlp} err/scale={err:.3e} "
              f"(merged vs plain restatement {apart:.3e}; flag off vs the plain one {_ratio(join_frame(off, F), ref_plain):.3e})")
        assert apart > 10 * BLOCK_TOL[dtype], "the merged and the plain restatement must differ far beyond the tolerance"
        assert err < BLOCK_TOL[dtype], err
        # after remove_patch + apply_patch the flag is gone
        vidtome_amd.update_patch(unet, **flags)
        vidtome_amd.remove_patch(unet)
        assert not any(hasattr(b, "merge_crossattn") for b in unet.blocks)
        blk = _apply(unet, merge_global)
        assert not any(hasattr(b, "merge_crossattn") for b in unet.blocks)
        again, _ = _forward(blk, chunks, cond)
        assert torch.equal(again, off)
    finally:
        vidtome_amd.remove_patch(unet)


# ---------------------------------------------------------------------------------------------------
# 5. the "plain" conditions: the flag changes no bit
# ---------------------------------------------------------------------------------------------------
NOOP_SIDE = 16                     # 256 tokens per frame


class AdaNorm(torch.nn.Module):
    """AdaLayerNorm's call: (tokens, timestep)."""

    def __init__(self, c):
        super().__init__()
        self.norm = torch.nn.LayerNorm(c)

    def forward(self, x, timestep):
        return self.norm(x)


class ZeroAttention(torch.nn.Module):
    """attn2's own forward for the "module" route (the site stand-ins have none): zeros."""

    def forward(self, x, encoder_hidden_states=None, attention_mask=None, **kw):
        return torch.zeros_like(x)


NOOPS = ["flag False", "flag 1", "site that does not merge", "single-frame chunk", "local_merge_ratio 0", "blas route",
         "f32 route", "module route", "AdaLayerNorm block", "encoder_attention_mask", "IP-Adapter call",
         "control injecting", "control outside its schedule", "attention maps", "LocalBlend", "conditioning rows != B F"]


def _noop_case(what, monkeypatch):
    """(unet, block, hidden states, conditioning, forward keywords, the flag's value) of one "plain" condition."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch, sites as S
    import cross_control_standin
    import ip_adapter_standin
    dt = torch.float32 if what in ("f32 route", "module route") else torch.float16
    unmerged = what == "site that does not merge"
    frames = 1 if what == "single-frame chunk" else F
    unet = S.SiteUNet([S.Site("site", 2 if unmerged else 1, WC, HEADS)], seed=3, full=True).to(device=DEV, dtype=dt)
    vidtome_amd.apply_patch(unet, local_merge_ratio=0.0 if what == "local_merge_ratio 0" else 0.5, batch_size=B,
                            max_downsample=1, target_stride=2)
    unet.set_size((NOOP_SIDE, NOOP_SIDE))
    blk = unet.blocks[0]
    n, Nn = B * frames, (NOOP_SIDE // (2 if unmerged else 1)) ** 2
    g = torch.Generator().manual_seed(8)
    h = (torch.randn(B, 1, Nn, WC, generator=g) + 0.1 * torch.randn(B, frames, Nn, WC, generator=g)).reshape(n, Nn, WC)
    h = h.to(device=DEV, dtype=dt)
    enc = (torch.randn(n, COND, COND_DIM, generator=g) * 0.7).to(device=DEV, dtype=dt)
    kw, flag = {}, True
    if what == "flag False":
        flag = False
    elif what == "flag 1":
        flag = 1
    elif what == "blas route":
        monkeypatch.setattr(vpatch, "FF_MODE", "blas")
    elif what == "f32 route":
        vidtome_amd.update_patch(unet, fp32_projections=True)
    elif what == "module route":
        blk.attn2.__class__ = type("Attention", (ZeroAttention, type(blk.attn2)), {})
    elif what == "AdaLayerNorm block":
        for name in ("norm1", "norm2"):
            ada = AdaNorm(WC).to(device=DEV, dtype=dt)
            ada.norm.load_state_dict(getattr(blk, name).state_dict())
            setattr(blk, name, ada)
        blk.use_ada_layer_norm = True
        kw["timestep"] = torch.tensor([500], device=DEV)
    elif what == "encoder_attention_mask":
        live = torch.arange(COND)[None, :] < torch.tensor([57, 30, 77] * frames)[:, None]
        kw["encoder_attention_mask"] = ((1 - live.to(dt)) * -10000.0).unsqueeze(1).to(DEV)
    elif what == "IP-Adapter call":
        ip_adapter_standin.install(unet, (4, 16), (0.6, 0.3))
        enc = (enc, ip_adapter_standin.image_states((4, 16), n, COND_DIM, dt, DEV))
    elif what.startswith("control"):
        swap = cross_control_standin.edit_of(cross_control_standin.specs(COND)["replace"])
        vidtome_amd.register_cross_attention_control(unet, [981], 4, {1: vidtome_amd.CrossEdit.identity(COND), 2: swap})
        blk.attn2.t = 981 if what == "control injecting" else 941
    elif what == "attention maps":
        vidtome_amd.register_attention_maps(unet)
    elif what == "LocalBlend":
        w = torch.rand(2, COND, generator=g)
        vidtome_amd.register_local_blend(unet, vidtome_amd.LocalBlend({0: w[0], 1: w[1]}, B, n // B))
    elif what == "conditioning rows != B F":
        enc = torch.cat([enc, enc[:1]])                     # one row set too many: the plain path reads the first B F
    return unet, blk, h, enc, kw, flag


@pytest.mark.filterwarnings("ignore:vidtome_amd")
@pytest.mark.parametrize("what", NOOPS)
def test_plain_conditions_change_no_bit(L, what, monkeypatch):
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    monkeypatch.setattr(vpatch, "_warned", set())
    unet, blk, h, enc, kw, flag = _noop_case(what, monkeypatch)
    try:
        off, state_off = _forward(blk, [h], enc, **kw)
        vidtome_amd.update_patch(unet, merge_crossattn=flag)
        routes = []
        real_route = vpatch.cross_merge_route
        monkeypatch.setattr(vpatch, "cross_merge_route", lambda *a, **k: routes.append(real_route(*a, **k)) or routes[-1])
        monkeypatch.setattr(L, "attention_kv_segments", lambda *a, **k: pytest.fail("the segments kernel ran"))
        on, state_on = _forward(blk, [h], enc, **kw)
        assert routes == ["plain"], routes
        assert torch.equal(on, off) and torch.equal(state_on, state_off)
        assert bool(torch.isfinite(on.float()).all())
        vidtome_amd.remove_patch(unet)
        assert not any(hasattr(b, "merge_crossattn") for b in unet.blocks)
    finally:
        vidtome_amd.remove_patch(unet)


def test_the_merging_site_of_the_plain_cases_does_merge(L):
    """The control of the test above: the same block, the same tokens, no "plain" condition -- the flag takes the merged
    route and changes the output."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    unet, blk, h, enc, kw, _ = _noop_case("none", None)
    try:
        off, _ = _forward(blk, [h], enc)
        vidtome_amd.update_patch(unet, merge_crossattn=True)
        routes = []
        real_route = vpatch.cross_merge_route
        vpatch.cross_merge_route = lambda *a, **k: routes.append(real_route(*a, **k)) or routes[-1]
        try:
            on, _ = _forward(blk, [h], enc)
        finally:
            vpatch.cross_merge_route = real_route
        assert routes == ["merged-panels"] and not torch.equal(on, off)
    finally:
        vidtome_amd.remove_patch(unet)
