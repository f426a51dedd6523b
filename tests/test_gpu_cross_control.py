"""GPU tests of Prompt-to-Prompt cross-attention control on the fused attn2 path (run with -m gpu on an MI355X):
vtm_attention_kv_sets_src and vtm_cross_edit_values through the C ABI against float64 on the same rounded operands, then
the patched block with register_cross_attention_control against the float64 restatement of P2P's controllers
(tests/cross_control_standin.py).

Tolerances are the project's own: TOL of the output scale for the attention core, BLOCK_TOL for a whole block
(INTEGRATION.md section 1).  vtm_cross_edit_values is held to the rounding of its own arithmetic, not to a tolerance."""
import numpy as np
import pytest
import torch

import cross_control_standin as CC

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = (torch.float16, torch.bfloat16)
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}            # the attention core's figures
BLOCK_TOL = {torch.float16: 2e-3, torch.bfloat16: 8e-3}      # the whole block's
ULP_HALF = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SENTINEL = -7.0
EINVAL = -1
# (B, h, Mq, K, d)
CASES = [(2, 2, 70, 77, 40),      # pad between the sets, two key tiles per set, partial query block
         (1, 5, 33, 1, 64),       # single-key sets: out = v'[0] + v''[0]
         (1, 2, 40, 64, 80),      # key tile edge
         (1, 2, 40, 65, 80),      # ... one past
         (2, 8, 65, 33, 8),       # smallest head dim
         (2, 1, 257, 256, 160)]   # the 4-wave instantiation, several query blocks, the key limit


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _r8(n):
    return (n + 7) // 8 * 8


def _operands(B, h, Mq, lens, d, dtype, seed, Mqp=None, Mqp_src=None, pad=0.0):
    """q, q_src (other data), k (B, sum of the sets' lengths rounded up to 8, C), v of the same rows; rows / columns
    outside the sets hold ``pad``.  Returns the host tensors and the sets' starts."""
    g = torch.Generator().manual_seed(seed)
    C = h * d
    q = torch.randn(B, Mqp or Mq, C, generator=g).to(dtype)
    q_src = torch.randn(B, Mqp_src or Mq, C, generator=g).to(dtype)
    starts, pos = [], 0
    for n in lens:
        starts.append(pos)
        pos += _r8(n)
    k = torch.full((B, pos, C), pad).to(dtype)
    v = torch.full((B, pos, C), pad).to(dtype)
    for s, n in zip(starts, lens):
        k[:, s:s + n] = torch.randn(B, n, C, generator=g).to(dtype)
        v[:, s:s + n] = torch.randn(B, n, C, generator=g).to(dtype)
    return q, q_src, k, v, starts


def _ref(q, q_src, k, v, h, Mq, sets, set_src):
    """float64 sum_s w_s softmax(Q_s k_s^T d^-0.5) v_s on the same 16-bit operands."""
    B, d = q.shape[0], q.shape[2] // h
    sh = lambda t: t.double().numpy().reshape(B, t.shape[1], h, d).transpose(0, 2, 1, 3)
    out = 0.0
    for (start, n, w), src in zip(sets, set_src):
        s = sh((q_src if src else q)[:, :Mq]) @ sh(k[:, start:start + n]).transpose(0, 1, 3, 2) * float(d) ** -0.5
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        out = out + w * (p @ sh(v[:, start:start + n]))
    return out.transpose(0, 2, 1, 3).reshape(B, Mq, h * d)


def _vt(v):
    return v.transpose(1, 2).contiguous()


def _raw(L, q, q_src, k, vt, out, h, Mq, d, sets, set_src, code=None, ldq_src=None, Mqp_src=None, q_src_ptr=None, ldo=None):
    n = len(sets)
    i64, f32, i32 = L._i64, L._f32, L._int
    return L.lib().vtm_attention_kv_sets_src(
        q.data_ptr(), q.stride(1), q_src.data_ptr() if q_src_ptr is None else q_src_ptr,
        q_src.stride(1) if ldq_src is None else ldq_src, q_src.shape[1] if Mqp_src is None else Mqp_src, k.data_ptr(),
        k.stride(1), vt.data_ptr(), vt.stride(1), out.data_ptr(), out.stride(1) if ldo is None else ldo,
        L.dtype_code(q) if code is None else code, q.shape[0], h, Mq, q.shape[1], k.shape[1], d, d ** -0.5, n,
        (i64 * n)(*[s[0] for s in sets]), (i64 * n)(*[s[1] for s in sets]), (f32 * n)(*[s[2] for s in sets]),
        (i32 * n)(*set_src), torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------
# 1. vtm_attention_kv_sets_src
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernel_vs_float64(L, case, dtype):
    B, h, Mq, K, d = case
    q, q_src, k, v, starts = _operands(B, h, Mq, (K, K), d, dtype, seed=sum(case))
    sets, set_src = [(starts[0], K, 1.0), (starts[1], K, 1.0)], (1, 0)
    dev = [t.to(DEV) for t in (q, q_src, k, _vt(v))]
    got = L.attention_kv_sets_src(dev[0], dev[1], dev[2], dev[3], h, Mq, sets, d ** -0.5, set_src)
    ref = _ref(q, q_src, k, v, h, Mq, sets, set_src)
    osc = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got.double().cpu().numpy() - ref).max()) / osc
    print(f"attention_kv_sets_src {case} {dtype} err/scale={err:.3e} tol={TOL[dtype]:.0e}")
    assert err < TOL[dtype], (case, err)
    if K == 1:      # every probability is 1: the sum of the two value rows, rounded once
        want = (v[:, starts[0]].float() + v[:, starts[1]].float()).to(dtype)[:, None].expand(B, Mq, h * d)
        assert float((got.cpu().float() - want.float()).abs().max()) <= 2 * ULP_HALF[dtype] * float(want.float().abs().max())
    again = L.attention_kv_sets_src(dev[0], dev[1], dev[2], dev[3], h, Mq, sets, d ** -0.5, set_src)
    assert torch.equal(got, again), "two calls differ"
    # the source sample's queries matter: the same call on q alone is another result (but for one key, probability 1)
    assert K == 1 or not torch.equal(got, L.attention_kv_sets(dev[0], dev[2], dev[3], h, Mq, sets, d ** -0.5))


@pytest.mark.parametrize("dtype", DTYPES)
def test_three_sets_mixed_sources_and_weights(L, dtype):
    B, h, Mq, d = 2, 2, 70, 40
    lens = (77, 5, 64)
    q, q_src, k, v, starts = _operands(B, h, Mq, lens, d, dtype, seed=11)
    sets = [(s, n, w) for s, n, w in zip(starts, lens, (1.0, -0.5, 2.0))]
    set_src = (0, 1, 0)
    dev = [t.to(DEV) for t in (q, q_src, k, _vt(v))]
    got = L.attention_kv_sets_src(dev[0], dev[1], dev[2], dev[3], h, Mq, sets, d ** -0.5, set_src)
    ref = _ref(q, q_src, k, v, h, Mq, sets, set_src)
    osc = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got.double().cpu().numpy() - ref).max()) / osc
    print(f"attention_kv_sets_src three sets {dtype} err/scale={err:.3e}")
    assert err < TOL[dtype], err
    assert torch.equal(got, L.attention_kv_sets_src(dev[0], dev[1], dev[2], dev[3], h, Mq, sets, d ** -0.5, set_src))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [40, 160])
def test_bit_identities_with_the_plain_sets_kernel(L, d, dtype):
    B, h, Mq, K = 2, 2, 70, 77
    q, q_src, k, v, starts = _operands(B, h, Mq, (K, K), d, dtype, seed=d)
    sets = [(starts[0], K, 1.0), (starts[1], K, 0.75)]
    qd, qs, kd, vtd = [t.to(DEV) for t in (q, q_src, k, _vt(v))]
    plain = L.attention_kv_sets(qd, kd, vtd, h, Mq, sets, d ** -0.5)
    assert torch.equal(L.attention_kv_sets_src(qd, qs, kd, vtd, h, Mq, sets, d ** -0.5, (0, 0)), plain), "set_src all 0"
    assert torch.equal(L.attention_kv_sets_src(qd, qd, kd, vtd, h, Mq, sets, d ** -0.5, (1, 0)), plain), "q_src is q"
    assert torch.equal(L.attention_kv_sets_src(qd, qd, kd, vtd, h, Mq, sets, d ** -0.5, (1, 1)), plain), "q_src is q, both"


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_strides_pads_and_sentinels(L, dtype):
    """q_src with another leading dimension and more rows than Mq (NaN in its pad rows and around its columns), NaN in the
    key rows outside both sets and the V^T columns outside both ranges, ``out`` wider than h d and longer than Mq."""
    B, h, Mq, K, d = 2, 2, 70, 77, 40
    C, Mqp, Mqp_src = h * d, 72, 80
    q, q_src, k, v, starts = _operands(B, h, Mq, (K, K), d, dtype, seed=5, Mqp=Mqp, Mqp_src=Mqp_src, pad=float("nan"))
    q[:, Mq:] = float("nan")
    q_src[:, Mq:] = float("nan")
    wide = torch.full((B, Mqp_src, 3 * C), float("nan"), dtype=dtype)
    wide[:, :, C:2 * C] = q_src
    qs = wide.to(DEV)[:, :, C:2 * C]
    assert qs.stride(1) == 3 * C != C
    sets, set_src = [(starts[0], K, 1.0), (starts[1], K, 1.0)], (1, 0)
    qd, kd, vtd = q.to(DEV), k.to(DEV), _vt(v).to(DEV)
    ldo = C + 8
    out = torch.full((B, Mqp, ldo), SENTINEL, dtype=dtype, device=DEV)
    rc = _raw(L, qd, qs, kd, vtd, out, h, Mq, d, sets, set_src)
    assert rc == 0, L.lib().vtm_last_error()
    torch.cuda.synchronize()
    assert bool((out[:, Mq:] == SENTINEL).all()) and bool((out[:, :, C:] == SENTINEL).all())
    ref = _ref(q, q_src, k, v, h, Mq, sets, set_src)
    osc = max(1.0, float(np.abs(ref).max()))
    got = out[:, :Mq, :C].double().cpu().numpy()
    assert np.isfinite(got).all()
    assert float(np.abs(got - ref).max()) / osc < TOL[dtype]
    # the wrapper on the same views gives the same bits
    via = L.attention_kv_sets_src(qd, qs, kd, vtd, h, Mq, sets, d ** -0.5, set_src)
    assert torch.equal(via[:, :Mq], out[:, :Mq, :C]) and bool((via[:, Mq:] == 0).all())


def test_bad_arguments_launch_nothing(L):
    B, h, Mq, K, d = 1, 2, 40, 33, 40
    dtype = torch.float16
    q, q_src, k, v, starts = _operands(B, h, Mq, (K, K), d, dtype, seed=1)
    qd, qs, kd, vtd = [t.to(DEV) for t in (q, q_src, k, _vt(v))]
    out = torch.full((B, Mq, h * d), SENTINEL, dtype=dtype, device=DEV)
    sets, src = [(starts[0], K, 1.0), (starts[1], K, 1.0)], (1, 0)
    err = lambda: L.lib().vtm_last_error().decode()
    assert _raw(L, qd, qs, kd, vtd, out, h, Mq, d, sets, src, q_src_ptr=0) == EINVAL and "vtm_attention_kv_sets_src" in err()
    for bad in ((2, 0), (0, -1)):
        assert _raw(L, qd, qs, kd, vtd, out, h, Mq, d, sets, bad) == EINVAL and "vtm_attention_kv_sets_src" in err()
    assert _raw(L, qd, qs, kd, vtd, out, h, Mq, d, sets, src, Mqp_src=Mq - 1) == EINVAL and "Mqp_src" in err()
    assert _raw(L, qd, qs, kd, vtd, out, h, Mq, d, sets, src, ldq_src=h * d + 4) == EINVAL and "ldq_src" in err()
    assert _raw(L, qd, qs, kd, vtd, out, h, Mq, d, sets, src, code=L.VTM_F32) == EINVAL and "vtm_attention_kv_sets_src" in err()
    odd = [(starts[0], K, 1.0), (starts[1] + 4, K - 4, 1.0)]                                  # a set that starts off a multiple of 8
    assert _raw(L, qd, qs, kd, vtd, out, h, Mq, d, odd, src) == EINVAL and "vtm_attention_kv_sets_src" in err()
    assert _raw(L, qd, qs, kd, vtd, out, h, Mq, d, odd, (0, 0)) == EINVAL and "vtm_attention_kv_sets_src" in err()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert _raw(L, qd, qs, kd, vtd, out, h, Mq, d, sets, src) == 0                            # the good call runs
    assert _raw(L, qd, qs, kd, vtd, out, h, Mq, d, sets, (0, 0), q_src_ptr=0) == 0           # no set reads q_src: not looked at
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


# ---------------------------------------------------------------------------------------------------
# 2. vtm_cross_edit_values
# ---------------------------------------------------------------------------------------------------
def _edit_operands(B, C, K, dtype, seed, v_start=8):
    g = torch.Generator().manual_seed(seed)
    ldvt = v_start + _r8(K) + 8
    vt = torch.full((B, C, ldvt), float("nan")).to(dtype)
    vt[:, :, v_start:v_start + K] = torch.randn(B, C, K, generator=g).to(dtype)
    mapper = torch.randn(K, K, generator=g) * ((torch.rand(K, K, generator=g) < 0.3) | torch.eye(K, dtype=torch.bool))
    a, b = torch.randn(K, generator=g), torch.randn(K, generator=g)
    return vt, mapper.contiguous(), a, b


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [1, 77, 256])
def test_edit_values_vs_float64(L, K, dtype):
    """Every element of the src range within (K + 2) 2^-24 sum_n |M[w, n] a[n] V[n, c]| -- the rounding of the fp32 product
    and of the fp32 fmaf chain -- plus half an ulp of the dtype at the reference value, the one final rounding; the own range
    bit-equal to round(fp32(b[n]) * fp32(V)); columns outside the two ranges keep their sentinel."""
    B, C, v_start = 2, 44, 8                              # (44 channels: a partial channel group)
    vt, mapper, a, b = _edit_operands(B, C, K, dtype, seed=K, v_start=v_start)
    K8 = _r8(K)
    start_src, start_own, ld_out = 8, 16 + K8, 32 + 2 * K8
    out = torch.full((B, C, ld_out), SENTINEL, dtype=dtype, device=DEV)
    got = L.cross_edit_values(vt.to(DEV), v_start, K, mapper.to(DEV), a.to(DEV), b.to(DEV), start_src, start_own, out=out)
    assert got is out
    o = out.cpu()
    keep = torch.ones(ld_out, dtype=torch.bool)
    keep[start_src:start_src + K] = False
    keep[start_own:start_own + K] = False
    assert bool((o[:, :, keep] == SENTINEL).all()), "a column outside the ranges was written"
    V = vt[:, :, v_start:v_start + K]                                                        # (B, C, K) = V[b, n, c]^T
    own = (b.float() * V.float()).to(dtype)
    got_own = o[:, :, start_own:start_own + K]
    for i in (got_own != own).nonzero()[:4].tolist():
        print(f"own range differs at {i}: b={float(b[i[2]])!r} V={float(V[tuple(i)])!r} got={float(got_own[tuple(i)])!r} "
              f"want={float(own[tuple(i)])!r}")
    assert torch.equal(got_own, own), "own range"
    ma = (mapper.double() * a.double())                                                       # (w, n)
    ref = torch.einsum("wn,bcn->bcw", ma, V.double())
    mag = torch.einsum("wn,bcn->bcw", ma.abs(), V.double().abs())
    bound = (K + 2) * 2.0 ** -24 * mag + ULP_HALF[dtype] * ref.abs() + 2.0 ** -25          # (+ the smallest subnormal step)
    over = (o[:, :, start_src:start_src + K].double() - ref).abs() - bound
    print(f"cross_edit_values K={K} {dtype} max(err - bound)={float(over.max()):.3e} max|ref|={float(ref.abs().max()):.3e}")
    assert float(over.max()) <= 0.0, float(over.max())
    again = torch.full_like(out, SENTINEL)
    L.cross_edit_values(vt.to(DEV), v_start, K, mapper.to(DEV), a.to(DEV), b.to(DEV), start_src, start_own, out=again)
    assert torch.equal(again, out), "two calls differ"


def test_edit_values_bad_arguments_launch_nothing(L):
    B, C, K, dtype = 1, 16, 33, torch.float16
    vt, mapper, a, b = _edit_operands(B, C, K, dtype, seed=3)
    vtd, md, ad, bd = vt.to(DEV), mapper.to(DEV), a.to(DEV), b.to(DEV)
    big = torch.zeros(300, 300, device=DEV)
    out = torch.full((B, C, 640), SENTINEL, dtype=dtype, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def raw(vt_=vtd, K_=K, out_=out, start_src=0, start_own=40, ld_out=640, m=md, code=None, ldvt=None, v_start=8):
        return L.lib().vtm_cross_edit_values(vt_.data_ptr(), vt_.shape[2] if ldvt is None else ldvt, v_start,
                                             L.dtype_code(vt_) if code is None else code, B, C, K_, m.data_ptr(), ad.data_ptr(),
                                             bd.data_ptr(), out_.data_ptr(), ld_out, start_src, start_own, st)
    err = lambda: L.lib().vtm_last_error().decode()
    assert raw(start_own=32) == EINVAL and "vtm_cross_edit_values" in err() and "overlap" in err()      # 0 + 33 > 32
    assert raw(start_src=40, start_own=8) == EINVAL and "overlap" in err()
    assert raw(start_own=36) == EINVAL and "multiples of 8" in err()
    assert raw(start_own=616) == EINVAL and "ldvt_out" in err()                                         # 616 + 33 > 640
    assert raw(K_=257, m=big, ldvt=300, start_own=264) == EINVAL and "257" in err()                     # K > 256
    assert raw(K_=0) == EINVAL
    assert raw(out_=vtd) == EINVAL and "overlaps vt" in err()                                           # aliasing
    assert raw(code=L.VTM_F32) == EINVAL and "vtm_cross_edit_values" in err()
    assert raw(v_start=vtd.shape[2] - 8) == EINVAL                                                      # keys outside vt
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert raw() == 0
    torch.cuda.synchronize()
    assert not bool((out[:, :, :K] == SENTINEL).any()) and bool((out[:, :, K:40] == SENTINEL).all())
    with pytest.raises(RuntimeError, match="1 .. 256 keys"):
        L.cross_edit_values(torch.zeros(1, 8, 264, dtype=dtype, device=DEV), 0, 257, big[:257, :257].contiguous(),
                            big[0, :257].contiguous(), big[0, :257].contiguous())


# ---------------------------------------------------------------------------------------------------
# 3. the patched block
# ---------------------------------------------------------------------------------------------------
def _forward(unet, h, cond, **kw):
    with torch.no_grad():
        return unet.block(h, encoder_hidden_states=cond, **kw)


def _spies(monkeypatch, L):
    """Counts the launches of the attn2 segment and keeps the q / k rows the probabilities launch read."""
    seen = {"kv": [], "sets_src": [], "edit": 0, "probs": 0}
    orig_kv, orig_src, orig_edit, orig_probs = L.attention_kv, L.attention_kv_sets_src, L.cross_edit_values, L.attention_probs

    def kv(*a, **kw):
        if a[5] == CC.COND:                                   # (attn1's launches have other key counts)
            seen["kv"].append(a[0].shape[0])
        return orig_kv(*a, **kw)

    def src(*a, **kw):
        seen["sets_src"].append((a[0].shape[0], tuple(a[8]), [s[:2] for s in a[6]]))
        return orig_src(*a, **kw)

    def edit(*a, **kw):
        seen["edit"] += 1
        return orig_edit(*a, **kw)

    def probs(*a, **kw):
        seen["probs"] += 1
        seen["q"], seen["k"] = a[0], a[1]
        return orig_probs(*a, **kw)
    monkeypatch.setattr(L, "attention_kv", kv)
    monkeypatch.setattr(L, "attention_kv_sets_src", src)
    monkeypatch.setattr(L, "cross_edit_values", edit)
    monkeypatch.setattr(L, "attention_probs", probs)
    return seen


@pytest.fixture(scope="module")
def block_case():
    """{(C, dtype, mode): (unet, h, cond, unregistered output)}: one patched block and its uncontrolled output per case,
    shared by the three controllers (the output behind a warm-up forward: DESIGN.md section 9)."""
    import vidtome_amd
    cache = {}

    def get(C, dtype, mode):
        key = (C, dtype, mode)
        if key not in cache:
            unet = CC.patched(C, dtype, DEV)
            h, cond = CC.inputs(C, dtype, DEV)
            _forward(unet, h, cond)
            cache[key] = (unet, h, cond, _forward(unet, h, cond))
        return cache[key]
    yield get
    for unet, *_ in cache.values():
        vidtome_amd.remove_patch(unet)


@pytest.mark.parametrize("name", ["replace", "refine", "refine_reweight"])
@pytest.mark.parametrize("mode", ["panels", "blas"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [320, 640])
def test_controlled_block_vs_float64_p2p(L, block_case, C, dtype, mode, name, monkeypatch):
    """The stand-in block (attn1's and attn2's module forward raise) through apply_patch, [source | uncond | cond] x 2 frames
    of 70 tokens, 77 text tokens, C = 320 / d = 40 and C = 640 / d = 80, the cond group edited, fractional alpha_words:
    every row of the output against the float64 restatement of P2P within BLOCK_TOL of the output scale; the edit moves the
    cond rows by more than 2 BLOCK_TOL; source and uncond rows, and the whole output outside the schedule, are the bits of
    the unregistered run.  ``blas``: the library-GEMM route around the core (VIDTOME_FF=blas)."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch, pnp
    import standin
    if mode == "blas":
        monkeypatch.setattr(vpatch, "FF_MODE", "blas")
    unet, h, cond, base = block_case(C, dtype, mode)
    seen = _spies(monkeypatch, L)
    spec = CC.specs()[name]
    assert vidtome_amd.register_cross_attention_control(unet, [981, 961], CC.NUM_INPUTS, {2: CC.edit_of(spec)}) == [CC.BLOCK]
    pnp.register_time(standin.Pipe(unet), 961)
    out = _forward(unet, h, cond)
    F2 = 2 * CC.FRAMES
    assert seen["kv"] == [F2] and seen["edit"] == 1 and seen["sets_src"] == [(CC.FRAMES, (1, 0), [(0, 77), (80, 77)])], seen
    ref = CC.block64(unet.block, h, cond, {2: spec})
    osc = max(1.0, float(ref.abs().max()))
    err = float((out.double().cpu() - ref).abs().max()) / osc
    moved = float((out[F2:].double() - base[F2:].double()).abs().max()) / osc
    print(f"controlled block {name} C={C} {dtype} {mode} err/scale={err:.3e} edit/scale={moved:.3e} tol={BLOCK_TOL[dtype]:.0e}")
    assert err < BLOCK_TOL[dtype], (name, C, err)
    assert moved > 2 * BLOCK_TOL[dtype], "the edit is not noise"
    assert torch.equal(out[:F2], base[:F2]), "source / uncond rows changed"
    pnp.register_time(standin.Pipe(unet), 941)                                               # outside the schedule
    seen.update(kv=[], sets_src=[], edit=0)
    assert torch.equal(_forward(unet, h, cond), base), "a step outside the schedule changed"
    assert seen["kv"] == [CC.NUM_INPUTS * CC.FRAMES] and seen["edit"] == 0 and seen["sets_src"] == []
    vidtome_amd.unregister_cross_attention_control(unet)
    pnp.register_time(standin.Pipe(unet), 961)
    assert torch.equal(_forward(unet, h, cond), base), "unregistering did not switch the control off"


@pytest.mark.parametrize("dtype", DTYPES)
def test_maps_of_an_edited_group_are_the_edited_maps(L, block_case, dtype, monkeypatch):
    """With register_attention_maps on the same block: attn2_probs of the edited group within (K + 8) 2^-24 (1 + sum |a| +
    sum |b|) of the float64 edited head-average on the 16-bit q / k rows the core read; the unedited groups' maps are the bits
    of a run without the control."""
    import vidtome_amd
    from vidtome_amd import pnp
    import attention_maps_standin as AM
    import standin
    C, name = 320, "refine_reweight"
    unet, h, cond, base = block_case(C, dtype, "panels")
    blk = unet.block
    vidtome_amd.register_attention_maps(unet)
    assert torch.equal(_forward(unet, h, cond), base)
    plain = blk.attn2_probs
    seen = _spies(monkeypatch, L)
    spec = CC.specs()[name]
    e = CC.edit_of(spec)
    vidtome_amd.register_cross_attention_control(unet, [981], CC.NUM_INPUTS, {2: e})
    pnp.register_time(standin.Pipe(unet), 981)
    _forward(unet, h, cond)
    got = blk.attn2_probs
    F2 = 2 * CC.FRAMES
    assert seen["probs"] == 1 and tuple(got.shape) == (3 * CC.FRAMES, CC.TOKENS, CC.COND) and got.dtype == torch.float32
    assert torch.equal(got[:F2], plain[:F2]), "an unedited group's map changed"
    n, heads = h.shape[0], CC.HEADS
    sh = lambda t, rows: t[:, :rows].double().cpu().view(n, rows, heads, -1).transpose(1, 2)
    per_head = torch.softmax(sh(seen["q"], CC.TOKENS) @ sh(seen["k"], CC.COND).transpose(-1, -2) * blk.attn2.scale, dim=-1)
    assert float((plain.double().cpu() - per_head.mean(1)).abs().max()) <= (CC.COND + 8) * 2.0 ** -24
    bound = (CC.COND + 8) * 2.0 ** -24 * (1 + float(e.src_weight.abs().sum()) + float(e.own_weight.abs().sum()))
    for f in range(CC.FRAMES):
        want = CC.controlled_probs(spec, per_head[f], per_head[F2 + f]).mean(0)
        err = float((got[F2 + f].double().cpu() - want).abs().max())
        print(f"edited map {dtype} frame {f}: max|map - float64|={err:.3e} bound={bound:.3e}")
        assert err <= bound, err
    assert float((got[F2:] - plain[F2:]).abs().max()) > 1e-3, "the map was not edited"
    vidtome_amd.unregister_cross_attention_control(unet)
    vidtome_amd.unregister_attention_maps(unet)


class IPAdapterAttnProcessor2_0:
    """An IP-Adapter processor stand-in: the name is what the block looks at."""


@pytest.mark.parametrize("case", ["fp32", "mask", "ip_adapter", "K=257"])
def test_what_the_control_does_not_take_raises_before_any_launch(L, case, monkeypatch):
    import vidtome_amd
    from vidtome_amd import pnp
    import standin
    C = 320
    dtype = torch.float32 if case == "fp32" else torch.float16
    K = 257 if case == "K=257" else CC.COND
    unet = CC.patched(C, dtype, DEV)
    h, cond = CC.inputs(C, dtype, DEV, K=K)
    kw = {}
    if case == "mask":
        kw["encoder_attention_mask"] = torch.zeros(h.shape[0], 1, K, dtype=dtype, device=DEV)
    if case == "ip_adapter":
        unet.block.attn2.processor = IPAdapterAttnProcessor2_0()
    vidtome_amd.register_cross_attention_control(unet, [981], CC.NUM_INPUTS, {2: vidtome_amd.CrossEdit.replace(torch.eye(K), 0.5)})
    pnp.register_time(standin.Pipe(unet), 981)
    seen = _spies(monkeypatch, L)
    launched = []
    for fn in ("layernorm_panels", "linear_panels", "to_panels", "layernorm"):
        orig = getattr(L, fn)
        monkeypatch.setattr(L, fn, lambda *a, _o=orig, _n=fn, **k: (launched.append((_n, a[0])), _o(*a, **k))[1])
    h0 = h.clone()
    with pytest.raises(RuntimeError, match=CC.BLOCK.replace(".", r"\.")) as ei:
        _forward(unet, h, cond, **kw)
    print(f"{case}: {ei.value}")
    assert {"fp32": "float32", "mask": "attention_mask", "ip_adapter": "IP-Adapter", "K=257": "K = 257"}[case] in str(ei.value)
    assert seen["kv"] == [] and seen["sets_src"] == [] and seen["edit"] == 0 and seen["probs"] == 0
    # nothing of the attn2 segment ran: every LayerNorm launch so far was norm1's (attn1's segment) on the block's input
    assert all(x.shape == h.shape for n_, x in launched if n_ in ("layernorm_panels", "layernorm"))
    assert len([1 for n_, _ in launched if n_ in ("layernorm_panels", "layernorm")]) <= 1
    assert torch.equal(h, h0), "the hidden states were touched"
    vidtome_amd.remove_patch(unet)
