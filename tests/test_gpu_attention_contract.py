"""GPU test of the operand contract of the ten attention wrappers of vidtome_amd._lib (attention, attention_kv,
attention_kv_sets / _sets_masked / _sets_src, attention_kv_bias, attention_kv_segments, attention_probs, attention_word_map,
attention_key_mass): every rule their shared helpers state (_out_like_q, _half_operands, _kv_shapes, _key_sets, _key_rows,
_qk_views), broken once per wrapper that has it, raises a RuntimeError whose whole text is pinned here; a single sample
that is not a dense stride away is refused by attention_probs alone; one valid call each.

Every violation keeps all operands as large as the sizes passed (a wrong dtype, a view, a too-small declared bound, a CPU
tensor -- never a short buffer): a check that wrongly let one through would end in a library VTM_EINVAL or a wrong number.

Tolerances of the valid calls, against float64 softmax attention on the same fp16 operands: fp16 results 1e-2 -- |v| <= 2.5
here, the result and P are each rounded to fp16 once (2^-11 relative: 1.2e-3 each), five times that; fp32 maps 1e-4 -- fp32
arithmetic on exact fp16 products, a few dozen roundings of 2^-24 and an exponent off by |s| 2^-23 give 1e-5 relative on
probabilities <= 1 (sums over 8 queries: <= 8), ten times that."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, H, D, C, M = 2, 2, 8, 16, 8          # Mq = Mqp = Mk = Mkp = M
SCALE = D ** -0.5
F16, ROWS = "fp16 / bf16", "fp32 on q's device, (B, >= Mk) or (1, >= Mk), contiguous along its last axis"
HINT = " (fp32 models keep the module path)"
SETS = [(0, 8, 1.0), (0, 8, 0.5)]


@pytest.fixture(scope="module")
def ops():
    g = torch.Generator().manual_seed(11)

    def rnd(*shape, dtype=torch.float16):
        return (torch.randn(*shape, generator=g) * 0.6).clamp(-2.5, 2.5).to(dtype).cuda()
    o = dict(q=rnd(B, M, C), k=rnd(B, M, C), vt=rnd(B, C, M), q_src=rnd(B, M, C), bias=rnd(B, M, dtype=torch.float32),
             w=rnd(B, M, dtype=torch.float32).abs(), mask=rnd(2, M, dtype=torch.float32).abs())
    o["seg_off"] = torch.tensor([0, M, 2 * M], dtype=torch.int32, device="cuda")
    return o


def rejects(text, fn, *a, **kw):
    with pytest.raises(RuntimeError) as e:
        fn(*a, **kw)
    assert str(e.value) == text


def ref_probs(q, k, bias=None):
    """(B, H, Mq, Mk) float64"""
    qh = q.double().view(q.shape[0], -1, H, D).transpose(1, 2)
    kh = k.double().view(k.shape[0], -1, H, D).transpose(1, 2)
    s = qh @ kh.transpose(2, 3) * SCALE
    if bias is not None:
        s = s + bias.double()[:, None, None, :]
    return s.softmax(-1)


def ref_out(p, vt):
    """p (B, H, Mq, Mk), vt (B, C, Mk) -> (B, Mq, C)"""
    vh = vt.double().transpose(1, 2).reshape(vt.shape[0], -1, H, D).transpose(1, 2)
    return (p @ vh).transpose(1, 2).reshape(p.shape[0], p.shape[2], C)


def close(got, ref, tol):
    assert torch.isfinite(got).all() and (got.double() - ref).abs().max().item() <= tol


def test_valid_calls(ops):
    from vidtome_amd import _lib
    q, k, vt, q_src, bias, w, mask = (ops[n] for n in ("q", "k", "vt", "q_src", "bias", "w", "mask"))
    p, p_src, p_b = ref_probs(q, k), ref_probs(q_src, k), ref_probs(q, k, bias)
    close(_lib.attention(q, k, vt, H, M, SCALE), ref_out(p, vt), 1e-2)
    close(_lib.attention_kv(q, k, vt, H, M, M, SCALE), ref_out(p, vt), 1e-2)
    close(_lib.attention_kv_sets(q, k, vt, H, M, SETS, SCALE), 1.5 * ref_out(p, vt), 1e-2)
    wq = torch.stack([mask[0], mask[0]])[:, :, None].double()        # (B, Mq, 1): set 0 is weighted by row 0 of the table
    close(_lib.attention_kv_sets_masked(q, k, vt, H, M, SETS, SCALE, [0, -1], mask), (wq + 0.5) * ref_out(p, vt), 1e-2)
    close(_lib.attention_kv_sets_src(q, q_src, k, vt, H, M, SETS, SCALE, [0, 1]), ref_out(p, vt) + 0.5 * ref_out(p_src, vt), 1e-2)
    close(_lib.attention_kv_bias(q, k, vt, H, M, M, SCALE, bias), ref_out(p_b, vt), 1e-2)
    got = _lib.attention_kv_segments(q.view(B * M, C), k, vt, H, ops["seg_off"], M, M, SCALE)
    close(got.view(B, M, C), ref_out(p, vt), 1e-2)
    close(_lib.attention_probs(q, k, H, M, M, SCALE, bias), p_b.mean(1), 1e-4)
    out = torch.zeros(B, M, device="cuda")
    close(_lib.attention_word_map(q, k, H, M, M, SCALE, w, out, bias=bias), (p_b.mean(1) * w.double()[:, None, :]).sum(-1), 1e-4)
    close(_lib.attention_key_mass(q, k, H, M, M, SCALE), p.mean(1).sum(1), 1e-4)


def test_out_like_q(ops):
    from vidtome_amd import _lib
    q, k, vt, q_src = (ops[n] for n in ("q", "k", "vt", "q_src"))
    calls = {"attention": lambda out: _lib.attention(q, k, vt, H, M, SCALE, out=out),
             "attention_kv": lambda out: _lib.attention_kv(q, k, vt, H, M, M, SCALE, out=out),
             "attention_kv_sets_src": lambda out: _lib.attention_kv_sets_src(q, q_src, k, vt, H, M, SETS, SCALE, [0, 1], out=out)}
    bad = [torch.empty(B, M, C, dtype=torch.bfloat16, device="cuda"), torch.empty(B, M, 2 * C, dtype=q.dtype, device="cuda"),
           torch.empty(B, C, M, dtype=q.dtype, device="cuda").transpose(1, 2), torch.empty(B, M, C, dtype=q.dtype)]
    for who, fn in calls.items():
        for out in bad:
            rejects(f"{who}: out must be a contiguous tensor of q's shape, dtype and device", fn, out)


def _kv_calls(_lib, ops):
    """who -> fn(q, k, vt) of the wrappers that take k and v transposed, and the hint their dtype message ends with"""
    q_src, bias, mask = ops["q_src"], ops["bias"], ops["mask"]
    return {"attention_kv_sets": (lambda q, k, vt: _lib.attention_kv_sets(q, k, vt, H, M, SETS, SCALE), HINT),
            "attention_kv_sets_masked": (lambda q, k, vt: _lib.attention_kv_sets_masked(q, k, vt, H, M, SETS, SCALE, [0, -1], mask), ""),
            "attention_kv_sets_src": (lambda q, k, vt: _lib.attention_kv_sets_src(q, q_src, k, vt, H, M, SETS, SCALE, [0, 1]), ""),
            "attention_kv_bias": (lambda q, k, vt: _lib.attention_kv_bias(q, k, vt, H, M, M, SCALE, bias), HINT)}


def _map_calls(_lib, ops):
    """who -> fn(q, k, heads=, Mq=, Mk=, bias=, w=) of the three map wrappers"""
    def words(q, k, heads=H, Mq=M, Mk=M, bias=None, w=None):
        out = torch.zeros(q.shape[0], M, device="cuda")
        return _lib.attention_word_map(q, k, heads, Mq, Mk, SCALE, ops["w"][:q.shape[0]] if w is None else w, out, bias=bias)
    return {"attention_probs": lambda q, k, heads=H, Mq=M, Mk=M, bias=None: _lib.attention_probs(q, k, heads, Mq, Mk, SCALE, bias),
            "attention_word_map": words,
            "attention_key_mass": lambda q, k, heads=H, Mq=M, Mk=M: _lib.attention_key_mass(q, k, heads, Mq, Mk, SCALE)}


def test_half_operands_and_kv_shapes(ops):
    from vidtome_amd import _lib
    q, k, vt = ops["q"], ops["k"], ops["vt"]
    for who, (fn, hint) in _kv_calls(_lib, ops).items():
        text = f"{who}: q, k and vt must share one of {F16}{hint}"
        rejects(text, fn, q.float(), k.float(), vt.float())
        rejects(text, fn, q, k.bfloat16(), vt)
        rejects(text, fn, q, k, vt.bfloat16())
        shapes = f"{who}: k must be (B, Mkp, C) and vt (B, C, ldvt)"
        rejects(shapes, fn, q, torch.cat([k, k], 2), vt)              # k (B, Mkp, 2 C)
        # vt (B, 2 C, ldvt), the samples C rows apart as the stride rule in front of this one wants them
        rejects(shapes, fn, q, k, torch.cat([vt, vt[:1]], 0).as_strided((B, 2 * C, M), (C * M, M, 1)))
        rejects(shapes, fn, q, torch.cat([k, k, k[:1]], 0), torch.cat([vt, vt, vt[:1]], 0))   # 5 samples of k and vt
    seg = lambda q, k, vt: _lib.attention_kv_segments(q.reshape(B * M, C), k, vt, H, ops["seg_off"], M, M, SCALE)
    for bad in ((q.float(), k.float(), vt.float()), (q, k.bfloat16(), vt), (q, k, vt.bfloat16())):
        rejects(f"attention_kv_segments: q, k and vt must share one of {F16}", seg, *bad)
    for who, fn in _map_calls(_lib, ops).items():
        rejects(f"{who}: q and k must share one of {F16}", fn, q.float(), k.float())
        rejects(f"{who}: q and k must share one of {F16}", fn, q, k.bfloat16())


def test_key_sets(ops):
    from vidtome_amd import _lib
    q, k, vt, q_src, mask = (ops[n] for n in ("q", "k", "vt", "q_src", "mask"))
    nine = [(0, 8, 1.0)] * 9
    rejects("attention_kv_sets: 1 .. 8 key sets, got 0", _lib.attention_kv_sets, q, k, vt, H, M, [], SCALE)
    rejects("attention_kv_sets: 1 .. 8 key sets, got 9", _lib.attention_kv_sets, q, k, vt, H, M, nine, SCALE)
    # (no set is masked: the call is attention_kv_sets')
    rejects("attention_kv_sets: 1 .. 8 key sets, got 0", _lib.attention_kv_sets_masked, q, k, vt, H, M, [], SCALE, [], mask)
    rejects("attention_kv_sets_masked: 1 .. 8 key sets, got 9", _lib.attention_kv_sets_masked, q, k, vt, H, M, nine, SCALE,
            [0] + [-1] * 8, mask)
    rejects("attention_kv_sets_masked: 2 sets but 1 mask rows", _lib.attention_kv_sets_masked, q, k, vt, H, M, SETS, SCALE, [0],
            mask)
    rejects("attention_kv_sets_src: 1 .. 8 key sets, got 0", _lib.attention_kv_sets_src, q, q_src, k, vt, H, M, [], SCALE, [])
    rejects("attention_kv_sets_src: 1 .. 8 key sets, got 9", _lib.attention_kv_sets_src, q, q_src, k, vt, H, M, nine, SCALE,
            [1] * 9)
    rejects("attention_kv_sets_src: 2 sets but 1 set_src entries", _lib.attention_kv_sets_src, q, q_src, k, vt, H, M, SETS, SCALE,
            [1])


def test_key_rows(ops):
    from vidtome_amd import _lib
    q, k, vt, bias = ops["q"], ops["k"], ops["vt"], ops["bias"]
    maps = _map_calls(_lib, ops)
    uses = {"attention_kv_bias: bias must be": lambda t: _lib.attention_kv_bias(q, k, vt, H, M, M, SCALE, t),
            "attention_probs: bias must be None or": lambda t: maps["attention_probs"](q, k, bias=t),
            "attention_word_map: bias must be": lambda t: maps["attention_word_map"](q, k, bias=t),
            "attention_word_map: weights must be": lambda t: maps["attention_word_map"](q, k, w=t)}
    wide = torch.cat([bias, bias], 1)                                                   # (B, 2 Mk)
    bad = [bias.half(), bias.cpu(), wide[:, :M // 2],                                   # dtype; device; declared rows of Mk / 2
           torch.cat([bias, bias], 0).t().contiguous().t()[:B],                         # stride 1 along the samples, not the row
           bias[None], torch.cat([bias, bias[:1]], 0),                                  # 3-D; 3 rows for 2 samples
           wide.as_strided((B, M), (M // 2, 1))]                                        # rows that overlap (stride 1 .. Mk - 1)
    for opening, fn in uses.items():
        for t in bad:
            rejects(f"{opening} {ROWS}", fn, t)
    rejects(f"attention_kv_bias: bias must be {ROWS}", uses["attention_kv_bias: bias must be"], None)
    rejects("attention_word_map: weights are required", lambda: _lib.attention_word_map(q, k, H, M, M, SCALE, None, torch.zeros(
        B, M, device="cuda")))
    # an expanded row (stride 0) and one row for all are the same call
    a = _lib.attention_kv_bias(q, k, vt, H, M, M, SCALE, bias[:1].expand(B, M))
    assert torch.equal(a, _lib.attention_kv_bias(q, k, vt, H, M, M, SCALE, bias[:1]))


def test_qk_views(ops):
    from vidtome_amd import _lib
    q, k = ops["q"], ops["k"]
    tall = torch.cat([q, q], 1)                                       # (B, 2 M, C): [:, :M] is not dense over the samples
    wide = torch.cat([q, q[:, :, :4]], 2)                             # (B, M, C + 4): rows 40 bytes apart
    off = torch.cat([q.reshape(-1), q.reshape(-1)[:4]])[4:].view(B, M, C)   # 8 bytes off a 16-byte boundary
    for who, fn in _map_calls(_lib, ops).items():
        gpu = f"{who}: q must be (B, Mqp, C) and k (B, Mkp, C) on one GPU"
        rejects(gpu, fn, q[0], k)
        rejects(gpu, fn, q, k.reshape(B * M, C))
        rejects(gpu, fn, q.cpu(), k.cpu())
        rejects(gpu, fn, q, k.cpu())
        heads = f"{who}: k must be (B, Mkp, C) with C a multiple of heads"
        rejects(heads, fn, q, torch.cat([k, k], 2))
        rejects(heads, fn, q, torch.cat([k, k[:1]], 0))
        rejects(heads, fn, q, k, heads=3)
        rejects(heads, fn, q, k, heads=0)
        inside = f"{who}: Mq / Mk must lie inside q / k"
        for kw in (dict(Mq=M + 1), dict(Mk=M + 1), dict(Mq=0), dict(Mk=0)):
            rejects(inside, fn, q, k, **kw)
        for name, args in (("q", lambda t: (t, k)), ("k", lambda t: (q, t))):
            rows = f"{who}: {name} must be 16-byte aligned rows (stride a multiple of 8), dense over the samples"
            for t in (tall[:, :M], wide[:, :, :C], off, q.transpose(1, 2).contiguous().transpose(1, 2)):
                rejects(rows, fn, *args(t))


def test_single_sample_need_not_be_dense_except_for_probs(ops):
    from vidtome_amd import _lib
    q, k = ops["q"][:1], ops["k"][:1]
    q1, k1 = torch.cat([q, q], 1)[:, :M], torch.cat([k, k], 1)[:, :M]     # stride(0) = 2 M C: what a dense view does not have
    assert q1.stride(0) != M * q1.stride(1) and torch.equal(q1, q)
    maps = _map_calls(_lib, ops)
    for name, args in (("q", (q1, k)), ("k", (q, k1))):
        rejects(f"attention_probs: {name} must be 16-byte aligned rows (stride a multiple of 8), dense over the samples",
                maps["attention_probs"], *args)
    for who in ("attention_word_map", "attention_key_mass"):
        assert torch.equal(maps[who](q1, k1), maps[who](q, k))
