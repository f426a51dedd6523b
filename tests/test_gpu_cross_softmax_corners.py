"""GPU tests of the cross-attention side kernels at their online-softmax corners (run with -m gpu on an MI355X):
vtm_attention_kv_sets / _sets_masked / _sets_src, vtm_attention_kv_bias, vtm_attention_probs and vtm_attention_word_map
through their _lib wrappers on the scenarios of tests/softmax_corners.py -- a maximum that jumps late, climbs in every tile
above and just below the deferred-rescale threshold, a dominant first key, rows far below zero, wide scores, a jump that only
the bias makes, fully masked tiles in front, in the middle and at the end, and a set that must not inherit the state of the
one before it -- against the float64 expression on the same 16-bit operands, within the bars the kernels already have.
test_softmax_corners_host.py proves on the host that every scenario here reaches its branch.

Then the XCD-pinned item order of the sets and bias families: 64 query blocks per (sample, head) with B * h a multiple of 8,
where the planner pins the pairs to XCDs, next to 63 blocks and to B * h = 6, where it does not.

Every case prints its error over its bar (-s); profiles/cross_softmax_corners.txt holds one run."""
import functools

import numpy as np
import pytest
import torch

import softmax_corners as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.0


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _vt(v):
    return v.transpose(1, 2).contiguous().to(DEV)


def _run(L, c, weights=None, mask=None):
    """The case through its kernel's wrapper: (B, Mq, C) in the operands' dtype, the (B, Mq, Mk) map, or the (B, Mq) word
    map.  ``weights``: other set weights; ``mask``: another mask table."""
    scale = c.d ** -0.5
    qd, kd = c.q.to(DEV), c.k.to(DEV)
    sets = c.sets if weights is None else [(s, n, w) for (s, n, _), w in zip(c.sets, weights)]
    bias = None if c.bias is None else c.bias.to(DEV)
    if c.kind == "sets":
        return L.attention_kv_sets(qd, kd, _vt(c.v), SC.H, c.Mq, sets, scale)[:, :c.Mq]
    if c.kind == "sets_masked":
        table = (c.mask if mask is None else mask).contiguous().to(DEV)
        return L.attention_kv_sets_masked(qd, kd, _vt(c.v), SC.H, c.Mq, sets, scale, c.set_mask, table)[:, :c.Mq]
    if c.kind.startswith("sets_src"):
        return L.attention_kv_sets_src(qd, c.q_src.to(DEV), kd, _vt(c.v), SC.H, c.Mq, sets, scale, c.set_src)[:, :c.Mq]
    if c.kind == "bias":
        return L.attention_kv_bias(qd, kd, _vt(c.v), SC.H, c.Mq, c.Mk, scale, bias)[:, :c.Mq]
    if c.kind == "probs":
        return L.attention_probs(qd, kd, SC.H, c.Mq, c.Mk, scale, bias)
    out = torch.full((SC.B, c.Mq), SENTINEL, dtype=torch.float32, device=DEV)
    return L.attention_word_map(qd, kd, SC.H, c.Mq, c.Mk, scale, c.w.to(DEV), out, accumulate=False, bias=bias)


def _one_key_exact(L, c, key_of):
    """All of a row's probability sits on one key (p = 1 exactly, every other exp2 is 0, l = 1): the sets and bias kernels
    return that key's v row bit for bit -- one rounding of an exact value; per set, with the other sets' weights 0 and a mask
    table of ones --, the map is exactly 1.0 there and 0.0 elsewhere, the word map exactly w[key] (h = 2: (w + w) / 2)."""
    if SC.is_pv(c.kind):
        ones = None if c.mask is None else torch.ones_like(c.mask)
        for s, (start, _, _) in enumerate(c.sets):
            hot = [1.0 if i == s else 0.0 for i in range(len(c.sets))]
            got = _run(L, c, weights=hot if len(c.sets) > 1 else None, mask=ones).cpu()
            for b in range(SC.B):
                want = c.v[b, start + key_of(b)][None, :].expand(c.Mq, -1)
                assert torch.equal(got[b], want), (s, b, "not the key's v row bit for bit")
    elif c.kind == "probs":
        got = _run(L, c).cpu()
        for b in range(SC.B):
            want = torch.zeros(c.Mq, c.Mk)
            want[:, key_of(b)] = 1.0
            assert torch.equal(got[b], want), b
    else:
        got = _run(L, c).cpu()
        for b in range(SC.B):
            assert bool((got[b] == c.w[b, key_of(b)]).all()), b


def _other_finite_rows(c, seed):
    """The case with the k / v rows of its masked keys replaced by other finite values."""
    g = torch.Generator().manual_seed(seed)
    k, v = c.k.clone(), c.v.clone()
    for b in range(SC.B):
        n = len(c.masked[b])
        k[b, c.masked[b]] = (torch.randn(n, k.shape[2], generator=g) * 4).to(c.dtype)
        v[b, c.masked[b]] = (torch.randn(n, k.shape[2], generator=g) * 100).to(c.dtype)
    return c.replace(k=k, v=v)


@pytest.mark.parametrize("case", SC.gpu_cases(), ids=SC.case_id)
def test_corner(L, case):
    """Every layout of the case: finite, within the kernel's existing bar of the float64 reference (for the map and the
    word map plus softmax_corners.score_term where |score|max > 16 log2 units, derived there from the operands), the same
    bits from a second call, and what the scenario promises exactly."""
    name, kind, d, dtype = case
    for layout in SC.layouts_of(kind):
        c = SC.scenario(name, kind, d, dtype, layout)
        ref = SC.reference(c)
        bar = SC.bar(c, ref)
        got = _run(L, c)
        assert torch.equal(got, _run(L, c)), "two calls differ"
        g = got.double().cpu().numpy()
        finite = bool(np.isfinite(g).all())
        err = float(np.abs(g - ref).max()) if finite else float("inf")
        print(f"corner {SC.case_id(case)} layout={layout} err={err:.3e} bar={bar:.3e} ratio={err / bar:.3f}")
        assert finite, (layout, "not finite")
        assert err <= bar, (layout, err, bar)
        if name == "first_key_dominant":
            _one_key_exact(L, c, lambda b: 0)
        elif name == "masked_tiles:single":
            _one_key_exact(L, c, lambda b: c.meta["single"][b])
        if name.startswith("masked_tiles"):
            assert torch.equal(_run(L, _other_finite_rows(c, seed=d)), got), (layout, "a masked key's rows were read")
        if name == "set_isolation":
            # the state of a finished set does not reach the next one: with set 0 weighted 0, another spike in set 0
            # (60 instead of 40 log2 units over the block's other scores) changes no bit
            other = SC.scenario(name, kind, d, dtype, layout, height=60.0)
            assert not torch.equal(other.k, c.k) and torch.equal(other.q, c.q) and torch.equal(other.v, c.v)
            w = (0.0, 1.0, 0.7)[:len(c.sets)]
            a, b_ = _run(L, c, weights=w), _run(L, other, weights=w)
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b_), (layout, "set 0 reached the next set")


# ---------------------------------------------------------------------------------------------------
# the XCD-pinned grid of the sets and bias families
# ---------------------------------------------------------------------------------------------------
# (d, B, h, Mq, dtype): 64 query blocks per (sample, head) and B * h a multiple of 8 pin the pairs to XCDs
GRID_CASES = {"pinned-1-per-xcd": (40, 1, 8, 16384, torch.float16),
              "pinned-2-per-xcd": (40, 2, 8, 16384, torch.bfloat16),
              "control-63-blocks": (40, 1, 8, 16128, torch.float16),
              "pinned-d160": (160, 2, 4, 8192, torch.float16),
              "control-6-pairs": (40, 1, 6, 16384, torch.float16)}
GRID_SETS = ((77, 1.0), (16, 0.6))
GRID_MK = 93
GRID_PAD = 8                      # rows Mq .. Mqp of the output keep a sentinel


@functools.lru_cache(maxsize=1)
def _grid_operands(which):
    """Random data per (sample, head, row) -- a permuted or dropped work item misses grossly -- and the float64 per-set
    results for both query operands, computed once per case and shared by the four kernels."""
    d, Bg, h, Mq, dtype = GRID_CASES[which]
    g = torch.Generator().manual_seed(sum(map(ord, which)))
    C, Mqp = h * d, Mq + GRID_PAD
    sets, end = [], 0
    for n, w in GRID_SETS:
        sets.append((end, n, w))
        end = SC._r8(end + n)
    end = max(end, SC._r8(GRID_MK))
    q = torch.randn(Bg, Mqp, C, generator=g).to(dtype)
    q_src = torch.randn(Bg, Mqp, C, generator=g).to(dtype)
    k = torch.randn(Bg, end, C, generator=g).to(dtype)
    v = torch.randn(Bg, end, C, generator=g).to(dtype)
    bias = torch.rand(Bg, GRID_MK, generator=g) * 4 - 2
    mask = torch.rand(Bg, len(sets), Mqp, generator=g) * 0.75 + 0.25
    sh = lambda t, n0, n: t[:, n0:n0 + n].double().view(Bg, n, h, d).transpose(1, 2)

    def softmax_v(qq, start, n, add=None):
        s = sh(qq, 0, Mq) @ sh(k, start, n).transpose(-1, -2) * d ** -0.5
        if add is not None:
            s = s + add.double()[:, None, None, :]
        return (torch.softmax(s, dim=-1) @ sh(v, start, n)).transpose(1, 2).reshape(Bg, Mq, C)

    per_set = {(op, s): softmax_v(qq, st, n) for op, qq in ((0, q), (1, q_src)) for s, (st, n, _) in enumerate(sets)}
    return dict(q=q, q_src=q_src, k=k, v=v, bias=bias, mask=mask, sets=sets, per_set=per_set,
                bias_ref=softmax_v(q, 0, GRID_MK, bias))


@pytest.mark.parametrize("kernel", ["sets", "sets_masked", "sets_src", "bias"])
@pytest.mark.parametrize("which", list(GRID_CASES))
def test_sets_and_bias_xcd_pinned_grid(L, which, kernel):
    """Every row below Mq within the bar of float64, rows Mq .. Mqp untouched."""
    d, Bg, h, Mq, dtype = GRID_CASES[which]
    o = _grid_operands(which)
    sets, scale, C = o["sets"], d ** -0.5, h * d
    qd, kd, vtd = o["q"].to(DEV), o["k"].to(DEV), _vt(o["v"])
    out = torch.full((Bg, Mq + GRID_PAD, C), SENTINEL, dtype=dtype, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    n = len(sets)
    i64, f32, i32 = L._i64 * n, L._f32 * n, L._int * n
    starts, lens, ws = i64(*[s for s, _, _ in sets]), i64(*[m for _, m, _ in sets]), f32(*[w for _, _, w in sets])
    common = (kd.data_ptr(), C, vtd.data_ptr(), vtd.stride(1), out.data_ptr(), C, L.dtype_code(qd), Bg, h, Mq, Mq + GRID_PAD)
    if kernel == "sets":
        rc = L.lib().vtm_attention_kv_sets(qd.data_ptr(), C, *common, kd.shape[1], d, scale, n, starts, lens, ws, stream)
        ref = sum(w * o["per_set"][(0, s)] for s, (_, _, w) in enumerate(sets))
    elif kernel == "sets_masked":
        table = o["mask"].to(DEV)
        rc = L.lib().vtm_attention_kv_sets_masked(qd.data_ptr(), C, *common, kd.shape[1], d, scale, n, starts, lens, ws,
                                                  i32(*range(n)), table.data_ptr(), table.shape[2],
                                                  n * table.shape[2], stream)
        ref = sum(w * o["mask"][:, s, :Mq, None].double() * o["per_set"][(0, s)] for s, (_, _, w) in enumerate(sets))
    elif kernel == "sets_src":
        qs, src = o["q_src"].to(DEV), (1, 0)
        rc = L.lib().vtm_attention_kv_sets_src(qd.data_ptr(), C, qs.data_ptr(), C, qs.shape[1], *common, kd.shape[1], d,
                                               scale, n, starts, lens, ws, i32(*src), stream)
        ref = sum(w * o["per_set"][(src[s], s)] for s, (_, _, w) in enumerate(sets))
    else:
        bd = o["bias"].to(DEV)
        rc = L.lib().vtm_attention_kv_bias(qd.data_ptr(), C, *common, GRID_MK, kd.shape[1], d, scale, bd.data_ptr(),
                                           GRID_MK, GRID_MK, stream)
        ref = o["bias_ref"]
    assert rc == 0, L.lib().vtm_last_error()
    torch.cuda.synchronize()
    assert bool((out[:, Mq:] == SENTINEL).all()), "rows >= Mq were written"
    got = out[:, :Mq].double().cpu()
    assert bool(torch.isfinite(got).all())
    bar = SC.TOL[dtype] * max(1.0, float(ref.abs().max()))
    rows = (got - ref).abs().amax(-1)                       # per (sample, row)
    err = float(rows.max())
    print(f"grid {which} {kernel} err={err:.3e} bar={bar:.3e} ratio={err / bar:.3f}")
    assert err < bar, (which, kernel, err, bar, int((rows >= bar).sum()), "rows miss")
