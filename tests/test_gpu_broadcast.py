"""GPU tests of attention broadcast (run with -m gpu on an MI355X): csrc/broadcast.hip's three kernels and the patched block
under vidtome_amd.AttentionBroadcast.  Every comparison is BITWISE against the torch restatements of tests/broadcast_ref.py,
``(a.float() - b.float()).to(T)`` and ``(h.float() + d.float()).to(T)``, or against the project's own primitives run on
them; the one bound, the record -> replay round trip, is derived from the two roundings (see that test).  Inputs are finite;
one case has a sum that overflows fp16 to inf."""
import functools
import inspect

import pytest
import torch

import broadcast_ref as R
import first_forward as FF

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
SENTINEL = 5.0
NF, IDS = 5, (4, 0, 2)
GUARD = 16


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _rand(shape, dtype, seed, scale=1.0, on_device=False):
    """Seeded normals; ``on_device``: drawn on the GPU (the large cases: seconds faster)."""
    if on_device:
        return (torch.randn(shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV) * scale).to(dtype)
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype).to(DEV)


def _placed(t, offset, fill=SENTINEL):
    """(a copy of ``t`` that starts ``offset`` elements into a sentinel-filled buffer, the buffer): offset 0 is 16-byte
    aligned (the allocator's), offset 1 is not; GUARD elements of the buffer lie behind the copy."""
    buf = torch.full((offset + t.numel() + GUARD,), fill, dtype=t.dtype, device=DEV)
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == (offset * t.element_size()) % 16
    return view, buf


def _guards_intact(buf, offset, numel):
    return bool((buf[:offset] == SENTINEL).all()) and bool((buf[offset + numel:] == SENTINEL).all())


def _ids(ids):
    return None if ids is None else torch.tensor(ids, dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------------
# 1. record and replay
# ---------------------------------------------------------------------------------------------------
LAYOUTS = {"vec": (24 * 64, 0), "odd": (35, 0), "misaligned": (24 * 64, 1)}      # name: (E, element offset of every operand)


def _record_replay(L, dtype, G, ids, E, offset, seed=0):
    Fg = NF if ids is None else len(ids)
    shape = (G * Fg, E)
    h_in, _ = _placed(_rand(shape, dtype, seed + 1, 2.0), offset)
    h_out, _ = _placed(_rand(shape, dtype, seed + 2, 2.0), offset)
    dev_ids = _ids(ids)
    caches, bufs = [], []
    for k in range(2):
        c, buf = _placed(torch.full((G, NF, E), SENTINEL, dtype=dtype, device=DEV), offset)
        src = h_out if k == 0 else _rand(shape, dtype, seed + 3, 0.5)
        want = R.record_into(c, h_in, src, ids)
        assert L.residual_record(h_in, src, c, dev_ids) is c
        torch.cuda.synchronize()
        assert _same(c, want), f"cache {k}"
        if ids is not None:                                               # rows the ids do not name keep the fill
            rest = [i for i in range(NF) if i not in ids]
            assert bool((c[:, rest] == SENTINEL).all()) and not bool((c[:, list(ids)] == SENTINEL).all())
        assert _guards_intact(buf, offset, c.numel()), "a store outside the cache"
        caches.append(c)
        bufs.append(buf)
    h, _ = _placed(_rand(shape, dtype, seed + 4, 2.0), offset)
    for cs in (caches[:1], caches):                                       # one delta, two deltas
        out, obuf = _placed(torch.full(shape, SENTINEL, dtype=dtype, device=DEV), offset)
        got = L.residual_replay(h, cs[0], cs[1] if len(cs) > 1 else None, dev_ids, out=out)
        torch.cuda.synchronize()
        want = R.replay_from(h, ids, *cs)
        assert got is out and _same(out, want), f"{len(cs)} deltas"
        assert _guards_intact(obuf, offset, out.numel()), "a store outside out"
        assert _same(L.residual_replay(h, cs[0], cs[1] if len(cs) > 1 else None, dev_ids), want)      # (allocating form)
        hh, hbuf = _placed(h, offset)                                     # out is h
        assert L.residual_replay(hh, cs[0], cs[1] if len(cs) > 1 else None, dev_ids, out=hh) is hh
        torch.cuda.synchronize()
        assert _same(hh, want) and _guards_intact(hbuf, offset, hh.numel()), "in place"
    # round trip: record, then replay on the same h_in.  d = rnd(h_out - h_in) is off by at most half a spacing at
    # |h_out - h_in| <= 2 max(|h_in|, |h_out|); h_in + d differs from h_out by that error, and its rounding adds at most half a
    # spacing at |h_in + d| <= |h_out| + that error, again no more than 2 max: together at most one spacing of T at 2 max.
    back = L.residual_replay(h_in, caches[0], None, dev_ids)
    torch.cuda.synchronize()
    bound = R.ulp(2 * torch.maximum(h_in.double().abs(), h_out.double().abs()), dtype)
    err = (back.double() - h_out.double()).abs()
    print(f"round trip {_name(dtype)} E={E}: max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
@pytest.mark.parametrize("ids", [IDS, None], ids=["ids402", "whole"])
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=_name)
def test_record_and_replay(L, dtype, G, ids, layout):
    E, offset = LAYOUTS[layout]
    _record_replay(L, dtype, G, ids, E, offset, seed=10 * G + E % 7)


def test_record_and_replay_past_the_launch_cap(L):
    """G Fg E / 8 chunks = 1 125 000 > 4096 blocks x 256 threads: the grid-stride loop takes a second round."""
    G, E = 2, 1_500_000
    assert G * len(IDS) * (E // 8) > 4096 * 256
    _record_replay(L, F16, G, IDS, E, 0, seed=99)


def test_replay_overflows_to_inf_like_torch(L):
    h = torch.full((3, 64), 60000.0, dtype=F16, device=DEV)
    c1 = torch.full((1, NF, 64), 60000.0, dtype=F16, device=DEV)
    c2 = torch.full((1, NF, 64), -60000.0, dtype=F16, device=DEV)
    ids = _ids(IDS)
    one, two = L.residual_replay(h, c1, None, ids), L.residual_replay(h, c1, c2, ids)
    torch.cuda.synchronize()
    assert bool(torch.isinf(one).all()) and _same(one, R.replay_from(h, IDS, c1))
    assert bool(torch.isinf(two).all()) and _same(two, R.replay_from(h, IDS, c1, c2))     # the intermediate rounding is kept
    d = torch.full((1, NF, 64), SENTINEL, dtype=F16, device=DEV)
    L.residual_record(-h, h, d, ids)                                      # 120000 is no fp16
    torch.cuda.synchronize()
    assert bool(torch.isinf(d[:, list(IDS)]).all()) and _same(d, R.record_into(torch.full_like(d, SENTINEL), -h, h, IDS))


def test_wrappers_refuse_mismatched_operands(L):
    h = torch.zeros((6, 7, 64), dtype=F16, device=DEV)
    c = torch.zeros((2, NF, 7, 64), dtype=F16, device=DEV)
    ids = _ids(IDS)
    for bad in (c.float(), c[:, :, :6].contiguous(), c.transpose(0, 1)):
        with pytest.raises(RuntimeError):
            L.residual_replay(h, bad, None, ids)
    with pytest.raises(RuntimeError, match="group-major"):
        L.residual_replay(h[:5].contiguous(), c, None, ids)
    with pytest.raises(RuntimeError, match="int32"):
        L.residual_replay(h, c, None, ids.long())
    with pytest.raises(RuntimeError, match="group-major"):
        L.residual_replay(h, c, None, None)                               # no ids: the call must carry all 5 frames
    with pytest.raises(RuntimeError, match="like h_in"):
        L.residual_record(h, h.float(), c, ids)
    with pytest.raises(RuntimeError, match="failed"):
        L.residual_replay_layernorm(h.float(), c.float(), None, ids, None, None, 1e-5)


# ---------------------------------------------------------------------------------------------------
# 2. the fused launch
# ---------------------------------------------------------------------------------------------------
def _fused(L, dtype, G, ids, nf, N, C, two, affine=True, seed=0, in_place=False, big=False):
    Fg = nf if ids is None else len(ids)
    rows = G * Fg * N
    h = _rand((G * Fg, N, C), dtype, seed + 1, 1.5, big) + 0.25
    c1 = _rand((G, nf, N, C), dtype, seed + 2, 0.5, big)
    c2 = _rand((G, nf, N, C), dtype, seed + 3, 0.5, big) if two else None
    gamma = _rand((C,), dtype, seed + 4) if affine else None
    beta = _rand((C,), dtype, seed + 5) if affine else None
    dev_ids = _ids(ids)
    want_rows = L.residual_replay(h, c1, c2, dev_ids)
    assert _same(want_rows, R.replay_from(h, ids, *([c1, c2] if two else [c1])))
    want_panels = L.layernorm_panels(want_rows, gamma, beta, 1e-5)
    # the raw call into sentinel-filled outputs: padding rows and a guard panel stay untouched
    pr = L.panel_rows(rows)
    out = h.clone() if in_place else torch.full_like(h, SENTINEL)
    pbuf = torch.full((C // 8 + 1, pr, 8), SENTINEL, dtype=dtype, device=DEV)
    rc = L.lib().vtm_residual_replay_layernorm(h.data_ptr() if not in_place else out.data_ptr(), c1.data_ptr(),
                                               None if c2 is None else c2.data_ptr(), None if ids is None else dev_ids.data_ptr(),
                                               None if gamma is None else gamma.data_ptr(),
                                               None if beta is None else beta.data_ptr(), 1e-5, L.dtype_code(h), G, Fg, nf, N, C,
                                               out.data_ptr(), pbuf.data_ptr(), pr, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.lib().vtm_last_error()
    torch.cuda.synchronize()
    assert _same(out, want_rows), "out_rows is not vtm_residual_replay's"
    assert _same(pbuf[:-1, :rows], want_panels[:, :rows]), "panel rows are not vtm_layernorm_panels'"
    assert bool((pbuf[:-1, rows:] == SENTINEL).all()), "a store into the panels' padding rows"
    assert bool((pbuf[-1] == SENTINEL).all()), "a store past the last panel"
    got_rows, got_panels = L.residual_replay_layernorm(h, c1, c2, dev_ids, gamma, beta, 1e-5)
    torch.cuda.synchronize()
    assert tuple(got_panels.shape) == (C // 8, pr, 8)
    assert _same(got_rows, want_rows) and _same(got_panels[:, :rows], want_panels[:, :rows])


@pytest.mark.parametrize("two", [False, True], ids=["cache1", "cache1+2"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=_name)
@pytest.mark.parametrize("N", [1, 7])
@pytest.mark.parametrize("C", [64, 320, 1280, 2048])
def test_fused_replay_layernorm(L, C, N, dtype, two):
    """G = 2, Fg = 3 of 5 frames: 6 or 42 token rows -- fewer than a block holds, and more than one block with a partial last
    one in both families (4 rows per block with a wave per row; 32 at C = 320, 8 lanes per row)."""
    _fused(L, dtype, 2, IDS, NF, N, C, two, seed=C + N)


@pytest.mark.parametrize("C", [640, 1024, 1536])
def test_fused_replay_layernorm_other_widths(L, C):
    """The instantiations the four widths above leave out: 16 lanes per row (C = 640), 2 pieces per lane and 3 with every lane
    busy (C = 1024, 1536; C = 1280 above is 3 with the last partly idle); the whole video without ids; no affine part;
    out_rows = h."""
    _fused(L, F16, 2, IDS, NF, 7, C, True, seed=C)
    _fused(L, BF16, 1, None, NF, 3, C, False, affine=False, seed=C + 1)
    _fused(L, F16, 2, IDS, NF, 7, C, True, seed=C + 2, in_place=True)


def test_fused_replay_layernorm_takes_the_family_layernorm_panels_takes(L):
    """C = 1280 is summed by the lanes-per-row kernel from 32768 rows on (a wave per row below: the 42-row case above):
    G Fg N = 2 * 3 * 5462 = 32772 rows select it in vtm_layernorm_panels, so the fused launch must follow."""
    N = 5462
    assert 2 * 3 * N >= 32768 > 2 * 3 * (N - 1)
    _fused(L, F16, 2, None, 3, N, 1280, True, seed=5, big=True)


# ---------------------------------------------------------------------------------------------------
# 3. the patched block
# ---------------------------------------------------------------------------------------------------
G, N, C, HEADS, LATENT, KEYS = 2, 64, 320, 8, (8, 8), 16
T4 = [999, 666, 333, 0]
WIDE = (-1, 1000)


@functools.lru_cache(maxsize=None)
def _unet(dtype=F16):
    """One full SD block (C = 320, 8 heads) with every parameter random, patched; 8 x 8 latents: 64 tokens per frame."""
    import vidtome_amd
    from vidtome_amd import sites as S
    unet = S.SiteUNet([S.Site("up3.0", 1, C, HEADS)], seed=3, full=True)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for p in unet.parameters():
            if p.ndim == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.3 + (1.0 if p is unet.blocks[0].norm3.weight else 0.0))
    unet = unet.to(device=DEV, dtype=dtype)
    vidtome_amd.apply_patch(unet, local_merge_ratio=0.5, batch_size=G)
    unet.set_size(LATENT)
    return unet


@functools.lru_cache(maxsize=None)
def _inputs(seed):
    """(hidden states (G NF, N, C), conditioning (G NF, KEYS, 768)) of the whole 5-frame video: shared, left unchanged."""
    return _rand((G * NF, N, C), F16, seed, 1.2), _rand((G * NF, KEYS, 768), F16, seed + 1, 0.5)


def _rows_of(ids):
    return [g * NF + i for g in range(G) for i in ids]


class Spy:
    """Every launching wrapper of vidtome_amd._lib, wrapped: ``names`` in call order, ``args`` the positional arguments."""

    def __init__(self, monkeypatch, L):
        self.names, self.args = [], []
        for name, fn in list(vars(L).items()):
            if inspect.isfunction(fn) and not name.startswith("_") and name not in FF.HOST_ONLY:
                monkeypatch.setattr(L, name, self._wrap(name, fn))

    def _wrap(self, name, fn):
        @functools.wraps(fn)
        def wrapped(*a, **k):
            self.names.append(name)
            self.args.append(a)
            return fn(*a, **k)
        return wrapped

    def clear(self):
        del self.names[:], self.args[:]

    def new(self):
        return [n for n in self.names if n.startswith("residual_")]


def _run(blk, x, cond, bc=None, step=None, ids=None):
    """One forward of the block from the same generator state; (output, generator state behind it)."""
    blk.generator = torch.Generator().manual_seed(11)
    if bc is not None:
        bc.set_step(step)
        bc.set_frames(ids)
    with torch.no_grad():
        out = blk(x, encoder_hidden_states=cond)
    torch.cuda.synchronize()
    return out, blk.generator.get_state()


@pytest.fixture
def world(L, monkeypatch):
    """(block, unregistered output and generator state on inputs 0, the spy, a fresh AttentionBroadcast factory); the block
    leaves unregistered."""
    import vidtome_amd
    unet = _unet()
    blk = unet.blocks[0]
    vidtome_amd.unregister_attention_broadcast(unet)
    x, cond = _inputs(20)
    base, state = _run(blk, x, cond)                                      # (also packs the panel weights)
    spy = Spy(monkeypatch, L)

    def make(**kw):
        args = dict(attn1_every=2, attn2_every=2, attn1_window=WIDE, attn2_window=WIDE)
        args.update(kw)
        bc = vidtome_amd.AttentionBroadcast(T4, NF, **args)
        assert vidtome_amd.register_attention_broadcast(unet, bc) == ["blocks.0"]
        return bc
    yield blk, base, state, spy, make
    vidtome_amd.unregister_attention_broadcast(unet)
    for flag in ("vtm_attention_maps", "vtm_local_blend", "vtm_cross_control", "vtm_sag", "merge_mlp"):
        blk.__dict__.pop(flag, None)
    blk.use_ada_layer_norm = blk.use_ada_layer_norm_zero = False


def test_unregistered_and_compute_steps_are_the_parents(world):
    """(a)"""
    blk, base, state, spy, make = world
    x, cond = _inputs(20)
    again, state2 = _run(blk, x, cond)
    plain = list(spy.names)
    assert _same(again, base) and torch.equal(state, state2) and plain and spy.new() == []
    bc = make(attn1_window=(1000, 2000), attn2_window=(1000, 2000))       # registered, but no step is inside the window
    for step in range(4):
        spy.clear()
        assert bc.modes(step) == ("compute", "compute")
        out, st = _run(blk, x, cond, bc, step)
        assert _same(out, base) and torch.equal(st, state) and spy.names == plain
    assert bc.nbytes() == 0
    bc = make()                                                           # the last step of a run computes
    assert bc.modes(3) == ("reuse", "reuse") and bc.modes(2) == ("record", "record")
    bc = make(attn1_every=None, attn2_every=1)
    spy.clear()
    out, _ = _run(blk, x, cond, bc, 1)
    assert _same(out, base) and spy.names == plain


def test_record_step(world):
    """(b)"""
    blk, base, state, spy, make = world
    x, cond = _inputs(20)
    spy.clear()
    _run(blk, x, cond)
    plain = list(spy.names)
    bc = make()
    assert bc.modes(0) == ("record", "record")
    spy.clear()
    out, st = _run(blk, x, cond, bc, 0)
    assert _same(out, base) and torch.equal(st, state)
    assert spy.new() == ["residual_record", "residual_record"]
    assert [n for n in spy.names if not n.startswith("residual_")] == plain              # nothing else changed
    (in1, out1, cache1, ids1), (in2, out2, cache2, ids2) = [a for n, a in zip(spy.names, spy.args) if n == "residual_record"]
    assert ids1 is None and ids2 is None
    # the segments' inputs and outputs: the block's input, attn1's output = attn2's input, and what the feed-forward reads
    from vidtome_amd import patch as vpatch
    assert _same(in1, x) and out1.data_ptr() == in2.data_ptr()
    assert _same(out, vpatch.norm_feed_forward_residual(blk.norm3, blk.ff, out2))
    assert cache1 is bc.cache("blocks.0", "attn1") and cache2 is bc.cache("blocks.0", "attn2")
    assert tuple(cache1.shape) == tuple(cache2.shape) == (G, NF, N, C) and cache1.dtype == F16
    assert _same(cache1.view(G * NF, N, C), R.delta(out1, x)) and _same(cache2.view(G * NF, N, C), R.delta(out2, out1))
    assert bc.nbytes() == 2 * G * NF * N * C * 2
    # one kind alone records one delta
    bc = make(attn2_every=None)
    spy.clear()
    out, _ = _run(blk, x, cond, bc, 0)
    assert _same(out, base) and spy.new() == ["residual_record"]
    assert _same(bc.cache("blocks.0", "attn1"), cache1)


def test_reuse_step_is_one_launch_and_the_feed_forward(world):
    """(c)"""
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    blk, base, state, spy, make = world
    x, cond = _inputs(20)
    x2, cond2 = _inputs(30)
    bc = make()
    _run(blk, x, cond, bc, 0)
    c1, c2 = bc.cache("blocks.0", "attn1").clone(), bc.cache("blocks.0", "attn2").clone()
    assert bc.modes(1) == ("reuse", "reuse")
    spy.clear()
    out, st = _run(blk, x2, cond2, bc, 1)
    launched = list(spy.names)
    assert launched == ["residual_replay_layernorm", "ff_geglu", "linear_panels"]
    assert torch.equal(st, torch.Generator().manual_seed(11).get_state()), "a reuse step drew from the block's generator"
    want = vpatch.norm_feed_forward_residual(blk.norm3, blk.ff, R.replay_from(x2, None, c1, c2))
    torch.cuda.synchronize()
    assert _same(out, want) and not _same(out, _run(blk, x2, cond2, bc, 0)[0])
    assert _same(bc.cache("blocks.0", "attn1"), R.delta(spy.args[spy.names.index("residual_record")][1], x2).view(G, NF, N, C))
    # merge_mlp has no local map on such a step: the plain path, the same bits
    _run(blk, x, cond, bc, 0)
    vidtome_amd.update_patch(_unet(), merge_mlp=True)
    try:
        assert _same(_run(blk, x2, cond2, bc, 1)[0], want)
    finally:
        vidtome_amd.update_patch(_unet(), merge_mlp=False)
    # where the feed-forward is not the fused one: one replay of both deltas, then today's feed-forward
    import vidtome_amd.patch as P
    spy.clear()
    try:
        P.FF_MODE = "blas"
        out_blas, _ = _run(blk, x2, cond2, bc, 1)
        h2 = R.replay_from(x2, None, c1, c2)
        want_blas = vpatch.feed_forward(blk.ff, vpatch.layer_norm(blk.norm3, h2)) + h2
    finally:
        P.FF_MODE = "panels"
    torch.cuda.synchronize()
    assert spy.new() == ["residual_replay"] and "residual_replay_layernorm" not in spy.names
    assert _same(out_blas, want_blas)


def test_reuse_step_ignores_the_chunking(world):
    """(d)"""
    blk, base, state, spy, make = world
    x, cond = _inputs(20)
    x2, cond2 = _inputs(30)
    bc = make()
    _run(blk, x, cond, bc, 0)                                             # one cache state: the whole video recorded at once
    whole, _ = _run(blk, x2, cond2, bc, 1)
    for chunks in ([[0, 1, 2], [3, 4]], [[4, 2], [0], [3, 1]]):
        got = torch.empty_like(whole)
        for ids in chunks:
            rows = _rows_of(ids)
            out, _ = _run(blk, x2[rows].contiguous(), cond2[rows].contiguous(), bc, 1, ids)
            got[rows] = out
        assert _same(got, whole), chunks
    # and a record step in chunks fills the same cache rows a reuse reads in other chunks
    bc = make()
    for ids in ([3, 1, 4], [0, 2]):
        rows = _rows_of(ids)
        _run(blk, x[rows].contiguous(), cond[rows].contiguous(), bc, 0, ids)
    for ids in ([0, 1], [2, 3, 4]):
        rows = _rows_of(ids)
        out, _ = _run(blk, x2[rows].contiguous(), cond2[rows].contiguous(), bc, 1, ids)
        want = R.replay_from(x2[rows], ids, bc.cache("blocks.0", "attn1"), bc.cache("blocks.0", "attn2"))
        from vidtome_amd import patch as vpatch
        assert _same(out, vpatch.norm_feed_forward_residual(blk.norm3, blk.ff, want))


def test_one_kind_reused_alone(world):
    """(e) attn2-only reuse: attn1 computed, attn2 replayed; and its mirror image."""
    from vidtome_amd import patch as vpatch
    blk, base, state, spy, make = world
    x, cond = _inputs(20)
    x2, cond2 = _inputs(30)
    bc = make(attn1_every=None)
    assert bc.modes(0) == ("compute", "record") and bc.modes(1) == ("compute", "reuse")
    _run(blk, x, cond, bc, 0)
    c2 = bc.cache("blocks.0", "attn2")
    spy.clear()
    out, st = _run(blk, x2, cond2, bc, 1)
    launched = list(spy.names)
    blk.generator = torch.Generator().manual_seed(11)
    spy.clear()
    with torch.no_grad():
        h1 = vpatch.self_attention_segment(blk, x2)
    # attn1's launches as ever, one replay in place of the whole attn2 segment, the feed-forward
    assert launched == spy.names + ["residual_replay", "layernorm_panels", "ff_geglu", "linear_panels"]
    assert torch.equal(st, blk.generator.get_state())                     # attn1 drew what it always draws
    want = vpatch.norm_feed_forward_residual(blk.norm3, blk.ff, R.replay_from(h1, None, c2))
    torch.cuda.synchronize()
    assert _same(out, want)
    # attn1-only reuse: the unregistered block with its attn1 segment replaced by the torch replay
    bc = make(attn2_every=None)
    assert bc.modes(1) == ("reuse", "compute")
    _run(blk, x, cond, bc, 0)
    c1 = bc.cache("blocks.0", "attn1")
    spy.clear()
    out, st = _run(blk, x2, cond2, bc, 1)
    launched = list(spy.names)
    assert torch.equal(st, torch.Generator().manual_seed(11).get_state())
    import vidtome_amd
    vidtome_amd.unregister_attention_broadcast(_unet())
    orig = vpatch.self_attention_segment
    spy.clear()
    try:
        vpatch.self_attention_segment = lambda block, h, *a, **k: R.replay_from(h, None, c1)
        want, _ = _run(blk, x2, cond2)
    finally:
        vpatch.self_attention_segment = orig
    assert _same(out, want) and launched == ["residual_replay"] + spy.names        # one replay, then attn2 and the rest as ever


def test_forward_refusals(world):
    """(f) every raise of the contract, at the forward and before any new launch."""
    blk, base, state, spy, make = world
    x, cond = _inputs(20)
    bc = make()
    with pytest.raises(RuntimeError, match="set_step"):
        _run(blk, x, cond)
    # a reuse whose frames were not (all) recorded at the latest record step
    rows = _rows_of([0, 1, 2])
    _run(blk, x[rows].contiguous(), cond[rows].contiguous(), bc, 0, [0, 1, 2])
    spy.clear()
    rows = _rows_of([2, 3])
    with pytest.raises(RuntimeError, match=r"block 'blocks.0'.*frames \[3\] were not recorded at step 0"):
        _run(blk, x[rows].contiguous(), cond[rows].contiguous(), bc, 1, [2, 3])
    with pytest.raises(RuntimeError, match=r"frames \[3, 4\] were not recorded"):
        _run(blk, x, cond, bc, 1)
    # a record step that was skipped altogether: step 2 records, step 3 must not read step 0's rows
    rows = _rows_of([0, 1, 2])
    with pytest.raises(RuntimeError, match=r"frames \[0, 1, 2\] were not recorded at step 2"):
        _run(blk, x[rows].contiguous(), cond[rows].contiguous(), bc, 3, [0, 1, 2])
    # B % Fg, another G, another N
    with pytest.raises(RuntimeError, match="not a multiple of the chunk's 3 frames"):
        _run(blk, x[:4].contiguous(), cond[:4].contiguous(), bc, 1, [0, 1, 2])
    with pytest.raises(RuntimeError, match="must not change between calls"):
        _run(blk, x[:3].contiguous(), cond[:3].contiguous(), bc, 1, [0, 1, 2])           # G = 1
    with pytest.raises(RuntimeError, match="must not change between calls"):
        _run(blk, x[rows][:, :16].contiguous(), cond[rows].contiguous(), bc, 1, [0, 1, 2])   # N = 16
    with pytest.raises(RuntimeError, match="must not change between calls"):
        bc.replay("blocks.0", ("attn1",), x[rows].float())                               # dtype
    assert spy.new() == []
    # the consumers of a map a replayed segment does not make; an AdaLayerNorm block
    bc = make()
    _run(blk, x, cond, bc, 0)
    spy.clear()
    for attr, value, word in (("vtm_attention_maps", True, "attention maps"), ("vtm_sag", True, "self-attention guidance"),
                              ("vtm_cross_control", object(), "cross-attention control"),
                              ("vtm_local_blend", (object(), "blocks.0"), "LocalBlend")):
        blk.__dict__[attr] = value
        with pytest.raises(RuntimeError, match="block 'blocks.0'.*" + word):
            _run(blk, x, cond, bc, 1)
        del blk.__dict__[attr]
    for flag in ("use_ada_layer_norm", "use_ada_layer_norm_zero"):
        setattr(blk, flag, True)
        with pytest.raises(RuntimeError, match="block 'blocks.0'.*AdaLayerNorm"):
            _run(blk, x, cond, bc, 0)
        setattr(blk, flag, False)
    assert spy.names == []
    # reset: the bookkeeping and the caches go
    bc.reset()
    assert bc.nbytes() == 0
    with pytest.raises(RuntimeError, match="not recorded"):
        _run(blk, x, cond, bc, 1)
