"""CPU tests of the cross-attention control's host side (vidtome_amd.p2p and the attn2 segment of patch.py): the CrossEdit
constructors against Prompt-to-Prompt's controllers in float64 (tests/cross_control_standin.py), registration and what
clears it, what raises at forward, the host protocol of an injecting block with the three launches stubbed in torch, and the
C-ABI surface of the two exports."""
import ctypes
import os
import re

import pytest
import torch

import attention_maps_standin as AM
import cross_control_standin as CC
import standin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 64


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


def _dyadic(g, shape, steps=16, lo=0):
    """Random multiples of 1 / steps: products of a few of them are exact in fp32, which is what a CrossEdit keeps."""
    return torch.randint(lo, steps + 1, shape, generator=g).double() / steps


def _random_specs(K, g):
    mapper = _dyadic(g, (K, K), 8)
    index = torch.randperm(K, generator=g)
    alphas = _dyadic(g, (K,), 8)
    new = int(torch.randint(0, K, (1,), generator=g))
    index[new], alphas[new] = -1, 0.0
    aw, eq = _dyadic(g, (K,), 16), _dyadic(g, (K,), 4, lo=-8)
    return [{"kind": "replace", "mapper": mapper},
            {"kind": "replace", "mapper": mapper, "alpha_words": 0.625},                 # a fractional alpha_words
            {"kind": "replace", "mapper": mapper, "alpha_words": aw},
            {"kind": "refine", "index": index, "alphas": alphas, "alpha_words": aw},
            {"kind": "refine", "index": index, "alphas": alphas, "alpha_words": aw, "equalizer": eq},   # refine, then reweight
            {"kind": "replace", "mapper": mapper, "alpha_words": 0.375, "equalizer": eq},
            {"kind": "reweight", "equalizer": eq, "alpha_words": aw}]


@pytest.mark.parametrize("K", [1, 5, 77])
def test_constructors_restate_the_p2p_controllers(K):
    g = torch.Generator().manual_seed(K)
    probs = lambda: torch.softmax(3 * torch.randn(2, 6, K, generator=g, dtype=torch.float64), dim=-1)
    base, own = probs(), probs()
    for spec in _random_specs(K, g):
        e = CC.edit_of(spec)
        assert e.K == K and all(t.dtype == torch.float32 for t in (e.mapper, e.src_weight, e.own_weight))
        got = (base @ e.mapper.double()) * e.src_weight.double() + own * e.own_weight.double()
        ref = CC.controlled_probs(spec, base, own)
        err = float((got - ref).abs().max())
        assert err <= 1e-12, (spec["kind"], sorted(spec), err)
    if K == 77:                                     # the specs the GPU tests use: M, a, b round to fp32 once
        for name, spec in CC.specs(K).items():
            e = CC.edit_of(spec)
            got = (base @ e.mapper.double()) * e.src_weight.double() + own * e.own_weight.double()
            # (a and b are rounded once: half an ulp of each, times probabilities <= 1)
            bound = float((e.src_weight.abs() + e.own_weight.abs()).max()) * 2.0 ** -24 + 1e-12
            assert float((got - CC.controlled_probs(spec, base, own)).abs().max()) <= bound, name


def test_identity_and_what_counts_as_unedited():
    from vidtome_amd import CrossEdit
    e = CrossEdit.identity(5)
    assert e.is_identity and torch.equal(e.mapper, torch.eye(5)) and e.K == 5
    assert CrossEdit.replace(torch.rand(5, 5), alpha_words=0.0).is_identity          # aw = 0: the own probabilities
    assert CrossEdit.refine(torch.arange(5), torch.zeros(5)).is_identity
    assert not CrossEdit.replace(torch.eye(5)).is_identity                            # the source's probabilities
    assert not CrossEdit.identity(5).reweight(torch.full((5,), 2.0)).is_identity      # (b is scaled)
    # any float dtype goes in, fp32 is kept; integer indices only
    e = CrossEdit(torch.eye(3, dtype=torch.float64), torch.ones(3, dtype=torch.float16), torch.zeros(3, dtype=torch.bfloat16))
    assert all(t.dtype == torch.float32 for t in e.on("cpu"))
    assert e.on("cpu")[0] is e.on("cpu")[0]
    with pytest.raises(ValueError, match=r"\(K, K\)"):
        CrossEdit(torch.eye(3)[:2], torch.ones(3), torch.ones(3))
    with pytest.raises(ValueError, match="shape"):
        CrossEdit(torch.eye(3), torch.ones(4), torch.ones(3))
    with pytest.raises(ValueError, match="alphas must be 0"):
        CrossEdit.refine([0, -1, 1], [1.0, 0.5, 1.0])
    with pytest.raises(TypeError, match="integers"):
        CrossEdit.refine([0.0, 1.0], [1.0, 1.0])
    with pytest.raises(ValueError, match="-1 .. 1"):
        CrossEdit.refine([0, 2], [1.0, 1.0])


def _model(built):
    import vidtome_amd
    unet = standin.StandInUNet(C, 2, full=True, cond_dim=32)
    vidtome_amd.apply_patch(unet)
    return unet


def _names(unet):
    return [n for n, m in unet.named_modules() if m.__class__.__name__ == "ToMeBlock"]


def test_public_names():
    import vidtome_amd
    from vidtome_amd import p2p
    assert vidtome_amd.CrossEdit is p2p.CrossEdit
    assert vidtome_amd.register_cross_attention_control is p2p.register_cross_attention_control
    assert {"CrossEdit", "register_cross_attention_control", "unregister_cross_attention_control"} <= set(vidtome_amd.__all__)


def test_registration_selection_reregistration_and_clearing(built):
    import vidtome_amd
    from vidtome_amd import CrossEdit
    unet = _model(built)
    names = _names(unet)
    blocks = dict(unet.named_modules())
    on = lambda: sorted(n for n in names if "vtm_cross_control" in blocks[n].__dict__)
    e1, e2 = CrossEdit.replace(torch.eye(4)), CrossEdit.replace(torch.eye(4), 0.5)
    assert vidtome_amd.register_cross_attention_control(unet, [1, 2], 3, {2: e1}) == sorted(names) == on()
    assert blocks[names[0]].vtm_cross_control[:3] == ([1, 2], 3, {2: e1}) and blocks[names[0]].vtm_cross_control[3] == names[0]
    # by names; registering again replaces the schedule, the edits and the selection
    assert vidtome_amd.register_cross_attention_control(unet, [5], 3, {1: e2, 2: e1}, names[2:4]) == sorted(names[2:4]) == on()
    assert blocks[names[2]].vtm_cross_control[:3] == ([5], 3, {1: e2, 2: e1})
    # by predicate
    top = lambda name, blk: name.startswith("up_blocks.3.") and blk is blocks[name]
    got = vidtome_amd.register_cross_attention_control(unet, [5], 2, {1: e2}, top)
    assert got == on() == sorted(n for n in names if n.startswith("up_blocks.3.")) and len(got) == 3
    with pytest.raises(ValueError, match="not patched blocks"):
        vidtome_amd.register_cross_attention_control(unet, [5], 2, {1: e2}, ["up_blocks.9.nothing"])
    # group 0 is the source; groups beyond num_inputs do not exist; a refused call changes nothing
    for bad in ({0: e1}, {3: e1}, {-1: e1}, {"1": e1}):
        with pytest.raises(ValueError, match="group 0 is the source"):
            vidtome_amd.register_cross_attention_control(unet, [5], 3, bad)
    with pytest.raises(TypeError, match="not a CrossEdit"):
        vidtome_amd.register_cross_attention_control(unet, [5], 3, {1: torch.eye(4)})
    with pytest.raises(ValueError, match="num_inputs"):
        vidtome_amd.register_cross_attention_control(unet, [5], 1, {})
    assert on() == got
    vidtome_amd.unregister_cross_attention_control(unet)
    assert on() == []
    vidtome_amd.register_cross_attention_control(standin.Pipe(unet), [5], 3, {2: e1}, names[:2])     # the pipeline form
    assert on() == sorted(names[:2])
    vidtome_amd.remove_patch(unet)
    assert on() == []
    with pytest.raises(RuntimeError, match="nothing is patched"):
        vidtome_amd.register_cross_attention_control(unet, [5], 3, {2: e1})


def test_a_block_injects_by_the_pnp_rule(built):
    import vidtome_amd
    from vidtome_amd import CrossEdit, patch as vpatch, pnp
    unet = CC.patched(C, torch.float32, "cpu", heads=2)
    blk = unet.block
    edits = {2: CrossEdit.replace(torch.eye(4))}
    assert vpatch.cross_control(blk) is None                                          # not registered
    assert vidtome_amd.register_cross_attention_control(unet, [981, 961], 3, edits) == [CC.BLOCK]
    assert vpatch.cross_control(blk) is None                                          # no timestep stamped
    for t, injects in ((981, True), (941, False), (1000, True), (961, True), (torch.tensor(941), False)):
        pnp.register_time(standin.Pipe(unet), t)
        assert (vpatch.cross_control(blk) is not None) == injects, t
    pnp.register_time(standin.Pipe(unet), 981)
    assert vpatch.cross_control(blk) == (3, edits, CC.BLOCK)
    vidtome_amd.unregister_cross_attention_control(unet)
    assert vpatch.cross_control(blk) is None
    vidtome_amd.remove_patch(unet)


# ---------------------------------------------------------------------------------------------------
# the forward, with attn1 a computing stand-in and the three launches of an injecting attn2 segment stubbed in torch
# ---------------------------------------------------------------------------------------------------
def _heads(t, heads):
    return t.float().view(t.shape[0], t.shape[1], heads, -1).transpose(1, 2)


def _stub_core(monkeypatch, calls):
    """fp32 torch stand-ins of _lib.attention_kv, _lib.cross_edit_values and _lib.attention_kv_sets_src on host tensors."""
    from vidtome_amd import _lib

    def softmax_pv(q, k, vt, heads, Mq, start, Mk, scale):
        p = torch.softmax(_heads(q[:, :Mq], heads) @ _heads(k[:, start:start + Mk], heads).transpose(-1, -2) * scale, dim=-1)
        v = _heads(vt[:, :, start:start + Mk].transpose(1, 2), heads)
        return (p @ v).transpose(1, 2).reshape(q.shape[0], Mq, -1)

    def attention_kv(q, k, vt, heads, Mq, Mk, scale, out=None, **kw):
        calls.append(("kv", q.shape[0]))
        assert out is not None and not kw
        out[:, :Mq] = softmax_pv(q, k, vt, heads, Mq, 0, Mk, scale).to(out.dtype)
        return out

    def cross_edit_values(vt, v_start, K, mapper, src_w, own_w, start_src=0, start_own=None, out=None):
        calls.append(("edit", vt.shape[0]))
        v = vt[:, :, v_start:v_start + K].float()
        out[:, :, start_src:start_src + K] = torch.einsum("wn,bcn->bcw", mapper * src_w, v).to(out.dtype)
        out[:, :, start_own:start_own + K] = (own_w * v).to(out.dtype)
        return out

    def attention_kv_sets_src(q, q_src, k, vt, heads, Mq, sets, scale, set_src, out=None):
        calls.append(("sets_src", q.shape[0], tuple(set_src), [s[:2] for s in sets]))
        acc = 0
        for (start, n, w), from_src in zip(sets, set_src):
            acc = acc + w * softmax_pv(q_src if from_src else q, k, vt, heads, Mq, start, n, scale)
        out[:, :Mq] = acc.to(out.dtype)
        return out
    from vidtome_amd import patch as vpatch
    monkeypatch.setattr(_lib, "attention_probs", lambda q, k, heads, Mq, Mk, scale, bias=None:
                        vpatch._probs_torch(q[:, :Mq], k[:, :Mk], heads, scale, bias))
    monkeypatch.setattr(_lib, "attention_kv", attention_kv)
    monkeypatch.setattr(_lib, "cross_edit_values", cross_edit_values)
    monkeypatch.setattr(_lib, "attention_kv_sets_src", attention_kv_sets_src)


def _cpu_block(built, dtype=torch.bfloat16, K=CC.COND):
    """The stand-in block on the host with a computing attn1: attn2 of an injecting step is then all that needs the
    library, and ``fused_attention_ok`` only refuses the host tensors."""
    unet = CC.ControlUNet(C, heads=2)
    unet.block.attn1 = AM.ComputingSelf(C, 2)
    unet.block.attn1.load_state_dict(CC.ControlUNet(C, heads=2).block.attn1.state_dict())
    unet = unet.to(dtype)
    import vidtome_amd
    vidtome_amd.apply_patch(unet, batch_size=CC.NUM_INPUTS)
    unet.set_size(CC.LATENT)
    h, cond = CC.inputs(C, dtype, "cpu", K=K)
    return unet, h, cond


def test_layout_errors_raise_at_forward_and_name_the_block(built, monkeypatch):
    import vidtome_amd
    from vidtome_amd import pnp
    unet, h, cond = _cpu_block(built)
    calls = []
    _stub_core(monkeypatch, calls)
    pnp.register_time(standin.Pipe(unet), 981)
    vidtome_amd.register_cross_attention_control(unet, [981], 3, {2: CC.edit_of(CC.specs(5)["replace"])})
    with torch.no_grad():
        with pytest.raises(RuntimeError, match=rf"'{re.escape(CC.BLOCK)}'.*K = 5 tokens, the conditioning has 77"):
            unet.block(h, encoder_hidden_states=cond)
        vidtome_amd.register_cross_attention_control(unet, [981], 4, {2: CC.edit_of(CC.specs()["replace"])})
        with pytest.raises(RuntimeError, match=rf"'{re.escape(CC.BLOCK)}'.*6 samples is not 4 groups"):
            unet.block(h, encoder_hidden_states=cond)
        vidtome_amd.register_cross_attention_control(unet, [981], 3, {2: CC.edit_of(CC.specs()["replace"])})
        with pytest.raises(RuntimeError, match=rf"'{re.escape(CC.BLOCK)}'.*IP-Adapter"):
            unet.block(h, encoder_hidden_states=(cond, [cond[:, :4]]))
        with pytest.raises(RuntimeError, match=rf"'{re.escape(CC.BLOCK)}'.*attention_mask"):
            unet.block(h, encoder_hidden_states=cond, encoder_attention_mask=torch.zeros(6, 1, 77, dtype=h.dtype))
        with pytest.raises(RuntimeError, match=rf"'{re.escape(CC.BLOCK)}'.*processor kwargs \['scale'\]"):
            unet.block(h, encoder_hidden_states=cond, cross_attention_kwargs={"scale": 1.0})
        with pytest.raises(RuntimeError, match=rf"'{re.escape(CC.BLOCK)}'.*fused_attention_ok"):
            unet.block(h, encoder_hidden_states=cond)                                    # (host tensors)
    assert calls == []                                                                   # nothing was launched
    vidtome_amd.remove_patch(unet)


@pytest.mark.parametrize("name", ["replace", "refine", "refine_reweight"])
def test_host_protocol_of_an_injecting_block(built, name, monkeypatch):
    """The attn2 segment of an injecting block with its launches stubbed: one plain core over the contiguous run of unedited
    groups [source, uncond] on slices of the q / out buffers, then per edited group one value pre-pass and one two-set launch
    with ``set_src = (1, 0)`` at 0 and K rounded up to 8; the block output against the float64 P2P restatement within the
    bf16 block tolerance (the stubs compute in fp32 and round q, k, v, V', V'' and the core's output to bf16 as the kernels
    do); the edited head-averaged map against the restatement's."""
    import vidtome_amd
    from vidtome_amd import patch as vpatch, pnp
    unet, h, cond = _cpu_block(built)
    blk = unet.block
    calls = []
    _stub_core(monkeypatch, calls)
    monkeypatch.setattr(vpatch, "fused_attention_ok", lambda attn, x, self_attn=True, **kw: not self_attn)   # (attn2 alone)
    spec = CC.specs()[name]
    pnp.register_time(standin.Pipe(unet), 981)
    vidtome_amd.register_cross_attention_control(unet, [981], 3, {1: vidtome_amd.CrossEdit.identity(CC.COND), 2: CC.edit_of(spec)})
    vidtome_amd.register_attention_maps(unet)
    with torch.no_grad():
        out = blk(h, encoder_hidden_states=cond)
    assert calls == [("kv", 4), ("edit", 2), ("sets_src", 2, (1, 0), [(0, 77), (80, 77)])], calls
    ref = CC.block64(blk, h, cond, {2: spec})
    plain = CC.block64(blk, h, cond)
    osc = max(1.0, float(ref.abs().max()))
    err = float((out.double() - ref).abs().max()) / osc
    moved = float((ref - plain)[4:].abs().max()) / osc
    print(f"host protocol {name}: err/scale={err:.3e} edit/scale={moved:.3e}")
    assert err < 8e-3 and moved > 2 * 8e-3, (err, moved)
    assert float((out.double() - plain)[:4].abs().max()) / osc < 8e-3                     # source and uncond: not edited
    # the map: groups 0 and 1 are the plain head-average, group 2 the edited one
    got = blk.attn2_probs
    assert tuple(got.shape) == (6, CC.TOKENS, CC.COND) and got.dtype == torch.float32
    x2 = torch.nn.functional.layer_norm(_attn2_input(blk, h), (C,), blk.norm2.weight, blk.norm2.bias, blk.norm2.eps)
    q, k = blk.attn2.to_q(x2).detach(), blk.attn2.to_k(cond).detach()
    per_head = torch.softmax(_heads(q, 2).double() @ _heads(k, 2).double().transpose(-1, -2) * blk.attn2.scale, dim=-1)
    want = per_head.mean(1)
    for f in range(2):
        want[4 + f] = CC.controlled_probs(spec, per_head[f], per_head[4 + f]).mean(0)
    e = CC.edit_of(spec)
    bound = (CC.COND + 8) * 2.0 ** -24 * (1 + float(e.src_weight.abs().sum()) + float(e.own_weight.abs().sum()))
    assert float((got.double() - want).abs().max()) <= bound                              # (the same bf16 q / k rows)
    assert float((got.double() - want)[:4].abs().max()) <= (CC.COND + 8) * 2.0 ** -24
    # outside the schedule the block asks for nothing of this: the module path's stand-in forward raises
    pnp.register_time(standin.Pipe(unet), 941)
    calls.clear()
    monkeypatch.undo()
    with torch.no_grad(), pytest.raises(RuntimeError, match="must not be called"):
        blk(h, encoder_hidden_states=cond)
    vidtome_amd.remove_patch(unet)


def _attn2_input(blk, h):
    """The hidden states attn2's segment sees: attn1's segment of the computing stand-in on the host."""
    with torch.no_grad():
        x1 = blk.norm1(h)
        return blk.attn1(x1) + h


def test_header_declares_and_lib_binds_both_exports(built):
    from vidtome_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    lib = ctypes.CDLL(built)
    for name, nargs, source in (("vtm_attention_kv_sets_src", 25, "attention_sets.hip"),
                                ("vtm_cross_edit_values", 15, "cross_edit.hip")):
        decl = re.search(rf"int {name}\((.*?)\);", hdr, re.S)
        assert decl and hasattr(lib, name) and name in _lib.exported_symbols(), name
        assert len(decl.group(1).split(",")) == len(_lib._SIGNATURES[name][0]) == nargs, name
        assert f"{name} --" in hdr[:decl.start()] and source in build.SOURCES
    assert re.search(r"#define VTM_ABI_VERSION 2\b", hdr) and _lib.lib().vtm_version() == _lib.ABI_VERSION == 2
    assert callable(_lib.attention_kv_sets_src) and callable(_lib.cross_edit_values)


def test_wrappers_refuse_bad_operands_before_any_launch():
    from vidtome_amd import _lib
    q, k, vt = torch.zeros(2, 16, C).half(), torch.zeros(2, 16, C).half(), torch.zeros(2, C, 16).half()
    sets = [(0, 5, 1.0), (8, 5, 1.0)]
    with pytest.raises(RuntimeError, match="2 sets but 1 set_src"):
        _lib.attention_kv_sets_src(q, q, k, vt, 2, 16, sets, 0.125, (1,))
    with pytest.raises(RuntimeError, match="0 .q. or 1 .q_src."):
        _lib.attention_kv_sets_src(q, q, k, vt, 2, 16, sets, 0.125, (2, 0))
    with pytest.raises(RuntimeError, match="fp16 / bf16"):
        _lib.attention_kv_sets_src(q.float(), q.float(), k.float(), vt.float(), 2, 16, sets, 0.125, (1, 0))
    with pytest.raises(RuntimeError, match="q_src must be"):
        _lib.attention_kv_sets_src(q, q[:, :8], k, vt, 2, 16, sets, 0.125, (1, 0))       # fewer rows than Mq
    with pytest.raises(RuntimeError, match="fp16 / bf16"):
        _lib.cross_edit_values(vt.float(), 0, 5, torch.eye(5), torch.ones(5), torch.ones(5))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        _lib.cross_edit_values(vt, 0, 5, torch.eye(5), torch.ones(5), torch.ones(5))
