"""CPU tests of LoHa / LoKr (LyCORIS) recognition (vidtome_amd/lora.py): every accepted form is read by the fused path, every
refused form keeps the module path without raising, every adapter-state change -- and nothing else -- changes the state
token, the C ABI declares and binds the fold exports, and their argument checks answer before any launch.  Also the
stand-in's own consistency: its forward is the Linear host_fold_lycoris describes, before and after merge."""
import itertools
import os

import pytest
import torch

from lycoris_standin import LoHaLinear, LoKrLinear, host_fold_lycoris, kron_split, wrap_lycoris

C_OUT, C_IN = 48, 64                    # 48 = 6 x 8, 64 = 8 x 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeCuda(torch.Tensor):          # the predicates need x.is_cuda; emulate it without a device
    @property
    def is_cuda(self):
        return True


def _base(seed=0, bias=True, co=C_OUT, ci=C_IN):
    base = torch.nn.Linear(ci, co, bias=bias)
    with torch.no_grad():
        base.weight.copy_(torch.randn(co, ci, generator=torch.Generator().manual_seed(seed)) * ci ** -0.5)
    return base


def _loha(n=1, r=4, seed=0, co=C_OUT, ci=C_IN, bias=True):
    g = torch.Generator().manual_seed(seed + 1)
    m = LoHaLinear(_base(seed, bias, co, ci))
    rn = lambda *s: torch.randn(*s, generator=g) * 0.3
    for i in range(n):
        m.update_layer(f"a{i}", rn(co, r), rn(r, ci), rn(co, r), rn(r, ci), 0.5)
    return m


def _lokr(forms=("full", "full"), n=1, r=3, seed=0, co=C_OUT, ci=C_IN, bias=True):
    g = torch.Generator().manual_seed(seed + 1)
    m = LoKrLinear(_base(seed, bias, co, ci))
    (a1, a2), (b1, b2) = kron_split(co), kron_split(ci)
    rn = lambda *s: torch.randn(*s, generator=g) * 0.3
    f = lambda form, rows, cols: rn(rows, cols) if form == "full" else (rn(rows, r), rn(r, cols))
    for i in range(n):
        m.update_layer(f"a{i}", f(forms[0], a1, b1), f(forms[1], a2, b2), 0.5)
    return m


def _accepted(m, kind, co=C_OUT):
    """recognise names the kind, and a self-attention whose to_v is the layer passes the fused path's predicate."""
    from standin import Attention
    from vidtome_amd import lora
    from vidtome_amd import patch as vpatch
    if lora.recognise(m) != kind or lora.base_linear(m) is not m.base_layer:
        return False
    if m.in_features != m.out_features:
        return True
    a = Attention(m.in_features, 2)
    a.to_v = m
    return bool(vpatch.fused_attention_ok(a, torch.zeros(2, 8, m.in_features).as_subclass(FakeCuda)))


FORMS = list(itertools.product(("full", "lowrank"), repeat=2))


def test_recogniser_accepts_loha():
    from vidtome_amd import lora
    assert lora.LOHA == "loha" and lora.LOKR == "lokr"
    assert _accepted(_loha(), lora.LOHA)
    assert _accepted(_loha(co=64), lora.LOHA)                         # square: through fused_attention_ok too
    assert _accepted(_loha(2, co=64), lora.LOHA)                      # two active adapters
    assert _accepted(_loha(r=1, bias=False), lora.LOHA)
    m = _loha(2, co=64)
    m.set_adapter("a1")
    assert _accepted(m, lora.LOHA)
    m.set_adapter(["a1", "missing"])                                  # a name without weights on this layer is skipped
    assert _accepted(m, lora.LOHA) and len(lora.state_token(m)) == len(lora.state_token(_loha(co=64)))
    m = _loha(co=64)
    m.rank_dropout["a0"] = 0.5
    m.module_dropout["a0"] = 0.5
    m.eval()                                                          # eval-mode dropout is the identity
    assert _accepted(m, lora.LOHA)


@pytest.mark.parametrize("forms", FORMS)
def test_recogniser_accepts_every_lokr_form(forms):
    from vidtome_amd import lora
    assert _accepted(_lokr(forms), lora.LOKR)
    assert _accepted(_lokr(forms, co=64), lora.LOKR)
    assert _accepted(_lokr(forms, n=2, co=64), lora.LOKR)             # two active adapters
    m = _lokr(forms, co=64)
    m.merge()
    assert m.merged and _accepted(m, lora.LOKR)


def test_merged_and_disabled_layers_give_the_base_tensors_without_a_fold():
    """No device is needed when the forward adds no adapter: the base tensors under the state token, cached on the module."""
    from vidtome_amd import lora
    for m in (_loha(2), _lokr(("full", "lowrank"), n=2)):
        for how in ("merge", "disable"):
            m.merge() if how == "merge" else m.enable_adapters(False)
            w, b, k = lora.linear_params(m)
            assert w.data_ptr() == m.base_layer.weight.data_ptr() and b.data_ptr() == m.base_layer.bias.data_ptr()
            assert k == lora.state_token(m) and lora.linear_params(m)[0] is w
            m.unmerge() if how == "merge" else m.enable_adapters(True)


def _refused():
    rejected = {}
    for fam, make in (("loha", _loha), ("lokr", _lokr)):
        m = make()
        m.base_layer = torch.nn.Conv1d(C_IN, C_OUT, 1)
        rejected[f"{fam}: non-Linear base"] = m
        for drop in ("rank_dropout", "module_dropout"):
            m = make()
            getattr(m, drop)["a0"] = 0.1
            rejected[f"{fam}: {drop} in training mode"] = m
        m = make()
        m.merge()
        m.enable_adapters(False)
        rejected[f"{fam}: merged and disabled"] = m
        m = make()
        m.lora_A = torch.nn.ModuleDict()
        rejected[f"{fam}: also has lora_A"] = m
        m = make()
        del m.scaling["a0"]
        rejected[f"{fam}: no scaling entry"] = m
        m = make()
        m.scaling = 0.5
        rejected[f"{fam}: scaling is not a dict"] = m
        m = make()
        del m.merged_adapters
        m.__class__ = type("NoMergedList", (type(m),), {"merged": False})
        rejected[f"{fam}: no merged_adapters"] = m
    P = lambda *s: torch.nn.Parameter(torch.randn(*s), requires_grad=False)
    for t in ("hada_t1", "hada_t2"):
        m = _loha()
        getattr(m, t)["a0"] = P(4, 4, 1, 1)
        rejected[f"loha: {t} entry"] = m
    m = _lokr()
    m.lokr_t2["a0"] = P(4, 4, 1, 1)
    rejected["lokr: lokr_t2 entry"] = m
    m = _loha()
    m.hada_w2_b["a0"] = P(4, C_IN + 1)
    rejected["loha: w2b columns"] = m
    m = _loha()
    m.hada_w1_a["a0"] = P(C_OUT - 1, 4)
    rejected["loha: w1a rows"] = m
    m = _loha()
    m.hada_w2_a["a0"], m.hada_w2_b["a0"] = P(C_OUT, 5), P(5, C_IN)
    rejected["loha: the two products' ranks differ"] = m
    m = _loha()
    m.hada_w1_b["a0"] = P(5, C_IN)
    rejected["loha: inner sizes differ"] = m
    m = _loha()
    del m.hada_w2_a["a0"]
    rejected["loha: a factor is missing"] = m
    m = _loha()
    m.hada_w1_a["a0"] = torch.nn.Parameter(torch.ones(C_OUT, 4, dtype=torch.int32), requires_grad=False)
    rejected["loha: integer factor"] = m
    m = _loha()
    m.hada_w1_b["a0"] = P(4, C_IN, 1)
    rejected["loha: 3-d factor"] = m
    m = _lokr()
    m.lokr_w1["a0"] = P(5, 8)
    rejected["lokr: rows do not multiply out"] = m
    m = _lokr()
    m.lokr_w2["a0"] = P(8, 9)
    rejected["lokr: columns do not multiply out"] = m
    m = _lokr(("lowrank", "full"))
    m.lokr_w1_b["a0"] = P(4, 8)
    rejected["lokr: low-rank inner sizes differ"] = m
    m = _lokr(("full", "lowrank"))
    del m.lokr_w2_b["a0"]
    rejected["lokr: half a low-rank pair"] = m
    m = _lokr()
    m.lokr_w1_a["a0"], m.lokr_w1_b["a0"] = P(6, 2), P(2, 8)
    rejected["lokr: a factor both full and low-rank"] = m
    m = _lokr()
    m.hada_w1_a = torch.nn.ParameterDict()
    rejected["both families' factor dicts"] = m
    return rejected


def test_recogniser_refuses_the_rest_without_raising():
    from standin import Attention
    from vidtome_amd import lora
    from vidtome_amd import patch as vpatch
    rejected = _refused()
    for what, m in rejected.items():
        assert lora.recognise(m) is None, what
        assert lora.linear_params(m) is None, what
    x = torch.zeros(2, 8, 64).as_subclass(FakeCuda)
    for fam, make in (("loha", _loha), ("lokr", _lokr)):              # ... and through the fused path's predicate
        for edit in ("dropout", "merged+disabled", "tucker"):
            m = make(co=64)
            if edit == "dropout":
                m.rank_dropout["a0"] = 0.1
            elif edit == "merged+disabled":
                m.merge()
                m.enable_adapters(False)
            else:
                (m.hada_t1 if fam == "loha" else m.lokr_t2)["a0"] = torch.nn.Parameter(torch.zeros(2, 2, 1, 1))
            for slot in ("to_q", "to_v"):
                a = Attention(64, 2)
                setattr(a, slot, m)
                assert not vpatch.fused_attention_ok(a, x), (fam, edit, slot)
    # only ACTIVE adapters are looked at: an inactive Tucker adapter does not matter
    m = _loha(2)
    m.hada_t1["a1"] = torch.nn.Parameter(torch.zeros(2, 2, 1, 1))
    m.set_adapter("a0")
    assert lora.recognise(m) == lora.LOHA


@pytest.mark.parametrize("make", [lambda: _loha(2), lambda: _lokr(("lowrank", "full"), n=2)], ids=["loha", "lokr"])
def test_state_token_tracks_every_state_change_and_nothing_else(make):
    from vidtome_amd import lora
    m = make()
    tok = lambda: lora.state_token(m)
    t0 = tok()
    assert tok() == t0 and t0[0] == lora.recognise(m)
    m(torch.randn(3, C_IN))                                           # a forward, eval(), an unrelated attribute: no change
    m.eval()
    m.some_flag = 1
    assert tok() == t0
    steps = []

    def changed(what):
        t = tok()
        assert t != (steps[-1][1] if steps else t0), what
        assert tok() == t, what                                       # stable while nothing changes
        steps.append((what, t))

    factors = [n for n in m.factor_names if "a0" in getattr(m, n)]
    assert len(factors) == (4 if isinstance(m, LoHaLinear) else 3)
    for n in factors:
        with torch.no_grad():
            getattr(m, n)["a0"].mul_(1.01)
        changed(f"in-place edit of {n}")
    with torch.no_grad():
        getattr(m, factors[-1])["a1"].add_(0.5)
    changed("in-place edit of the second adapter")
    n = factors[0]
    getattr(m, n)["a0"] = torch.nn.Parameter(getattr(m, n)["a0"].detach().clone(), requires_grad=False)
    changed("a new factor tensor")
    m.scaling["a1"] = 0.25
    changed("scaling")
    m.scaling["a1"] = 0.25 + 2 ** -40                                 # the EXACT scaling is part of the token
    changed("scaling by one part in 2^40")
    m.set_adapter("a0")
    changed("set_adapter: a0 alone")
    m.set_adapter(["a1", "a0"])
    changed("both, in the other order")
    m.set_adapter(["a0", "a1"])
    changed("both again")
    m.enable_adapters(False)
    changed("disable")
    m.enable_adapters(True)
    changed("enable")
    ptr, ver = m.base_layer.weight.data_ptr(), m.base_layer.weight._version
    m.merge()
    assert (m.base_layer.weight.data_ptr(), m.base_layer.weight._version) == (ptr, ver)   # .data edits are invisible
    changed("merge")
    m.unmerge()
    changed("unmerge")
    with torch.no_grad():
        m.base_layer.weight.add_(1.0)
    changed("in-place edit of the base weight")
    with torch.no_grad():
        m.base_layer.bias.add_(1.0)
    changed("in-place edit of the base bias")


def test_header_declares_and_lib_binds_the_exports():
    from vidtome_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    for name in ("vtm_loha_delta", "vtm_lokr_delta", "vtm_delta_fold"):
        assert f"int {name}(" in hdr and name in _lib.exported_symbols(), name
        assert getattr(_lib.lib(), name).restype is not None
    assert "generate.py:93-94" in hdr[hdr.index("vtm_loha_delta"):]
    assert "#define VTM_ABI_VERSION 2" in hdr and _lib.ABI_VERSION == 2   # the exports are additive: the ABI version stays
    assert _lib.lib().vtm_version() == 2


def test_argument_checks_answer_before_any_launch():
    """Fake (never dereferenced) pointers: every bad argument returns -1 from the host-side checks."""
    from vidtome_amd import _lib
    L = _lib.lib()
    p = 4096
    for args in ((0, 64, 4), (64, 0, 4), (64, 64, 0), (-1, 64, 4), (64, 64, -4), (64 * 70000, 64, 4)):
        assert L.vtm_loha_delta(p, p, p, p, *args, 0, p, None) == -1, args
    assert b"vtm_loha_delta" in L.vtm_last_error()
    assert L.vtm_loha_delta(p, p, p, p, 64, 64, 4, 2, p, None) == -1
    for i in range(5):
        ptrs = [p] * 5
        ptrs[i] = None
        assert L.vtm_loha_delta(*ptrs[:4], 64, 64, 4, 0, ptrs[4], None) == -1, i
    for args in ((0, 8, 8, 8, 0, 64), (8, 8, 8, 0, 64, 0), (8, 8, -8, 8, -64, 64), (8, 8, 8, 8, 64, 65), (8, 8, 8, 8, 63, 64),
                 (5, 7, 8, 9, 40, 64), (5, 7, 8, 9, 41, 63), (2 ** 31, 1, 1, 1, 2 ** 31, 1), (1, 2 ** 12, 1, 2 ** 13, 1, 2 ** 25)):
        assert L.vtm_lokr_delta(p, p, *args, 0, p, None) == -1, args
    assert b"vtm_lokr_delta" in L.vtm_last_error()
    assert L.vtm_lokr_delta(p, p, 8, 8, 8, 8, 64, 64, -1, p, None) == -1
    for i in range(3):
        ptrs = [p] * 3
        ptrs[i] = None
        assert L.vtm_lokr_delta(ptrs[0], ptrs[1], 8, 8, 8, 8, 64, 64, 0, ptrs[2], None) == -1, i
    for args in ((0, 64), (64, 0), (-64, 64), (64, -1), (2 ** 31, 1), (2 ** 30, 2 ** 30)):
        assert L.vtm_delta_fold(p, 1, p, *args, p, None) == -1, args
    assert b"vtm_delta_fold" in L.vtm_last_error()
    for code in (3, 7, -1):
        assert L.vtm_delta_fold(p, code, p, 64, 64, p, None) == -1, code
    for i in range(3):
        ptrs = [p] * 3
        ptrs[i] = None
        assert L.vtm_delta_fold(ptrs[0], 1, ptrs[1], 64, 64, ptrs[2], None) == -1, i


@pytest.mark.parametrize("make", [lambda: _loha(2)] + [lambda f=f: _lokr(f, n=2) for f in FORMS],
                         ids=["loha"] + ["lokr-" + "-".join(f) for f in FORMS])
def test_stand_in_forward_is_the_folded_linear(make):
    """The stand-in's forward equals x W_eff^T + b of host_fold_lycoris; merge() keeps it and unmerge() restores it; the
    adapters matter."""
    m = make().double()
    x = torch.randn(16, C_IN, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    w, b = host_fold_lycoris(m)
    want = x @ w.T + b
    assert torch.allclose(m(x), want, atol=1e-12, rtol=0)
    w0, _ = host_fold_lycoris(m, adapters=False)
    assert torch.equal(w0, m.base_layer.weight.detach()) and (x @ w0.T + b - want).abs().max() > 1e-2 * want.abs().max()
    m.merge()
    assert torch.allclose(m(x), want, atol=1e-12, rtol=0)
    assert torch.equal(host_fold_lycoris(m)[0], m.base_layer.weight.detach())
    m.unmerge()
    assert torch.allclose(m(x), want, atol=1e-12, rtol=0)
    m.set_adapter("a1")
    assert not torch.allclose(m(x), want, atol=1e-6, rtol=0)
    assert torch.allclose(m(x), x @ host_fold_lycoris(m)[0].T + b, atol=1e-12, rtol=0)


def test_wrap_lycoris_covers_every_projection_of_a_full_block():
    from vidtome_amd import lora, sites
    for kind, forms in (("loha", None), ("lokr", ("full", "full")), ("lokr", ("lowrank", "lowrank"))):
        unet = sites.SiteUNet([sites.Site("top", 1, 64, 2)], seed=0, full=True)
        wrapped = wrap_lycoris(unet, kind, rank=4, n_adapters=2, forms=forms or ("full", "full"), seed=1)
        assert len(wrapped) == 10
        blk = unet.blocks[0]
        assert blk.attn2.to_k in wrapped and blk.ff.net[2] in wrapped
        for m in wrapped:
            assert lora.recognise(m) == kind
            W = m.base_layer.weight.detach()
            delta = host_fold_lycoris(m)[0] - W.double()
            assert 0.2 <= float(delta.norm() / W.norm()) <= 0.4, kind
