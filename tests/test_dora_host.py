"""CPU tests of DoRA recognition (vidtome_amd/lora.py): the one unambiguous DoRA layout -- a single active DoRA adapter,
first, with a magnitude vector of either container form and no lora_B bias -- and merged DoRA are read by the fused path;
every other DoRA layout keeps the module path; every adapter-state change, the magnitudes included, changes the state
token.  Also the stand-in's own consistency: its forward is the Linear host_fold_dora describes, before and after merge."""
import pytest
import torch

from dora_standin import DoraLinearLayer, DoraPeftLinear, host_fold_dora

C = 64


class FakeCuda(torch.Tensor):          # the predicates need x.is_cuda; emulate it without a device
    @property
    def is_cuda(self):
        return True


def _dora(container="module", trailing=0, r=4, bias=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    base = torch.nn.Linear(C, C, bias=bias)
    with torch.no_grad():
        base.weight.copy_(torch.randn(C, C, generator=g) * C ** -0.5)
    m = DoraPeftLinear(base, container)
    mag = base.weight.detach().norm(dim=1) * (1 + 0.05 * torch.randn(C, generator=g))
    m.update_layer("d0", torch.randn(r, C, generator=g) * C ** -0.5, torch.randn(C, r, generator=g) * 0.1, 0.5, magnitude=mag)
    if trailing:
        m.update_layer("a1", torch.randn(trailing, C, generator=g) * C ** -0.5, torch.randn(C, trailing, generator=g) * 0.1,
                       0.75, b_bias=torch.randn(C, generator=g) * 0.1 if bias else None)
    return m


def _accepted(m):
    from standin import Attention
    from vidtome_amd import lora
    from vidtome_amd import patch as vpatch
    a = Attention(C, 2)
    a.to_q = m
    return lora.recognise(m) == lora.PEFT and vpatch.fused_attention_ok(a, torch.zeros(2, 8, C).as_subclass(FakeCuda))


@pytest.mark.parametrize("container", ["module", "param"])
def test_recogniser_accepts_a_first_dora_adapter(container):
    assert _accepted(_dora(container))
    assert _accepted(_dora(container, trailing=8))
    m = _dora(container, trailing=8)
    m.lora_dropout["d0"] = torch.nn.Dropout(0.1)
    m.eval()                                                          # eval-mode dropout is the identity
    assert _accepted(m)
    m = _dora(container, trailing=8)
    m.set_adapter("a1")                                               # DoRA inactive: a plain LoRA layer
    assert _accepted(m)


def test_recogniser_accepts_merged_dora():
    from vidtome_amd import lora
    m = _dora(trailing=8, bias=True)
    m.merge()
    assert m.merged and _accepted(m)
    w, b, k = lora.linear_params(m)                                   # the merged base weight, nothing folded
    assert w.data_ptr() == m.base_layer.weight.data_ptr() and b.data_ptr() == m.base_layer.bias.data_ptr()
    assert k == lora.state_token(m)
    m.merge()
    m.merged_adapters = m.merged_adapters[:1]                         # merged, with DoRA no longer first among the rest:
    m.set_adapter(["a1", "d0"])                                       # PEFT's forward is still the base layer
    assert _accepted(m)


def test_recogniser_rejects_every_other_dora_layout():
    from vidtome_amd import lora
    rejected = {}
    m = _dora(trailing=8)
    m.set_adapter(["a1", "d0"])
    rejected["DoRA after a plain adapter"] = m
    m = _dora()
    mag = m.magnitude("d0").detach() * 1.1
    m.update_layer("d1", torch.randn(4, C), torch.randn(C, 4), 0.5, magnitude=mag)
    rejected["two DoRA adapters"] = m
    m = _dora()
    m.set_adapter(["d0"])
    m.update_layer("d1", torch.randn(4, C), torch.randn(C, 4), 0.5, magnitude=mag)
    m.set_adapter(["d1", "d0"])
    rejected["two DoRA adapters, the other first"] = m
    m = _dora()
    m.lora_B["d0"] = torch.nn.Linear(4, C, bias=True)
    rejected["DoRA with a lora_B bias"] = m
    m = _dora()
    m.lora_dropout["d0"] = torch.nn.Dropout(0.1)
    rejected["training-mode dropout on the DoRA adapter"] = m
    for container in ("module", "param"):
        m = _dora(container)
        if container == "module":
            m.lora_magnitude_vector["d0"] = DoraLinearLayer(torch.ones(C - 1))
        else:
            m.lora_magnitude_vector["d0"] = torch.nn.Parameter(torch.ones(1, C), requires_grad=False)
        rejected[f"wrongly shaped magnitude ({container})"] = m
    m = _dora()
    del m.lora_magnitude_vector["d0"]
    rejected["use_dora without a magnitude"] = m
    m = _dora()
    del m.lora_magnitude_vector
    rejected["no lora_magnitude_vector at all"] = m
    m = _dora()
    m.lora_magnitude_vector["d0"].fan_in_fan_out = True
    rejected["magnitude module with fan_in_fan_out"] = m
    m = _dora()
    m.fan_in_fan_out = True
    rejected["fan_in_fan_out"] = m
    m = _dora()
    m.merge()
    m.enable_adapters(False)
    rejected["merged and disabled"] = m
    for what, m in rejected.items():
        assert lora.recognise(m) is None, what
        assert lora.linear_params(m) is None, what
        assert not _accepted(m), what


def test_state_token_tracks_every_dora_state_change():
    from vidtome_amd import lora
    m = _dora(trailing=8)
    tok = lambda: lora.state_token(m)
    t0 = tok()
    assert tok() == t0 and any("dora" in part for part in t0 if isinstance(part, tuple))
    steps = []

    def changed(what):
        t = tok()
        assert t != (steps[-1][1] if steps else t0), what
        assert tok() == t, what                                       # stable while nothing changes
        steps.append((what, t))

    with torch.no_grad():
        m.magnitude("d0").mul_(1.01)
    changed("in-place edit of the magnitude")
    m.lora_magnitude_vector["d0"] = DoraLinearLayer(m.magnitude("d0").detach() * 1.0)
    changed("a new magnitude tensor")
    m.scaling["d0"] = 0.25
    changed("DoRA scaling")
    m.scaling["d0"] = 0.25 + 2 ** -40
    changed("DoRA scaling by one part in 2^40")
    m.scaling["a1"] = 0.5
    changed("trailing scaling")
    m.set_adapter("a1")
    changed("set_adapters: plain only")
    m.set_adapter("d0")
    changed("set_adapters: DoRA only")
    m.set_adapter(["d0", "a1"])
    changed("set_adapters: both again")
    m.enable_adapters(False)
    changed("disable")
    m.enable_adapters(True)
    changed("enable")
    m.merge()
    changed("merge")
    m.unmerge()
    changed("unmerge")
    with torch.no_grad():
        m.lora_A["d0"].weight.add_(1.0)
    changed("in-place edit of the DoRA A")
    with torch.no_grad():
        m.base_layer.weight.add_(1.0)
    changed("in-place edit of the base weight")

    p = _dora("param")
    t0 = lora.state_token(p)
    with torch.no_grad():
        p.magnitude("d0").add_(0.5)
    assert lora.state_token(p) != t0                                  # the older PEFT container too


@pytest.mark.parametrize("container", ["module", "param"])
@pytest.mark.parametrize("trailing", [0, 8])
def test_stand_in_forward_is_the_folded_linear(container, trailing):
    """PEFT's DoRA forward (running result, bias handling) equals x W_eff^T + b_eff of host_fold_dora; merge() keeps it and
    unmerge() restores it; the magnitudes matter (r = 1 is far off)."""
    m = _dora(container, trailing=trailing, bias=True).double()
    x = torch.randn(16, C, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    w, b = host_fold_dora(m)
    want = x @ w.T + b
    assert torch.allclose(m(x), want, atol=1e-12, rtol=0)
    w1, _ = host_fold_dora(m, magnitude=False)
    assert (x @ w1.T + b - want).abs().max() > 1e-3 * want.abs().max()
    m.merge()                           # (the stand-ins' delta weight is computed in fp32, as PEFT's is for 16-bit)
    assert torch.allclose(m(x), want, atol=1e-5, rtol=0)
    assert torch.equal(host_fold_dora(m)[0], m.base_layer.weight.detach())
    m.unmerge()
    assert torch.allclose(m(x), want, atol=1e-5, rtol=0)
