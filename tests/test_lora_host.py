"""CPU tests of the LoRA recogniser and its state token (vidtome_amd/lora.py): what the fused path accepts, and that every
adapter-state change -- and nothing else -- changes the key the folded weights and the packed caches are rebuilt by."""
import pytest
import torch

from lora_standin import LoRACompatibleLinear, LoRALinearLayer, PeftLinear, wrap_lora


class FakeCuda(torch.Tensor):          # the predicates need x.is_cuda; emulate it without a device
    @property
    def is_cuda(self):
        return True


def _peft(n_adapters=1, C=64, r=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    m = PeftLinear(torch.nn.Linear(C, C, bias=False))
    for i in range(n_adapters):
        m.update_layer(f"a{i}", torch.randn(r, C, generator=g), torch.randn(C, r, generator=g), 0.5)
    return m


def _legacy(C=64, r=4, bias=True):
    m = LoRACompatibleLinear(C, C, bias=bias)
    m.lora_layer = LoRALinearLayer(C, C, r, network_alpha=2.0)
    return m


def test_recogniser_accepts_the_complete_layers_and_rejects_the_rest():
    from standin import Attention
    from vidtome_amd import lora
    from vidtome_amd import patch as vpatch
    x = torch.zeros(2, 8, 64).as_subclass(FakeCuda)
    assert lora.recognise(torch.nn.Linear(64, 64)) == lora.PLAIN
    assert lora.recognise(LoRACompatibleLinear(64, 64)) == lora.PLAIN
    assert lora.recognise(_peft()) == lora.PEFT and lora.recognise(_peft(2)) == lora.PEFT
    assert lora.recognise(_legacy()) == lora.LEGACY
    a = Attention(64, 2)
    a.to_q, a.to_k, a.to_v = _peft(), _peft(2), _legacy(bias=False)
    a.to_out[0] = _legacy()
    assert vpatch.fused_attention_ok(a, x)

    rejected = {}
    m = _peft()
    m.use_dora["a0"] = True
    rejected["dora"] = m
    m = _peft()
    m.fan_in_fan_out = True
    rejected["fan_in_fan_out"] = m
    m = _peft()
    m.lora_dropout["a0"] = torch.nn.Dropout(0.1)
    rejected["training dropout"] = m
    m = _peft()
    m.lora_A["a0"] = torch.nn.Conv1d(64, 4, 1)
    rejected["conv adapter"] = m
    m = _peft()
    m.lora_B["a0"] = torch.nn.Sequential(torch.nn.Linear(4, 64, bias=False))
    rejected["non-Linear lora_B"] = m
    m = _peft()
    m.base_layer = torch.nn.Conv1d(64, 64, 1)
    rejected["non-Linear base"] = m
    m = _legacy()
    m.lora_layer = torch.nn.Linear(64, 64)                                    # the old stand-in of test_host.py
    rejected["lora_layer = Linear"] = m
    m = _legacy()
    m.lora_layer.up = torch.nn.Identity()
    rejected["legacy up not a Linear"] = m

    class BaseOnly(torch.nn.Module):                                          # the other old stand-in: base_layer alone
        def __init__(self, base):
            super().__init__()
            self.base_layer = base
            self.weight = base.weight
    rejected["base_layer only"] = BaseOnly(torch.nn.Linear(64, 64))

    class Subclass(torch.nn.Linear):                                          # an unknown Linear subclass (own forward)
        pass
    rejected["unknown subclass"] = Subclass(64, 64)
    for what, m in rejected.items():
        assert lora.recognise(m) is None, what
        assert lora.linear_params(m) is None, what
        a = Attention(64, 2)
        a.to_v = m
        assert not vpatch.fused_attention_ok(a, x), what

    # dropout with p > 0 is the identity in eval mode (PEFT: lora_dropout is a Dropout module)
    m = rejected["training dropout"].eval()
    assert lora.recognise(m) == lora.PEFT
    # merged and disabled at once: PEFT's forward unmerges first -- a side effect only the module path performs
    m = _peft()
    m.merge()
    m.enable_adapters(False)
    assert lora.recognise(m) is None


def test_state_token_tracks_every_adapter_state_change():
    from vidtome_amd import lora
    m = _peft(2)
    tok = lambda: lora.state_token(m)
    t0 = tok()
    assert tok() == t0 == lora.state_token(m)
    steps = []

    def changed(what):
        t = tok()
        assert t != steps[-1][1] if steps else t != t0, what
        assert tok() == t, what                                               # stable while nothing changes
        steps.append((what, t))

    m.scaling["a1"] = 0.25
    changed("scaling")
    m.scaling["a1"] = 0.25 + 2 ** -40                                         # the EXACT scaling is part of the token
    changed("scaling by one part in 2^40")
    m.set_adapter("a0")
    changed("active-adapter switch")
    m.set_adapter(["a0", "a1"])
    changed("both adapters again")
    m.enable_adapters(False)
    changed("disable")
    m.enable_adapters(True)
    changed("enable")
    ptr, ver = m.base_layer.weight.data_ptr(), m.base_layer.weight._version
    m.merge()
    assert (m.base_layer.weight.data_ptr(), m.base_layer.weight._version) == (ptr, ver)   # the trap: .data edits are invisible
    changed("merge")
    m.unmerge()
    changed("unmerge")
    with torch.no_grad():
        m.lora_A["a0"].weight.add_(1.0)
    changed("in-place edit of A")
    with torch.no_grad():
        m.lora_B["a1"].weight.mul_(2.0)
    changed("in-place edit of B")
    with torch.no_grad():
        m.base_layer.weight.add_(1.0)
    changed("in-place edit of the base weight")

    legacy = _legacy()
    t0 = lora.state_token(legacy)
    assert lora.state_token(legacy) == t0
    legacy.lora_layer.network_alpha = 3.0
    assert lora.state_token(legacy) != t0
    t1 = lora.state_token(legacy)
    with torch.no_grad():
        legacy.lora_layer.down.weight.add_(1.0)
    assert lora.state_token(legacy) != t1


def test_linear_params_without_adapters_to_fold_needs_no_device():
    """Plain Linears give their own tensors under (pointer, version) keys; a disabled PEFT layer gives its base tensors
    under the state token (no fold runs), cached on the module: repeated calls return the same tensors and key."""
    from vidtome_amd import lora
    lin = torch.nn.Linear(64, 32)
    w, b, k = lora.linear_params(lin)
    assert w is lin.weight and b is lin.bias and lora.linear_params(lin)[2] == k
    with torch.no_grad():
        lin.weight.add_(1.0)
    assert lora.linear_params(lin)[2] != k
    m = _peft()
    m.enable_adapters(False)
    w, b, k = lora.linear_params(m)
    assert w.data_ptr() == m.base_layer.weight.data_ptr() and b is None and k == lora.state_token(m)
    w2, _, k2 = lora.linear_params(m)
    assert w2 is w and k2 == k
    wh, _, _ = lora.linear_params(m, torch.float64)
    assert wh.dtype == torch.float64 and m.__dict__["_vtm_lora"][1] is w


def test_wrap_lora_covers_every_projection_of_a_full_block():
    from vidtome_amd import sites
    sl = [sites.Site("top", 1, 64, 2)]
    unet = sites.SiteUNet(sl, seed=0, full=True)
    ref = {n: p.detach().clone() for n, p in unet.named_parameters()}
    wrapped = wrap_lora(unet, ranks=(4, 8), ratio=0.3)
    assert len(wrapped) == 10 and all(isinstance(m, PeftLinear) for m in wrapped)
    blk = unet.blocks[0]
    assert isinstance(blk.attn2.to_k, PeftLinear) and isinstance(blk.ff.net[2], PeftLinear)
    for m in wrapped:
        W = m.base_layer.weight.detach()
        delta = sum(m.scaling[a] * m.lora_B[a].weight @ m.lora_A[a].weight for a in m.active_adapters)
        assert 0.2 <= float(delta.norm() / W.norm()) <= 0.5
    x = torch.randn(3, 64)
    m = blk.attn1.to_q
    want = x @ ref["blocks.0.attn1.to_q.weight"].T + sum(
        m.scaling[a] * (x @ m.lora_A[a].weight.T) @ m.lora_B[a].weight.T for a in m.active_adapters)
    assert torch.allclose(m(x), want, atol=1e-5)


@pytest.mark.parametrize("kind", ["peft", "legacy"])
def test_merge_and_unmerge_edit_the_base_weight_in_place(kind):
    from vidtome_amd import sites
    unet = sites.SiteUNet([sites.Site("top", 1, 64, 2)], seed=0)
    m = wrap_lora(unet, kind=kind, ranks=(4,))[0]
    x = torch.randn(5, 64)
    y = m(x)
    base = m.base_layer if kind == "peft" else m
    ptr = base.weight.data_ptr()
    m.merge()
    assert base.weight.data_ptr() == ptr and torch.allclose(m(x), y, atol=1e-5)
    m.unmerge()
    assert torch.allclose(m(x), y, atol=1e-5)
