"""Stand-in LoRA layers for the tests (neither PEFT nor Diffusers is installed here or on the GPU box), written from the
documented forward semantics:

* PEFT's LoRA ``Linear`` (what ``pipe.load_lora_weights`` installs with the PEFT backend):
  ``base(x) + sum over active adapters of lora_B(lora_A(dropout(x))) * scaling``; ``merge()`` / ``unmerge()`` add / subtract
  the delta into the base weight through ``.data`` (no version bump), as PEFT does;
* Diffusers' legacy ``LoRACompatibleLinear`` + ``LoRALinearLayer``: ``base(x) + scale * up(down(x)) * alpha / rank``.

`wrap_lora` wraps the eight projections of every block (attn1 / attn2 to_q, to_k, to_v, to_out.0, ff.net.0.proj,
ff.net.2); the random adapters are sized so that ||s B A||_F is a set fraction (default 0.3) of ||W||_F.  `folded_twin` is
the plain model whose Linears hold vtm_lora_fold's outputs.  `SDPAAttention` is a computing Attention (the block stand-ins'
own forward raises) for module-path comparisons.
"""
import copy

import torch
import torch.nn.functional as F

PROJECTIONS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v",
               "attn2.to_out.0", "ff.net.0.proj", "ff.net.2")


class PeftLinear(torch.nn.Module):
    """PEFT's lora.Linear (peft/tuners/lora/layer.py), the parts its forward and merge use."""

    def __init__(self, base: torch.nn.Linear):
        super().__init__()
        self.base_layer = base
        self.in_features, self.out_features = base.in_features, base.out_features
        self.lora_A = torch.nn.ModuleDict()
        self.lora_B = torch.nn.ModuleDict()
        self.lora_dropout = torch.nn.ModuleDict()
        self.scaling = {}
        self.use_dora = {}
        self.fan_in_fan_out = False
        self.merged_adapters = []
        self._active_adapter = []
        self._disable_adapters = False

    def update_layer(self, name, A: torch.Tensor, B: torch.Tensor, scaling: float, dropout: float = 0.0,
                     b_bias: torch.Tensor = None):
        r = A.shape[0]
        a = torch.nn.Linear(self.in_features, r, bias=False, device=A.device, dtype=A.dtype)
        b = torch.nn.Linear(r, self.out_features, bias=b_bias is not None, device=B.device, dtype=B.dtype)
        with torch.no_grad():
            a.weight.copy_(A)
            b.weight.copy_(B)
            if b_bias is not None:
                b.bias.copy_(b_bias)
        self.lora_A[name], self.lora_B[name] = a, b
        self.lora_dropout[name] = torch.nn.Dropout(dropout) if dropout > 0 else torch.nn.Identity()
        self.scaling[name] = scaling
        self.use_dora[name] = False
        self._active_adapter.append(name)

    @property
    def weight(self):
        return self.base_layer.weight           # PEFT: the BASE weight

    @property
    def bias(self):
        return self.base_layer.bias

    @property
    def active_adapters(self):
        return list(self._active_adapter)

    def set_adapter(self, names):
        self._active_adapter = [names] if isinstance(names, str) else list(names)

    @property
    def merged(self):
        return bool(self.merged_adapters)

    @property
    def disable_adapters(self):
        return self._disable_adapters

    def enable_adapters(self, enabled: bool):
        self._disable_adapters = not enabled

    def get_delta_weight(self, name):
        w = self.lora_B[name].weight.float() @ self.lora_A[name].weight.float() * self.scaling[name]
        return w.to(self.base_layer.weight.dtype)

    def merge(self):
        for name in self.active_adapters:
            if name in self.lora_A and name not in self.merged_adapters:
                self.base_layer.weight.data += self.get_delta_weight(name)
                if self.lora_B[name].bias is not None:
                    self.base_layer.bias.data += self.lora_B[name].bias.data * self.scaling[name]
                self.merged_adapters.append(name)

    def unmerge(self):
        while self.merged_adapters:
            name = self.merged_adapters.pop()
            self.base_layer.weight.data -= self.get_delta_weight(name)
            if self.lora_B[name].bias is not None:
                self.base_layer.bias.data -= self.lora_B[name].bias.data * self.scaling[name]

    def forward(self, x, *args, **kwargs):
        if self.disable_adapters:
            if self.merged:
                self.unmerge()
            return self.base_layer(x)
        if self.merged:
            return self.base_layer(x)
        result = self.base_layer(x)
        for name in self.active_adapters:
            if name not in self.lora_A:
                continue
            A, B = self.lora_A[name], self.lora_B[name]
            result = result + B(A(self.lora_dropout[name](x.to(A.weight.dtype)))) * self.scaling[name]
        return result


class LoRALinearLayer(torch.nn.Module):
    """Diffusers' legacy LoRALinearLayer (models/lora.py)."""

    def __init__(self, in_features, out_features, rank, network_alpha=None, device=None, dtype=None):
        super().__init__()
        self.down = torch.nn.Linear(in_features, rank, bias=False, device=device, dtype=dtype)
        self.up = torch.nn.Linear(rank, out_features, bias=False, device=device, dtype=dtype)
        self.network_alpha = network_alpha
        self.rank = rank

    def forward(self, hidden_states):
        orig = hidden_states.dtype
        up = self.up(self.down(hidden_states.to(self.down.weight.dtype)))
        if self.network_alpha is not None:
            up = up * (self.network_alpha / self.rank)
        return up.to(orig)


class LoRACompatibleLinear(torch.nn.Linear):
    """Diffusers' legacy LoRACompatibleLinear (models/lora.py)."""

    def __init__(self, *args, lora_layer=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.lora_layer = lora_layer
        self._merged_layer = None

    def _delta(self, ll):
        s = 1.0 if ll.network_alpha is None else ll.network_alpha / ll.rank
        return (ll.up.weight.float() @ ll.down.weight.float() * s).to(self.weight.dtype)

    def merge(self):
        self.weight.data += self._delta(self.lora_layer)
        self._merged_layer, self.lora_layer = self.lora_layer, None

    def unmerge(self):
        self.weight.data -= self._delta(self._merged_layer)
        self.lora_layer, self._merged_layer = self._merged_layer, None

    def forward(self, hidden_states, scale: float = 1.0):
        out = super().forward(hidden_states)
        if self.lora_layer is None:
            return out
        return out + scale * self.lora_layer(hidden_states)


class SDPAAttention(torch.nn.Module):
    """A computing Diffusers-style Attention (to_q / to_k / to_v / to_out, heads, scale) on torch's SDPA."""

    def __init__(self, src: torch.nn.Module):
        super().__init__()
        self.heads, self.scale = src.heads, src.scale
        self.to_q, self.to_k, self.to_v, self.to_out = src.to_q, src.to_k, src.to_v, src.to_out

    def forward(self, x, encoder_hidden_states=None, attention_mask=None, **kw):
        ctx = x if encoder_hidden_states is None else encoder_hidden_states
        B, N, _ = x.shape
        q, k, v = self.to_q(x), self.to_k(ctx), self.to_v(ctx)
        sh = lambda t: t.view(B, t.shape[1], self.heads, -1).transpose(1, 2)
        o = F.scaled_dot_product_attention(sh(q), sh(k), sh(v), scale=self.scale)
        o = o.transpose(1, 2).reshape(B, N, -1)
        return self.to_out[1](self.to_out[0](o))


def _get(block, path):
    m = block
    for p in path.split("."):
        m = m[int(p)] if p.isdigit() else getattr(m, p, None)
        if m is None:
            return None
    return m


def _set(block, path, new):
    parent, last = path.rsplit(".", 1)
    p = _get(block, parent)
    if last.isdigit():
        p[int(last)] = new
    else:
        setattr(p, last, new)


def _adapter(W: torch.Tensor, r: int, scale: float, ratio: float, g: torch.Generator):
    """(A (r, in), B (out, r)) in W's dtype with ||scale * B A||_F = ratio * ||W||_F."""
    out_f, in_f = W.shape
    A = torch.randn(r, in_f, generator=g) * in_f ** -0.5
    B = torch.randn(out_f, r, generator=g) * r ** -0.5
    B *= ratio * W.detach().float().cpu().norm() / (scale * (B @ A)).norm()
    return A.to(device=W.device, dtype=W.dtype), B.to(device=W.device, dtype=W.dtype)


def wrap_lora(model, kind="peft", ranks=(64,), scalings=None, ratio=0.3, seed=0, b_bias=False, projections=PROJECTIONS):
    """Wrap the projections of every block of `model` (anything with `.blocks`) in LoRA layers.  kind "peft": one adapter
    per entry of `ranks` (names a0, a1, ...; scaling 0.5 unless given; the adapters together reach `ratio`), "legacy": one
    LoRALinearLayer of ranks[0] with network_alpha = rank / 2.  Returns the list of wrapped modules."""
    g = torch.Generator().manual_seed(seed)
    wrapped = []
    for blk in model.blocks:
        for path in projections:
            lin = _get(blk, path)
            if lin is None:
                continue
            W = lin.weight
            if kind == "peft":
                new = PeftLinear(lin)
                for i, r in enumerate(ranks):
                    s = 0.5 if scalings is None else scalings[i]
                    A, B = _adapter(W, r, s, ratio / len(ranks) ** 0.5, g)
                    bb = (torch.randn(W.shape[0], generator=g) * 0.1).to(device=W.device, dtype=W.dtype) if b_bias else None
                    new.update_layer(f"a{i}", A, B, s, b_bias=bb)
            else:
                r = ranks[0]
                new = LoRACompatibleLinear(lin.in_features, lin.out_features, bias=lin.bias is not None, device=W.device,
                                           dtype=W.dtype)
                with torch.no_grad():
                    new.weight.copy_(lin.weight)
                    if lin.bias is not None:
                        new.bias.copy_(lin.bias)
                ll = LoRALinearLayer(lin.in_features, lin.out_features, r, network_alpha=r / 2, device=W.device, dtype=W.dtype)
                A, B = _adapter(W, r, 0.5, ratio, g)
                with torch.no_grad():
                    ll.down.weight.copy_(A)
                    ll.up.weight.copy_(B)
                new.lora_layer = ll
            _set(blk, path, new)
            wrapped.append(new)
    return wrapped


def adapter_terms(m):
    """[(scale, A, B, B's bias)] of the adapters a stand-in LoRA layer's forward adds right now."""
    if isinstance(m, PeftLinear):
        if m.disable_adapters or m.merged:
            return []
        return [(m.scaling[a], m.lora_A[a].weight, m.lora_B[a].weight, m.lora_B[a].bias) for a in m.active_adapters
                if a in m.lora_A]
    if isinstance(m, LoRACompatibleLinear) and m.lora_layer is not None:
        ll = m.lora_layer
        return [(ll.network_alpha / ll.rank, ll.down.weight, ll.up.weight, None)]
    return []


def base_of(m):
    return m.base_layer if isinstance(m, PeftLinear) else m


def kernel_fold(m):
    """(weight, bias) of the effective Linear with the weight from vtm_lora_fold (the twin's Linears)."""
    from vidtome_amd import _lib
    base = base_of(m)
    w, b = base.weight.detach(), None if base.bias is None else base.bias.detach()
    terms = adapter_terms(m)
    if not terms:
        return w.clone(), None if b is None else b.clone()
    up = torch.cat([B.detach().float() * float(s) for s, _, B, _ in terms], dim=1).contiguous()
    down = torch.cat([A.detach().float() for _, A, _, _ in terms], dim=0).contiguous()
    wf = _lib.lora_fold(w.contiguous(), up, down)
    if any(bb is not None for *_, bb in terms):
        acc = torch.zeros(w.shape[0], dtype=torch.float32, device=w.device) if b is None else b.float()
        for s, _, _, bb in terms:
            if bb is not None:
                acc = acc + float(s) * bb.detach().float()
        b = acc.to(w.dtype)
    return wf, b


def host_fold(m):
    """(weight, bias) of the effective Linear in float64 on the host (the oracles' weights)."""
    base = base_of(m)
    w = base.weight.detach().double().cpu()
    b = None if base.bias is None else base.bias.detach().double().cpu()
    for s, A, B, bb in adapter_terms(m):
        w = w + float(s) * (B.detach().double().cpu() @ A.detach().double().cpu())
        if bb is not None:
            b = (torch.zeros(w.shape[0], dtype=torch.float64) if b is None else b) + float(s) * bb.detach().double().cpu()
    return w, b


def folded_twin(model):
    """A deep copy of the UNPATCHED `model` whose LoRA layers are plain Linears holding vtm_lora_fold's outputs."""
    twin = copy.deepcopy(model)
    for blk_t, blk in zip(twin.blocks, model.blocks):
        for path in PROJECTIONS:
            m = _get(blk, path)
            if isinstance(m, (PeftLinear, LoRACompatibleLinear)):
                w, b = kernel_fold(m)
                lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=b is not None, device=w.device, dtype=w.dtype)
                _set(blk_t, path, lin)
    refold_twin(twin, model)
    return twin


def refold_twin(twin, model):
    """Copy the current effective weights of `model`'s LoRA layers (vtm_lora_fold) into the twin's Linears, in place."""
    with torch.no_grad():
        for blk_t, blk in zip(twin.blocks, model.blocks):
            for path in PROJECTIONS:
                m = _get(blk, path)
                if isinstance(m, (PeftLinear, LoRACompatibleLinear)):
                    w, b = kernel_fold(m)
                    lin = _get(blk_t, path)
                    lin.weight.copy_(w)
                    if b is not None:
                        lin.bias.copy_(b)
