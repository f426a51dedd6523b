"""Stand-in DoRA layers for the tests (PEFT is not installed here or on the GPU box), written from PEFT's documented forward
of ``lora.Linear`` with a ``DoraLinearLayer`` (weight-decomposed LoRA, ``use_dora=True``).  It has NOT been checked against
PEFT itself.  For an active DoRA adapter d (scaling s, magnitude m (c_out,)) the layer adds, to its running result
``base_result`` (the base layer's output plus the adapters before d):

    (r - 1) * (base_result - b) + r * s * lora_B(lora_A(x)),    r = m / ||W + s B A||  (row norms, detached)

and ``merge()`` writes ``r (W + s B A)`` into the base weight's ``.data`` (the norm kept for ``unmerge()``), as PEFT does.
``lora_magnitude_vector`` holds either ``DoraLinearLayer`` modules (current PEFT: the vector is their ``.weight``) or bare
Parameters (older PEFT).

`wrap_dora` wraps the projections of every block with one DoRA adapter (magnitudes ||W|| per row, perturbed by a few
percent so that r != 1 matters) and optionally a trailing plain adapter; `host_fold_dora` is the float64 effective Linear
(the oracles' weights), `kernel_fold_any` the one vtm_dora_fold / vtm_lora_fold make (the folded twins' weights).
"""
import copy

import torch

from lora_standin import PROJECTIONS, PeftLinear, _adapter, _get, _set, host_fold, kernel_fold


class DoraLinearLayer(torch.nn.Module):
    """PEFT's DoraLinearLayer: the magnitude vector as ``.weight``."""

    def __init__(self, magnitude: torch.Tensor):
        super().__init__()
        self.fan_in_fan_out = False
        self.weight = torch.nn.Parameter(magnitude.clone(), requires_grad=False)


def weight_norm(weight: torch.Tensor, lora_weight: torch.Tensor, scaling: float) -> torch.Tensor:
    """PEFT's DoraLinearLayer.get_weight_norm: row norms of W + s B A in W's dtype."""
    return torch.linalg.norm(weight + scaling * lora_weight, dim=1).to(weight.dtype)


class DoraPeftLinear(PeftLinear):
    """PEFT's lora.Linear with DoRA adapters; `container` "module" (DoraLinearLayer) or "param" (bare Parameters)."""

    def __init__(self, base: torch.nn.Linear, container: str = "module"):
        super().__init__(base)
        self.container = container
        self.lora_magnitude_vector = torch.nn.ModuleDict() if container == "module" else torch.nn.ParameterDict()
        self._dora_norms = {}

    def update_layer(self, name, A, B, scaling, dropout=0.0, b_bias=None, magnitude=None):
        super().update_layer(name, A, B, scaling, dropout=dropout, b_bias=b_bias)
        if magnitude is not None:
            self.use_dora[name] = True
            if self.container == "module":
                self.lora_magnitude_vector[name] = DoraLinearLayer(magnitude)
            else:
                self.lora_magnitude_vector[name] = torch.nn.Parameter(magnitude.clone(), requires_grad=False)

    def magnitude(self, name) -> torch.Tensor:
        v = self.lora_magnitude_vector[name]
        return v.weight if self.container == "module" else v

    def _dora_delta(self, name, x, base_result):
        A, B, s = self.lora_A[name], self.lora_B[name], self.scaling[name]
        base = self.base_layer
        x_eye = torch.eye(A.weight.shape[1], device=A.weight.device, dtype=x.dtype)
        lora_weight = B(A(x_eye)).T
        weight = base.weight.to(x.dtype)
        norm = weight_norm(weight, lora_weight.detach(), s).detach()
        r = (self.magnitude(name) / norm).view(1, -1)
        if base.bias is not None:
            base_result = base_result - base.bias
        return (r - 1) * base_result + r * B(A(x)) * s

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
            A, B, drop = self.lora_A[name], self.lora_B[name], self.lora_dropout[name]
            xa = x.to(A.weight.dtype)
            if not self.use_dora[name]:
                result = result + B(A(drop(xa))) * self.scaling[name]
            else:                       # (training-mode dropout would pass base_result=None; not modelled)
                result = result + self._dora_delta(name, xa, result)
        return result

    def merge(self):
        for name in self.active_adapters:
            if name not in self.lora_A or name in self.merged_adapters:
                continue
            if not self.use_dora[name]:
                w = self.base_layer.weight
                w.data += self.get_delta_weight(name)
                if self.lora_B[name].bias is not None:
                    self.base_layer.bias.data += self.lora_B[name].bias.data * self.scaling[name]
            else:
                w = self.base_layer.weight
                delta = self.get_delta_weight(name)
                norm = weight_norm(w.data, delta, 1.0).detach()
                self._dora_norms[name] = norm
                factor = (self.magnitude(name) / norm).view(-1, 1)
                w.data = (factor * (w.data + delta)).to(w.dtype)
            self.merged_adapters.append(name)

    def unmerge(self):
        while self.merged_adapters:
            name = self.merged_adapters.pop()
            w = self.base_layer.weight
            if not self.use_dora[name]:
                w.data -= self.get_delta_weight(name)
                if self.lora_B[name].bias is not None:
                    self.base_layer.bias.data -= self.lora_B[name].bias.data * self.scaling[name]
            else:
                factor = self.magnitude(name) / self._dora_norms.pop(name)
                w.data = (w.data / factor.view(-1, 1) - self.get_delta_weight(name)).to(w.dtype)


def wrap_dora(model, rank=64, trailing=None, container="module", ratio=0.3, jitter=0.05, seed=0, projections=PROJECTIONS):
    """Wrap the projections of every block of `model` in DoraPeftLinear layers: adapter "d0" is DoRA (rank `rank`,
    scaling 0.5, ||s B A||_F = ratio ||W||_F, magnitudes ||W||_row (1 + jitter N(0, 1))); `trailing` = the rank of a
    plain adapter "a1" after it (scaling 0.75), or None.  Returns the list of wrapped modules."""
    g = torch.Generator().manual_seed(seed)
    wrapped = []
    for blk in model.blocks:
        for path in projections:
            lin = _get(blk, path)
            if lin is None:
                continue
            W = lin.weight
            new = DoraPeftLinear(lin, container)
            A, B = _adapter(W, rank, 0.5, ratio, g)
            norm = W.detach().float().cpu().norm(dim=1)
            mag = norm * (1 + jitter * torch.randn(norm.shape, generator=g))
            new.update_layer("d0", A, B, 0.5, magnitude=mag.to(device=W.device, dtype=W.dtype))
            if trailing:
                A, B = _adapter(W, trailing, 0.75, ratio / 2, g)
                new.update_layer("a1", A, B, 0.75)
            _set(blk, path, new)
            wrapped.append(new)
    return wrapped


def _dora_terms(m):
    """(DoRA (scale, A, B, magnitude) or None, [(scale, A, B, B's bias)] of the plain adapters after it) of what the
    forward adds right now."""
    if m.disable_adapters or m.merged:
        return None, []
    names = [a for a in m.active_adapters if a in m.lora_A]
    dora = None
    if names and m.use_dora[names[0]]:
        d = names.pop(0)
        dora = (m.scaling[d], m.lora_A[d].weight, m.lora_B[d].weight, m.magnitude(d))
    assert not any(m.use_dora[a] for a in names), "only a first DoRA adapter is modelled"
    return dora, [(m.scaling[a], m.lora_A[a].weight, m.lora_B[a].weight, m.lora_B[a].bias) for a in names]


def host_fold_dora(m, magnitude=True):
    """(weight, bias) of the effective Linear in float64 on the host; magnitude=False: r = 1 (the magnitudes ignored)."""
    if not isinstance(m, DoraPeftLinear):
        return host_fold(m)
    d64 = lambda t: t.detach().double().cpu()
    w, b = d64(m.base_layer.weight), None if m.base_layer.bias is None else d64(m.base_layer.bias)
    dora, plain = _dora_terms(m)
    if dora is not None:
        s, A, B, mag = dora
        w = w + float(s) * (d64(B) @ d64(A))
        if magnitude:
            w = (d64(mag) / w.norm(dim=1))[:, None] * w
    for s, A, B, bb in plain:
        w = w + float(s) * (d64(B) @ d64(A))
        if bb is not None:
            b = (torch.zeros(w.shape[0], dtype=torch.float64) if b is None else b) + float(s) * d64(bb)
    return w, b


def kernel_fold_any(m):
    """(weight, bias) of the effective Linear with the weight from vtm_dora_fold (a first DoRA adapter) or vtm_lora_fold."""
    from vidtome_amd import _lib
    if not isinstance(m, DoraPeftLinear):
        return kernel_fold(m)
    dora, plain = _dora_terms(m)
    if dora is None:
        return kernel_fold(m)
    w, b = m.base_layer.weight.detach(), m.base_layer.bias
    b = None if b is None else b.detach()
    s, A, B, mag = dora
    terms = [(s, A, B)] + [(sa, Aa, Ba) for sa, Aa, Ba, _ in plain]
    up = torch.cat([Bt.detach().float() * float(st) for st, _, Bt in terms], dim=1).contiguous()
    down = torch.cat([At.detach().float() for _, At, _ in terms], dim=0).contiguous()
    wf = _lib.dora_fold(w.contiguous(), up, down, mag.detach().float().contiguous(), A.shape[0])
    if any(bb is not None for *_, bb in plain):
        acc = torch.zeros(w.shape[0], dtype=torch.float32, device=w.device) if b is None else b.float()
        for sa, _, _, bb in plain:
            if bb is not None:
                acc = acc + float(sa) * bb.detach().float()
        b = acc.to(w.dtype)
    return wf, b


def _is_adapted(m):
    return isinstance(m, PeftLinear) or type(m).__name__ == "LoRACompatibleLinear"


def folded_twin_dora(model):
    """A deep copy of the UNPATCHED `model` whose adapted layers are plain Linears holding the kernels' folds."""
    twin = copy.deepcopy(model)
    for blk_t, blk in zip(twin.blocks, model.blocks):
        for path in PROJECTIONS:
            m = _get(blk, path)
            if m is not None and _is_adapted(m):
                w, b = kernel_fold_any(m)
                lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=b is not None, device=w.device, dtype=w.dtype)
                _set(blk_t, path, lin)
    refold_twin_dora(twin, model)
    return twin


def refold_twin_dora(twin, model):
    """Copy the current effective weights of `model`'s adapted layers (the kernels' folds) into the twin's Linears."""
    with torch.no_grad():
        for blk_t, blk in zip(twin.blocks, model.blocks):
            for path in PROJECTIONS:
                m = _get(blk, path)
                if m is not None and _is_adapted(m):
                    w, b = kernel_fold_any(m)
                    lin = _get(blk_t, path)
                    lin.weight.copy_(w)
                    if b is not None:
                        lin.bias.copy_(b)
