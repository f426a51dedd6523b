"""Stand-in LyCORIS layers for the tests (PEFT is not installed here or on the GPU box), written from the documented
forward of PEFT's LyCORIS ``Linear`` layers (``LoHaConfig`` / ``LoKrConfig``).  They have NOT been checked against PEFT
itself.  The layer computes the base layer's output plus, per active adapter a, ``F.linear(x, get_delta_weight(a))`` with
the delta built in the factors' dtype:

    LoHa:  delta = ((hada_w1_a @ hada_w1_b) * (hada_w2_a @ hada_w2_b)) * scaling        (* elementwise)
    LoKr:  delta = kron(w1, w2) * scaling,   w1 = lokr_w1 or lokr_w1_a @ lokr_w1_b,  w2 = lokr_w2 or lokr_w2_a @ lokr_w2_b

``merge()`` / ``unmerge()`` add / subtract the delta into the base weight through ``.data`` (no version bump), as PEFT does;
these adapters carry no bias.  ``hada_t1`` / ``hada_t2`` / ``lokr_t2`` (the Tucker forms of conv layers) exist as empty dicts.

`wrap_lycoris` wraps the projections of every block; the random adapters are sized so that ||delta||_F is a set fraction
(default 0.3) of ||W||_F, like `lora_standin._adapter`.  `host_fold_lycoris` is the float64 effective Linear (the oracles'
weights), `kernel_fold_lycoris` the one vtm_loha_delta / vtm_lokr_delta / vtm_delta_fold make (the folded twins' weights).
"""
import copy

import torch
import torch.nn.functional as F

from lora_standin import PROJECTIONS, _get, _set, host_fold, kernel_fold

LOHA_FACTORS = ("hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b")
LOKR_FACTORS = ("lokr_w1", "lokr_w1_a", "lokr_w1_b", "lokr_w2", "lokr_w2_a", "lokr_w2_b")


class LycorisLinear(torch.nn.Module):
    """What PEFT's LoHa / LoKr ``Linear`` share (peft/tuners/lycoris_utils.py), the parts forward and merge use."""

    factor_names = ()

    def __init__(self, base: torch.nn.Linear):
        super().__init__()
        self.base_layer = base
        self.in_features, self.out_features = base.in_features, base.out_features
        for n in self.factor_names:
            setattr(self, n, torch.nn.ParameterDict())
        self.r, self.alpha, self.scaling = {}, {}, {}
        self.rank_dropout, self.module_dropout = {}, {}
        self.merged_adapters = []
        self._active_adapter = []
        self._disable_adapters = False

    def _register(self, name, scaling, **factors):
        for n, t in factors.items():
            getattr(self, n)[name] = torch.nn.Parameter(t.detach().clone(), requires_grad=False)
        self.scaling[name] = scaling
        self.rank_dropout[name], self.module_dropout[name] = 0.0, 0.0
        self._active_adapter.append(name)

    def _has(self, name) -> bool:
        return any(name in getattr(self, n) for n in self.factor_names)

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

    def get_delta_weight(self, name) -> torch.Tensor:
        raise NotImplementedError

    def merge(self):
        for name in self.active_adapters:
            if self._has(name) and name not in self.merged_adapters:
                w = self.base_layer.weight
                w.data += self.get_delta_weight(name).to(w.dtype)
                self.merged_adapters.append(name)

    def unmerge(self):
        while self.merged_adapters:
            name = self.merged_adapters.pop()
            w = self.base_layer.weight
            w.data -= self.get_delta_weight(name).to(w.dtype)

    def forward(self, x, *args, **kwargs):
        if self.disable_adapters:
            if self.merged:
                self.unmerge()
            return self.base_layer(x)
        if self.merged:
            return self.base_layer(x)
        result = self.base_layer(x)
        for name in self.active_adapters:
            if not self._has(name):
                continue
            delta = self.get_delta_weight(name)
            result = result + F.linear(x.to(delta.dtype), delta)
        return result


class LoHaLinear(LycorisLinear):
    """PEFT's loha.Linear: delta = ((w1a @ w1b) * (w2a @ w2b)) * scaling."""

    factor_names = LOHA_FACTORS + ("hada_t1", "hada_t2")

    def update_layer(self, name, w1a, w1b, w2a, w2b, scaling):
        self._register(name, scaling, hada_w1_a=w1a, hada_w1_b=w1b, hada_w2_a=w2a, hada_w2_b=w2b)

    def get_delta_weight(self, name):
        w = (self.hada_w1_a[name] @ self.hada_w1_b[name]) * (self.hada_w2_a[name] @ self.hada_w2_b[name])
        return w * self.scaling[name]


class LoKrLinear(LycorisLinear):
    """PEFT's lokr.Linear: delta = kron(w1, w2) * scaling, either factor full or a low-rank pair."""

    factor_names = LOKR_FACTORS + ("lokr_t2",)

    def update_layer(self, name, w1, w2, scaling):
        """w1 / w2: a tensor (the full factor) or a pair of tensors (its low-rank form)."""
        fs = {}
        for key, f in (("lokr_w1", w1), ("lokr_w2", w2)):
            if isinstance(f, torch.Tensor):
                fs[key] = f
            else:
                fs[key + "_a"], fs[key + "_b"] = f
        self._register(name, scaling, **fs)

    def factor(self, which, name) -> torch.Tensor:
        full = getattr(self, f"lokr_{which}")
        if name in full:
            return full[name]
        return getattr(self, f"lokr_{which}_a")[name] @ getattr(self, f"lokr_{which}_b")[name]

    def get_delta_weight(self, name):
        return torch.kron(self.factor("w1", name), self.factor("w2", name).contiguous()) * self.scaling[name]


def kron_split(n: int):
    """(small, large) with small * large = n and small the largest divisor <= sqrt(n) (PEFT's default factorisation)."""
    s = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return s, n // s


def _randn(g, rows, cols, std):
    return torch.randn(rows, cols, generator=g) * std


def loha_adapter(W: torch.Tensor, r: int, scale: float, ratio: float, g: torch.Generator):
    """(w1a, w1b, w2a, w2b) in W's dtype with ||scale (w1a w1b) * (w2a w2b)||_F = ratio ||W||_F, the two products of
    like size."""
    co, ci = W.shape
    w1a, w1b, w2a, w2b = _randn(g, co, r, r ** -0.5), _randn(g, r, ci, 1.0), _randn(g, co, r, r ** -0.5), _randn(g, r, ci, 1.0)
    f = ratio * W.detach().float().cpu().norm() / (scale * (w1a @ w1b) * (w2a @ w2b)).norm()
    w1a, w2a = w1a * f ** 0.5, w2a * f ** 0.5
    return tuple(t.to(device=W.device, dtype=W.dtype) for t in (w1a, w1b, w2a, w2b))


def lokr_adapter(W: torch.Tensor, forms, r: int, scale: float, ratio: float, g: torch.Generator):
    """(w1, w2) in W's dtype, each a full factor ("full") or a low-rank pair ("lowrank", rank r) as `forms` says, with
    ||scale kron(w1, w2)||_F = ratio ||W||_F; w1 is (a1, b1), w2 (a2, b2) from the near-square splits of W's sides."""
    (a1, a2), (b1, b2) = kron_split(W.shape[0]), kron_split(W.shape[1])
    fs, full = [], []
    for form, (rows, cols) in zip(forms, ((a1, b1), (a2, b2))):
        if form == "full":
            fs.append([_randn(g, rows, cols, 1.0)])
        else:
            fs.append([_randn(g, rows, r, r ** -0.5), _randn(g, r, cols, 1.0)])
        full.append(fs[-1][0] if form == "full" else fs[-1][0] @ fs[-1][1])
    f = ratio * W.detach().float().cpu().norm() / (scale * torch.kron(full[0], full[1])).norm()
    for p in fs:
        p[0] = p[0] * f ** 0.5
    to = lambda t: t.to(device=W.device, dtype=W.dtype)
    return tuple(to(p[0]) if len(p) == 1 else (to(p[0]), to(p[1])) for p in fs)


def wrap_lycoris(model, kind, rank=64, n_adapters=1, forms=("full", "full"), scaling=0.5, ratio=0.3, seed=0,
                 projections=PROJECTIONS):
    """Wrap the projections of every block of `model` (anything with `.blocks`) in LoHaLinear (kind "loha": rank `rank`) or
    LoKrLinear (kind "lokr": factors as `forms` says, low-rank ones of rank `rank`) layers with `n_adapters` adapters a0, a1,
    ... of scaling `scaling`, together reaching ||delta||_F = ratio ||W||_F.  Returns the list of wrapped modules."""
    g = torch.Generator().manual_seed(seed)
    wrapped = []
    for blk in model.blocks:
        for path in projections:
            lin = _get(blk, path)
            if lin is None:
                continue
            W = lin.weight
            new = LoHaLinear(lin) if kind == "loha" else LoKrLinear(lin)
            for i in range(n_adapters):
                each = ratio / n_adapters ** 0.5
                if kind == "loha":
                    new.update_layer(f"a{i}", *loha_adapter(W, rank, scaling, each, g), scaling)
                else:
                    new.update_layer(f"a{i}", *lokr_adapter(W, forms, rank, scaling, each, g), scaling)
            _set(blk, path, new)
            wrapped.append(new)
    return wrapped


def lycoris_terms(m):
    """[(scale, factors)] of the adapters a stand-in layer's forward adds right now: LoHa factors (w1a, w1b, w2a, w2b),
    LoKr factors ((w1,) or (w1_a, w1_b), (w2,) or (w2_a, w2_b))."""
    if m.disable_adapters or m.merged:
        return []
    out = []
    for a in m.active_adapters:
        if not m._has(a):
            continue
        if isinstance(m, LoHaLinear):
            out.append((m.scaling[a], tuple(getattr(m, n)[a] for n in LOHA_FACTORS)))
        else:
            pick = lambda w: (getattr(m, w)[a],) if a in getattr(m, w) else (getattr(m, w + "_a")[a], getattr(m, w + "_b")[a])
            out.append((m.scaling[a], (pick("lokr_w1"), pick("lokr_w2"))))
    return out


def host_fold_lycoris(m, adapters=True):
    """(weight, bias) of the effective Linear in float64 on the host; adapters=False: the base layer alone."""
    if not isinstance(m, LycorisLinear):
        return host_fold(m)
    d64 = lambda t: t.detach().double().cpu()
    w, b = d64(m.base_layer.weight), None if m.base_layer.bias is None else d64(m.base_layer.bias)
    for s, fs in (lycoris_terms(m) if adapters else []):
        if isinstance(m, LoHaLinear):
            w1a, w1b, w2a, w2b = map(d64, fs)
            w = w + float(s) * ((w1a @ w1b) * (w2a @ w2b))
        else:
            full = [d64(f[0]) if len(f) == 1 else d64(f[0]) @ d64(f[1]) for f in fs]
            w = w + float(s) * torch.kron(full[0], full[1])
    return w, b


def kernel_fold_lycoris(m):
    """(weight, bias) of the effective Linear with the weight from the fold kernels: the adapters' fp32 deltas (the scale
    multiplied into the first factor in fp32) summed in order by vtm_loha_delta / vtm_lokr_delta, vtm_delta_fold on top."""
    from vidtome_amd import _lib
    if not isinstance(m, LycorisLinear):
        return kernel_fold(m)
    w, b = m.base_layer.weight.detach(), m.base_layer.bias
    b = None if b is None else b.detach().clone()
    terms = lycoris_terms(m)
    if not terms:
        return w.clone(), b
    f32 = lambda t: t.detach().to(device=w.device, dtype=torch.float32).contiguous()

    def full(f, s=None):
        first = f32(f[0]) if s is None else (f32(f[0]) * float(s)).contiguous()
        if len(f) == 1:
            return first
        second = f32(f[1])
        return _lib.lora_fold(torch.zeros(first.shape[0], second.shape[1], device=w.device), first, second)

    delta = None
    for s, fs in terms:
        if isinstance(m, LoHaLinear):
            delta = _lib.loha_delta((f32(fs[0]) * float(s)).contiguous(), f32(fs[1]), f32(fs[2]), f32(fs[3]), out=delta,
                                    accumulate=delta is not None)
        else:
            delta = _lib.lokr_delta(full(fs[0], s), full(fs[1]), out=delta, accumulate=delta is not None)
    return _lib.delta_fold(w.contiguous(), delta), b


def _is_adapted(m):
    return isinstance(m, LycorisLinear)


def folded_twin_lycoris(model):
    """A deep copy of the UNPATCHED `model` whose LyCORIS layers are plain Linears holding the kernels' folds."""
    twin = copy.deepcopy(model)
    for blk_t, blk in zip(twin.blocks, model.blocks):
        for path in PROJECTIONS:
            m = _get(blk, path)
            if m is not None and _is_adapted(m):
                w, b = m.base_layer.weight, m.base_layer.bias
                lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=b is not None, device=w.device, dtype=w.dtype)
                _set(blk_t, path, lin)
    refold_twin_lycoris(twin, model)
    return twin


def refold_twin_lycoris(twin, model):
    """Copy the current effective weights of `model`'s LyCORIS layers (the kernels' folds) into the twin's Linears."""
    with torch.no_grad():
        for blk_t, blk in zip(twin.blocks, model.blocks):
            for path in PROJECTIONS:
                m = _get(blk, path)
                if m is not None and _is_adapted(m):
                    w, b = kernel_fold_lycoris(m)
                    lin = _get(blk_t, path)
                    lin.weight.copy_(w)
                    if b is not None:
                        lin.bias.copy_(b)
