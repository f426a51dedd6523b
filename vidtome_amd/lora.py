"""The effective weight of a block projection: plain Linear, or LoRA-adapted and folded.

The reference loads LoRA adapters as a documented option (`use_lora` / `lora:`, configs/default.yaml:63-69 ->
`pipe.load_lora_weights(**gene_config.lora)`, generate.py:93-94).  With the PEFT backend Diffusers then wraps every
projection of a BasicTransformerBlock -- attn1 / attn2 to_q / to_k / to_v / to_out.0, ff.net.0.proj, ff.net.2 -- in a
LoRA layer whose forward is ``base(x) + sum_a lora_B_a(lora_A_a(dropout(x))) * scaling_a``.  For inference that is the
Linear ``W_eff = W + sum_a s_a B_a A_a`` (bias + s_a b_B_a), folded once per adapter state by vtm_lora_fold and fed to the
projection kernels that exist: the per-step cost is zero.

`linear_params` is the ONE place the patched block reads a projection's weight and bias from.  A LoRA wrapper's
``.weight`` is the BASE weight, and PEFT's ``merge()`` adds the adapter into it through ``.data`` (no version bump), so
the folded tensors are keyed by a state token that covers the base and adapter tensors (pointer + version), every
active adapter's exact scaling, ``merged`` / ``merged_adapters`` and ``disable_adapters``.  Downstream caches (stacked
q | k weights, panel packs) key on the token too, so a scaling change, an adapter switch, disable, merge and unmerge
all rebuild them, and a merged adapter is never counted twice.

Two structures are recognised by duck typing (neither PEFT nor Diffusers is a dependency):
* PEFT's LoRA ``Linear``: ``base_layer`` (a plain Linear), ``lora_A`` / ``lora_B`` (ModuleDicts of Linear), ``scaling``,
  ``active_adapters``, ``merged``, ``disable_adapters``, ``use_dora``, ``lora_dropout``;
* Diffusers' legacy ``LoRACompatibleLinear`` with a ``lora_layer`` that has ``down``, ``up``, ``network_alpha`` and
  ``rank`` (its forward adds ``scale * up(down(x)) * network_alpha / rank``, the forward's ``scale`` being 1.0 here).
DoRA (PEFT ``use_dora=True``, weight-decomposed LoRA) is recognised in its one unambiguous form: exactly one active DoRA
adapter ``d``, FIRST in PEFT's order, with a magnitude vector ``m`` of shape (c_out,) in ``lora_magnitude_vector[d]`` (a
tensor, or a module whose ``.weight`` it is) and no ``lora_B`` bias.  PEFT then computes
``base + (r - 1) (base - b) + r s_d x (B_d A_d)^T`` with ``r = m / ||W + s_d B_d A_d||`` per output row and the running
result ``base``, so the layer is the Linear ``diag(r) (W + s_d B_d A_d) + sum_{plain a after d} s_a B_a A_a`` (bias
``b + sum_a s_a b_B_a``), folded by vtm_dora_norms + vtm_dora_fold (a zero norm divides as IEEE does, like PEFT).  A merged
DoRA adapter is already in the base weight (PEFT's ``merge()`` writes ``r (W + s_d B_d A_d)`` into ``.data``) and is read like
any merged adapter.  The state token adds the magnitude's (pointer, version).  The extra memory is the LoRA fold's: one
folded copy per adapted projection.

LyCORIS layers (PEFT's ``LoHaConfig`` / ``LoKrConfig``, the same ten projections) are recognised as two more kinds, LOHA
and LOKR: a ``base_layer`` (a plain Linear), ``active_adapters``, ``merged``, ``merged_adapters``, ``disable_adapters``, a
``scaling`` dict and the factor ParameterDicts -- ``hada_w1_a`` (c_out, r), ``hada_w1_b`` (r, c_in), ``hada_w2_a``,
``hada_w2_b`` for LoHa; ``lokr_w1`` (a1, b1) or the pair ``lokr_w1_a`` / ``lokr_w1_b``, and ``lokr_w2`` (a2, b2) or the pair
``lokr_w2_a`` / ``lokr_w2_b`` with a1 a2 = c_out, b1 b2 = c_in for LoKr.  Their forward adds ``F.linear(x, delta_a)`` per active
adapter, ``delta_a = s_a (W1a W1b) * (W2a W2b)`` (elementwise) or ``s_a kron(W1, W2)``, so the layer is the Linear
``W + sum_a delta_a`` with the base bias (these adapters carry none): vtm_loha_delta / vtm_lokr_delta sum the deltas in
fp32 in PEFT's adapter order and vtm_delta_fold adds them to the base weight and rounds once (the fp32 delta is a
temporary of the fold; what stays is one folded copy, as for LoRA).  The token covers every factor tensor's (pointer,
version).  Not recognised: Tucker / conv forms (an active adapter with a ``hada_t1`` / ``hada_t2`` / ``lokr_t2`` entry),
``rank_dropout`` / ``module_dropout`` > 0 in training mode, merged and disabled at once, a layer that also has ``lora_A``
(or both families' factors), and any shape mismatch.

Anything else -- DoRA after another adapter or on more than one adapter (which running result PEFT scales there has
changed between releases), DoRA without a magnitude vector or with a ``lora_B`` bias, ``fan_in_fan_out``, dropout with
p > 0 in training mode, adapters that are not Linears, other wrappers -- is not recognised and the patched block keeps the
module's own forward.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib

PLAIN, PEFT, LEGACY = "plain", "peft", "legacy"
LOHA, LOKR = "loha", "lokr"
_WRAPPED = (PEFT, LOHA, LOKR)           # the kinds whose base weight lives in ``base_layer``
_LOHA_DICTS = ("hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b")
_LOKR_DICTS = ("lokr_w1", "lokr_w1_a", "lokr_w1_b", "lokr_w2", "lokr_w2_a", "lokr_w2_b")


def _plain(m) -> bool:
    """A Linear whose forward is `x W^T + b` (Diffusers' LoRA-compatible subclass with no LoRA attached included)."""
    return (isinstance(m, torch.nn.Linear) and type(m).__name__ in ("Linear", "LoRACompatibleLinear")
            and getattr(m, "lora_layer", None) is None)


def _adapter_linear(m, in_features: int, out_features: int, bias_ok: bool) -> bool:
    return (type(m) is torch.nn.Linear and m.in_features == in_features and m.out_features == out_features
            and (bias_ok or m.bias is None))


def _flag(v, name: str) -> bool:
    """PEFT keeps some switches per adapter (dict) and some as one bool."""
    return bool(v.get(name, False)) if isinstance(v, dict) else bool(v)


def _active(m):
    """PEFT: the active adapters that have weights on this layer, in PEFT's order."""
    names = m.active_adapters
    names = [names] if isinstance(names, str) else list(names)
    return [a for a in names if a in m.lora_A]


def _magnitude(m, a: str) -> Optional[torch.Tensor]:
    """PEFT: DoRA adapter `a`'s magnitude vector (c_out,) -- a tensor / Parameter (older PEFT) or the ``.weight`` of a
    DoraLinearLayer -- or None when it is missing or not of that form."""
    mv = getattr(m, "lora_magnitude_vector", None)
    try:
        v = mv[a] if mv is not None and a in mv else None
    except TypeError:
        return None
    if v is not None and not isinstance(v, torch.Tensor):
        if getattr(v, "fan_in_fan_out", False):
            return None
        v = getattr(v, "weight", None)
    if not isinstance(v, torch.Tensor) or not v.is_floating_point() or tuple(v.shape) != (m.base_layer.out_features,):
        return None
    return v


def _dora_ok(m, active) -> bool:
    """The DoRA adapters among `active` (if any) are one adapter, first, with a magnitude vector and no lora_B bias."""
    dora = [a for a in active if _flag(m.use_dora, a)]
    if not dora:
        return True
    d = dora[0]
    return len(dora) == 1 and d == active[0] and _magnitude(m, d) is not None and m.lora_B[d].bias is None


def _peft_ok(m) -> bool:
    if not all(hasattr(m, a) for a in ("base_layer", "lora_A", "lora_B", "scaling", "active_adapters", "merged",
                                       "disable_adapters", "use_dora", "lora_dropout")):
        return False
    base = m.base_layer
    if not _plain(base) or getattr(m, "fan_in_fan_out", False):
        return False
    if not isinstance(m.lora_A, torch.nn.ModuleDict) or not isinstance(m.lora_B, torch.nn.ModuleDict):
        return False
    for a, A in m.lora_A.items():
        B = m.lora_B[a] if a in m.lora_B else None
        if type(A) is not torch.nn.Linear or A.in_features != base.in_features or A.bias is not None:
            return False
        if B is None or not _adapter_linear(B, A.out_features, base.out_features, bias_ok=True):
            return False
    if m.disable_adapters and m.merged:
        return False            # PEFT's forward unmerges first (a side effect the module path performs)
    active = _active(m)
    if not m.merged and not _dora_ok(m, active):
        return False            # a merged DoRA adapter is in the base weight: PEFT's forward is then the base layer
    for a in active:
        if a not in m.scaling:
            return False
        d = m.lora_dropout[a] if a in m.lora_dropout else torch.nn.Identity()
        if type(d) is torch.nn.Identity:
            continue
        if not isinstance(d, torch.nn.Dropout) or (d.training and d.p > 0):
            return False
    return True


def _legacy_ok(m) -> bool:
    ll = m.lora_layer
    if not all(hasattr(ll, a) for a in ("down", "up", "network_alpha", "rank")):
        return False
    down, up = ll.down, ll.up
    return (type(down) is torch.nn.Linear and down.in_features == m.in_features and down.bias is None
            and _adapter_linear(up, down.out_features, m.out_features, bias_ok=True))


def _entry(m, dict_name: str, a: str):
    """LyCORIS: adapter `a`'s entry in the ParameterDict `dict_name` of the layer, or None."""
    d = getattr(m, dict_name, None)
    try:
        return d[a] if d is not None and a in d else None
    except TypeError:
        return None


def _lyco_kind(m) -> Optional[str]:
    """LOHA / LOKR by the factor dicts the layer carries, "" for a layer that carries both families', None for neither."""
    loha = any(hasattr(m, n) for n in _LOHA_DICTS)
    lokr = any(hasattr(m, n) for n in _LOKR_DICTS)
    return "" if loha and lokr else LOHA if loha else LOKR if lokr else None


def _lyco_active(m, kind: str):
    """LyCORIS: the active adapters that have weights on this layer, in PEFT's order."""
    names = m.active_adapters
    names = [names] if isinstance(names, str) else list(names)
    has = (lambda a: _entry(m, "hada_w1_a", a) is not None) if kind == LOHA else \
        (lambda a: _entry(m, "lokr_w1", a) is not None or _entry(m, "lokr_w1_a", a) is not None)
    return [a for a in names if has(a)]


def _matrix(t, rows: Optional[int] = None, cols: Optional[int] = None) -> bool:
    return (isinstance(t, torch.Tensor) and t.is_floating_point() and t.dim() == 2 and min(t.shape) > 0
            and rows in (None, t.shape[0]) and cols in (None, t.shape[1]))


def _lokr_factor(m, which: str, a: str):
    """LoKr: adapter `a`'s factor "w1" / "w2" as (W,) or the low-rank pair (Wa (rows, r), Wb (r, cols)), or None."""
    full, lo_a, lo_b = (_entry(m, f"lokr_{which}{sfx}", a) for sfx in ("", "_a", "_b"))
    if full is not None:
        return (full,) if lo_a is None and lo_b is None and _matrix(full) else None
    if not (_matrix(lo_a) and _matrix(lo_b, rows=lo_a.shape[1])):
        return None
    return (lo_a, lo_b)


def _lyco_factors(m, kind: str, a: str):
    """Adapter `a`'s factor tensors when they multiply out to the base weight's shape, else None: LoHa (w1a, w1b, w2a, w2b)
    with one rank; LoKr (factor w1, factor w2), each as `_lokr_factor` gives it."""
    c_out, c_in = m.base_layer.out_features, m.base_layer.in_features
    if kind == LOHA:
        w1a, w1b, w2a, w2b = (_entry(m, n, a) for n in _LOHA_DICTS)
        if not (_matrix(w1a, rows=c_out) and _matrix(w1b, rows=w1a.shape[1], cols=c_in)
                and _matrix(w2a, rows=c_out, cols=w1a.shape[1]) and _matrix(w2b, rows=w1a.shape[1], cols=c_in)):
            return None
        return (w1a, w1b, w2a, w2b)
    f1, f2 = _lokr_factor(m, "w1", a), _lokr_factor(m, "w2", a)
    if f1 is None or f2 is None:
        return None
    if f1[0].shape[0] * f2[0].shape[0] != c_out or f1[-1].shape[1] * f2[-1].shape[1] != c_in:
        return None
    return (f1, f2)


def _lyco_ok(m, kind: str) -> bool:
    if not all(hasattr(m, a) for a in ("base_layer", "active_adapters", "merged", "merged_adapters", "disable_adapters",
                                       "scaling")):
        return False
    if not _plain(m.base_layer) or not isinstance(m.scaling, dict):
        return False
    if m.disable_adapters and m.merged:
        return False            # PEFT's forward unmerges first (a side effect the module path performs)
    for a in _lyco_active(m, kind):
        if any(_entry(m, t, a) is not None for t in ("hada_t1", "hada_t2", "lokr_t2")):
            return False        # Tucker / conv forms
        if a not in m.scaling or _lyco_factors(m, kind, a) is None:
            return False
        for drop in ("rank_dropout", "module_dropout"):
            p = getattr(m, drop, 0.0)
            p = p.get(a, 0.0) if isinstance(p, dict) else p
            if m.training and float(p or 0.0) > 0:
                return False
    return True


def recognise(m) -> Optional[str]:
    """PLAIN / PEFT / LEGACY / LOHA / LOKR, or None when the fused path must not read this projection (the module path
    keeps running)."""
    if not isinstance(m, torch.nn.Linear) and hasattr(m, "base_layer"):
        kind = _lyco_kind(m)
        if kind is not None:
            return kind if kind and not hasattr(m, "lora_A") and _lyco_ok(m, kind) else None
    if isinstance(m, torch.nn.Linear):
        name = type(m).__name__
        if name not in ("Linear", "LoRACompatibleLinear"):
            return None
        if getattr(m, "lora_layer", None) is None:
            return PLAIN
        return LEGACY if name == "LoRACompatibleLinear" and _legacy_ok(m) else None
    if hasattr(m, "base_layer") and hasattr(m, "lora_A"):
        return PEFT if _peft_ok(m) else None
    return None


def base_linear(m) -> torch.nn.Linear:
    """The Linear holding the base weight (shapes, dtype and device of the effective weight) of a recognised projection."""
    return m.base_layer if recognise(m) in _WRAPPED else m


def _tkey(t: Optional[torch.Tensor]):
    return None if t is None else (t.data_ptr(), t._version)


def _param_key(w: torch.Tensor, b: Optional[torch.Tensor]):
    return (w.data_ptr(), w._version, w.dtype, w.device) + ((None,) if b is None else (b.data_ptr(), b._version, b.dtype))


def _adapters(m, kind: str):
    """[(name, scale, A (r, c_in), B (c_out, r), B's bias or None, DoRA magnitude or None)] of the adapters the forward
    adds; a DoRA adapter is always the first (recognise)."""
    if kind == LEGACY:
        ll = m.lora_layer
        s = 1.0 if ll.network_alpha is None else float(ll.network_alpha) / float(ll.rank)
        return [("lora_layer", s, ll.down.weight, ll.up.weight, ll.up.bias, None)]
    if m.disable_adapters or m.merged:
        return []
    return [(a, m.scaling[a], m.lora_A[a].weight, m.lora_B[a].weight, m.lora_B[a].bias,
             _magnitude(m, a) if _flag(m.use_dora, a) else None) for a in _active(m)]


def _lyco_terms(m, kind: str):
    """[(name, scale, factor tensors as `_lyco_factors` gives them)] of the LyCORIS adapters the forward adds."""
    if m.disable_adapters or m.merged:
        return []
    return [(a, m.scaling[a], _lyco_factors(m, kind, a)) for a in _lyco_active(m, kind)]


def _tkeys(ts) -> tuple:
    return tuple(_tkeys(t) if isinstance(t, tuple) else _tkey(t) for t in ts)


def state_token(m, kind: Optional[str] = None) -> tuple:
    """Everything the effective weight of a LoRA layer depends on that the fold cannot see in the tensors themselves."""
    kind = kind or recognise(m)
    base = m.base_layer if kind in _WRAPPED else m
    tok = (kind, _param_key(base.weight, base.bias))
    if kind in _WRAPPED:
        merged = tuple(getattr(m, "merged_adapters", ()))
        tok += (bool(m.disable_adapters), bool(m.merged), merged)
        if kind != PEFT:
            return tok + tuple((a, float(s), _tkeys(ts)) for a, s, ts in _lyco_terms(m, kind))
    elif kind == LEGACY:
        tok += (m.lora_layer.network_alpha, m.lora_layer.rank)
    return tok + tuple((a, float(s), _tkey(A), _tkey(B), _tkey(bB)) + (() if mag is None else ("dora", _tkey(mag)))
                       for a, s, A, B, bB, mag in _adapters(m, kind))


def _fold_lycoris(m, kind: str, w: torch.Tensor):
    """The folded weight of a LoHa / LoKr layer, or None when its forward adds no adapter right now.  The fp32 delta is a
    temporary: the adapters' deltas summed in PEFT's order, added to fp32(w) and rounded once."""
    terms = _lyco_terms(m, kind)
    if not terms:
        return None
    f32 = lambda t: t.detach().to(device=w.device, dtype=torch.float32).contiguous()

    def factor(f, s=None):      # a LoKr factor as one fp32 matrix; a low-rank pair is multiplied out by vtm_lora_fold from zero
        first = f32(f[0]) if s is None else (f32(f[0]) * float(s)).contiguous()
        if len(f) == 1:
            return first
        second = f32(f[1])
        zero = torch.zeros((first.shape[0], second.shape[1]), dtype=torch.float32, device=w.device)
        return _lib.lora_fold(zero, first, second)

    with torch.no_grad():
        delta = None
        for _, s, ts in terms:
            if kind == LOHA:
                delta = _lib.loha_delta((f32(ts[0]) * float(s)).contiguous(), f32(ts[1]), f32(ts[2]), f32(ts[3]), out=delta,
                                        accumulate=delta is not None)
            else:
                delta = _lib.lokr_delta(factor(ts[0], s), factor(ts[1]), out=delta, accumulate=delta is not None)
        return _lib.delta_fold(w.contiguous(), delta)


def _fold(m, kind: str):
    """(weight, bias, folded?) of the adapted layer, in the base weight's dtype on its device."""
    base = m.base_layer if kind in _WRAPPED else m
    w, b = base.weight.detach(), None if base.bias is None else base.bias.detach()
    if kind in (LOHA, LOKR):
        wf = _fold_lycoris(m, kind, w)
        return (w, b, False) if wf is None else (wf, b, True)
    ads = _adapters(m, kind)
    if not ads:
        return w, b, False
    with torch.no_grad():
        up = torch.cat([B.detach().float() * float(s) for _, s, _, B, _, _ in ads], dim=1).contiguous()
        down = torch.cat([A.detach().float() for _, _, A, _, _, _ in ads], dim=0).contiguous()
        mag = ads[0][5]
        if mag is None:
            wf = _lib.lora_fold(w.contiguous(), up.to(w.device), down.to(w.device))
        else:                   # DoRA first: its rank is the first k columns of up / rows of down
            wf = _lib.dora_fold(w.contiguous(), up.to(w.device), down.to(w.device),
                                mag.detach().float().to(w.device).contiguous(), ads[0][2].shape[0])
        if any(bB is not None for *_, bB, _ in ads):
            acc = torch.zeros(w.shape[0], dtype=torch.float32, device=w.device) if b is None else b.float()
            for _, s, _, _, bB, _ in ads:
                if bB is not None:
                    acc = acc + float(s) * bB.detach().float()
            b = acc.to(w.dtype)
    return wf, b, True


def linear_params(m, dtype: Optional[torch.dtype] = None, device=None
                  ) -> Optional[Tuple[torch.Tensor, Optional[torch.Tensor], tuple]]:
    """(weight, bias, key) of the Linear the projection computes, or None when `m` is neither a plain Linear nor a
    recognised LoRA / LyCORIS layer.  A plain Linear gives its own tensors, key = their (pointer, version, dtype, device).  A LoRA
    layer gives the folded weight / bias (one copy of the projection weight in the model dtype, cached on the module under
    its state token, which is also the key); a chunk on another HIP stream than the fold's waits for it on the device.
    ``dtype`` / ``device``: the tensors are returned converted (a no-op when they already are; not cached)."""
    kind = recognise(m)
    if kind is None:
        return None
    if kind == PLAIN:
        w, b = m.weight, m.bias
        key = _param_key(w, b)
    else:
        key = state_token(m, kind)
        hit = m.__dict__.get("_vtm_lora")
        if hit is None or hit[0] != key:
            w, b, folded = _fold(m, kind)
            from .patch import _built_here
            hit = (key, w, b, _built_here(w.device) if folded else None)
            m.__dict__["_vtm_lora"] = hit
        else:
            from .patch import _built_before
            _built_before(hit[3], hit[1].device)
        w, b = hit[1], hit[2]
    if (dtype is not None and w.dtype != dtype) or (device is not None and w.device != torch.device(device)):
        w = w.to(device=device, dtype=dtype)
        b = None if b is None else b.to(device=device, dtype=dtype)
    return w, b, key
