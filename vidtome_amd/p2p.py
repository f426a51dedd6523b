"""Prompt-to-Prompt cross-attention control on patched blocks, on the fused attn2 path.

    pnp.register_time(pipe, t)                                            # every step, as for PnP
    register_cross_attention_control(pipe, schedule, num_inputs=3,
                                     edits={2: CrossEdit.replace(mapper, alpha_words)})
    ...one UNet call on a [source | uncond | cond] x frames batch...

Prompt-to-Prompt replaces, per head and per query i of an edited sample, attn2's probabilities by

    P_edit[i, n] = a[n] * sum_w P_src[i, w] * M[w, n]  +  b[n] * P_own[i, n]

where P_src is the softmax of the SOURCE sample's query against the source sample's keys and P_own the sample's own.  Its
three controllers and the ``cross_replace_alpha`` blend ``attn_new * aw + (1 - aw) * attn_own`` are instances:

    replace    M = the word mapper                     a = aw           b = 1 - aw
    refine     M = one-hot columns of the index map    a = aw alpha     b = aw (1 - alpha) + (1 - aw)
    reweight   on top of either (or of the source)     a times eq       the aw part of b times eq

The form is linear in the probabilities, so the patched block never builds them: P_edit V = P_src (M diag(a) V) +
P_own (diag(b) V), two softmaxes over two key sets with two value operands (the controlled core of patch._attn2_core:
vtm_cross_edit_values + one vtm_attention_kv_sets_src launch per edited group).

The batch is group-major like PnP's: sample b = g * (BF / num_inputs) + f, group 0 the source, and the source of sample b is
b % (BF / num_inputs).  A block injects when ``attn2.t in injection_schedule or attn2.t == 1000`` (the PnP rule); at every
other step, and on unregistered blocks, it launches what it launches without the control.  At an injecting step a call
the fused control does not take (fp32 or AdaLayerNorm blocks, an IP-Adapter call, an attention mask, processor kwargs, a
module that is not the plain arithmetic, more than 256 text tokens, an edit of another token count) raises: an edit that is
silently not applied is worse than a stop."""
from __future__ import annotations

from typing import Callable, Dict, Iterable, Optional, Union

import torch

from .maps import select_blocks
from .patch import _patched_roots

ATTR = "vtm_cross_control"


def _f32(t, shape, name: str) -> torch.Tensor:
    t = torch.as_tensor(t)
    if not (t.is_floating_point() or name == "mapper" and t.dtype in (torch.int32, torch.int64, torch.bool)):
        raise TypeError(f"CrossEdit: {name} must be a floating-point tensor, got {t.dtype}")
    t = t.detach().to(torch.float32)
    if tuple(t.shape) != shape:
        raise ValueError(f"CrossEdit: {name} must have shape {shape}, got {tuple(t.shape)}")
    return t.contiguous()


def _per_word(v, K: int, name: str) -> torch.Tensor:
    """A scalar or a (K,) / (1, .., K) tensor of per-word values -> (K,) float64 on the host."""
    t = torch.as_tensor(v, dtype=torch.float64).detach().cpu()
    if t.numel() == 1:
        return t.reshape(1).expand(K).clone()
    if t.numel() != K or t.shape[-1] != K:
        raise ValueError(f"CrossEdit: {name} must be a scalar or hold {K} per-word values, got shape {tuple(t.shape)}")
    return t.reshape(K).clone()


class CrossEdit:
    """One sample group's edit: ``mapper`` (K, K), ``src_weight`` (K,), ``own_weight`` (K,) -- M, a, b of the form above,
    K the conditioning's token count.  Any float dtype or device is taken; the edit keeps fp32 and follows the model to its
    device (``on``)."""

    def __init__(self, mapper, src_weight, own_weight, _parts=None):
        m = torch.as_tensor(mapper)
        if m.dim() != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 1:
            raise ValueError(f"CrossEdit: mapper must be (K, K), got {tuple(m.shape)}")
        K = m.shape[0]
        self.mapper = _f32(m, (K, K), "mapper")
        self.src_weight = _f32(src_weight, (K,), "src_weight")
        self.own_weight = _f32(own_weight, (K,), "own_weight")
        # (a, b, aw) of the controller result a * P_src M + b * P_own BEFORE the alpha_words blend, float64 on the host:
        # what ``reweight`` scales.  An edit given as plain (M, a, b) is its own controller result (aw = 1).
        self._parts = _parts if _parts is not None else (self.src_weight.double().cpu(), self.own_weight.double().cpu(),
                                                         torch.ones(K, dtype=torch.float64))
        self._on: Dict[torch.device, tuple] = {}

    @property
    def K(self) -> int:
        return self.mapper.shape[0]

    @property
    def is_identity(self) -> bool:
        """The edit leaves the probabilities as they are (a == 0, b == 1): the group is not edited."""
        return bool((self.src_weight == 0).all()) and bool((self.own_weight == 1).all())

    def on(self, device) -> tuple:
        """(M, a, b) contiguous fp32 on ``device``, moved once."""
        device = torch.device(device)
        hit = self._on.get(device)
        if hit is None:
            hit = self._on[device] = tuple(t.to(device).contiguous() for t in (self.mapper, self.src_weight, self.own_weight))
        return hit

    @classmethod
    def _blend(cls, mapper, a, b, aw) -> "CrossEdit":
        """The edit of the controller result (a, b) blended with the own probabilities: aw * (.) + (1 - aw) * P_own."""
        return cls(mapper, aw * a, aw * b + (1.0 - aw), _parts=(a, b, aw))

    @classmethod
    def identity(cls, K: int) -> "CrossEdit":
        return cls(torch.eye(K), torch.zeros(K), torch.ones(K))

    @classmethod
    def replace(cls, mapper, alpha_words=1.0) -> "CrossEdit":
        """AttentionReplace: ``einsum('hpw,bwn->bhpn', attn_base, mapper)``, then the ``alpha_words`` blend."""
        m = torch.as_tensor(mapper)
        if m.dim() == 3 and m.shape[0] == 1:
            m = m[0]
        K = m.shape[-1]
        return cls._blend(m, torch.ones(K, dtype=torch.float64), torch.zeros(K, dtype=torch.float64),
                          _per_word(alpha_words, K, "alpha_words"))

    @classmethod
    def refine(cls, index, alphas, alpha_words=1.0) -> "CrossEdit":
        """AttentionRefine: ``attn_base[:, :, index] * alphas + attn_own * (1 - alphas)``, then the ``alpha_words`` blend.
        ``index`` (K,) ints: the source word every word reads, -1 for a new word, which needs ``alphas == 0`` there."""
        idx = torch.as_tensor(index).detach().cpu().reshape(-1)
        if idx.is_floating_point() or idx.dtype == torch.bool:
            raise TypeError("CrossEdit.refine: index must hold integers")
        idx = idx.long()
        K = idx.numel()
        al = _per_word(alphas, K, "alphas")
        if bool(((idx < -1) | (idx >= K)).any()):
            raise ValueError(f"CrossEdit.refine: index entries must lie in -1 .. {K - 1}")
        if bool((al[idx < 0] != 0).any()):
            raise ValueError("CrossEdit.refine: a new word (index -1) has no source word: alphas must be 0 there")
        m = torch.zeros(K, K)
        cols = torch.nonzero(idx >= 0).reshape(-1)
        m[idx[cols], cols] = 1.0
        return cls._blend(m, al, 1.0 - al, _per_word(alpha_words, K, "alpha_words"))

    def reweight(self, equalizer) -> "CrossEdit":
        """AttentionReweight on top of this edit: its controller result times ``equalizer`` (K,) per word, then the same
        ``alpha_words`` blend.  On ``identity`` nothing comes of it (P2P re-weights the SOURCE's words: start from
        ``CrossEdit.replace(torch.eye(K))``)."""
        a, b, aw = self._parts
        eq = _per_word(equalizer, self.K, "equalizer")
        return CrossEdit._blend(self.mapper, a * eq, b * eq, aw)


def _clear(block: torch.nn.Module) -> None:
    block.__dict__.pop(ATTR, None)


def register_cross_attention_control(model: torch.nn.Module, injection_schedule, num_inputs: int,
                                     edits: Dict[int, CrossEdit],
                                     blocks: Optional[Union[Iterable[str], Callable[[str, torch.nn.Module], bool]]] = None):
    """Switch the control on: ``model`` and ``blocks`` as for ``register_attention_maps`` (None: every patched block of the
    UNet; names; or a predicate).  ``injection_schedule``: the timesteps at which the blocks inject (``pnp.register_time``
    stamps the current one).  ``edits``: {group index in 1 .. num_inputs - 1: CrossEdit}; group 0 is the source.  Registering
    again only replaces the schedule, the edits and the selection -- that is how ``alpha_words`` changes from step to step.
    Returns the selected names, sorted."""
    who = "register_cross_attention_control"
    num_inputs = int(num_inputs)
    if num_inputs < 2:
        raise ValueError(f"{who}: num_inputs must be at least 2 (the source and one group to edit)")
    edits = dict(edits)
    for g, e in edits.items():
        if not isinstance(g, int) or isinstance(g, bool) or not 1 <= g < num_inputs:
            raise ValueError(f"{who}: edits are keyed by the group index 1 .. {num_inputs - 1} (group 0 is the source), got {g!r}")
        if not isinstance(e, CrossEdit):
            raise TypeError(f"{who}: the edit of group {g} is not a CrossEdit")
    schedule = injection_schedule                      # (kept as given, like pnp.register_attention_control's)
    every, chosen = select_blocks(model, blocks, who)
    for (name, blk, _), on in zip(every, chosen):
        if on:
            setattr(blk, ATTR, (schedule, num_inputs, edits, name))
        else:
            _clear(blk)
    return sorted({name for (name, _, _), on in zip(every, chosen) if on})


def unregister_cross_attention_control(model: torch.nn.Module) -> None:
    """Switch the control off everywhere (``remove_patch`` does the same)."""
    _, roots = _patched_roots(model, controlnet_on_unet=False)
    for root in roots:
        for module in root.modules():
            _clear(module)
