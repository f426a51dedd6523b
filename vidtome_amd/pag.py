"""Perturbed-attention guidance (PAG) on the HIP path: recognise the perturbed batch of attn1, split it.

Diffusers turns PAG on by installing ``PAGIdentitySelfAttnProcessor2_0`` (batch = org | perturbed) or
``PAGCFGIdentitySelfAttnProcessor2_0`` (batch = uncond | cond | perturbed) on attn1 of the layers named by
``pag_applied_layers`` (default "mid").  Both processors chunk the batch, run the plain attention on the leading part and
replace the softmax of the last chunk by the identity:

    out[:n_org] = to_out(softmax(q k^T * scale) v)          out[n_org:] = to_out(to_v(x[n_org:]))

The perturbed samples need no q, no k and no attention launch, so the patched block drives its own kernels on sub-batches
(patch.py: the org samples take the route's body on the leading sub-batch, the perturbed samples one V projection at the
rows the output projection reads, written behind the cores' output; to_out, the unmerge and the residual run once over
all samples).  This module says WHEN: `groups_of` recognises the processors by class NAME, as `ip_adapter` does (Diffusers
is not a dependency; tests/pag_standin.py restates the published arithmetic), or by the marker that
`register_perturbed_attention` leaves for hosts without Diffusers.  Any other ``PAG*`` processor (Hunyuan, Joint, ...) is not
understood and keeps the module path.

Where the batch sits: at a site that merges, a sample of attn1's batch is the whole joined chunk of one batch entry, so the
batch is ``apply_patch``'s ``batch_size`` (3 for [uncond | cond | perturbed]); at a site that does not merge it is the
``B * F`` frame rows, frame-minor per sample, whose last ``B * F // groups`` frames are the perturbed sample's.  The pairing
on the sampler side is ``GuidedDPMSolver(weights=(1 - s, s + p, -p))`` over (uncond, cond, perturbed).
"""
from __future__ import annotations

from typing import Iterable, Optional, Tuple, Union

import torch

PROCESSORS = {"PAGIdentitySelfAttnProcessor2_0": 2, "PAGCFGIdentitySelfAttnProcessor2_0": 3}   # class name -> batch groups
MARK = "vtm_pag_groups"          # on attn1 of a registered block


def registered(attn: torch.nn.Module) -> Optional[int]:
    """The groups `register_perturbed_attention` marked ``attn`` with, or None."""
    return attn.__dict__.get(MARK)


def groups_of(attn: torch.nn.Module) -> Optional[int]:
    """2 (org | perturbed) or 3 (uncond | cond | perturbed) when ``attn`` is a PAG attn1 -- its processor carries one of
    the two published names, or its block was registered -- else None."""
    g = registered(attn)
    if g is not None:
        return g
    proc = getattr(attn, "processor", None)
    return None if proc is None else PROCESSORS.get(type(proc).__name__)


def split(B: int, groups: int) -> Tuple[int, int]:
    """(n_org, n_ptb) of a batch of B leading samples: the last ``B // groups`` are perturbed, as
    ``hidden_states.chunk(groups)`` has it."""
    if groups not in (2, 3):
        raise ValueError(f"perturbed attention: groups must be 2 or 3, got {groups!r}")
    if B <= 0 or B % groups:
        raise ValueError(f"perturbed attention: a batch of {B} does not split into {groups} equal groups")
    n_ptb = B // groups
    return B - n_ptb, n_ptb


def register_perturbed_attention(model: torch.nn.Module, layers: Union[str, Iterable[str]] = ("mid",), groups: int = 3):
    """Mark attn1 of every patched block whose module name contains one of ``layers`` as perturbed attention over
    ``groups`` batch groups (3: [uncond | cond | perturbed], 2: [org | perturbed]) -- what installing the Diffusers
    processors does, for hosts without Diffusers.  ``model`` is what ``apply_patch`` took.  Registering again only changes
    the selection.  A block whose attn1 shares probabilities under PnP at this moment is refused.  Returns the marked
    names, sorted."""
    from .maps import _patched_blocks
    from .patch import _pnp_share_groups
    if isinstance(groups, bool) or groups not in (2, 3):
        raise ValueError(f"register_perturbed_attention: groups must be 2 or 3, got {groups!r}")
    layers = (layers,) if isinstance(layers, str) else tuple(layers)
    every = _patched_blocks(model)
    if not every:
        raise RuntimeError("register_perturbed_attention: nothing is patched (call apply_patch first)")
    chosen = [(name, blk) for name, blk, _ in every if any(l in name for l in layers)]
    if not chosen:
        raise ValueError(f"register_perturbed_attention: no patched block's name contains one of {list(layers)}")
    for name, blk in chosen:
        if _pnp_share_groups(blk.attn1) != 1:
            raise RuntimeError(f"register_perturbed_attention: attn1 of {name} shares probabilities under PnP injection; "
                               "the perturbed samples have none to share")
    remove_perturbed_attention(model)
    for _, blk in chosen:
        blk.attn1.__dict__[MARK] = int(groups)
    return sorted({name for name, _ in chosen})


def remove_perturbed_attention(model: torch.nn.Module) -> None:
    """Drop every marker (``remove_patch`` does the same)."""
    from .patch import _patched_roots
    _, roots = _patched_roots(model, controlnet_on_unet=False)
    for root in roots:
        for module in root.modules():
            module.__dict__.pop(MARK, None)
