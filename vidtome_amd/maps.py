"""Head-averaged cross-attention maps of patched blocks.

    register_attention_maps(model)                       # every patched block of the UNet
    ...one UNet call...
    maps = collect_from_patch(model, "attn2_probs")      # {block name: (B F, N, K) float32}

A registered block leaves ``block.attn2_probs`` after every forward: the mean over the heads of attn2's softmax
probabilities, fp32, (B F, N, K) with K the text token count of that call (an IP-Adapter call: of its text set).  The tensor
is new on every forward -- never accumulated, no autograd history -- and lives on the stream the block ran on; a chunked
UNet call overwrites it chunk by chunk, so collect after each call.  Blocks whose attn2 runs fused get it from one
vtm_attention_probs launch on the q / k rows the segment already holds (csrc/attention_probs.hip); every other route from a
torch restatement of to_q / to_k (patch._module_path_probs), or None where the projections cannot be read.  The block's
output does not depend on the switch, and an unregistered block launches what it launched before."""
from __future__ import annotations

from typing import Callable, Iterable, Optional, Union

import torch

from .patch import _patched_roots

FLAG, ATTR = "vtm_attention_maps", "attn2_probs"


def _patched_blocks(model: torch.nn.Module):
    """[(name, block, in the UNet)] of the patched blocks, under the names ``collect_from_patch`` returns (a ControlNet's
    blocks carry the names of the UNet's down and mid blocks: a name then means both)."""
    unet, roots = _patched_roots(model, controlnet_on_unet=False)
    return [(name, module, root is unet) for root in roots for name, module in root.named_modules()
            if module.__class__.__name__ == "ToMeBlock" and hasattr(module, "_tome_info")]


def _clear(block: torch.nn.Module) -> None:
    block.__dict__.pop(FLAG, None)
    block.__dict__.pop(ATTR, None)


def register_attention_maps(model: torch.nn.Module,
                            blocks: Optional[Union[Iterable[str], Callable[[str, torch.nn.Module], bool]]] = None):
    """Switch the cross-attention maps on: ``model`` is what ``apply_patch`` took.  ``blocks`` = None: every patched block of
    the UNet (not of a ControlNet); an iterable of module names (the keys ``collect_from_patch`` returns); or a predicate
    ``(name, block) -> bool`` over all patched blocks, a ControlNet's included.  Registering again only changes the
    selection: blocks no longer selected lose the switch and their stored map.  Returns the selected names, sorted."""
    every, chosen = select_blocks(model, blocks, "register_attention_maps")
    for (name, blk, _), on in zip(every, chosen):
        if on:
            setattr(blk, FLAG, True)
        else:
            _clear(blk)
    return sorted({name for (name, _, _), on in zip(every, chosen) if on})


def select_blocks(model: torch.nn.Module, blocks, who: str):
    """(every patched block as ``_patched_blocks`` lists them, [selected or not]) for the ``blocks`` argument of ``who``
    (``register_attention_maps`` states its three forms); raises when nothing is patched or a name is not a patched block's."""
    every = _patched_blocks(model)
    if not every:
        raise RuntimeError(f"{who}: nothing is patched (call apply_patch first)")
    if blocks is None:
        chosen = [in_unet for _, _, in_unet in every]
    elif callable(blocks):
        chosen = [bool(blocks(name, blk)) for name, blk, _ in every]
    else:
        names = {blocks} if isinstance(blocks, str) else set(blocks)
        unknown = sorted(names - {name for name, _, _ in every})
        if unknown:
            raise ValueError(f"{who}: not patched blocks: {unknown}")
        chosen = [name in names for name, _, _ in every]
    return every, chosen


def unregister_attention_maps(model: torch.nn.Module) -> None:
    """Switch the maps off everywhere and drop the stored ones (``remove_patch`` does the same)."""
    _, roots = _patched_roots(model, controlnet_on_unet=False)
    for root in roots:
        for module in root.modules():
            _clear(module)
