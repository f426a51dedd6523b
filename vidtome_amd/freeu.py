"""FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net"; Diffusers' ``pipe.enable_freeu(s1, s2, b1, b2)``) on one fused
HIP launch per up-block resnet.

    register_freeu(pipe, s1=0.9, s2=0.2, b1=1.5, b2=1.6)         # or, on a pipeline that called enable_freeu(...):
    register_freeu(pipe)                                          # take the factors over from the blocks

FreeU scales the lower half of the backbone channels of the first two up blocks by ``b`` and the four lowest frequency bins of
the skip connection's planes by ``s``, in front of every resnet of those blocks.  Diffusers does it with a chain of torch ops
(a slice multiply, an fp32 upcast, fftn, fftshift, a mask, ifftshift, ifftn, .real, a cast back) on both halves before it
concatenates them; here every resnet of ``unet.up_blocks[0]`` (``b1``, ``s1``) and ``unet.up_blocks[1]`` (``b2``, ``s2``) gets
a forward PRE-hook that runs ``vtm_freeu`` in place on the concatenation it is about to read (csrc/freeu.hip: no FFT, one
pass, fp32 inside, one rounding per stored value).  Pre-hooks run in front of a replaced ``forward`` as well, so
``pnp.register_conv_control``'s closure sees the FreeU-treated tensor, the order Diffusers has.

While registered the blocks' own ``s1, s2, b1, b2`` attributes are None: Diffusers' torch branch stays off and nothing is
applied twice.  ``unregister_freeu`` (and ``remove_patch``) removes the hooks and gives the attributes back as found.  Nothing
falls back silently: a tensor the kernel does not take (CPU, another dtype, non-contiguous, a plane beyond 16384 elements)
raises where it is met, and so does one that requires grad while grad is enabled (the write is in place)."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib

KEY = "vtm_freeu"
ATTRS = ("s1", "s2", "b1", "b2")
_ABSENT = object()


def _unet(model):
    return model.unet if hasattr(model, "unet") else model


def release(block: torch.nn.Module) -> None:
    """Drop ``block``'s registration, if it has one: hooks off, the attributes Diffusers reads back as they were found."""
    state = block.__dict__.pop(KEY, None)
    if state is None:
        return
    for handle in state["handles"]:
        handle.remove()
    for name, value in state["found"].items():
        if value is _ABSENT:
            block.__dict__.pop(name, None)
        else:
            setattr(block, name, value)


def _channels_hook(state):
    def pre(block, args, kwargs):
        hidden = kwargs["hidden_states"] if "hidden_states" in kwargs else (args[0] if args else None)
        if not isinstance(hidden, torch.Tensor) or hidden.dim() != 4:
            raise ValueError("freeu: the up block was called without a (B, C, H, W) hidden_states tensor")
        state["C_h"] = int(hidden.shape[1])
    return pre


def _resnet_hook(state, block, j: int):
    def pre(resnet, args, kwargs):
        x = args[0] if args else kwargs.get("input_tensor")
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise ValueError(f"freeu: resnet {j} was called without a (B, C, H, W) input tensor")
        C_h = state["C_h"] if j == 0 else int(block.resnets[j - 1].out_channels)
        if C_h is None:
            raise RuntimeError("freeu: resnet 0 ran outside its up block's forward: the backbone channel count is read from "
                               "the block's hidden_states argument")
        if x.shape[1] - C_h <= 0:
            raise ValueError(f"freeu: resnet {j} got {x.shape[1]} channels of which {C_h} are the backbone's: C_s = "
                             f"{x.shape[1] - C_h} skip channels, at least 1 is needed")
        if x.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("freeu: the resnet's input requires grad: the in-place write would corrupt autograd (run under "
                               "torch.no_grad(), or unregister_freeu for training)")
        _lib.freeu(x, C_h, state["b"], state["s"], state["version"])
    return pre


def register_freeu(model, s1: Optional[float] = None, s2: Optional[float] = None, b1: Optional[float] = None,
                   b2: Optional[float] = None, version: int = 1):
    """Switch FreeU on for ``model`` (what ``apply_patch`` takes: a pipeline or a UNet; it need not be patched -- but
    ``apply_patch`` begins with ``remove_patch``, so register after it).  ``unet.up_blocks[0]`` uses ``(b1, s1)``,
    ``unet.up_blocks[1]`` uses ``(b2, s2)``; later blocks are untouched.  With all four factors None they are read from the
    blocks, where Diffusers' ``enable_freeu`` left them.  ``version`` 1 is Diffusers' constant backbone factor, 2 the original
    repository's per-pixel one (include/vidtome_hip.h).  Registering again replaces the factors; no hook is stacked."""
    who = "register_freeu"
    version = int(version)
    if version not in (1, 2):
        raise ValueError(f"{who}: version = {version}: 1 (Diffusers) or 2 (the original repository) is taken")
    blocks = list(getattr(_unet(model), "up_blocks", []))[:2]
    if len(blocks) < 2 or any(not hasattr(blk, "resnets") for blk in blocks):
        raise ValueError(f"{who}: the UNet needs two up blocks with resnets (unet.up_blocks[0], unet.up_blocks[1])")
    given = dict(s1=s1, s2=s2, b1=b1, b2=b2)
    takeover = all(v is None for v in given.values())
    if not takeover and any(v is None for v in given.values()):
        raise ValueError(f"{who}: pass all of s1, s2, b1, b2 or none of them (got "
                         + ", ".join(f"{k} = {v}" for k, v in given.items()) + ")")
    plans = []
    for i, blk in enumerate(blocks):
        old = blk.__dict__.get(KEY)
        # what Diffusers' own branch would read: the attributes as found (of the first registration, when this is a second)
        found = old["found"] if old is not None else {n: blk.__dict__.get(n, _ABSENT) for n in ATTRS}
        if takeover:
            values = {n: (None if found[n] is _ABSENT else found[n]) for n in ATTRS}
            if not all(values.values()):
                raise ValueError(f"{who}: up_blocks[{i}] carries no FreeU factors ("
                                 + ", ".join(f"{n} = {values[n]}" for n in ATTRS)
                                 + "): call pipe.enable_freeu(...) first or pass the factors")
        else:
            values = given
        b, s = float(values["b%d" % (i + 1)]), float(values["s%d" % (i + 1)])
        plans.append((blk, found, b, s))
    for blk, found, b, s in plans:
        release(blk)
        state = {"b": b, "s": s, "version": version, "found": found, "C_h": None, "handles": []}
        state["handles"].append(blk.register_forward_pre_hook(_channels_hook(state), with_kwargs=True))
        for j, resnet in enumerate(blk.resnets):
            state["handles"].append(resnet.register_forward_pre_hook(_resnet_hook(state, blk, j), with_kwargs=True))
        for name in ATTRS:
            setattr(blk, name, None)
        blk.__dict__[KEY] = state
    return model


def unregister_freeu(model):
    """Switch FreeU off: the hooks go, the blocks' ``s1, s2, b1, b2`` come back as ``register_freeu`` found them (so a model
    taken over from ``enable_freeu`` runs Diffusers' torch branch again)."""
    for blk in getattr(_unet(model), "up_blocks", []):
        release(blk)
    return model
