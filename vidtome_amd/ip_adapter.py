"""IP-Adapter cross-attention on the HIP path: recognise the processor, build the key sets.

After ``pipe.load_ip_adapter(...)`` Diffusers replaces the processor of every attn2 by an ``IPAdapterAttnProcessor`` and
hands the block ``encoder_hidden_states = (text_states, [image_states, ...])``.  The processor computes, per head,

    out = softmax(q K_text^T * scale) V_text  +  sum_a  s_a * softmax(q K_a^T * scale) V_a

with ``K_a = to_k_ip[a](image_a)``, ``V_a = to_v_ip[a](image_a)`` and the same q: one more key / value set per loaded
adapter, every set with a softmax of its own, added with the adapter's scale in front of ``to_out``.  That is what
vtm_attention_kv_sets computes in one launch (include/vidtome_hip.h); this module decides WHEN the patched block may use
it and turns the call into its operands.

`recognise` is strict in the spirit of `lora.recognise`: anything it does not fully understand means the module's own
forward, never a guess.  It accepts a processor when
* its class is named IPAdapterAttnProcessor, IPAdapterAttnProcessor2_0 or IPAdapterXFormersAttnProcessor;
* ``to_k_ip`` / ``to_v_ip`` are ModuleLists of equal length n >= 1 whose entries `lora.recognise` reads as one Linear each,
  without bias, ``out_features == C``, weights of the tokens' dtype; ``num_tokens`` is a sequence of n positive ints and
  ``scale`` a sequence of n plain numbers (a per-layer list of scales is not understood);
* the call is the plain one: no attention mask, ``cross_attention_kwargs`` empty or holding only ``ip_adapter_masks`` that
  is None, all None, or region masks in the published form (below);
* ``encoder_hidden_states`` is the tuple ``(text, images)`` -- text (B, T, D), images a list / tuple of n tensors, each
  (B, T_a, D) or (B, m, T_a, D) (m images: m * T_a keys, like the processor's ``view(B, -1, ...)``) -- or the legacy single
  tensor with the image tokens appended, split at ``shape[1] - num_tokens[0]`` (then n must be 1).
Neither Diffusers nor an adapter checkpoint is a dependency: the contract is duck-typed against the published processor
(tests/ip_adapter_standin.py restates it); a release whose processor differs is not recognised and keeps the module path.

Region masks (``cross_attention_kwargs={"ip_adapter_masks": [...]}``, one entry per adapter): an entry is None -- the adapter
acts everywhere, one set of ``m * T_a`` keys as above -- or a tensor (1, m_a, H, W) for an adapter whose image tensor is 4-D
with ``m_a`` images.  The processor then gives every image a softmax of its own and weighs it per query,

    out += s_a * softmax(q K_{a,i}^T * scale) V_{a,i} * downsample(mask[:, i], B, N, C)

which is one key set per image with a row of per-query weights: vtm_attention_kv_sets_masked.  The downsample (bicubic, to
the site's token grid) is NOT restated here: it is ``IPAdapterMaskProcessor.downsample`` of the module that defines the
processor class, called as ``downsample(mask[:, i], 1, N, 1)``, and its (N,) row is kept in fp32.  A mask in another form (the
3-D tensors of custom processors), a masked adapter with a 3-D image tensor, more than 8 sets in all, a module without that
name or a result of another shape keep the module path.  The one arithmetic difference: the masked term is weighted in fp32
and the sum is rounded once, where the processor rounds the mask and every term to the model's dtype and adds there.

``scale`` is read at every call (``pipe.set_ip_adapter_scale`` takes effect on the next forward).  An adapter whose
scale is 0 is left out, as the processor skips it -- a NaN in its unused image tokens never reaches the output -- and with
every scale 0 the block issues exactly the launches of a block without an adapter.
"""
from __future__ import annotations

import numbers
import sys
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import lora

PROCESSORS = ("IPAdapterAttnProcessor", "IPAdapterAttnProcessor2_0", "IPAdapterXFormersAttnProcessor")
MAX_ADAPTERS = 7             # vtm_attention_kv_sets takes 8 sets: the text and 7 adapters
MAX_KEY_SETS = 8             # ... and with region masks every image of a masked adapter is a set of its own
SET_ALIGN = 8                # a set starts on a multiple of 8 keys (V^T is fetched in 16-byte pieces)


class Call(NamedTuple):
    """One recognised attn2 call: the conditioning split into its parts."""
    text: torch.Tensor                   # (B, T, D)
    images: List[torch.Tensor]           # n tensors (B, T_a, D)
    k_proj: List[torch.nn.Module]        # to_k_ip
    v_proj: List[torch.nn.Module]        # to_v_ip
    scales: List[float]
    masks: Optional[List[Optional[torch.Tensor]]] = None   # region masks: per adapter None, or (m_a, N) fp32 query weights
                                                           # -- one row, and one key set, per image of the adapter


def is_ip_processor(attn) -> bool:
    """attn.processor carries one of the three class names (the cheap test every attn2 call pays)."""
    proc = getattr(attn, "processor", None)
    return proc is not None and type(proc).__name__ in PROCESSORS


def _plain_number(v) -> bool:
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


def _no_bias(m, kind: str) -> bool:
    """The effective Linear has no bias -- read from the modules, without folding anything."""
    if lora.base_linear(m).bias is not None:
        return False
    if kind == lora.PEFT:
        return all(b.bias is None for b in m.lora_B.values())
    return kind != lora.LEGACY or m.lora_layer.up.bias is None


def _projection_ok(m, C: int, dtype) -> bool:
    kind = lora.recognise(m)
    if kind is None:
        return False
    base = lora.base_linear(m)
    return base.out_features == C and base.weight.dtype == dtype and _no_bias(m, kind)


def masks_absent(kwargs) -> bool:
    """``cross_attention_kwargs`` of the plain call: empty, or only ``ip_adapter_masks`` = None / all None."""
    if not kwargs:
        return True
    if set(kwargs) != {"ip_adapter_masks"}:
        return False
    masks = kwargs["ip_adapter_masks"]
    return masks is None or (isinstance(masks, (list, tuple)) and all(m is None for m in masks))


def _region_masks(kwargs, n: int):
    """``ip_adapter_masks`` when ``cross_attention_kwargs`` holds nothing else and it is a list / tuple of n entries, each
    None or a 4-D floating-point tensor (1, m, H, W); else None."""
    if not kwargs or set(kwargs) != {"ip_adapter_masks"}:
        return None
    masks = kwargs["ip_adapter_masks"]
    if not isinstance(masks, (list, tuple)) or len(masks) != n:
        return None
    for m in masks:
        if m is not None and not (isinstance(m, torch.Tensor) and m.dim() == 4 and m.shape[0] == 1 and m.shape[1] >= 1
                                  and m.shape[2] >= 1 and m.shape[3] >= 1 and m.is_floating_point()):
            return None
    return list(masks)


def _mask_rows(proc, mask: torch.Tensor, N: int, device) -> Optional[torch.Tensor]:
    """(m, N) fp32 per-query weights of a (1, m, H, W) region mask at a site of N tokens, by the processor's own
    ``IPAdapterMaskProcessor.downsample`` -- found in the module that defines the processor class, where Diffusers'
    attention_processor imports it -- or None when that cannot be resolved or gives something else than (1, N, 1)."""
    mod = sys.modules.get(type(proc).__module__)
    downsample = getattr(getattr(mod, "IPAdapterMaskProcessor", None), "downsample", None)
    if not callable(downsample):
        return None
    rows = []
    for i in range(mask.shape[1]):
        row = downsample(mask[:, i], 1, N, 1)
        if not isinstance(row, torch.Tensor) or tuple(row.shape) != (1, N, 1) or not row.is_floating_point():
            return None
        rows.append(row.reshape(N).to(device=device, dtype=torch.float32))
    return torch.stack(rows)


def recognise(attn, x: torch.Tensor, encoder_hidden_states, attention_mask=None, kwargs=None) -> Optional[Call]:
    """The parts of a plain IP-Adapter call of ``attn`` on tokens ``x`` (B, N, C), or None (the module path).  What
    `patch.fused_attention_ok` asks of the module itself is the caller's to check."""
    if not is_ip_processor(attn) or attention_mask is not None:
        return None
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.dtype not in (torch.float16, torch.bfloat16):
        return None
    proc = attn.processor
    k_ip, v_ip = getattr(proc, "to_k_ip", None), getattr(proc, "to_v_ip", None)
    if not isinstance(k_ip, torch.nn.ModuleList) or not isinstance(v_ip, torch.nn.ModuleList):
        return None
    n = len(k_ip)
    if not 1 <= n <= MAX_ADAPTERS or len(v_ip) != n:
        return None
    num_tokens, scale = getattr(proc, "num_tokens", None), getattr(proc, "scale", None)
    if not isinstance(num_tokens, (list, tuple)) or len(num_tokens) != n \
            or not all(isinstance(t, int) and not isinstance(t, bool) and t > 0 for t in num_tokens):
        return None
    if not isinstance(scale, (list, tuple)) or len(scale) != n or not all(_plain_number(s) for s in scale):
        return None
    region = None
    if not masks_absent(kwargs):
        region = _region_masks(kwargs, n)
        if region is None:
            return None
    B, _, C = x.shape
    if not all(_projection_ok(m, C, x.dtype) for m in list(k_ip) + list(v_ip)):
        return None
    enc = encoder_hidden_states
    if isinstance(enc, tuple):
        if len(enc) != 2:
            return None
        text, images = enc
        if not isinstance(images, (list, tuple)) or len(images) != n:
            return None
        images = list(images)
    elif isinstance(enc, torch.Tensor):                      # legacy: the image tokens ride behind the text tokens
        if n != 1 or enc.dim() != 3 or enc.shape[1] <= num_tokens[0]:
            return None
        end = enc.shape[1] - num_tokens[0]
        text, images = enc[:, :end], [enc[:, end:]]
    else:
        return None
    if not isinstance(text, torch.Tensor) or text.dim() != 3 or text.shape[0] != B or text.shape[1] < 1 \
            or not text.is_floating_point() or text.device != x.device:
        return None
    flat, n_sets = [], 1
    for a, im in enumerate(images):
        if not isinstance(im, torch.Tensor) or im.dim() not in (3, 4) or im.shape[0] != B or not im.is_floating_point() \
                or im.device != x.device:
            return None
        if region is not None and region[a] is not None:     # a masked adapter: one image, one mask channel, one key set
            if im.dim() != 4 or im.shape[1] != region[a].shape[1]:
                return None
            n_sets += im.shape[1] if float(scale[a]) != 0.0 else 0
        else:
            n_sets += 1 if float(scale[a]) != 0.0 else 0
        if im.dim() == 4:
            im = im.reshape(B, im.shape[1] * im.shape[2], im.shape[3])
        if im.shape[1] < 1 or im.shape[2] != lora.base_linear(k_ip[a]).in_features \
                or im.shape[2] != lora.base_linear(v_ip[a]).in_features:
            return None
        flat.append(im)
    scales = [float(s) for s in scale]
    if region is None:
        return Call(text, flat, list(k_ip), list(v_ip), scales)
    if n_sets > MAX_KEY_SETS:
        return None
    rows = []
    for a, m in enumerate(region):
        # (an adapter of scale 0 takes no part: the processor never downsamples its mask either)
        rows.append(None if m is None or scales[a] == 0.0 else _mask_rows(proc, m, x.shape[1], x.device))
        if m is not None and scales[a] != 0.0 and rows[-1] is None:
            return None
    return Call(text, flat, list(k_ip), list(v_ip), scales, rows)


def key_sets(text_len: int, image_lens: Sequence[int], scales: Sequence[float]
             ) -> Tuple[List[Tuple[int, int, float]], List[int], int]:
    """The layout of the shared k / V^T buffers: ([(start, length, weight)], the adapters that take part, total keys
    padded).  Set 0 is the text at key 0 with weight 1; every adapter whose scale is not 0 follows, in order, at the next
    multiple of 8 keys, weighted by its scale; adapters of scale 0 get no keys at all."""
    sets = [(0, int(text_len), 1.0)]
    active = []
    end = _round_up(text_len)
    for a, (n, s) in enumerate(zip(image_lens, scales)):
        if float(s) == 0.0:
            continue
        sets.append((end, int(n), float(s)))
        active.append(a)
        end = _round_up(end + n)
    return sets, active, end


def masked_key_sets(text_len: int, image_lens: Sequence[int], scales: Sequence[float], images: Sequence[int]
                    ) -> Tuple[List[Tuple[int, int, float]], List[int], int, List[int]]:
    """`key_sets` for a call with region masks: ``images[a]`` is 0 for an adapter without a mask -- one set of
    ``image_lens[a]`` keys, as in `key_sets` -- or m_a, the images of a masked adapter, whose ``image_lens[a] = m_a * T_a`` keys
    become m_a sets of T_a keys, each on the next multiple of 8 keys and each weighted by the adapter's scale.  The fourth
    result names every set's row of the weight table: -1, or 0, 1, ... over the masked sets in order (the rows of the active
    adapters' ``Call.masks``, concatenated)."""
    sets, rows = [(0, int(text_len), 1.0)], [-1]
    active = []
    end, row = _round_up(text_len), 0
    for a, (n, s, m) in enumerate(zip(image_lens, scales, images)):
        if float(s) == 0.0:
            continue
        active.append(a)
        parts = max(int(m), 1)
        for _ in range(parts):
            sets.append((end, int(n) // parts, float(s)))
            rows.append(row if m else -1)
            row += 1 if m else 0
            end = _round_up(end + int(n) // parts)
    return sets, active, end, rows


def _round_up(n: int) -> int:
    return (int(n) + SET_ALIGN - 1) // SET_ALIGN * SET_ALIGN


def drop_caches(attn) -> None:
    """Forget what the fused path cached on the processor's projections (`remove_patch`): panel packs, folded LoRA weights."""
    proc = getattr(attn, "processor", None)
    for name in ("to_k_ip", "to_v_ip"):
        mods = getattr(proc, name, None)
        if isinstance(mods, torch.nn.ModuleList):
            for m in mods.modules():
                m.__dict__.pop("_vtm_packed", None)
                m.__dict__.pop("_vtm_lora", None)
