"""Stand-in for Diffusers' IP-Adapter processors WITH region masks, and for the mask processor they call.

tests/ip_adapter_standin.py restates the unmasked processor (and multiplies by a 3-D mask as custom processors do).  This
module restates the published masked form, ``cross_attention_kwargs={"ip_adapter_masks": [...]}``: one entry per adapter,
None or a tensor (1, m_a, H, W) for an adapter whose image tensor is (B, m_a, T_a, D).  A masked adapter of scale != 0 loops
over its m_a images; every image has a softmax of its own and its term is multiplied by
``IPAdapterMaskProcessor.downsample(mask[:, i], B, N, C)`` in the model's dtype before it is added:

    out += scale_a * (softmax(q K_{a,i}^T s) V_{a,i} * downsample(mask[:, i], B, N, C))

An adapter whose entry is None is the unmasked term (one softmax over all m_a * T_a keys).  `IPAdapterMaskProcessor` lives at
module level because that is where the fused path looks for it: in the module that defines the processor class (Diffusers'
attention_processor imports the name).  Its ``downsample`` is written as the published one: bicubic ``F.interpolate`` to the
token grid of the site, flattened, repeated over the batch and over the channels.

The three classes carry the published names, so `vidtome_amd.ip_adapter` recognises them; `install` is
ip_adapter_standin.install with these classes."""
import math

import torch
import torch.nn.functional as F

import ip_adapter_standin as base


class IPAdapterMaskProcessor:
    @staticmethod
    def downsample(mask: torch.Tensor, batch_size: int, num_queries: int, value_embed_dim: int) -> torch.Tensor:
        """mask (1, H, W) -> (batch_size, num_queries, value_embed_dim): the mask resampled to the token grid whose aspect
        ratio is the mask's."""
        o_h, o_w = mask.shape[1], mask.shape[2]
        ratio = o_w / o_h
        mask_h = int(math.sqrt(num_queries / ratio))
        mask_h = int(mask_h) + int((num_queries % int(mask_h)) != 0)
        mask_w = num_queries // mask_h
        down = F.interpolate(mask.unsqueeze(0), size=(mask_h, mask_w), mode="bicubic").squeeze(0)
        if down.shape[0] < batch_size:
            down = down.repeat(batch_size, 1, 1)
        down = down.view(down.shape[0], -1)
        area = mask_h * mask_w
        if area < num_queries:                     # aspect ratios differ: pad / cut to the token count
            down = F.pad(down, (0, num_queries - down.shape[1]), value=0.0)
        if area > num_queries:
            down = down[:, :num_queries]
        return down.view(down.shape[0], down.shape[1], 1).repeat(1, 1, value_embed_dim)


class IPAdapterAttnProcessor(base.IPAdapterAttnProcessor):
    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, scale=1.0,
                 ip_adapter_masks=None):
        self.calls += 1
        text, ip_states = encoder_hidden_states
        if ip_adapter_masks is not None:
            if not len(ip_adapter_masks) == len(self.scale) == len(ip_states):
                raise ValueError("ip_adapter_masks, scale and the image states must have one entry per adapter")
            for m, s, st in zip(ip_adapter_masks, self.scale, ip_states):
                if m is None:
                    continue
                if not isinstance(m, torch.Tensor) or m.ndim != 4:
                    raise ValueError("each element of ip_adapter_masks must be a tensor (1, num_images, H, W)")
                if m.shape[1] != st.shape[1]:
                    raise ValueError("the number of masks does not match the number of image states")
                if isinstance(s, list) and len(s) != m.shape[1]:
                    raise ValueError("the number of masks does not match the number of scales")
        else:
            ip_adapter_masks = [None] * len(self.scale)
        q = self._heads(attn, attn.to_q(hidden_states))
        mask = None if attention_mask is None else attention_mask[:, None]
        o = F.scaled_dot_product_attention(q, self._heads(attn, attn.to_k(text)), self._heads(attn, attn.to_v(text)),
                                           attn_mask=mask, scale=attn.scale)
        out = o.transpose(1, 2).reshape(o.shape[0], o.shape[2], -1)
        for states, s, to_k, to_v, m in zip(ip_states, self.scale, self.to_k_ip, self.to_v_ip, ip_adapter_masks):
            if (isinstance(s, list) and all(si == 0 for si in s)) or (not isinstance(s, list) and s == 0):
                continue
            if m is not None:
                s = s if isinstance(s, list) else [s] * m.shape[1]
                for i in range(m.shape[1]):
                    cur = self._core(attn, q, to_k(states[:, i]), to_v(states[:, i])).to(q.dtype)
                    down = IPAdapterMaskProcessor.downsample(m[:, i], cur.shape[0], cur.shape[1], cur.shape[2])
                    out = out + s[i] * (cur * down.to(dtype=q.dtype, device=q.device))
            else:
                flat = states.reshape(states.shape[0], -1, states.shape[-1])
                out = out + s * self._core(attn, q, to_k(flat), to_v(flat))
        return attn.to_out[1](attn.to_out[0](out))


class IPAdapterAttnProcessor2_0(IPAdapterAttnProcessor):
    pass


class IPAdapterXFormersAttnProcessor(IPAdapterAttnProcessor):
    pass


PROCESSOR_CLASSES = {c.__name__: c for c in (IPAdapterAttnProcessor, IPAdapterAttnProcessor2_0,
                                             IPAdapterXFormersAttnProcessor)}


def install(model, num_tokens=(4,), scale=(1.0,), cond_dim=768, name="IPAdapterAttnProcessor2_0", seed=11):
    """ip_adapter_standin.install with the processors of this module (the same weights for the same seed)."""
    saved = base.PROCESSOR_CLASSES[name]
    base.PROCESSOR_CLASSES[name] = PROCESSOR_CLASSES[name]
    try:
        return base.install(model, num_tokens, scale, cond_dim, name, seed)
    finally:
        base.PROCESSOR_CLASSES[name] = saved
