"""Stand-in for Diffusers' IP-Adapter attention processors (Diffusers is not installed here or on the GPU box).

`vidtome_amd.ip_adapter` recognises the processor by its class NAME and by duck typing (``to_k_ip`` / ``to_v_ip`` /
``num_tokens`` / ``scale``), so classes with the three published names that carry those attributes are what it sees after
``pipe.load_ip_adapter``.  ``__call__`` restates the published processor: split the ``(text, images)`` tuple (or the legacy
single tensor at ``shape[1] - num_tokens[0]``), ``to_q``, the text term, one SDPA term per adapter -- skipped when its
scale is 0 -- times its scale (and its mask, when one is given), the sum, ``to_out``.  A list-valued scale entry weighs
the m images of a 4-D image tensor one by one (the per-image form the fused path does not understand).

`IPAttention` is a computing attn2 whose forward hands ``encoder_hidden_states`` to the processor untouched; `install`
puts one on every block of a stand-in model (tests/standin.py blocks, test_gpu_lora._StandInSites, sites.SiteUNet)."""
import torch
import torch.nn.functional as F


class IPAdapterAttnProcessor(torch.nn.Module):
    def __init__(self, hidden_size, cross_attention_dim, num_tokens=(4,), scale=1.0):
        super().__init__()
        self.hidden_size, self.cross_attention_dim = hidden_size, cross_attention_dim
        self.num_tokens = list(num_tokens) if isinstance(num_tokens, (list, tuple)) else [num_tokens]
        self.scale = list(scale) if isinstance(scale, (list, tuple)) else [scale] * len(self.num_tokens)
        n = len(self.num_tokens)
        self.to_k_ip = torch.nn.ModuleList([torch.nn.Linear(cross_attention_dim, hidden_size, bias=False) for _ in range(n)])
        self.to_v_ip = torch.nn.ModuleList([torch.nn.Linear(cross_attention_dim, hidden_size, bias=False) for _ in range(n)])
        self.calls = 0

    @staticmethod
    def _heads(attn, t):
        return t.view(t.shape[0], -1, attn.heads, t.shape[-1] // attn.heads).transpose(1, 2)

    def _core(self, attn, q, k, v):
        o = F.scaled_dot_product_attention(q, self._heads(attn, k), self._heads(attn, v), scale=attn.scale)
        return o.transpose(1, 2).reshape(o.shape[0], o.shape[2], -1)

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, scale=1.0,
                 ip_adapter_masks=None):
        self.calls += 1
        ip_states = []
        if encoder_hidden_states is None:
            encoder_hidden_states = hidden_states
        elif isinstance(encoder_hidden_states, tuple):
            encoder_hidden_states, ip_states = encoder_hidden_states
        else:
            end = encoder_hidden_states.shape[1] - self.num_tokens[0]
            encoder_hidden_states, ip_states = encoder_hidden_states[:, :end], [encoder_hidden_states[:, end:]]
        if ip_adapter_masks is None:
            ip_adapter_masks = [None] * len(self.scale)
        q = self._heads(attn, attn.to_q(hidden_states))
        mask = None
        if attention_mask is not None:          # (B, 1 or N, keys) additive, one for all heads
            mask = attention_mask[:, None]
        o = F.scaled_dot_product_attention(q, self._heads(attn, attn.to_k(encoder_hidden_states)),
                                           self._heads(attn, attn.to_v(encoder_hidden_states)), attn_mask=mask,
                                           scale=attn.scale)
        out = o.transpose(1, 2).reshape(o.shape[0], o.shape[2], -1)
        for states, s, to_k, to_v, m in zip(ip_states, self.scale, self.to_k_ip, self.to_v_ip, ip_adapter_masks):
            if isinstance(s, (list, tuple)):
                if all(si == 0 for si in s):
                    continue
                terms = [si * self._core(attn, q, to_k(states[:, i]), to_v(states[:, i])) for i, si in enumerate(s)]
                term = sum(terms[1:], terms[0])
            else:
                if s == 0:
                    continue
                flat = states.reshape(states.shape[0], -1, states.shape[-1])
                term = s * self._core(attn, q, to_k(flat), to_v(flat))
            if m is not None:                   # (B or 1, N, 1): where on the image this adapter acts
                term = term * m.to(term.dtype)
            out = out + term
        return attn.to_out[1](attn.to_out[0](out))


class IPAdapterAttnProcessor2_0(IPAdapterAttnProcessor):
    pass


class IPAdapterXFormersAttnProcessor(IPAdapterAttnProcessor):
    pass


class UnknownIPProcessor(IPAdapterAttnProcessor):
    """The same attributes under a name the recogniser does not know."""


PROCESSOR_CLASSES = {c.__name__: c for c in (IPAdapterAttnProcessor, IPAdapterAttnProcessor2_0,
                                             IPAdapterXFormersAttnProcessor, UnknownIPProcessor)}


class IPAttention(torch.nn.Module):
    """A computing attn2 (the projections of ``src``) that calls its processor like Diffusers' Attention.forward."""

    def __init__(self, src, processor):
        super().__init__()
        self.heads, self.scale = src.heads, src.scale
        self.to_q, self.to_k, self.to_v, self.to_out = src.to_q, src.to_k, src.to_v, src.to_out
        self.processor = processor

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None, **cross_attention_kwargs):
        return self.processor(self, hidden_states, encoder_hidden_states=encoder_hidden_states,
                              attention_mask=attention_mask, **cross_attention_kwargs)


def install(model, num_tokens=(4,), scale=(1.0,), cond_dim=768, name="IPAdapterAttnProcessor2_0", seed=11):
    """Give attn2 of every block of ``model.blocks`` an IP-Adapter processor (weights N(0, 1 / cond_dim), in the model's dtype
    on its device); returns the processors."""
    g = torch.Generator().manual_seed(seed)
    procs = []
    for blk in model.blocks:
        src = blk.attn2
        p0 = src.to_q.weight
        proc = PROCESSOR_CLASSES[name](p0.shape[0], cond_dim, num_tokens, scale)
        with torch.no_grad():
            for p in proc.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[-1] ** -0.5)
        proc.to(device=p0.device, dtype=p0.dtype)
        blk.attn2 = IPAttention(src, proc)
        procs.append(proc)
    return procs


def image_states(num_tokens, B, cond_dim, dtype, device, seed=5, images=1):
    """One (B, T_a, D) tensor per adapter -- (B, images, T_a, D) with ``images`` > 1 -- of N(0, 1) image tokens."""
    g = torch.Generator().manual_seed(seed)
    shape = lambda t: (B, t, cond_dim) if images == 1 else (B, images, t, cond_dim)
    return [torch.randn(shape(t), generator=g).to(device=device, dtype=dtype) for t in num_tokens]
