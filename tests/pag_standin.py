"""Stand-in for Diffusers' perturbed-attention-guidance processors (Diffusers is not installed here or on the GPU box).

`vidtome_amd.pag` recognises the processors by class NAME, so classes with the two published names are what it sees after a
PAG pipeline has set ``pag_applied_layers``.  ``__call__`` restates the published arithmetic: chunk the batch into 2
(org | perturbed) or 3 (uncond | cond | perturbed); plain SDPA -- with the attention mask, when one is given -- on the org
part; ``to_out[0](to_v(ptb))`` on the perturbed part (the softmax replaced by the identity); cat.  ``calls`` counts the
calls, as the IP-Adapter stand-in does.

`PAGAttention` is a computing attn1 that hands its call to the processor like Diffusers' Attention.forward; `install` puts
one on attn1 of every block of a stand-in model (test_gpu_lora._StandInSites, sites.SiteUNet, tests/standin.py blocks)."""
import torch
import torch.nn.functional as F


class PAGIdentitySelfAttnProcessor2_0:
    groups = 2

    def __init__(self):
        self.calls = 0

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None):
        self.calls += 1
        parts = hidden_states.chunk(self.groups)
        ptb = parts[-1]
        org = parts[0] if self.groups == 2 else torch.cat(parts[:-1])
        B, N, _ = org.shape
        sh = lambda t: t.view(B, t.shape[1], attn.heads, -1).transpose(1, 2)
        mask = None
        if attention_mask is not None:          # (B_org, 1 or N, keys) additive, one for all heads
            mask = attention_mask[:, None]
        o = F.scaled_dot_product_attention(sh(attn.to_q(org)), sh(attn.to_k(org)), sh(attn.to_v(org)), attn_mask=mask,
                                           scale=attn.scale)
        org = attn.to_out[1](attn.to_out[0](o.transpose(1, 2).reshape(B, N, -1)))
        ptb = attn.to_out[1](attn.to_out[0](attn.to_v(ptb)))
        return torch.cat([org, ptb])


class PAGCFGIdentitySelfAttnProcessor2_0(PAGIdentitySelfAttnProcessor2_0):
    groups = 3


class PAGHunyuanAttnProcessor2_0(PAGIdentitySelfAttnProcessor2_0):
    """A published PAG processor of another model family: not understood by the recogniser."""


class PAGJointAttnProcessor2_0(PAGIdentitySelfAttnProcessor2_0):
    """(likewise)"""


PROCESSOR_CLASSES = {c.__name__: c for c in (PAGIdentitySelfAttnProcessor2_0, PAGCFGIdentitySelfAttnProcessor2_0,
                                             PAGHunyuanAttnProcessor2_0, PAGJointAttnProcessor2_0)}
BY_GROUPS = {2: "PAGIdentitySelfAttnProcessor2_0", 3: "PAGCFGIdentitySelfAttnProcessor2_0"}


class PAGAttention(torch.nn.Module):
    """A computing attn1 (the projections of ``src``) that calls its processor like Diffusers' Attention.forward."""

    def __init__(self, src, processor):
        super().__init__()
        self.heads, self.scale = src.heads, src.scale
        self.to_q, self.to_k, self.to_v, self.to_out = src.to_q, src.to_k, src.to_v, src.to_out
        self.processor = processor

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None, **cross_attention_kwargs):
        return self.processor(self, hidden_states, encoder_hidden_states=encoder_hidden_states,
                              attention_mask=attention_mask, **cross_attention_kwargs)


class PlainProcessor:
    """A plain processor under a name ``fused_attention_ok`` accepts: SDPA over the whole batch."""

    def __init__(self):
        self.calls = 0

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None):
        self.calls += 1
        B, N, _ = hidden_states.shape
        sh = lambda t: t.view(B, t.shape[1], attn.heads, -1).transpose(1, 2)
        o = F.scaled_dot_product_attention(sh(attn.to_q(hidden_states)), sh(attn.to_k(hidden_states)),
                                           sh(attn.to_v(hidden_states)), scale=attn.scale)
        return attn.to_out[1](attn.to_out[0](o.transpose(1, 2).reshape(B, N, -1)))


PlainProcessor.__name__ = "AttnProcessor2_0"


def install(model, groups=3, name=None):
    """Give attn1 of every block of ``model.blocks`` a PAG processor of ``groups`` batch groups (or the class ``name``;
    "plain": a plain processor); returns the processors."""
    procs = []
    for blk in model.blocks:
        proc = PlainProcessor() if name == "plain" else PROCESSOR_CLASSES[name or BY_GROUPS[groups]]()
        blk.attn1 = PAGAttention(blk.attn1, proc)
        procs.append(proc)
    return procs
