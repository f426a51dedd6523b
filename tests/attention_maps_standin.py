"""Stand-ins and float64 references shared by the attention-map tests (tests/test_gpu_attention_maps.py,
tests/test_attention_maps_host.py): one full tests/standin.py block behind a ``ModelMixin`` root, a computing attn2 with a
processor the fused path does not know (a "storing" processor: the module path), and the float64 evaluation of the
head-averaged probabilities."""
import torch
import torch.nn.functional as F

import standin

B, FRAMES, LATENT, COND, COND_DIM, HEADS = 2, 2, (8, 8), 77, 768, 8


class StoringProcessor:
    """What a user installs today to see the maps: an attention processor of a name the fused path does not accept."""


class _Computing(torch.nn.Module):
    """A computing, counting forward for a stand-in Attention: the module path."""

    def forward(self, x, encoder_hidden_states=None, attention_mask=None, **kw):
        self.calls = getattr(self, "calls", 0) + 1
        ctx = x if encoder_hidden_states is None else encoder_hidden_states
        n, N, _ = x.shape
        sh = lambda t: t.view(n, t.shape[1], self.heads, -1).transpose(1, 2)
        mask = attention_mask[:, None] if attention_mask is not None and attention_mask.dim() == 3 else attention_mask
        o = F.scaled_dot_product_attention(sh(self.to_q(x)), sh(self.to_k(ctx)), sh(self.to_v(ctx)), attn_mask=mask,
                                           scale=self.scale)
        return self.to_out[0](o.transpose(1, 2).reshape(n, N, -1))


class ComputingSelf(_Computing, standin.Attention):
    pass


class StoringCross(_Computing, standin.CrossAttention):
    """A computing attn2 carrying that processor: the block takes the module path."""

    def __init__(self, C, heads, cond_dim):
        super().__init__(C, heads, cond_dim)
        self.processor = StoringProcessor()
        self.calls = 0


class AdaNorm(torch.nn.Module):
    """AdaLayerNorm's call form (x, timestep) around a LayerNorm."""

    def __init__(self, ln):
        super().__init__()
        self.ln = ln

    def forward(self, x, timestep=None):
        return self.ln(x)


class OneBlock(standin.ModelMixin):
    """One full stand-in block at downsample 1 (its Attention.forward raises), 2-D weights N(0, 1 / fan_in) from ``seed``,
    the Linear biases N(0, 1 / fan_in) from a generator of their own (torch.nn.Linear draws them from the process-wide RNG:
    two blocks of one ``seed`` would not hold the same parameters, and the weights keep the values they always had);
    ``storing``: attn2 is a StoringCross with the same weights; ``computing_self``: attn1 computes too."""

    def __init__(self, C, heads=HEADS, storing=False, seed=0, computing_self=False):
        super().__init__()
        blk = standin.BasicTransformerBlock(C, heads, True, COND_DIM)
        if storing:
            blk.attn2 = StoringCross(C, heads, COND_DIM)
        if computing_self:
            blk.attn1 = ComputingSelf(C, heads)
        self.blocks = torch.nn.ModuleList([blk])
        g = torch.Generator().manual_seed(seed)
        gb = torch.Generator().manual_seed(seed + 7919)
        with torch.no_grad():
            for p in self.parameters():
                if p.ndim == 2:
                    p.copy_(torch.randn(p.shape, generator=g) * p.shape[-1] ** -0.5)
            for m in self.modules():
                if isinstance(m, torch.nn.Linear) and m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=gb) * m.in_features ** -0.5)

    def set_size(self, latent_hw):
        self._tome_info["size"] = latent_hw


def patched(C, dtype, device, latent=LATENT, **kw):
    """A fresh OneBlock through apply_patch, the RNG seeded so that two of them merge the same tokens."""
    import vidtome_amd
    unet = OneBlock(C, **kw).to(device=device, dtype=dtype)
    torch.manual_seed(123)
    vidtome_amd.apply_patch(unet, local_merge_ratio=0.5, merge_global=True, global_merge_ratio=0.5, batch_size=B)
    unet.set_size(latent)
    return unet


def inputs(C, dtype, device, tokens=LATENT[0] * LATENT[1], seed=70):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(B * FRAMES, tokens, C, generator=g).to(device=device, dtype=dtype)
    cond = torch.randn(B * FRAMES, COND, COND_DIM, generator=g).to(device=device, dtype=dtype)
    return h, cond


def prompt_mask(dtype, device):
    """Diffusers' additive form of an encoder_attention_mask, (B F, 1, 77) of 0 / -10000, another length in every row."""
    lengths = torch.tensor([20 + 9 * i for i in range(B * FRAMES)])
    keep = torch.arange(COND)[None, :] < lengths[:, None]
    return ((1 - keep.to(dtype)) * -10000.0).unsqueeze(1).to(device), keep


def probs64(q, k, heads, scale, bias=None):
    """float64 mean over the heads of softmax(q k^T scale + bias): q (n, N, C), k (n, K, C) of any dtype, bias (n or 1, K)."""
    n, N, C = q.shape
    sh = lambda t: t.double().cpu().view(n, t.shape[1], heads, C // heads).transpose(1, 2)
    s = sh(q) @ sh(k).transpose(-1, -2) * scale
    if bias is not None:
        s = s + bias.double().cpu()[:, None, None, :]
    return torch.softmax(s, dim=-1).mean(1)


def projection64(lin, x):
    """(x W^T in float64, |x| |W|^T): the projection of the module's own Linear and the magnitude sum that bounds what
    rounding its operands can move."""
    w, x = lin.weight.detach().double().cpu(), x.double().cpu()
    return x @ w.T, x.abs() @ w.abs().T
