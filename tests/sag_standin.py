"""Float64 restatement of self-attention guidance and a mid-block stand-in, shared by tests/test_sag_host.py and
tests/test_gpu_sag.py.  Nothing here imports vidtome_amd.sag: the key mass from 16-bit q / k, the Gaussian taps, torch's
"reflect" indices, the integer nearest-neighbour rule, the three prediction types, the select and add_noise are written out
again from the contract (include/vidtome_hip.h: vtm_attention_key_mass, vtm_sag_degrade)."""
import math

import numpy as np
import torch

import attention_maps_standin as AM
import standin

U = 2.0 ** -24
LOG2E = 1.4426950408889634
PREDS = ("epsilon", "v_prediction", "sample")
PRED_CODE = {"epsilon": 0, "v_prediction": 1, "sample": 2}
HALF_ULP = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
# fp32 roundings on the longest path of one degraded value: x0 5 (two coefficients, product, difference, quotient), the two
# blur passes 9 + 9 fused multiply-adds, eps 5, the re-noising 5 (two coefficients, two products, the sum): 33
ROUNDINGS = 33


# ---------------------------------------------------------------------------------------------------
# key mass
# ---------------------------------------------------------------------------------------------------
def _heads(t, n, h):
    B, _, C = t.shape
    return t.double().cpu().numpy()[:, :n].reshape(B, n, h, C // h).transpose(0, 2, 1, 3)


def key_mass64(q, k, h, Mq, Mk, scale):
    """float64 sum_i mean_head softmax(q k^T scale)[i, :] on the given (16-bit) operands: (B, Mk)."""
    s = _heads(q, Mq, h) @ _heads(k, Mk, h).transpose(0, 1, 3, 2) * scale
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return p.mean(1).sum(1)


def score_bound(q, k, h, Mq, Mk, scale):
    """(A, |score|max), both in log2 units: A = max over (sample, head, query, key) of sum_c |q_c k_c| scale log2(e), the
    magnitude sum behind a score (softmax_corners.score_term's A), and the largest |score| itself (score_absmax)."""
    qh, kh = _heads(q, Mq, h), _heads(k, Mk, h).transpose(0, 1, 3, 2)
    return float((np.abs(qh) @ np.abs(kh)).max()) * scale * LOG2E, float(np.abs(qh @ kh).max()) * scale * LOG2E


def mass_bound(Mq, Mk, d, A, score_max):
    """The RELATIVE bound of a key mass (every term is non-negative, so the errors of the terms add up to at most the bound
    times the sum).  A probability p = e_j / sum e of an fp32 evaluation carries (Mk + 8) 2^-24 p -- the project's bound of
    the map: Mk terms in the denominator, a handful of roundings on the score, the head mean; the column sum of Mq such
    terms adds at most Mq 2^-24 of itself.  Only where the operands' |score|max exceeds 16 log2 units (softmax_corners.bar's
    rule) softmax_corners.score_term's 4 ln 2 (d + 4) 2^-24 A p is added."""
    term = 4.0 * math.log(2.0) * (d + 4) * A if score_max > 16.0 else 0.0
    return ((Mk + 8) + Mq + term) * U


def mass_operands(B, h, Mq, Mk, d, dtype, seed, Mqp=None, Mkp=None, logit_std=2.5):
    """q (B, Mqp, h d), k (B, Mkp, h d) in ``dtype``, N(0, g^2) with g chosen so that q . k d^-0.5 has standard deviation
    ``logit_std``: that spreads the masses well away from 1."""
    g = torch.Generator().manual_seed(seed)
    gain = math.sqrt(logit_std)
    q = (torch.randn(B, Mqp or Mq, h * d, generator=g) * gain).to(dtype)
    k = (torch.randn(B, Mkp or Mk, h * d, generator=g) * gain).to(dtype)
    return q, k


# ---------------------------------------------------------------------------------------------------
# degrade
# ---------------------------------------------------------------------------------------------------
def taps64(r, sigma):
    """The 2 r + 1 taps exp(-0.5 (k / sigma)^2) in float64, normalised to sum 1, THEN rounded to fp32 (as float64 values)."""
    w = np.exp(-0.5 * (np.arange(-r, r + 1, dtype=np.float64) / sigma) ** 2)
    return (w / w.sum()).astype(np.float32).astype(np.float64)


def reflect_index(n, r):
    """(n, 2 r + 1) source indices of torch's "reflect" padding (the edge is not repeated): row i reads i - r .. i + r."""
    i = np.arange(n)[:, None] + np.arange(-r, r + 1)[None, :]
    i = np.abs(i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def blur64(x, taps):
    """The separable blur of (..., H, W) float64 planes: horizontal pass, then vertical."""
    r = len(taps) // 2
    H, W = x.shape[-2:]
    hor = (x[..., :, reflect_index(W, r)] * taps).sum(-1)
    return (hor[..., reflect_index(H, r), :] * taps[:, None]).sum(-2)


def upsample_nearest(m, H, W):
    """(F, h_m, w_m) -> (F, H, W) with the integer rule: source index floor(y * h_m / H)."""
    h_m, w_m = m.shape[-2:]
    return m[..., (np.arange(H) * h_m) // H, :][..., (np.arange(W) * w_m) // W]


def predict64(x, m, pred, sa, sb):
    """(x0, eps, |x0| terms, |eps| terms) of the three prediction types."""
    ax, am = np.abs(x), np.abs(m)
    if pred == "epsilon":
        return (x - sb * m) / sa, m, (ax + sb * am) / sa, am
    if pred == "v_prediction":
        return sa * x - sb * m, sa * m + sb * x, sa * ax + sb * am, sa * am + sb * ax
    return m, (x - sa * m) / sb, am, (ax + sa * am) / sb


def degrade64(x, m, mass, h_m, w_m, pred, sa, sb, taps, threshold=1.0):
    """float64 degrade of one chunk: x, m (F, C, H, W) float64 arrays (the chunk's rows of the latents, the chosen group's
    model output), mass (F, >= h_m w_m) float32.  Returns (out, A, mask): A the magnitude sum of out's terms, mask bool
    (F, H, W).  The comparison is made on the fp32 mass against the fp32 threshold, as the kernel makes it."""
    F_, C, H, W = x.shape
    x0, eps, a0, ae = predict64(x, m, pred, sa, sb)
    on = np.asarray(mass, dtype=np.float32)[:, :h_m * w_m].reshape(F_, h_m, w_m) > np.float32(threshold)
    mask = upsample_nearest(on, H, W)
    sel = mask[:, None].repeat(C, 1)
    deg = np.where(sel, blur64(x0, taps), x0)
    adeg = np.where(sel, blur64(a0, taps), a0)
    return sa * deg + sb * eps, sa * adeg + sb * ae, mask


def degrade_tol(ref, A, dtype):
    """Counted fp32 roundings times 2^-24 times the magnitude sum of the terms, plus half an ulp of the output dtype."""
    return HALF_ULP[dtype] * np.abs(ref) + ROUNDINGS * U * A


# ---------------------------------------------------------------------------------------------------
# a mid block
# ---------------------------------------------------------------------------------------------------
B, FRAMES, LATENT, TOKENS, C_MID, HEADS = 2, 2, (64, 64), (8, 8), 1280, 8
MID_NAME = "mid_block.attentions.0.transformer_blocks.0"


class _Mid(torch.nn.Module):
    def __init__(self, C, heads, cond_dim):
        super().__init__()
        self.attentions = torch.nn.ModuleList([standin._Attn2D(C, heads, True, cond_dim)])


class StoringSelfProcessor:
    """What SAG installs on attn1 today: a processor of a name the fused path does not accept."""


class MidBlock(standin.ModelMixin):
    """A UNet stand-in that is its mid block: one full stand-in block at ``mid_block.attentions.0.transformer_blocks.0``,
    seeded like attention_maps_standin.OneBlock (2-D weights N(0, 1 / fan_in) from ``seed``, the Linear biases from a
    generator of their own); ``computing_self``: attn1 computes itself and carries a storing processor (the module path)."""

    def __init__(self, C=C_MID, heads=HEADS, seed=0, computing_self=False):
        super().__init__()
        self.mid_block = _Mid(C, heads, AM.COND_DIM)
        if computing_self:
            self.block.attn1 = AM.ComputingSelf(C, heads)
            self.block.attn1.processor = StoringSelfProcessor()
        g = torch.Generator().manual_seed(seed)
        gb = torch.Generator().manual_seed(seed + 7919)
        with torch.no_grad():
            for p in self.parameters():
                if p.ndim == 2:
                    p.copy_(torch.randn(p.shape, generator=g) * p.shape[-1] ** -0.5)
            for m in self.modules():
                if isinstance(m, torch.nn.Linear) and m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=gb) * m.in_features ** -0.5)

    @property
    def block(self):
        return self.mid_block.attentions[0].transformer_blocks[0]

    def set_size(self, latent_hw):
        self._tome_info["size"] = latent_hw


def patched(dtype, device, latent=LATENT, C=C_MID, **kw):
    """A fresh MidBlock through apply_patch (max_downsample 2: a site 8 x down does not merge)."""
    import vidtome_amd
    unet = MidBlock(C, **kw).to(device=device, dtype=dtype)
    torch.manual_seed(123)
    vidtome_amd.apply_patch(unet, local_merge_ratio=0.5, merge_global=True, global_merge_ratio=0.5, batch_size=B)
    unet.set_size(latent)
    return unet


def inputs(dtype, device, tokens=TOKENS[0] * TOKENS[1], C=C_MID, frames=B * FRAMES, seed=70):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(frames, tokens, C, generator=g).to(device=device, dtype=dtype)
    cond = torch.randn(frames, AM.COND, AM.COND_DIM, generator=g).to(device=device, dtype=dtype)
    return h, cond
