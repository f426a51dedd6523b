"""Stand-ins and float64 references shared by the cross-attention control tests (tests/test_gpu_cross_control.py,
tests/test_cross_control_host.py): Prompt-to-Prompt's three controllers restated in float64 the way P2P writes them, one
full tests/standin.py block behind a UNet-shaped ``ModelMixin`` root (``pnp.register_time`` walks up_blocks / attentions /
transformer_blocks), and the float64 evaluation of that block with the controllers applied to attn2's per-head
probabilities.

The block sits at a site that does not merge (the latent is 4 x 4 times the token grid: downsample 4 > max_downsample 2,
like SD's mid block), so attn1 is per-frame attention and the whole block has a closed float64 form; the control is about
attn2, which never merges."""
import torch
import torch.nn.functional as F

import standin

NUM_INPUTS, FRAMES, GRID, COND, COND_DIM, HEADS = 3, 2, (7, 10), 77, 768, 8
TOKENS = GRID[0] * GRID[1]                  # 70: no multiple of 8, a partial query block
LATENT = (GRID[0] * 4, GRID[1] * 4)
BLOCK = "up_blocks.0.attentions.0.transformer_blocks.0"


# ---------------------------------------------------------------------------------------------------
# Prompt-to-Prompt's controllers (ptp_utils / the notebook's AttentionReplace, AttentionRefine, AttentionReweight)
# ---------------------------------------------------------------------------------------------------
def replace_cross_attention(spec, attn_base, att_replace):
    """``attn_base`` (h, P, K): the source sample's probabilities; ``att_replace`` (1, h, P, K): the edited sample's own.
    ``spec``: {"kind": "replace", "mapper": (K, K)} | {"kind": "refine", "index": (K,) ints, "alphas": (K,)}, optionally
    "equalizer": (K,) -- AttentionReweight with the first as its ``prev_controller`` -- or {"kind": "reweight",
    "equalizer"} alone."""
    kind = spec["kind"]
    if kind == "replace":
        mapper = torch.as_tensor(spec["mapper"], dtype=torch.float64)[None]                   # (1, K, K)
        out = torch.einsum('hpw,bwn->bhpn', attn_base, mapper)
    elif kind == "refine":
        mapper = torch.as_tensor(spec["index"]).long()[None]                                   # (1, K); -1 reads the last word
        alphas = torch.as_tensor(spec["alphas"], dtype=torch.float64).reshape(1, 1, 1, -1)
        attn_base_replace = attn_base[:, :, mapper].permute(2, 0, 1, 3)
        out = attn_base_replace * alphas + att_replace * (1 - alphas)
    elif kind == "reweight":
        out = attn_base[None, :, :, :]
    else:
        raise ValueError(kind)
    if spec.get("equalizer") is not None:
        equalizer = torch.as_tensor(spec["equalizer"], dtype=torch.float64).reshape(1, -1)
        out = out * equalizer[:, None, None, :]
    return out


def controlled_probs(spec, attn_base, attn_own):
    """AttentionControlEdit.forward on cross-attention: (h, P, K) source and own probabilities -> the edited ones."""
    K = attn_base.shape[-1]
    alpha_words = torch.as_tensor(spec.get("alpha_words", 1.0), dtype=torch.float64).reshape(-1)
    alpha_words = (alpha_words.expand(K) if alpha_words.numel() == 1 else alpha_words).reshape(1, 1, 1, K)
    attn_new = replace_cross_attention(spec, attn_base, attn_own[None]) * alpha_words + (1 - alpha_words) * attn_own[None]
    return attn_new[0]


def edit_of(spec):
    """The ``vidtome_amd.CrossEdit`` that restates ``spec``."""
    from vidtome_amd import CrossEdit
    aw = spec.get("alpha_words", 1.0)
    if spec["kind"] == "replace":
        e = CrossEdit.replace(spec["mapper"], aw)
    elif spec["kind"] == "refine":
        e = CrossEdit.refine(spec["index"], spec["alphas"], aw)
    else:
        e = CrossEdit.replace(torch.eye(len(spec["equalizer"])), aw)
    return e.reweight(spec["equalizer"]) if spec.get("equalizer") is not None else e


def specs(K=COND, seed=4):
    """One spec per controller, fractional ``alpha_words``: a word swap whose mapper moves, splits and drops words; a
    refinement with inserted words (index -1, alpha 0) and shifted ones; the refinement re-weighted."""
    g = torch.Generator().manual_seed(seed)
    mapper = torch.eye(K, dtype=torch.float64)
    if K > 12:
        mapper[3:9] = 0
        mapper[3, 5], mapper[4, 3], mapper[5, 4] = 1.0, 1.0, 1.0         # three words change places
        mapper[6, 6], mapper[6, 7] = 0.5, 0.5                             # one word becomes two
        mapper[8, 8] = 1.0                                                # (word 7 is dropped)
    aw = 0.25 + 0.5 * torch.rand(K, generator=g, dtype=torch.float64)
    index = torch.arange(K)
    alphas = torch.ones(K, dtype=torch.float64)
    if K > 12:
        index[5:] = torch.arange(3, K - 2)                                # two inserted words shift the rest
        index[3:5] = -1
        alphas[3:5] = 0.0
        alphas[9] = 0.5
    eq = torch.ones(K, dtype=torch.float64)
    eq[K // 2] = 4.0
    eq[0] = -0.5
    if K > 2:
        eq[2] = 2.5
    return {"replace": {"kind": "replace", "mapper": mapper, "alpha_words": 0.7},
            "refine": {"kind": "refine", "index": index, "alphas": alphas, "alpha_words": aw},
            "refine_reweight": {"kind": "refine", "index": index, "alphas": alphas, "alpha_words": aw, "equalizer": eq}}


# ---------------------------------------------------------------------------------------------------
# the block
# ---------------------------------------------------------------------------------------------------
class ControlUNet(standin.ModelMixin):
    """One full stand-in block (attn1's and attn2's module forward raise) where ``pnp.register_time`` finds it, 2-D weights
    N(0, 1 / fan_in) from ``seed``."""

    def __init__(self, C, heads=HEADS, seed=0):
        super().__init__()
        self.up_blocks = torch.nn.ModuleList([standin._UpBlock(C, heads, 1, 1, True, COND_DIM)])
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in self.parameters():
                if p.ndim == 2:
                    p.copy_(torch.randn(p.shape, generator=g) * p.shape[-1] ** -0.5)

    @property
    def block(self):
        return self.up_blocks[0].attentions[0].transformer_blocks[0]

    def set_size(self, latent_hw):
        self._tome_info["size"] = latent_hw


def patched(C, dtype, device, **kw):
    import vidtome_amd
    unet = ControlUNet(C, **kw).to(device=device, dtype=dtype)
    vidtome_amd.apply_patch(unet, batch_size=NUM_INPUTS)
    unet.set_size(LATENT)
    return unet


def inputs(C, dtype, device, K=COND, seed=70, n=NUM_INPUTS * FRAMES):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(n, TOKENS, C, generator=g).to(device=device, dtype=dtype)
    cond = torch.randn(n, K, COND_DIM, generator=g).to(device=device, dtype=dtype)
    return h, cond


def block64(blk, hidden, cond, edits=None, num_inputs=NUM_INPUTS):
    """float64 output (B F, N, C) of the stand-in block on 16-bit inputs, from the block's own modules: per-frame attn1,
    attn2 with the probabilities of group g replaced through ``controlled_probs(edits[g], ...)``, GEGLU feed-forward."""
    w = lambda m: m.weight.detach().double().cpu()
    lin = lambda m, x: x @ w(m).T + (0 if m.bias is None else m.bias.detach().double().cpu())
    ln = lambda n, x: F.layer_norm(x, x.shape[-1:], w(n), n.bias.detach().double().cpu(), n.eps)
    h, c = hidden.double().cpu(), cond.double().cpu()
    n = h.shape[0]
    sh = lambda t, heads: t.view(n, t.shape[1], heads, -1).transpose(1, 2)                    # (n, heads, rows, d)
    a1, a2 = blk.attn1, blk.attn2
    x1 = ln(blk.norm1, h)
    p1 = torch.softmax(sh(lin(a1.to_q, x1), a1.heads) @ sh(lin(a1.to_k, x1), a1.heads).transpose(-1, -2) * a1.scale, dim=-1)
    h = lin(a1.to_out[0], (p1 @ sh(lin(a1.to_v, x1), a1.heads)).transpose(1, 2).reshape(h.shape)) + h
    x2 = ln(blk.norm2, h)
    p2 = torch.softmax(sh(lin(a2.to_q, x2), a2.heads) @ sh(lin(a2.to_k, c), a2.heads).transpose(-1, -2) * a2.scale, dim=-1)
    if edits:
        fg = n // num_inputs
        own = p2.clone()
        for grp, spec in edits.items():
            for f in range(fg):
                p2[grp * fg + f] = controlled_probs(spec, own[f], own[grp * fg + f])
    h = lin(a2.to_out[0], (p2 @ sh(lin(a2.to_v, c), a2.heads)).transpose(1, 2).reshape(h.shape)) + h
    p = lin(blk.ff.net[0].proj, ln(blk.norm3, h))
    D = p.shape[-1] // 2
    return lin(blk.ff.net[2], p[..., :D] * F.gelu(p[..., D:])) + h
