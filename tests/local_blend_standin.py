"""Stand-ins and references shared by the LocalBlend tests (tests/test_gpu_local_blend.py, tests/test_local_blend_host.py):
two full tests/standin.py blocks of one resolution behind a UNet-shaped ``ModelMixin`` root (``pnp.register_time`` walks
up_blocks / attentions / transformer_blocks), the torch restatement of vtm_local_blend's formula, and a literal
transcription of Prompt-to-Prompt's ``LocalBlend.__call__`` tail.

Like tests/cross_control_standin.py the blocks sit at a site that does not merge (the latent is 4 x 4 times the token
grid), so attn1 is per-frame attention; LocalBlend is about attn2, which never merges."""
import torch
import torch.nn.functional as F

import cross_control_standin as CC
import standin

NUM_INPUTS, FRAMES, GRID, COND, COND_DIM, HEADS = 3, 2, (8, 8), 77, 768, 8
TOKENS = GRID[0] * GRID[1]
LATENT = (GRID[0] * 4, GRID[1] * 4)
BLOCKS = ["up_blocks.0.attentions.0.transformer_blocks.0", "up_blocks.1.attentions.0.transformer_blocks.0"]


class BlendUNet(standin.ModelMixin):
    """Two full stand-in blocks (attn1's and attn2's module forward raise) where ``pnp.register_time`` finds them, 2-D
    weights N(0, 1 / fan_in) from ``seed``."""

    def __init__(self, C, heads=HEADS, seed=0):
        super().__init__()
        self.up_blocks = torch.nn.ModuleList([standin._UpBlock(C, heads, 1, 1, True, COND_DIM) for _ in BLOCKS])
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in self.parameters():
                if p.ndim == 2:
                    p.copy_(torch.randn(p.shape, generator=g) * p.shape[-1] ** -0.5)

    @property
    def blocks(self):
        return [up.attentions[0].transformer_blocks[0] for up in self.up_blocks]

    def set_size(self, latent_hw):
        self._tome_info["size"] = latent_hw


def patched(C, dtype, device, **kw):
    import vidtome_amd
    unet = BlendUNet(C, **kw).to(device=device, dtype=dtype)
    vidtome_amd.apply_patch(unet, batch_size=NUM_INPUTS)
    unet.set_size(LATENT)
    return unet


def inputs(C, dtype, device, seed=70, n=NUM_INPUTS * FRAMES):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(n, TOKENS, C, generator=g).to(device=device, dtype=dtype)
    cond = torch.randn(n, COND, COND_DIM, generator=g).to(device=device, dtype=dtype)
    return h, cond


def forward(unet, h, cond, **kw):
    """Every block on the same hidden states; the list of their outputs."""
    with torch.no_grad():
        return [blk(h, encoder_hidden_states=cond, **kw) for blk in unet.blocks]


def words(K=COND, seed=11):
    """{0: a 0 / 1 row on three words, 2: a signed N(0, 1) row}: the source and the cond group; the uncond group has none."""
    g = torch.Generator().manual_seed(seed)
    w0 = torch.zeros(K)
    w0[[2, 5, K - 1]] = 1.0
    return {0: w0, 2: torch.randn(K, generator=g)}


# ---------------------------------------------------------------------------------------------------
# the blend tail
# ---------------------------------------------------------------------------------------------------
def blend_formula(acc, x, x_src, pool, threshold):
    """vtm_local_blend's formula in torch: acc (G, F, h, w) fp32, x / x_src (F, C, H, W) -> (out, mask bool (F, H, W)).
    pooled > fp32(threshold) * max in fp32, OR over the groups, a select."""
    G, Fr, h, w = acc.shape
    H, W = x.shape[2:]
    pooled = F.max_pool2d(acc, 2 * pool + 1, stride=1, padding=pool) if pool else acc
    up = pooled.repeat_interleave(H // h, dim=2).repeat_interleave(W // w, dim=3)      # nearest: cell = y h / H
    cut = torch.tensor(threshold, dtype=torch.float32, device=acc.device) * acc.amax(dim=(2, 3))
    mask = (up > cut[:, :, None, None]).any(dim=0)
    return torch.where(mask[:, None], x, x_src), mask


def p2p_local_blend(maps, x_t, k, threshold):
    """Prompt-to-Prompt's ``LocalBlend.__call__`` from its pooling on, written as P2P writes it: ``maps`` (B, 1, h, w) is the
    word-weighted, summed and averaged map of every prompt, ``x_t`` (B, C, H, W) the latents of the B prompts, prompt 0 the
    source.  Returns (x_t blended, mask (1, 1, H, W) as float)."""
    mask = F.max_pool2d(maps, (k * 2 + 1, k * 2 + 1), (1, 1), padding=(k, k))
    mask = F.interpolate(mask, size=(x_t.shape[2:]))
    mask = mask / mask.max(2, keepdims=True)[0].max(3, keepdims=True)[0]
    mask = mask.gt(threshold)
    mask = (mask[:1] + mask[1:]).float()
    x_t = x_t[:1] + mask * (x_t - x_t[:1])
    return x_t, mask


def edit_spec(name):
    """Two of tests/cross_control_standin.py's specs: a word swap, and a refinement that is re-weighted."""
    return CC.specs()[{"replace": "replace", "refine+reweight": "refine_reweight"}[name]]
