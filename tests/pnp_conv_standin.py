"""Stand-in for the Diffusers ResnetBlock2D that `register_conv_control` (utils/pnp_utils.py:108-172) patches: the
attributes its closure reads, small enough for a fixture (tests/golden/pnp_conv.npz), plus the case list shared by the
fixture script and the tests.  Weights and inputs are multiples of 1/64 (exact in fp32 and fp16)."""
import math

import numpy as np
import torch
import torch.nn as nn

GROUPS, C_IN, C_OUT, TEMB, HEIGHT, WIDTH = 4, 24, 16, 8, 3, 5
SCHEDULE = (981, 961, 941)          # injection timesteps of every case
ROOT2 = math.sqrt(2.0)
FIELDS = ("num_inputs", "B", "t", "shortcut", "scale")
# num_inputs 3 and 2; t in the schedule, not in it, and 1000 (not in it); with and without the 1x1 conv_shortcut;
# output_scale_factor 1 and sqrt 2; B = 7 with three inputs: the seventh row keeps its own result
CASES = (
    (3, 6, 961, True, 1.0),
    (3, 6, 500, False, ROOT2),
    (3, 6, 1000, True, ROOT2),
    (2, 6, 981, False, 1.0),
    (3, 7, 941, True, ROOT2),
    (2, 6, 500, True, 1.0),
    (3, 7, 961, False, 1.0),
)


def injects(t):
    return t in SCHEDULE or t == 1000


def surviving_rows(num_inputs, B, t):
    """Rows of the main branch whose result is used (what a hook on conv1 must see)."""
    if not injects(t):
        return B
    sbs = B // num_inputs
    return sbs + B - min(num_inputs, 3) * sbs


def _grid(shape, gen, spread=1.0, offset=0.0):
    return torch.round((torch.randn(shape, generator=gen) * spread + offset) * 64) / 64


class StandinResnet(nn.Module):
    """norm1 -> SiLU -> conv1 -> + time_emb_proj(SiLU(temb)) -> norm2 -> SiLU -> dropout -> conv2, a 1x1 conv_shortcut when
    ``shortcut`` (else the input itself, C_OUT channels in and out), divided by ``output_scale_factor``."""

    def __init__(self, shortcut=True, scale=1.0, time_embedding_norm="default", dropout=0.0, seed=11,
                 sizes=(GROUPS, C_IN, C_OUT, TEMB)):
        super().__init__()
        groups, c_in, c_out, temb = sizes               # (the measurement tool builds the SD-size block)
        cin = c_in if shortcut else c_out
        proj = c_out * (2 if time_embedding_norm == "scale_shift" else 1)
        self.norm1 = nn.GroupNorm(groups, cin, eps=1e-5)
        self.conv1 = nn.Conv2d(cin, c_out, 3, padding=1)
        self.time_emb_proj = nn.Linear(temb, proj)
        self.norm2 = nn.GroupNorm(groups, c_out, eps=1e-5)
        self.dropout = nn.Dropout(dropout)
        self.conv2 = nn.Conv2d(c_out, c_out, 3, padding=1)
        self.conv_shortcut = nn.Conv2d(cin, c_out, 1) if shortcut else None
        self.nonlinearity = nn.SiLU()
        self.upsample = self.downsample = None
        self.time_embedding_norm = time_embedding_norm
        self.output_scale_factor = scale
        gen = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name.startswith("norm"):         # non-trivial affine parameters
                    p.copy_(_grid(p.shape, gen, 0.3, 1.0 if name.endswith("weight") else 0.0))
                else:
                    fan = p[0].numel() if p.dim() > 1 else 16
                    p.copy_(_grid(p.shape, gen, 1.5 / math.sqrt(fan)))

    def forward(self, input_tensor, temb=None):
        h = self.conv1(self.nonlinearity(self.norm1(input_tensor)))
        if temb is not None:
            h = h + self.time_emb_proj(self.nonlinearity(temb))[:, :, None, None]
        h = self.conv2(self.dropout(self.nonlinearity(self.norm2(h))))
        sc = input_tensor if self.conv_shortcut is None else self.conv_shortcut(input_tensor)
        return (sc + h) / self.output_scale_factor


class _Holder:
    pass


def model_around(resnet):
    """An object with the path the registration walks: model.unet.up_blocks[1].resnets[1]."""
    model, block = _Holder(), _Holder()
    model.unet = _Holder()
    block.resnets = [None, resnet]
    model.unet.up_blocks = [None, block]
    return model


def inputs(B, shortcut, seed=5):
    gen = torch.Generator().manual_seed(seed + 10 * B + int(shortcut))
    x = _grid((B, C_IN if shortcut else C_OUT, HEIGHT, WIDTH), gen)
    temb = _grid((B, TEMB), gen)
    return x, temb


def load_weights(resnet, z, shortcut):
    """Copy the recorded weights of the variant (w1: with conv_shortcut, w0: without) into a stand-in."""
    with torch.no_grad():
        for name, p in resnet.named_parameters():
            p.copy_(torch.from_numpy(np.asarray(z[f"w{int(shortcut)}/{name}"])).to(p.dtype))
    return resnet


def closure_errors(n, z, dtype, device="cuda"):
    """Case ``n`` of the fixture on ``device`` in ``dtype``: the fused closure and the plain-torch fallback (the route
    check forced to refuse), each against the reference's recorded fp32 output.  Returns the two max abs errors, the
    spacing of ``dtype`` at the output's max magnitude, and the rows conv1 saw on each route."""
    from vidtome_amd import pnp
    num_inputs, B, t, shortcut, scale = CASES[n]
    want = torch.from_numpy(np.asarray(z[f"{n}/out"])).double()
    x, temb = (torch.from_numpy(np.asarray(z[f"{k}/B{B}s{int(shortcut)}"])).to(device=device, dtype=dtype) for k in ("x", "temb"))
    resnet = load_weights(StandinResnet(shortcut=shortcut, scale=scale), z, shortcut).eval().to(device=device, dtype=dtype)
    pnp.register_conv_control(model_around(resnet), list(SCHEDULE), num_inputs)
    resnet.t = t
    seen = []
    hook = resnet.conv1.register_forward_hook(lambda m, a, o: seen.append(a[0].shape[0]))
    route = pnp._fused_route
    errs = {}
    try:
        for name in ("fused", "module"):
            if name == "module":
                pnp._fused_route = lambda module, x: False
            with torch.no_grad():
                y = resnet.forward(x, temb)
            assert y.dtype == dtype and y.shape == want.shape
            errs[name] = float((y.double().cpu() - want).abs().max())
    finally:
        pnp._fused_route = route
        hook.remove()
    top = float(want.abs().max())
    mant = {torch.float32: 23, torch.float16: 10, torch.bfloat16: 7}[dtype]
    return {"e_fused": errs["fused"], "e_module": errs["module"], "ulp": 2.0 ** (math.floor(math.log2(top)) - mant),
            "out_max": top, "conv1_rows": seen}
