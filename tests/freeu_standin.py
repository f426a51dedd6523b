"""Not a test: what tests/test_freeu_host.py and tests/test_gpu_freeu.py share.

* ``freeu64``: the float64 restatement of vtm_freeu's contract (include/vidtome_hip.h), and ``skip_fft64``, the FFT form of
  its skip-plane filter (torch.fft in complex128, Diffusers' mask, .real);
* the tests' error bounds, built from ``_lib.freeu_rounding_counts``;
* stand-in up blocks named like Diffusers' (``UpBlock2D``, ``CrossAttnUpBlock2D``): ``resnets``, ``resolution_idx``, a forward
  that pops the skip tuple and concatenates, and Diffusers' own ``if s1 and s2 and b1 and b2`` torch branch in front of the
  concatenation.  Their resnets record their input and return a cheap deterministic function of it."""
import math

import numpy as np
import torch

U24 = 2.0 ** -24
U_T = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 0.0}
T_T = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0, torch.float32: 0.0}
DTYPES = (torch.float16, torch.bfloat16, torch.float32)

# (C_h, C_s, H, W) of the GPU tests' fixed cases; the boundary shapes come from boundary_planes()
SMALL = [(8, 4, 8, 8), (6, 3, 2, 2), (5, 3, 5, 7), (8, 4, 12, 20)]
LARGEST = (2, 2, 128, 128)
IDENTITY_ONLY = [(2, 2), (2, 3), (3, 2), (5, 7), (12, 20), (64, 64)]


# ---- float64 restatements -------------------------------------------------------------------------------------------------
def skip64(v, s):
    """The skip-plane filter on v (..., H, W) float64: v + (s - 1) / P * the projection on the bins ky, kx in {0, -1}."""
    v = np.asarray(v, np.float64)
    H, W = v.shape[-2:]
    a = (2.0 * np.pi * np.arange(H) / H)[:, None]
    b = (2.0 * np.pi * np.arange(W) / W)[None, :]
    waves = [np.ones((H, W)), np.cos(a) + 0 * b, np.sin(a) + 0 * b, np.cos(b) + 0 * a, np.sin(b) + 0 * a, np.cos(a + b),
             np.sin(a + b)]
    proj = np.zeros_like(v)
    for w in waves:
        proj = proj + (v * w).sum((-2, -1), keepdims=True) * w
    return v + (s - 1.0) / (H * W) * proj


def skip_fft64(v, s):
    """Re ifftn(ifftshift(mask * fftshift(fftn(v)))) in complex128 with mask = s on [H//2 - 1 : H//2 + 1, W//2 - 1 : W//2 + 1]."""
    t = torch.as_tensor(np.asarray(v, np.float64))
    H, W = t.shape[-2:]
    f = torch.fft.fftshift(torch.fft.fftn(t.to(torch.complex128), dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(t.shape, dtype=torch.float64)
    mask[..., H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = s
    return torch.fft.ifftn(torch.fft.ifftshift(f * mask, dim=(-2, -1)), dim=(-2, -1)).real.numpy()


def gain64(X, C_h, b, version):
    """The backbone gain g (B, 1, H, W) float64 and, for version 2, (max - min, max_p mean_c |X|) per sample."""
    X = np.asarray(X, np.float64)
    if version == 1:
        return np.full((X.shape[0], 1) + X.shape[2:], float(b)), None
    m = X[:, :C_h].mean(1, keepdims=True)
    lo, hi = m.min((2, 3), keepdims=True), m.max((2, 3), keepdims=True)
    spread = hi - lo
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where(spread == 0, 1.0, 1.0 + (b - 1.0) * (m - lo) / np.where(spread == 0, 1.0, spread))
    mag = np.abs(X[:, :C_h]).mean(1, keepdims=True).max((2, 3), keepdims=True)
    return g, (spread, mag)


def freeu64(X, C_h, b, s, version=1):
    """The whole contract on X (B, C_h + C_s, H, W), float64 out."""
    X = np.asarray(X, np.float64)
    out = X.copy()
    g, _ = gain64(X, C_h, b, version)
    out[:, :C_h // 2] = X[:, :C_h // 2] * g
    out[:, C_h:] = skip64(X[:, C_h:], s)
    return out


# ---- the bounds (the issue's, built from the kernel's counted roundings) -------------------------------------------------
def bounds(X, C_h, b, s, version, dtype, counts):
    """Per-element bound on |out - freeu64| for the kernel's output in ``dtype``: float64 array of X's shape (0 on the untouched
    range: those bytes must be the input's).  ``counts`` = _lib.freeu_rounding_counts(P, C_h)."""
    X = np.asarray(X, np.float64)
    K_s, K_m = counts
    ref = freeu64(X, C_h, b, s, version)
    P = X.shape[2] * X.shape[3]
    out = np.zeros_like(X)
    v = np.abs(X[:, C_h:])
    out[:, C_h:] = U_T[dtype] * np.abs(ref[:, C_h:]) + T_T[dtype] \
        + K_s * U24 * (v + abs(s - 1.0) * 4.0 * v.sum((2, 3), keepdims=True) / P)
    h = C_h // 2
    out[:, :h] = U_T[dtype] * np.abs(ref[:, :h]) + T_T[dtype] + 4.0 * U24 * np.abs(ref[:, :h])
    if version == 2:
        _, (spread, mag) = gain64(X, C_h, b, version)
        delta = K_m * U24 * mag
        with np.errstate(invalid="ignore", divide="ignore"):
            extra = np.where(spread == 0, 0.0, 3.0 * delta / np.where(spread == 0, 1.0, spread)) + 2.0 ** -22
        out[:, :h] += np.abs(X[:, :h]) * abs(b - 1.0) * extra
    return out, ref


def well_spread(X, C_h):
    """Version 2's input condition: max - min >= 0.25 max_p mean_c |X| for every sample (checked before the launch)."""
    _, (spread, mag) = gain64(X, C_h, 1.5, 2)
    return bool((spread >= 0.25 * mag).all())


def make_input(B, C_h, C_s, H, W, dtype, seed):
    """N(0, 1) plus, on the backbone channels, a per-pixel ramp over [-1, 1] whose direction differs per sample: the mean map
    then spreads over about 2 while mean |X| stays about 1.  Returned rounded to ``dtype`` (CPU)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C_h + C_s, H, W, generator=g, dtype=torch.float64)
    line = torch.linspace(-1.0, 1.0, H * W, dtype=torch.float64)
    for n in range(B):
        ramp = line.reshape(1, 1, H, W) if n % 2 == 0 else -line.reshape(1, 1, W, H).transpose(-1, -2)   # row- / column-major
        x[n:n + 1, :C_h] += ramp * (1.0 + 0.25 * n)
    return x.to(dtype)


# ---- shapes on both sides of every form boundary, read from the library's rule -------------------------------------------
def _most_square(P):
    best = None
    for h in range(2, int(math.isqrt(P)) + 1):
        if P % h == 0:
            best = (h, P // h)
    return best


def boundary_planes(lanes, max_plane):
    """[(H, W)]: for every P where ``lanes(P)`` changes, the largest factorable plane at or below the boundary and the smallest
    above it (H, W >= 2, the most square factorisation)."""
    out = []
    for P in range(4, max_plane):
        if lanes(P) != lanes(P + 1):
            lo = next(_most_square(q) for q in range(P, 3, -1) if _most_square(q))
            hi = next(_most_square(q) for q in range(P + 1, max_plane + 1) if _most_square(q))
            assert lanes(lo[0] * lo[1]) == lanes(P) and lanes(hi[0] * hi[1]) == lanes(P + 1)
            out += [lo, hi]
    return out


# ---- stand-in up blocks ----------------------------------------------------------------------------------------------------
def fourier_filter_torch(x_in, scale):
    """Diffusers' chain on the skip features, restated: upcast, fftn, fftshift, a mask of ``scale`` on the 2 x 2 centre,
    ifftshift, ifftn, .real, cast back.  (Always upcast to fp32 here: half-precision FFTs are not what is under test.)"""
    x = x_in.to(torch.float32)
    H, W = x.shape[-2:]
    f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(x.shape, device=x.device)
    mask[..., H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = scale
    f = torch.fft.ifftshift(f * mask, dim=(-2, -1))
    return torch.fft.ifftn(f, dim=(-2, -1)).real.to(x_in.dtype)


class RecordingResnet(torch.nn.Module):
    """Keeps a copy of its input; returns (first out_channels planes + last out_channels planes) / 2."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.seen = []

    def forward(self, input_tensor, temb=None):
        assert input_tensor.shape[1] == self.in_channels
        self.seen.append(input_tensor.detach().clone())
        o = self.out_channels
        return ((input_tensor[:, :o] + input_tensor[:, -o:]) * 0.5).contiguous()


class _UpBlock(torch.nn.Module):
    def __init__(self, resolution_idx, prev_channels, skip_channels, out_channels, upsample):
        super().__init__()
        ins = [prev_channels] + [out_channels] * (len(skip_channels) - 1)
        self.resnets = torch.nn.ModuleList(RecordingResnet(i + k, out_channels) for i, k in zip(ins, skip_channels))
        self.resolution_idx, self.upsample = resolution_idx, upsample

    def _run(self, hidden_states, res_hidden_states_tuple, temb):
        enabled = getattr(self, "s1", None) and getattr(self, "s2", None) and getattr(self, "b1", None) \
            and getattr(self, "b2", None)
        for resnet in self.resnets:
            res = res_hidden_states_tuple[-1]
            res_hidden_states_tuple = res_hidden_states_tuple[:-1]
            if enabled and self.resolution_idx in (0, 1):
                b, s = (self.b1, self.s1) if self.resolution_idx == 0 else (self.b2, self.s2)
                half = hidden_states.shape[1] // 2
                hidden_states = hidden_states.clone()
                hidden_states[:, :half] = hidden_states[:, :half] * b
                res = fourier_filter_torch(res, s)
            hidden_states = torch.cat([hidden_states, res], dim=1)
            hidden_states = resnet(hidden_states, temb)
        if self.upsample:
            hidden_states = hidden_states.repeat_interleave(2, -1).repeat_interleave(2, -2).contiguous()
        return hidden_states


class UpBlock2D(_UpBlock):
    def forward(self, hidden_states, res_hidden_states_tuple, temb=None, upsample_size=None):
        return self._run(hidden_states, res_hidden_states_tuple, temb)


class CrossAttnUpBlock2D(_UpBlock):
    def forward(self, hidden_states, res_hidden_states_tuple, temb=None, encoder_hidden_states=None, upsample_size=None):
        return self._run(hidden_states, res_hidden_states_tuple, temb)


class ModelMixin(torch.nn.Module):
    pass


class StandinUNet(ModelMixin):
    """Two up blocks in the SD-1.5 pattern the issue names, channels scaled by ``unit`` / 320 (unit = 320: 1280 | 1280,
    1280 | 1280, 1280 | 640, then 1280 | 640, 640 | 640, 640 | 320), the first at ``size`` x ``size`` with an upsampler behind it,
    the second at twice that; a third block that FreeU must leave alone."""

    def __init__(self, unit=8, size=8):
        super().__init__()
        u, self.size, self.unit = unit, size, unit
        self.up_blocks = torch.nn.ModuleList([
            UpBlock2D(0, 4 * u, (4 * u, 4 * u, 2 * u), 4 * u, upsample=True),
            CrossAttnUpBlock2D(1, 4 * u, (2 * u, 2 * u, u), 2 * u, upsample=False),
            UpBlock2D(2, 2 * u, (u,), u, upsample=False)])

    def operands(self, B, dtype, device, seed=3):
        g = torch.Generator().manual_seed(seed)
        u, z = self.unit, self.size
        mk = lambda c, side: torch.randn(B, c, side, side, generator=g).to(dtype).to(device)
        sample = mk(4 * u, z)
        # the skip tuple is popped from its END: resnet 0 of block 0 takes the last entry
        skips = (mk(u, 2 * z), mk(u, 2 * z), mk(2 * u, 2 * z), mk(2 * u, 2 * z), mk(2 * u, z), mk(4 * u, z), mk(4 * u, z))
        return sample, skips

    def forward(self, sample, skips):
        h = self.up_blocks[0](sample, skips[-3:])                                              # positional
        h = self.up_blocks[1](hidden_states=h, res_hidden_states_tuple=skips[-6:-3], encoder_hidden_states=None)
        return self.up_blocks[2](h, skips[-7:-6])

    def recorded(self):
        """[(block index, resnet index, input)] of the last forward, then forgotten."""
        out = []
        for i, blk in enumerate(self.up_blocks):
            for j, r in enumerate(blk.resnets):
                for t in r.seen:
                    out.append((i, j, t))
                r.seen = []
        return out
