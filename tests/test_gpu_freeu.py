"""vtm_freeu on the GPU against the float64 restatement of tests/freeu_standin.py.

Bounds (per element; u_T = 2^-11 / 2^-8 / 0 and t_T = 2^-25 / 0 / 0 for fp16 / bf16 / fp32; K_s, K_m from
_lib.freeu_rounding_counts, derived in csrc/freeu.hip's header):
    skip planes          u_T |ref| + t_T + K_s 2^-24 (|v| + |s - 1| 4 sum|v| / P)
    backbone, version 1  u_T |ref| + t_T + 4 2^-24 |ref|
    backbone, version 2  ... + |v| |b - 1| (3 delta / (max - min) + 2^-22),  delta = K_m 2^-24 max_p mean_c |X|
The torch chain of the stand-in blocks (Diffusers' branch restated: fp32 FFT there and back, one cast) is held to
    u_T |ref| + t_T + 16 log2(P) 2^-24 max(1, |s|) ||v||_2
per skip plane -- the normwise bound of a radix-2 FFT is about 5 log2(N) u ||v||_2 per transform (Higham, Accuracy and
Stability of Numerical Algorithms, 24.2), two 2-D transforms give 10 log2(P), and 16 leaves room for the twiddles of a library
FFT -- and to u_T |ref| + t_T on the backbone (one product in the model dtype)."""
import math

import numpy as np
import pytest
import torch

import freeu_standin as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                      # elements in front of and behind the tensor, in the same allocation
NAMES = {torch.float16: "fp16", torch.bfloat16: "bf16", torch.float32: "fp32"}


@pytest.fixture(scope="module")
def lib():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _launch(lib, x_cpu, C_h, b, s, version, guard=GUARD):
    """Run on a copy of x_cpu that sits between two guard strips of one allocation; returns the result (CPU) after checking
    that the guards kept their bits."""
    n = x_cpu.numel()
    buf = torch.full((n + 2 * guard,), 7.0, dtype=x_cpu.dtype, device=DEV)
    x = buf[guard:guard + n].view(x_cpu.shape)
    x.copy_(x_cpu)
    assert lib.freeu(x, C_h, b, s, version) is x
    host = buf.cpu()
    assert bool((host[:guard] == 7.0).all()) and bool((host[guard + n:] == 7.0).all()), "a guard strip was written"
    return host[guard:guard + n].view(x_cpu.shape).clone()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _check(lib, x_cpu, out, C_h, b, s, version, what):
    X = x_cpu.double().numpy()
    P = X.shape[2] * X.shape[3]
    bound, ref = S.bounds(X, C_h, b, s, version, x_cpu.dtype, lib.freeu_rounding_counts(P, C_h))
    err = np.abs(out.double().numpy() - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)
    h = C_h // 2
    print(f"{what}: worst error / bound  backbone {ratio[:, :h].max():.3f}  skip {ratio[:, C_h:].max():.3f}")
    assert bool((err[:, :h] <= bound[:, :h]).all()), (what, "backbone", float(ratio[:, :h].max()))
    assert bool((err[:, C_h:] <= bound[:, C_h:]).all()), (what, "skip", float(ratio[:, C_h:].max()))
    assert torch.equal(_bits(out[:, h:C_h]), _bits(x_cpu[:, h:C_h])), (what, "the untouched range changed")


def _shapes(lib):
    planes = S.boundary_planes(lib.freeu_lanes, lib.FREEU_MAX_PLANE)
    assert len(planes) == 6                                                    # three boundaries, a shape on each side
    return S.SMALL + [(4, 2, H, W) for H, W in planes] + [S.LARGEST]


@pytest.mark.parametrize("dtype", S.DTYPES, ids=lambda d: NAMES[d])
def test_every_form_against_float64(lib, dtype):
    """The fixed cases, a shape on each side of every form boundary (read from vtm_freeu_lanes) and the largest plane; both
    versions; B = 2 with different content per sample."""
    for C_h, C_s, H, W in _shapes(lib):
        x = S.make_input(2, C_h, C_s, H, W, dtype, seed=H * W + C_h)
        for version in (1, 2):
            if version == 2:
                assert S.well_spread(x.double().numpy(), C_h), (C_h, C_s, H, W)
            out = _launch(lib, x, C_h, 1.6, 0.2, version)
            _check(lib, x, out, C_h, 1.6, 0.2, version, f"{NAMES[dtype]} v{version} ({C_h}, {C_s}, {H}, {W}) G = {lib.freeu_lanes(H * W)}")


@pytest.mark.parametrize("dtype", S.DTYPES, ids=lambda d: NAMES[d])
def test_factors_over_the_small_shapes(lib, dtype):
    for C_h, C_s, H, W in S.SMALL:
        x = S.make_input(3, C_h, C_s, H, W, dtype, seed=11 + H)
        for s in (0.2, 0.9, 1.0, 1.4):
            for b in (1.0, 1.1, 1.6):
                out = _launch(lib, x, C_h, b, s, 1)
                _check(lib, x, out, C_h, b, s, 1, f"{NAMES[dtype]} ({C_h}, {C_s}, {H}, {W}) b = {b} s = {s}")
                if s == 1.0:
                    assert torch.equal(_bits(out[:, C_h:]), _bits(x[:, C_h:])), "s = 1 must leave the skip planes bitwise"
                if b == 1.0:
                    assert torch.equal(_bits(out[:, :C_h]), _bits(x[:, :C_h])), "b = 1 must leave the backbone bitwise"
        out = _launch(lib, x, C_h, 1.0, 1.0, 2)                               # version 2 computes g = 1 + 0 * q
        _check(lib, x, out, C_h, 1.0, 1.0, 2, f"{NAMES[dtype]} v2 b = 1 ({C_h}, {C_s}, {H}, {W})")


@pytest.mark.parametrize("shape", [(8, 4, 8, 8), (5, 3, 5, 7), (4, 2, 24, 24), (4, 2, 64, 64)], ids=str)
def test_bits_depend_on_the_plane_alone(lib, shape):
    """Two runs, two positions, and the two access paths (a base that is not 16-byte aligned takes the element-wise one):
    identical bits."""
    C_h, C_s, H, W = shape
    for dtype in S.DTYPES:
        x = S.make_input(2, C_h, C_s, H, W, dtype, seed=5)
        x[1, C_h + C_s - 1] = x[0, C_h]                                      # one skip plane's content at two (n, c)
        x[1, 0] = x[0, C_h // 2 - 1]                                         # and one backbone plane's (version 1)
        a = _launch(lib, x, C_h, 1.3, 0.5, 1)
        assert torch.equal(_bits(a), _bits(_launch(lib, x, C_h, 1.3, 0.5, 1)))
        assert torch.equal(_bits(a[1, C_h + C_s - 1]), _bits(a[0, C_h])) and torch.equal(_bits(a[1, 0]), _bits(a[0, C_h // 2 - 1]))
        assert torch.equal(_bits(a), _bits(_launch(lib, x, C_h, 1.3, 0.5, 1, guard=GUARD + 1))), "the access path changed bits"
        v2 = _launch(lib, x, C_h, 1.3, 0.5, 2)
        assert torch.equal(_bits(v2), _bits(_launch(lib, x, C_h, 1.3, 0.5, 2, guard=GUARD + 3)))
        assert torch.equal(_bits(v2[:, C_h:]), _bits(a[:, C_h:]))            # the skip planes do not see the version


def test_a_nan_stays_in_its_plane(lib):
    for dtype in S.DTYPES:
        for C_h, C_s, H, W in ((8, 4, 8, 8), (4, 3, 64, 64)):
            x = S.make_input(2, C_h, C_s, H, W, dtype, seed=9)
            clean = _launch(lib, x, C_h, 1.4, 0.3, 1)
            x[1, C_h + 1, H // 2, 1] = float("nan")
            out = _launch(lib, x, C_h, 1.4, 0.3, 1)
            assert bool(torch.isnan(out[1, C_h + 1]).all()), "the plane that holds the NaN"
            out[1, C_h + 1], clean[1, C_h + 1] = 0, 0
            assert torch.equal(_bits(out), _bits(clean)), "a NaN reached another plane"


def test_version_2_constant_map_gives_unit_gain(lib):
    """Sample 0's backbone channels cancel in pairs, exactly, in any summation order: its mean map is the constant 0,
    max == min, g = 1 -- its backbone comes back bitwise; sample 1 gets the normal result."""
    for dtype in S.DTYPES:
        C_h, C_s, H, W = 8, 4, 12, 20
        x = S.make_input(2, C_h, C_s, H, W, dtype, seed=21)
        x[0, 1:C_h:2] = -x[0, 0:C_h:2]
        out = _launch(lib, x, C_h, 1.6, 0.4, 2)
        _check(lib, x, out, C_h, 1.6, 0.4, 2, f"{NAMES[dtype]} constant map")
        assert torch.equal(_bits(out[0, :C_h]), _bits(x[0, :C_h]))
        assert not torch.equal(_bits(out[1, :C_h // 2]), _bits(x[1, :C_h // 2]))


def test_side_stream_with_its_own_workspace(lib):
    x = S.make_input(2, 8, 4, 16, 16, torch.float16, seed=2)
    want = _launch(lib, x, 8, 1.5, 0.6, 2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = _launch(lib, x, 8, 1.5, 0.6, 2)
    side.synchronize()
    assert torch.equal(_bits(got), _bits(want))
    keys = [k for k in lib._WS if k[2] == "freeu"]
    assert {side.cuda_stream, torch.cuda.current_stream().cuda_stream} <= {k[1] for k in keys}


def test_the_widest_tables(lib):
    """2 x 8192: the one shape whose cos / sin tables pass 64 KiB of LDS."""
    x = S.make_input(2, 2, 2, 2, 8192, torch.float16, seed=4)
    out = _launch(lib, x, 2, 1.2, 0.7, 1)
    _check(lib, x, out, 2, 1.2, 0.7, 1, "fp16 (2, 2, 2, 8192)")


# ---- through the hooks ---------------------------------------------------------------------------------------------------
def _untreated(unet, skips, sample, seen):
    """The concatenation each hooked resnet was handed BEFORE FreeU, rebuilt from the recorded (treated) inputs: a stand-in
    resnet's output is a deterministic function of its input, recomputed here with the same torch ops on the same device."""
    order = {(0, 0): -1, (0, 1): -2, (0, 2): -3, (1, 0): -4, (1, 1): -5, (1, 2): -6}
    out, prev = [], sample
    for i, j, x in seen:
        if (i, j) not in order:
            break
        out.append(torch.cat([prev, skips[order[(i, j)]]], 1))
        o = unet.up_blocks[i].resnets[j].out_channels
        prev = ((x[:, :o] + x[:, -o:]) * 0.5).contiguous()
        if (i, j) == (0, 2):
            prev = prev.repeat_interleave(2, -1).repeat_interleave(2, -2).contiguous()
    return out


def test_through_the_hooks_against_float64_and_the_torch_branch(lib):
    import vidtome_amd
    unet = S.StandinUNet(unit=8, size=8)                                       # 32 | 32, 32 | 32, 32 | 16; 32 | 16, 16 | 16, 16 | 8
    sample, skips = unet.operands(2, torch.float16, DEV)
    s1, s2, b1, b2 = 0.9, 0.2, 1.5, 1.6
    with torch.no_grad():
        unet(sample, skips)
    plain = unet.recorded()

    vidtome_amd.register_freeu(unet, s1=s1, s2=s2, b1=b1, b2=b2)
    with torch.no_grad():
        unet(sample, skips)
    seen = unet.recorded()
    raw = _untreated(unet, skips, sample, seen)
    assert len(raw) == 6
    for (i, j, x), x0 in zip(seen, raw):
        C_h = 32 if (i, j) != (1, 2) and (i, j) != (1, 1) else 16
        assert tuple(x.shape[2:]) == ((8, 8) if i == 0 else (16, 16)) and x.shape == x0.shape
        _check(lib, x0.cpu(), x.cpu(), C_h, b1 if i == 0 else b2, s1 if i == 0 else s2, 1, f"hooked resnet {i}.{j}")

    # unregistered: bitwise the untouched model
    vidtome_amd.unregister_freeu(unet)
    with torch.no_grad():
        unet(sample, skips)
    after = unet.recorded()
    assert len(after) == len(plain) == 7 and all(torch.equal(_bits(a[2]), _bits(p[2])) for a, p in zip(after, plain))

    # the same model with Diffusers' torch branch instead (the stand-in's own), against float64 with ITS bound
    for blk in unet.up_blocks:
        blk.s1, blk.s2, blk.b1, blk.b2 = s1, s2, b1, b2
    with torch.no_grad():
        unet(sample, skips)
    torch_seen = unet.recorded()
    for (i, j, x), x0 in zip(torch_seen, _untreated(unet, skips, sample, torch_seen)):
        C_h = 32 if (i, j) != (1, 2) and (i, j) != (1, 1) else 16
        b, s = (b1, s1) if i == 0 else (b2, s2)
        X = x0.double().cpu().numpy()
        ref = S.freeu64(X, C_h, b, s, 1)
        P = X.shape[2] * X.shape[3]
        u, t = S.U_T[torch.float16], S.T_T[torch.float16]
        err = np.abs(x.double().cpu().numpy() - ref)
        norm = np.sqrt((X[:, C_h:] ** 2).sum((2, 3), keepdims=True))
        assert (err[:, C_h:] <= u * np.abs(ref[:, C_h:]) + t + 16 * math.log2(P) * S.U24 * max(1.0, abs(s)) * norm).all(), (i, j)
        assert (err[:, :C_h // 2] <= u * np.abs(ref[:, :C_h // 2]) + t).all(), (i, j)
        assert np.array_equal(err[:, C_h // 2:C_h], np.zeros_like(err[:, C_h // 2:C_h])), (i, j)
