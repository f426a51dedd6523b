"""GPU tests of PnP feature injection: vtm_groupnorm_silu against a float64 restatement with the kernel's rounding points,
vtm_resnet_tail bit for bit against torch's expression, and the fused closure of vidtome_amd.pnp.register_conv_control
against the reference's recorded runs (tests/golden/pnp_conv.npz)."""
import math
import os

import numpy as np
import pytest
import torch

import pnp_conv_standin as st
from helpers import GOLDEN, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
MANT = {"fp32": (23, -126), "fp16": (10, -14), "bf16": (7, -126)}
Z = np.load(os.path.join(GOLDEN, "pnp_conv.npz"), allow_pickle=False)


def ulp(m, dt):
    """Spacing of the dtype at the magnitudes ``m`` (float64 numpy): the subnormal spacing below 2 ** emin."""
    mant, emin = MANT[dt]
    _, e = np.frexp(np.abs(m))                                       # |m| = f * 2 ** e, f in [0.5, 1)
    return np.ldexp(1.0, np.maximum(e - 1, emin) - mant)


def rounded(a, dtype):
    """float64 numpy -> nearest value of ``dtype`` -> float64."""
    return torch.from_numpy(a).to(dtype).double().numpy()


def groupnorm_case(shape, dt, act, with_add, with_gamma, with_beta, mu=0.0, seed=0):
    """Runs the kernel and the float64 restatement with the same rounding points; returns max(|z - z_ref| / tolerance)."""
    from vidtome_amd import _lib
    B, C, groups, HW = shape
    dtype = DTYPES[dt]
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, C, HW, generator=gen) + mu).to(dtype)
    add = (0.5 * torch.randn(B, C, generator=gen)).to(dtype) if with_add else None
    gamma = (1 + 0.3 * torch.randn(C, generator=gen)).to(dtype) if with_gamma else None
    beta = (0.3 * torch.randn(C, generator=gen)).to(dtype) if with_beta else None
    dev = lambda t: None if t is None else t.to(DEV)
    out = _lib.groupnorm_silu(dev(x), groups, dev(gamma), dev(beta), 1e-5, add=dev(add), act=bool(act))
    torch.cuda.synchronize()
    assert out.shape == x.shape and out.dtype == dtype
    z = out.double().cpu().numpy()
    # x' = round_T(x + add): the fp32 sum the kernel forms, rounded to the dtype
    xp = x if add is None else (x.float() + add.float()[:, :, None]).to(dtype)
    xp = xp.double().numpy().reshape(B, groups, -1)
    n = xp.shape[-1]
    mean = xp.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((xp - mean) ** 2).mean(-1, keepdims=True) + 1e-5)
    per_elem = lambda p, fill: (np.full(C, fill) if p is None else p.double().numpy())[None, :, None].repeat(HW, 2).reshape(1, groups, -1)
    g, b = per_elem(gamma, 1.0), per_elem(beta, 0.0)
    y_ref = rounded((xp - mean) * rstd * g + b, dtype)
    fp32_term = (math.log2(n) + 8) * 2.0 ** -24 * ((np.abs(xp) + np.abs(mean)) * rstd * np.abs(g) + np.abs(b))
    z_ref = rounded(y_ref / (1 + np.exp(-y_ref)), dtype) if act else y_ref         # act = 0: the output is y itself
    tol = 1.1 * ulp(y_ref, dt) + ulp(z_ref, dt) + fp32_term
    ratio = float((np.abs(z.reshape(z_ref.shape) - z_ref) / tol).max())
    print(f"groupnorm_silu {shape} {dt} act={act} add={with_add} gamma={with_gamma} beta={with_beta} mu={mu}: "
          f"max |z - z_ref| / tol = {ratio:.3f}")
    return ratio


SMALL = ((2, 32, 32, 15),        # one channel per group, odd HW: unaligned group starts
         (3, 24, 4, 15),         # n = 90
         (1, 8, 1, 64))          # one group
COMBOS = ((1, True, True, True), (0, False, False, False), (1, False, True, False), (0, True, False, True))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape", SMALL)
def test_groupnorm_silu_small_shapes(shape, dt):
    for k, (act, with_add, with_gamma, with_beta) in enumerate(COMBOS):
        assert groupnorm_case(shape, dt, act, with_add, with_gamma, with_beta, seed=k) <= 1.0


@pytest.mark.parametrize("mu", (0.0, 30.0))
@pytest.mark.parametrize("dt", list(DTYPES))
def test_groupnorm_silu_sd_size(dt, mu):
    """(2, 2560, 32, 256): n = 20 480.  mu = 30: a one-pass variance (E[x^2] - E[x]^2) misses this tolerance 2-6x."""
    assert groupnorm_case((2, 2560, 32, 256), dt, 1, True, True, True, mu=mu) <= 1.0


@pytest.mark.parametrize("shape,dt", (((1, 320, 2, 576), "fp32"), ((1, 640, 2, 576), "fp16"),
                                      ((1, 322, 2, 575), "fp32"), ((1, 642, 2, 575), "bf16")))
def test_groupnorm_silu_groups_larger_than_the_lds(shape, dt):
    """More than 160 KiB per group: the first part stays resident, the rest is read again.  The 575-pixel shapes put the
    second group on an unaligned start as well."""
    assert shape[1] // shape[2] * shape[3] * (4 if dt == "fp32" else 2) > 160 * 1024
    assert groupnorm_case(shape, dt, 1, True, True, True) <= 1.0
    assert groupnorm_case(shape, dt, 0, False, False, False, seed=1) <= 1.0


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("rows", ((6, 0, 0), (6, 6, 2), (7, 6, 2), (4, 4, 2)))
def test_resnet_tail_is_torch_expression_bit_for_bit(rows, dt):
    """(shortcut + hidden_full) / scale as torch evaluates it on the GPU: the sum rounded to the dtype, then the product
    with the fp32 reciprocal of the scale.  sqrt 2 included: the kernel does what torch does, so the bits are equal."""
    from vidtome_amd import _lib
    B, inject_rows, period = rows
    dtype = DTYPES[dt]
    gen = torch.Generator().manual_seed(B * 100 + inject_rows)
    for shape in ((15, 16), (3, 7, 5)):                        # 240 elements per row, and 105: no multiple of 8 (or 4)
        compact = B if inject_rows == 0 else period + B - inject_rows
        shortcut = torch.randn((B,) + shape, generator=gen).to(dtype).to(DEV)
        hidden = torch.randn((compact,) + shape, generator=gen).to(dtype).to(DEV)
        index = [b % period if b < inject_rows else b - inject_rows + period for b in range(B)]
        if rows == (7, 6, 2):
            assert index[6] == 2                                # the seventh row reads compact row 2
        full = hidden[torch.tensor(index, device=DEV)]
        for scale in (1.0, 2.0, math.sqrt(2.0)):
            got = _lib.resnet_tail(shortcut, hidden, inject_rows, period, scale)
            want = (shortcut + full) / scale
            assert got.dtype == dtype and bool(same_bits(got, want).all()), (rows, dt, shape, scale)


@pytest.mark.parametrize("dt", ("fp32", "fp16"))
@pytest.mark.parametrize("n", range(len(st.CASES)))
def test_fused_closure_equals_the_reference(n, dt):
    """The fused route against the recorded fp32 output: no further from it than twice the plain-torch fallback on the
    same GPU in the same dtype, plus one spacing of the dtype at the output's max magnitude (the fused route convolves a
    smaller batch, for which the library may pick another algorithm)."""
    num_inputs, B, t, shortcut, scale = st.CASES[n]
    r = st.closure_errors(n, Z, DTYPES[dt])
    print(f"case {n} {st.CASES[n]} {dt}: e_fused {r['e_fused']:.3e} e_module {r['e_module']:.3e} ulp {r['ulp']:.3e}")
    assert r["e_fused"] <= 2 * r["e_module"] + r["ulp"]
    rows = st.surviving_rows(num_inputs, B, t)
    assert r["conv1_rows"] == [rows, rows]
    sbs = B // num_inputs
    assert rows == ({6: sbs, 7: sbs + 1}[B] if st.injects(t) else B)


def _counting(monkeypatch):
    from vidtome_amd import _lib
    calls = {"groupnorm_silu": 0, "resnet_tail": 0}
    for name in calls:
        def counted(*a, _f=getattr(_lib, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(_lib, name, counted)
    return calls


def test_fused_route_runs_the_kernels_and_the_exceptions_take_the_fallback(monkeypatch):
    from vidtome_amd import pnp
    calls = _counting(monkeypatch)
    n = 4                                                   # (3, 7, in the schedule, conv_shortcut, sqrt 2)
    num_inputs, B, t, shortcut, scale = st.CASES[n]
    want = torch.from_numpy(Z[f"{n}/out"])
    x, temb = (torch.from_numpy(Z[f"{k}/B{B}s{int(shortcut)}"]).to(DEV) for k in ("x", "temb"))

    def run(resnet, x_in):
        resnet = resnet.to(DEV)
        pnp.register_conv_control(st.model_around(resnet), list(st.SCHEDULE), num_inputs)
        resnet.t = t
        seen = []
        resnet.conv1.register_forward_hook(lambda m, a, o: seen.append(a[0].shape[0]))
        before = dict(calls)
        with torch.no_grad():
            y = resnet.forward(x_in, temb)
        return y, seen, {k: calls[k] - before[k] for k in calls}

    recorded = lambda **kw: st.load_weights(st.StandinResnet(shortcut=shortcut, scale=scale, **kw), Z, shortcut)
    # fp32 throughout: sums of at most 216 products in whatever order the library picks, ~216 * 2^-24 = 1.3e-5 of the sum of
    # magnitudes in the worst case and a few 1e-7 of the output's max magnitude in practice (profiles/pnp_conv.json)
    close = lambda y, ref: float((y.cpu() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    y, seen, used = run(recorded().eval(), x)
    assert used == {"groupnorm_silu": 2, "resnet_tail": 1} and seen == [3] and close(y, want)
    # channels_last input: the fallback, same result
    y, seen, used = run(recorded().eval(), x.contiguous(memory_format=torch.channels_last))
    assert used == {"groupnorm_silu": 0, "resnet_tail": 0} and seen == [3] and close(y, want)
    # training mode with dropout p > 0: the fallback (the draws make the values random; the rows are still compacted)
    y, seen, used = run(recorded(dropout=0.25).train(), x)
    assert used == {"groupnorm_silu": 0, "resnet_tail": 0} and seen == [3] and bool(torch.isfinite(y).all())
    # ... and with p = 0 a training-mode resnet stays fused
    y, seen, used = run(recorded().train(), x)
    assert used == {"groupnorm_silu": 2, "resnet_tail": 1} and close(y, want)
    # a scale_shift resnet: the fallback, equal to the all-rows torch statement with the copies applied afterwards
    resnet = st.StandinResnet(shortcut=shortcut, scale=scale, time_embedding_norm="scale_shift").eval()
    y, seen, used = run(resnet, x)
    with torch.no_grad():
        h = resnet.conv1(resnet.nonlinearity(resnet.norm1(x)))
        s, b = resnet.time_emb_proj(resnet.nonlinearity(temb))[:, :, None, None].chunk(2, dim=1)
        h = resnet.conv2(resnet.nonlinearity(resnet.norm2(h) * (1 + s) + b))
        h[2:4], h[4:6] = h[:2], h[:2]
        ref = ((resnet.conv_shortcut(x) + h) / scale).cpu()
    assert used == {"groupnorm_silu": 0, "resnet_tail": 0} and seen[0] == 3 and close(y, ref)
