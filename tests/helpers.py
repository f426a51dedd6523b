"""Shared test helpers (fixture loading, torch-generator draws)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_cases(fname):
    z = np.load(os.path.join(GOLDEN, fname), allow_pickle=False)
    n = int(z["n_cases"])
    cases = [dict() for _ in range(n)]
    for k in z.files:
        if k == "n_cases":
            continue
        i, name = k.split("/", 1)
        v = z[k]
        cases[int(i)][name] = v.item() if v.ndim == 0 else v
    return cases


def load_chain(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    cfg = json.loads(str(z["cfg_json"]))
    return cfg, z


def forked_generator_from_state(rng_state):
    """vidtome/utils.py:22-23: torch.Generator('cpu').set_state(torch.get_rng_state())."""
    import torch
    return torch.Generator(device="cpu").set_state(torch.from_numpy(np.asarray(rng_state)))


# ---- the merge closures' reduce modes: torch's CPU scatter_reduce as the reference (test_gpu_merge_modes.py on the GPU,
# test_oracle_merge_modes.py on the CPU) ----
REDUCE_MODES = ("sum", "prod", "mean", "amax", "amin")
# members of a destination row (itself + its sources) around the largest count that the dtype still represents exactly
# (fp16: 2048, bf16: 256): "mean" divides by the count rounded to the tensors' dtype
MEMBER_COUNTS = {"fp16": (1, 2, 5, 2047, 2048, 2049, 2050, 2051, 2501, 4099),
                 "bf16": (1, 2, 5, 255, 256, 257, 258, 259, 301, 2501),
                 "fp32": (1, 2, 5, 2501)}


def scatter_reduce_reference(x, src_rows, dst_rows, dst_idx, mode):
    """merge.py:127-131 in plain torch on the CPU: the dst rows ``x[b, dst_rows]`` with the src rows ``x[b, src_rows]``
    folded in, ``dst.scatter_reduce(-2, dst_idx.expand(.., C), src, reduce=mode, include_self=True)`` -> (B, Nd, C)."""
    import torch
    assert x.device.type == "cpu"
    C = x.shape[-1]
    bi = torch.arange(x.shape[0])[:, None]
    dst, src = x[bi, dst_rows.long()], x[bi, src_rows.long()]
    return dst.scatter_reduce(-2, dst_idx.long()[..., None].expand(-1, -1, C), src, reduce=mode, include_self=True)


def same_bits(got, want):
    """Elementwise: equal bit patterns, a NaN equal to a NaN whatever its payload."""
    import torch
    assert got.shape == want.shape and got.dtype == want.dtype
    ints = torch.int32 if got.dtype == torch.float32 else torch.int16
    return (got.view(ints) == want.view(ints)) | (got.isnan() & want.isnan())


def interleaved_destinations(counts, seed):
    """(1, r) int32 destinations in which row j has counts[j] members, i.e. counts[j] - 1 sources, the pairs of different
    rows shuffled into one another (not laid out row by row: only a stable sort keeps a row's sources in index order)."""
    import torch
    per_row = torch.tensor(counts) - 1
    d = torch.repeat_interleave(torch.arange(len(counts)), per_row)
    d = d[torch.randperm(d.numel(), generator=torch.Generator().manual_seed(seed))]
    assert torch.equal(torch.bincount(d, minlength=len(counts)), per_row)
    for j in (per_row > 1).nonzero().flatten().tolist():
        at = (d == j).nonzero().flatten()
        assert int(at[-1] - at[0]) >= at.numel(), f"the sources of row {j} came out as one run"
    return d.to(torch.int32)[None]


def reduce_tokens(shape, dtype, seed, mode):
    """Tokens for a reduce-mode case, float32 values rounded to ``dtype``, random signs.  "prod": magnitudes 2 ** U(-0.32,
    0.32), so that a product over thousands of sources is a random walk of the exponent that stays finite and nonzero in
    fp32 (its deviation over 4098 factors: 2 ** +-12).  Otherwise 10 ** U(-2, 2): sums over mixed magnitudes round at every
    step, so they depend on the order and on the accumulator's precision."""
    import torch
    g = torch.Generator().manual_seed(seed)
    span = 0.32 if mode == "prod" else 2.0
    mag = torch.pow(2.0 if mode == "prod" else 10.0, (torch.rand(shape, generator=g) * 2 - 1) * span)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sign).to(dtype)


# ---- the 16-bit projection GEMMs (test_gpu_gemm16.py) ----
SENTINEL16 = 0x7FA5          # a NaN pattern in fp16 and in bf16 that no arithmetic of the kernels produces
EXACT_INT_MAX = {"fp16": 2048, "bf16": 256}    # every integer up to here is a value of the format


def int_uniform(shape, lo, hi, dtype, gen, device="cuda"):
    """Integers uniform in [lo, hi] held in ``dtype`` (exact: the callers keep |lo|, |hi| inside the format's integers)."""
    import torch
    return torch.randint(lo, hi + 1, shape, generator=gen, device=device).to(dtype)


def sentinel_filled(shape, dtype, device="cuda"):
    """A tensor of ``dtype`` (16 bits) whose every element holds the SENTINEL16 bit pattern."""
    import torch
    return torch.full(shape, SENTINEL16, dtype=torch.int16, device=device).view(dtype)


def is_sentinel(t):
    import torch
    return t.view(torch.int16) == SENTINEL16


def ulp16(m, dtype):
    """Spacing of ``dtype`` (fp16 / bf16) at the magnitudes ``m`` (float64, >= 0): 2 ** (max(floor(log2 m), emin) - p + 1),
    the subnormal spacing below 2 ** emin.  frexp, not log2: exact at the powers of two."""
    import torch
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    _, e = torch.frexp(m)                                   # m = f * 2 ** e, f in [0.5, 1)
    e = (e.to(torch.int64) - 1).clamp_min(emin) - mant
    return torch.ldexp(torch.ones_like(m), e)


def rounding_bound(ref, slack, dtype):
    """|RN_dtype(x) - ref| for any x within ``slack`` of ``ref`` (float64): slack + half a spacing at |ref| + slack."""
    return 0.5 * ulp16(ref.abs() + slack, dtype) + slack
