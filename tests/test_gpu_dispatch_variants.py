"""GPU tests of the size-selected kernel variants of the memory-bound and epilogue kernels (run with -m gpu on an MI355X):
every instantiation that the library picks from the call's size is run at the smallest shape that selects it and compared
with a plain torch expression of the same operation on the same device input -- float64 where arithmetic is involved,
indexing where the kernel is a pure move.

The thresholds are restated below as named constants; `_pinned` checks that the source line they restate still reads as
it did, so a change of a threshold fails the test's own precondition instead of silently testing the other branch.

dispatch condition                                             source                 reached by
-------------------------------------------------------------  ---------------------  ------------------------------------------
C == 1280 && rows >= 32768 -> layernorm_rows_kernel<T,32,..>    layernorm.hip:224,236  test_layernorm_lpr32_kernel
C == 1280 && rows <  32768 -> layernorm_kernel<T,3,2,..>        layernorm.hip:224,256  test_layernorm_c1280_below_the_lpr32_threshold
2 rows C sizeof(T) > STREAM_BYTES, C = 320 (rows kernel, NT)   layernorm.hip:218,234  test_layernorm_streaming[rows_kernel-fp16]
2 rows C sizeof(T) > STREAM_BYTES, C = 512 (wave per row, NT)  layernorm.hip:218,254  test_layernorm_streaming[wave_per_row-fp32|bf16]
gamma / beta null or not (four epilogues, both kernels)        layernorm.hip:129,206  test_layernorm_affine_combinations
blocks > 256 * 16 -> second grid-stride pass of the row moves  gather.hip:154-158      test_gather_rows_grid_stride, test_unmerge_add_grid_stride
2 total 16 > STREAM_BYTES -> gather_rows_kernel<true>           gather.hip:207         test_gather_rows_streaming
y + (1 | 2) rows > STREAM_BYTES -> unmerge_add_kernel<T,true>   gather.hip:226         test_unmerge_add_streaming
resid == nullptr (pure unmerge gather)                         gather.hip:81          test_unmerge_add_grid_stride[..-gather_only]
cdiv(n, 256) > 4096 -> second pass of cfg_ddim_kernel           ddim.hip:57            test_cfg_ddim_beyond_one_grid_pass
cdiv(total, 256) > 65536 -> second pass of geglu_kernel         geglu.hip:46           test_geglu_grid_stride
K % 320 == 0, N % 160 != 0 -> linear_rows_kernel<..160,80,true,128>  linear.hip:533,542  test_gpu_parity.py::test_linear_rows_vs_torch_fp32
                                                                                       [(320, 192) and (640, 96) rows]
"""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F32, F16, BF16]
IDS = {F32: "fp32", F16: "fp16", BF16: "bf16"}
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vidtome_amd", "csrc")

# ---- the thresholds, restated (each with the source text it restates) ----
STREAM_BYTES = 256 << 20             # common.h:76
LN_ROWS_KERNEL_ALWAYS = (320, 640)   # layernorm.hip:224
LN_LPR32_MIN_ROWS = 32768            # layernorm.hip:224 (C == 1280 only)
BLOCK = 256                          # threads per block of the row moves, cfg_ddim and geglu
MOVE_GRID_CAP = 256 * 16             # gather.hip:156
DDIM_GRID_CAP = 4096                 # ddim.hip:57
GEGLU_GRID_CAP = 65536               # geglu.hip:46
_PINS = {
    "common.h": ["constexpr int64_t STREAM_BYTES = 256ll << 20;"],
    "layernorm.hip": ["const bool nt = 2 * rows * C * (int64_t)sizeof(T) > vtm::STREAM_BYTES;",
                      "if (C == 320 || C == 640 || (C == 1280 && rows >= 32768)) {",
                      "constexpr int WAVES_PER_BLOCK = VTM_LN_WAVES;", "#define VTM_LN_WAVES 4"],
    "gather.hip": ["const int64_t cap = 256 * 16;", "if (2 * total * 16 > vtm::STREAM_BYTES)",
                   "const bool nt = (B * M * C * es + (resid ? 2 : 1) * total * 16) > vtm::STREAM_BYTES;"],
    "ddim.hip": ["std::min<int64_t>(vtm::cdiv(n, 256), 4096)"],
    "geglu.hip": ["std::min<int64_t>(vtm::cdiv(total, 256), 65536)"],
}


def _pinned(fname):
    """The test's precondition: the dispatch conditions of `fname` still read as the constants above restate them."""
    with open(os.path.join(CSRC, fname)) as f:
        src = f.read()
    for text in _PINS[fname]:
        assert text in src, f"{fname} no longer contains {text!r}: re-derive the shapes of this test from the new condition"


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _esize(dtype):
    return 4 if dtype == F32 else 2


def _poison(nbytes):
    """Fill a block of `nbytes` with 0xFF (NaN patterns) and hand it back to the caching allocator: the result that the
    library allocates next with torch.empty is likely to be this block, so elements that a kernel fails to write do not
    hold a leftover copy of the right answer."""
    torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _random_bits(shape, dtype, g):
    """Every bit pattern, NaNs and denormals included: for the pure moves."""
    if dtype == F32:
        return torch.randint(-2 ** 31, 2 ** 31, shape, dtype=torch.int32, device=DEV, generator=g).view(F32)
    return torch.randint(-2 ** 15, 2 ** 15, shape, dtype=torch.int16, device=DEV, generator=g).view(dtype)


# ---------------------------------------------------------------------------------------------------
# 1. LayerNorm
# ---------------------------------------------------------------------------------------------------
LN_EPS = 1e-5


def _ln_variant(rows, C, dtype):
    """(kernel family, streaming) that launch_layernorm picks, from the restated thresholds."""
    _pinned("common.h"), _pinned("layernorm.hip")
    rows_kernel = C in LN_ROWS_KERNEL_ALWAYS or (C == 1280 and rows >= LN_LPR32_MIN_ROWS)
    return ("rows" if rows_kernel else "wave_per_row"), 2 * rows * C * _esize(dtype) > STREAM_BYTES


def _ln_inputs(rows, C, dtype, seed, mean=0.7, std=3.0):
    g = _gen(seed)
    x = (torch.randn(rows, C, generator=g, device=DEV) * std + mean).to(dtype)
    w = (1.0 + 0.2 * torch.randn(C, generator=g, device=DEV)).to(dtype)
    b = (0.1 * torch.randn(C, generator=g, device=DEV)).to(dtype)
    return x, w, b


def _ln_ref64(x, w, b):
    x64 = x.double()
    x64 -= x64.mean(dim=-1, keepdim=True)
    x64 *= torch.rsqrt((x64 * x64).mean(dim=-1, keepdim=True) + LN_EPS)
    if w is not None:
        x64 *= w.double()
    if b is not None:
        x64 += b.double()
    return x64


def _ln_check(y, x, w, b, tag):
    """16-bit: every element is the correctly rounded float64 result or its neighbour in the model dtype (the form of
    test_layernorm_vs_torch_fp32).  fp32: the kernel's maximum error against float64 is at most twice that of torch's own
    fp32 layer_norm on the same input (the 2 is for a different summation order), plus 1e-7 max|ref|."""
    ref = _ln_ref64(x, w, b)
    assert y.shape == x.shape and y.dtype == x.dtype
    if x.dtype == F32:
        t = torch.nn.functional.layer_norm(x, x.shape[-1:], w, b, LN_EPS)
        e_kernel, e_torch = (y.double() - ref).abs().max().item(), (t.double() - ref).abs().max().item()
        print(f"\n[layernorm fp32] {tag}: kernel max err {e_kernel:.3e}, torch fp32 max err {e_torch:.3e}, "
              f"ratio {e_kernel / e_torch if e_torch else math.inf:.2f}")
        assert e_kernel <= 2.0 * e_torch + 1e-7 * ref.abs().max().item(), (tag, e_kernel, e_torch)
    else:
        rel = 2.0 ** (-10 if x.dtype == F16 else -7)
        y64 = y.double()
        y64 -= ref.to(x.dtype).double()
        assert (y64.abs_() <= ref.abs_() * rel + 1e-6).all(), tag


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_layernorm_lpr32_kernel(L, dtype):
    """layernorm_rows_kernel<T, 32, 1, false>: C = 1280 at the row threshold + 5 -- two rows per wave and four waves per
    block, so the last block has one full wave, one wave with a single live row and two idle waves.

    Measured fp32 error ratio kernel / torch (MI355X): see the table in test_layernorm_large_mean."""
    rows, C = LN_LPR32_MIN_ROWS + 5, 1280
    # (fp32: 336 MB of input + output, so that launch carries the streaming flag as well; the 16-bit cases are NT = false)
    assert _ln_variant(rows, C, dtype) == ("rows", dtype == F32)
    x, w, b = _ln_inputs(rows, C, dtype, 1)
    _poison(x.numel() * x.element_size())
    _ln_check(L.layernorm(x, w, b, LN_EPS), x, w, b, f"lpr32 {IDS[dtype]}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_layernorm_c1280_below_the_lpr32_threshold(L, dtype):
    """One row below the threshold C = 1280 takes the wave-per-row kernel, at the threshold the LPR = 32 kernel; both on the
    same data.  The two kernels add a row's channels in a different order (three strided chunks per lane and a 64-lane
    butterfly, against five chunks per lane and a 32-lane butterfly), so the fp32 statistics differ in the last bits and
    the results are NOT bit-identical: measured on an MI355X, 4 004 (fp16) and 373 (bf16) of 41 941 760 elements differ,
    and 11 230 258 in fp32.  Each variant is therefore held to the bound of _ln_check on its own, and the number
    of differing elements is printed."""
    rows, C = LN_LPR32_MIN_ROWS, 1280
    assert _ln_variant(rows - 1, C, dtype) == ("wave_per_row", dtype == F32)
    assert _ln_variant(rows, C, dtype) == ("rows", dtype == F32)
    x, w, b = _ln_inputs(rows, C, dtype, 2)
    y_rows = L.layernorm(x, w, b, LN_EPS)
    y_wave = L.layernorm(x[:rows - 1], w, b, LN_EPS)
    _ln_check(y_rows, x, w, b, f"c1280 at threshold {IDS[dtype]}")
    _ln_check(y_wave, x[:rows - 1], w, b, f"c1280 below threshold {IDS[dtype]}")
    differ = int((_bits(y_wave) != _bits(y_rows[:rows - 1])).sum())
    print(f"\n[layernorm] C = 1280 wave-per-row vs LPR = 32, {IDS[dtype]}: {differ} of {y_wave.numel()} elements differ")


@pytest.mark.parametrize("kernel,C,dtype", [("rows", 320, F16), ("wave_per_row", 512, F32), ("wave_per_row", 512, BF16)],
                         ids=["rows_kernel-fp16", "wave_per_row-fp32", "wave_per_row-bf16"])
def test_layernorm_streaming(L, kernel, C, dtype):
    """The NT = true instantiations: the smallest row count whose input + output exceed STREAM_BYTES, plus 3 (a ragged last
    wave).  For the 16-bit dtypes vtm_layernorm_panels must equal vtm_layernorm bit for bit at this shape too."""
    rows = STREAM_BYTES // (2 * C * _esize(dtype)) + 1 + 3
    assert _ln_variant(rows, C, dtype) == (kernel, True) and _ln_variant(rows - 4, C, dtype) == (kernel, False)
    x, w, b = _ln_inputs(rows, C, dtype, 3)
    _poison(x.numel() * x.element_size())
    y = L.layernorm(x, w, b, LN_EPS)
    _ln_check(y, x, w, b, f"streaming {kernel} C={C} {IDS[dtype]}")
    if dtype != F32:
        yp = L.layernorm_panels(x, w, b, LN_EPS)
        assert yp.shape == (C // 8, L.panel_rows(rows), 8)
        assert torch.equal(_bits(yp[:, :rows].permute(1, 0, 2).reshape(rows, C)), _bits(y))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("rows,C", [(37, 320), (5, 1280), (3, 8)])
def test_layernorm_affine_combinations(L, rows, C, dtype):
    """The four epilogues (gamma and beta, gamma only, beta only, neither) of the lanes-per-row kernel (C = 320) and of the
    wave-per-row kernel (C = 1280 with few rows, C = 8)."""
    x, w, b = _ln_inputs(rows, C, dtype, rows + C)
    for gamma, beta in ((w, b), (w, None), (None, b), (None, None)):
        tag = f"({rows}, {C}) {IDS[dtype]} gamma={'yes' if gamma is not None else 'no'} beta={'yes' if beta is not None else 'no'}"
        _ln_check(L.layernorm(x, gamma, beta, LN_EPS), x, gamma, beta, tag)


def test_layernorm_large_mean(L):
    """fp32, mean 100 and deviation 0.1: the variance must come from the centred second pass.  A one-pass E[x^2] - E[x]^2
    loses it (x^2 ~ 1e4 carries 6e-4 of fp32 rounding against a variance of 1e-2) and misses the bound by orders of
    magnitude.

    Measured fp32 ratios (kernel max error / torch fp32 max error against float64, MI355X):
        C = 1280, 32 773 rows (LPR = 32)        1.01        C = 1280, 32 768 rows (LPR = 32)        1.18
        C = 1280, 32 767 rows (wave per row)    1.05        C = 512, 65 540 rows (streaming)        1.07
        (37, 320) four affine combinations      0.98-1.31   (5, 1280)                               0.76-1.10
        (3, 8)                                  0.45-1.00   large mean (this test)                  1.58
    (large mean: 2.2e-4 against torch's 1.4e-4 -- both carry the fp32 rounding of a mean of 100 into a deviation of 0.1)"""
    rows, C = 64, 640
    assert _ln_variant(rows, C, F32) == ("rows", False)
    g = _gen(4)
    x = 100.0 + 0.1 * torch.randn(rows, C, generator=g, device=DEV)
    w = 1.0 + 0.2 * torch.randn(C, generator=g, device=DEV)
    b = 0.1 * torch.randn(C, generator=g, device=DEV)
    _ln_check(L.layernorm(x, w, b, LN_EPS), x, w, b, "large mean")


# ---------------------------------------------------------------------------------------------------
# 2. row moves: bitwise
# ---------------------------------------------------------------------------------------------------
def _move_regime(total_chunks, bytes_touched):
    """(more than one grid-stride pass, streaming) of a row move over `total_chunks` 16-byte chunks."""
    _pinned("common.h"), _pinned("gather.hip")
    return -(-total_chunks // BLOCK) > MOVE_GRID_CAP, bytes_touched > STREAM_BYTES


def _pool_rows(x0, x1, idx):
    pool = _bits(x0) if x1 is None else torch.cat([_bits(x0), _bits(x1)], dim=1)
    return pool[torch.arange(pool.shape[0], device=DEV)[:, None], idx.long()]


def _gather_case(L, dtype, B, C, M, P0, P1, pad_to, seed):
    g = _gen(seed)
    x0, x1 = _random_bits((B, P0, C), dtype, g), _random_bits((B, P1, C), dtype, g)
    idx = torch.randint(0, P0 + P1, (B, M), device=DEV, generator=g).to(torch.int32)
    idx[:, :4] = torch.tensor([0, P0 - 1, P0, P0 + P1 - 1], dtype=torch.int32, device=DEV)     # the pool's edges, per sample
    out = L.gather_rows(x0, x1, idx, pad_to=pad_to)
    Mp = out.shape[1]
    assert Mp > M and Mp % pad_to == 0 and out.shape == (B, Mp, C)
    assert torch.equal(_bits(out[:, :M]), _pool_rows(x0, x1, idx))
    assert not _bits(out[:, M:]).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_gather_rows_grid_stride(L, dtype):
    """gather_rows_kernel<false> with one block more than the grid cap holds: the last chunks are moved by the second
    iteration of the grid-stride loop.  Two-part pool with the four edge rows planted, zero padding rows behind."""
    B, C = 2, 320
    chunks = C * _esize(dtype) // 16
    M = MOVE_GRID_CAP * BLOCK // (B * chunks) + 1
    total = B * M * chunks
    assert _move_regime(total, 2 * total * 16) == (True, False)
    assert total - MOVE_GRID_CAP * BLOCK <= B * chunks         # the smallest such M
    pad_to = 64
    assert M % pad_to
    _gather_case(L, dtype, B, C, M, 3000, 1000, pad_to, 5)


def test_gather_rows_streaming(L):
    """gather_rows_kernel<true>: rows read + rows written just above STREAM_BYTES (fp16, C = 320)."""
    B, C, dtype = 2, 320, F16
    chunks = C * _esize(dtype) // 16
    M = STREAM_BYTES // (2 * 16 * B * chunks) + 1
    total = B * M * chunks
    assert _move_regime(total, 2 * total * 16) == (True, True)
    assert _move_regime(B * (M - 1) * chunks, 2 * B * (M - 1) * chunks * 16)[1] is False
    pad_to = 64
    assert M % pad_to
    _gather_case(L, dtype, B, C, M, 6000, 2000, pad_to, 6)


def _unmerge_case(L, dtype, B, C, Mr, Lr, with_resid, seed):
    """y (B, Mr, C), out rows Lr; the first half of every sample's positions read one merged row, the rest random ones."""
    g = _gen(seed)
    inv = torch.randint(0, Mr, (B, Lr), device=DEV, generator=g).to(torch.int32)
    inv[:, :Lr // 2] = torch.tensor([Mr - 1, 0][:B], dtype=torch.int32, device=DEV)[:, None]
    if with_resid:
        y = torch.randn(B, Mr, C, device=DEV, generator=g).to(dtype)
        resid = (3.0 * torch.randn(B, Lr, C, device=DEV, generator=g)).to(dtype)
        want = y[torch.arange(B, device=DEV)[:, None], inv.long()]
        want += resid                                     # torch's 16-bit add: the exact sum, rounded once
    else:
        y, resid = _random_bits((B, Mr, C), dtype, g), None
        want = y[torch.arange(B, device=DEV)[:, None], inv.long()]
    _poison(want.numel() * want.element_size())
    out = L.unmerge_add(y, inv, resid)
    assert out.shape == (B, Lr, C) and torch.equal(_bits(out), _bits(want))


@pytest.mark.parametrize("mode", ["residual", "gather_only"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_unmerge_add_grid_stride(L, dtype, mode):
    """unmerge_add_kernel<T, false> one block beyond the grid cap, with a residual (== torch.gather + resid bit for bit) and
    with resid = None (== torch.gather bit for bit, over every bit pattern); half of the rows read the same merged row."""
    B, C = 2, 320
    chunks = C * _esize(dtype) // 16
    Lr = MOVE_GRID_CAP * BLOCK // (B * chunks) + 1
    Mr = Lr // 2 + 1
    total = B * Lr * chunks
    with_resid = mode == "residual"
    assert _move_regime(total, B * Mr * chunks * 16 + (2 if with_resid else 1) * total * 16) == (True, False)
    _unmerge_case(L, dtype, B, C, Mr, Lr, with_resid, 7)


@pytest.mark.parametrize("mode", ["residual", "gather_only"])
def test_unmerge_add_streaming(L, mode):
    """unmerge_add_kernel<__half, true>: merged rows + residual + result just above STREAM_BYTES."""
    B, C, dtype, Mr = 2, 320, F16, 20000
    row_bytes = C * _esize(dtype)
    chunks = row_bytes // 16
    with_resid = mode == "residual"
    k = 2 if with_resid else 1
    Lr = (STREAM_BYTES - B * Mr * row_bytes) // (k * B * row_bytes) + 1
    touched = lambda l: B * Mr * row_bytes + k * B * l * row_bytes
    assert _move_regime(B * Lr * chunks, touched(Lr)) == (True, True) and touched(Lr - 1) <= STREAM_BYTES
    _unmerge_case(L, dtype, B, C, Mr, Lr, with_resid, 8)


# ---------------------------------------------------------------------------------------------------
# 3. cfg_ddim beyond one grid pass
# ---------------------------------------------------------------------------------------------------
def _ddim_chain(x, eu, ec, guidance, a, b, c, d):
    """generate.py:276-311 op by op in the tensor dtype, with the casts that vtm_cfg_ddim documents (_lib.cfg_ddim): the
    multipliers b, c, d rounded to the tensor dtype, the divisor a kept in fp32.  Every product and sum of two values of
    a 16-bit dtype is formed in fp32 and rounded once, on the device as on the CPU."""
    T, dev = eu.dtype, eu.device
    f32 = lambda v: torch.tensor(v, dtype=F32, device=dev)
    a, (b, c, d) = f32(a), (f32(v).to(T) for v in (b, c, d))
    eps = eu if ec is None else eu + (guidance * (ec - eu))
    if x is None:
        return None, eps
    x0 = ((x - b * eps).float() / a).to(T)
    return c * x0 + d * eps, eps


def _ddim_reference_cpu(x, eu, ec, guidance, a, b, c, d):
    """The reference's own expression on the CPU, coefficients as the 0-dim fp32 tensors it holds (what ddim.npz pins at
    latent size)."""
    a, b, c, d = (torch.tensor(v, dtype=F32) for v in (a, b, c, d))
    eps = eu if ec is None else eu + guidance * (ec - eu)
    if x is None:
        return None, eps
    pred_x0 = (x - b * eps) / a
    return c * pred_x0 + d * eps, eps


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_cfg_ddim_beyond_one_grid_pass(L, dtype):
    """n = one grid of 4096 blocks + 123 elements: the last 123 are computed by the second iteration of the loop.  Sampling
    and inversion coefficient order, eps_cond = None, x = None with the guided eps wanted: bit for bit against the chain on
    the device and against the reference's expression on the CPU."""
    _pinned("ddim.hip")
    n = DDIM_GRID_CAP * BLOCK + 123
    assert -(-n // BLOCK) > DDIM_GRID_CAP
    g = _gen(9)
    x, eu, ec = (torch.randn(n, device=DEV, generator=g).to(dtype) for _ in range(3))
    a_t, a_p = torch.tensor(0.4217, dtype=F32), torch.tensor(0.4563, dtype=F32)     # alphas_cumprod of two neighbouring steps
    mu, sigma, mu_p, sigma_p = (float(v) for v in (a_t ** 0.5, (1 - a_t) ** 0.5, a_p ** 0.5, (1 - a_p) ** 0.5))
    cases = {"sampling": (x, eu, ec, (mu, sigma, mu_p, sigma_p)), "inversion": (x, eu, ec, (mu_p, sigma_p, mu, sigma)),
             "no_cond": (x, eu, None, (mu, sigma, mu_p, sigma_p)), "eps_only": (None, eu, ec, (mu, sigma, mu_p, sigma_p))}
    bad = []
    for name, (x_, eu_, ec_, coef) in cases.items():
        _poison(n * _esize(dtype))
        if x_ is None:
            xn, eps = None, L.cfg_ddim(None, eu_, ec_, 7.5, *coef)
        else:
            xn, eps = L.cfg_ddim(x_, eu_, ec_, 7.5, *coef, want_eps=True)
        cpu = lambda t: None if t is None else t.cpu()
        for where, (xn_ref, eps_ref) in (("device", _ddim_chain(x_, eu_, ec_, 7.5, *coef)),
                                         ("cpu", _ddim_reference_cpu(cpu(x_), cpu(eu_), cpu(ec_), 7.5, *coef))):
            mism = int((_bits(eps.to(eps_ref.device)) != _bits(eps_ref)).sum())
            if xn is not None:
                mism += int((_bits(xn.to(xn_ref.device)) != _bits(xn_ref)).sum())
            print(f"\n[cfg_ddim] {IDS[dtype]} {name} vs {where} chain: {mism} elements differ")
            if mism:
                bad.append((name, where, mism))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------
# 4. gated activation: per element, in ulps
# ---------------------------------------------------------------------------------------------------
def _ordered(t):
    """Floating-point values as integers in value order (+0 and -0 both 0): |difference| = distance in ulps."""
    if t.dtype == F32:
        i = t.view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    i = t.view(torch.int16).long()
    return torch.where(i < 0, -(i & 0x7FFF), i)


def _round64(t64, dtype):
    """float64 -> dtype in ONE rounding.  (A conversion through fp32 rounds twice; here the fp32 step rounds to odd, which
    leaves the second rounding to see on which side of a tie the float64 value lies.)"""
    if dtype == F32:
        return t64.float()
    f = t64.float()
    i = f.view(torch.int32) - (f.double().abs() > t64.abs()).to(torch.int32)       # truncate the magnitude
    i = i | (i.view(F32).double() != t64).to(torch.int32)                          # sticky bit
    return i.view(F32).to(dtype)


def _gelu_ref(g):
    """gelu(g) = 0.5 g erfc(-g / sqrt 2) in float64, rounded once to the gate's dtype."""
    g64 = g.double()
    return _round64(0.5 * g64 * torch.special.erfc(-g64 / math.sqrt(2.0)), g.dtype)


def _all_16bit_gates(dtype):
    """All 65 536 bit patterns in pattern order 0x8000 .. 0xffff, 0x0000 .. 0x7fff.  The non-finite ones lie in runs that
    start and end at multiples of 64."""
    return torch.arange(-32768, 32768, dtype=torch.int32, device=DEV).to(torch.int16).view(dtype)


def _fp32_gates():
    """2^20 gates: magnitudes log-spaced over [1e-6, 12] with both signs, +-0 and +-inf."""
    m = torch.logspace(math.log10(1e-6), math.log10(12.0), 2 ** 19 - 2, dtype=torch.float64, device=DEV).float()
    return torch.cat([m, -m, torch.tensor([0.0, -0.0, math.inf, -math.inf], device=DEV)])


def _values(kind, like, seed):
    if kind == "normal":
        return torch.randn(like.shape, device=DEV, generator=_gen(seed)).to(like.dtype)
    return torch.full_like(like, kind)


REGIONS = (("all", -math.inf), ("g>=-6", -6.0), ("g>=-4", -4.0), ("g>=0", 0.0))

# Measured on an MI355X against _gelu_ref: (largest ulp distance of gelu(g), gates further than 1 ulp) per region of finite
# gates.  The tests assert the measured maximum + 1.
GELU_MEASURED = {
    # vtm_geglu evaluates torch's own form 0.5 g (1 + erf(g / sqrt 2)) in fp32: 1 + erf cancels on the negative side.  The
    # worst gates are around g = -5.5, where erff rounds to -1 and the result is 0 instead of -1e-7 (bf16 and fp32 resolve
    # that, fp16 does not); down to g = -4 the 16-bit results are within 1 ulp.
    ("vtm_geglu", "fp32"): {"all": (867252673, 68337), "g>=-6": (867252673, 46042), "g>=-4": (4091, 33001), "g>=0": (2, 13)},
    ("vtm_geglu", "fp16"): {"all": (2, 10), "g>=-6": (2, 10), "g>=-4": (1, 0), "g>=0": (1, 0)},
    ("vtm_geglu", "bf16"): {"all": (13215, 187), "g>=-6": (13215, 36), "g>=-4": (0, 0), "g>=0": (0, 0)},
    ("vtm_ff_geglu", "fp16"): {"all": (1, 0), "g>=-6": (1, 0), "g>=-4": (1, 0), "g>=0": (1, 0)},
    # the 106 gates all lie below g = -6 (|gelu(g)| < 6e-9); the largest distance is at g = -13.25, where the fp32 result
    # is itself subnormal
    ("vtm_ff_geglu", "bf16"): {"all": (33, 106), "g>=-6": (1, 0), "g>=-4": (1, 0), "g>=0": (0, 0)},
}


def _gelu_figures(kernel, got, gates):
    """Compare gelu(g) (the kernel's result with value = 1) with the float64 chain; print and return the figures."""
    ref = _gelu_ref(gates)
    fin = torch.isfinite(gates)
    assert torch.isfinite(got[fin]).all()
    d = (_ordered(got) - _ordered(ref)).abs()
    out = {}
    for name, lo in REGIONS:
        m = fin & (gates.double() >= lo)
        out[name] = (int(d[m].max()), int((d[m] > 1).sum()))
    worst = gates.flatten()[torch.where(fin, d, torch.zeros_like(d)).flatten().argmax()].item()
    print(f"\n[gelu ulps] {kernel} {IDS[gates.dtype]}: " + ", ".join(f"{k}: max {v[0]} ulp, {v[1]} gates > 1 ulp" for k, v in out.items())
          + f"; worst gate {worst!r}")
    return out


def _gelu_assert(kernel, dtype, figures):
    measured = GELU_MEASURED.get((kernel, IDS[dtype]))
    assert measured is not None, f"no measured figures for {kernel} {IDS[dtype]}: {figures}"
    for name, (mx, _) in figures.items():
        assert mx <= measured[name][0] + 1, (kernel, IDS[dtype], name, figures, measured)


def _product_check(got, value, gelu_kernel, gates, tag):
    """value * gelu(g): the kernel's own gelu(g) (its value = 1 result), times the value, rounded once.  The product of two
    16-bit values is exact in fp32."""
    fin = torch.isfinite(gates)
    want = (value.float() * gelu_kernel.float()).to(got.dtype)
    assert torch.equal(_ordered(got)[fin], _ordered(want)[fin]), tag


def _geglu_run(L, value, gates):
    D = 1024
    x = torch.cat([value.reshape(-1, D), gates.reshape(-1, D)], dim=1).contiguous()
    return L.geglu(x).reshape(gates.shape)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_geglu_every_gate_in_ulps(L, dtype):
    """vtm_geglu over every 16-bit gate (fp32: 2^20 gates), values 1, -3 and random normal.

    Measured figures: GELU_MEASURED and DESIGN.md (feed-forward section)."""
    gates = _fp32_gates() if dtype == F32 else _all_16bit_gates(dtype)
    gelu = _geglu_run(L, _values(1.0, gates, 0), gates)
    figures = _gelu_figures("vtm_geglu", gelu, gates)
    for kind in (-3.0, "normal"):
        v = _values(kind, gates, 10)
        _product_check(_geglu_run(L, v, gates), v, gelu, gates, (IDS[dtype], kind))
    _gelu_assert("vtm_geglu", dtype, figures)


def _fused_run(L, value, gates, bias=None):
    """vtm_ff_geglu with an exact projection: K = 64, token k is the unit vector e_k, so the GEMM returns column k of the
    weight panel.  value, gates: (D, 64) -- channel c of token k.  Weight rows packed tile by tile, 64 value rows then
    their 64 gate rows, as test_panel_gemm_fuzz_vs_torch_fp32 does."""
    D, K = value.shape
    assert K == 64 and D % 64 == 0
    x = torch.eye(K, dtype=value.dtype, device=DEV)
    w = torch.cat([value, gates], dim=0).contiguous()
    t = torch.arange(D // 64, device=DEV)[:, None] * 64 + torch.arange(64, device=DEV)[None, :]
    order = torch.cat([t, t + D], dim=1).reshape(-1).to(torch.int32)
    wp = L.to_panels(w, order)
    hp = L.ff_geglu(L.to_panels(x), K, wp, D, None if bias is None else bias[order.long()].contiguous())
    return hp[:, :K].permute(1, 0, 2).reshape(K, D).t().contiguous()


@pytest.mark.parametrize("dtype", [F16, BF16], ids=IDS.get)
def test_ff_geglu_every_gate_in_ulps(L, dtype):
    """The fused epilogue of vtm_ff_geglu (the A&S 7.1.26 erfc polynomial on the hardware reciprocal and exponential) over
    every 16-bit gate.  Gate c * 64 + k of the sweep is weight row D + c, column k; a non-finite weight spoils the other
    63 products of its row (0 * inf), and the non-finite patterns fill whole rows among themselves.

    Measured figures: GELU_MEASURED and DESIGN.md (feed-forward section)."""
    D = 1024
    gates = _all_16bit_gates(dtype).reshape(D, 64)
    gelu = _fused_run(L, _values(1.0, gates, 0), gates)
    figures = _gelu_figures("vtm_ff_geglu", gelu, gates)
    for kind in (-3.0, "normal"):
        v = _values(kind, gates, 11)
        _product_check(_fused_run(L, v, gates), v, gelu, gates, (IDS[dtype], kind))
    _gelu_assert("vtm_ff_geglu", dtype, figures)


def test_geglu_grid_stride(L):
    """geglu_kernel<__half> one row beyond 65 536 blocks: 131 073 rows of D = 1024 (0.5 GB in).  The input repeats a block of
    1 021 rows (a prime: no multiple of the grid's stride of 131 072 rows), so the result must repeat the result of that
    block, which is a single-pass launch, bit for bit."""
    _pinned("geglu.hip")
    D, base_rows, dtype = 1024, 1021, F16
    chunks = D * _esize(dtype) // 16
    rows = GEGLU_GRID_CAP * BLOCK // chunks + 1
    assert -(-rows * chunks // BLOCK) > GEGLU_GRID_CAP >= -(-base_rows * chunks // BLOCK)
    base = (2.0 * torch.randn(base_rows, 2 * D, device=DEV, generator=_gen(12))).to(dtype)
    want = L.geglu(base)
    reps = -(-rows // base_rows)
    x = base.repeat(reps, 1)[:rows].contiguous()
    _poison(rows * D * _esize(dtype))
    y = L.geglu(x)
    assert y.shape == (rows, D)
    full = (rows // base_rows) * base_rows
    assert (_bits(y[:full]).view(-1, base_rows, D) == _bits(want)[None]).all()
    assert torch.equal(_bits(y[full:]), _bits(want[:rows - full]))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_gelu_special_gates(L, dtype):
    """NaN stays NaN, gelu(+inf) = +inf, gelu(+-0) = 0; gelu(-inf) is NaN in both kernels, as in torch's erf form
    (0.5 * -inf * (1 + erf(-inf)) = -inf * 0).  The fused kernel gets its special gates through the fp32 bias over a zero
    projection."""
    specials = torch.tensor([math.nan, math.inf, -math.inf, 0.0, -0.0], device=DEV)
    t = torch.nn.functional.gelu(specials.to(dtype)).float()
    outs = {"torch": t}
    g = specials.to(dtype).repeat(8).reshape(1, 40)                               # D = 40: a multiple of 8
    outs["vtm_geglu"] = L.geglu(torch.cat([torch.ones_like(g), g], dim=1).contiguous()).float().reshape(-1)[:5]
    if dtype != F32:
        D = 64
        bias = torch.cat([torch.ones(D, device=DEV), specials.repeat(13)[:D]])   # value rows 1, gate rows the specials
        zeros = torch.zeros(D, 64, dtype=dtype, device=DEV)
        outs["vtm_ff_geglu"] = _fused_run(L, zeros, zeros, bias)[:5, 0].float()
    for name, o in outs.items():
        print(f"\n[gelu specials] {IDS[dtype]} {name}: {o.tolist()}")
        assert math.isnan(o[0]) and o[1] == math.inf and math.isnan(o[2]), name
        assert o[3] == 0 and o[4] == 0 and not torch.signbit(o[3]), name
        if name == "vtm_geglu":     # the sign of gelu(-0) as torch returns it for this dtype (measured: -0 in fp32 and bf16, +0 in
            assert torch.signbit(o[4]) == torch.signbit(t[4]), name     # fp16; the fused kernel's gate is +0 + bias = +0)
