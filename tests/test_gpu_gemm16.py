"""GPU tests of the two 16-bit projection GEMM families of the default path (run with -m gpu on an MI355X): `vtm_linear_rows`
(csrc/linear.hip: the weight-stationary K = 320 kernel, the tiled <160, 80> kernel, the small-K <32, 32> kernel) and the panel
GEMM behind `vtm_linear_panels` / `vtm_ff_geglu` (csrc/ff.hip).

1. exact integers   operands in {-1, 0, 1}, integer bias / residual: every product and every fp32 partial sum is exact and
                    the result is a value of the format, so the kernel must equal a float64 matmul BIT FOR BIT, in any
                    summation order, tile and layout.  Shapes cross every tile edge and launcher threshold (restated below
                    and pinned to the source text they restate).
2. rounding order   the same with the weights scaled so that sums land where the format's spacing is 2 ... 8: the chain of
                    roundings include/vidtome_hip.h promises, bit for bit, with planted elements where a single and a
                    double rounding differ.
3. poison           every output layout into a sentinel-filled buffer: nothing but the valid elements is written.
4. float64 bound    Gaussian data over 24 binades: |got - ref| <= 1/2 ulp(|ref| + gamma) + gamma per element,
                    gamma = 2 K 2^-24 (sum |a w| + |bias|), propagated through the chained epilogues.
5. inf / NaN rows   against torch's CPU result.

(A zero counts as equal to a zero of the other sign: the sign of an exact zero sum depends on the summation order.)
"""
import itertools
import math
import os
from types import SimpleNamespace

import pytest
import torch

from helpers import EXACT_INT_MAX, int_uniform, is_sentinel, rounding_bound, same_bits, sentinel_filled

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [F16, BF16]
IDS = {F16: "fp16", BF16: "bf16"}
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vidtome_amd", "csrc")

# ---- the launchers' constants and conditions, restated (each with the source text it restates) ----
TM = 128                                  # linear.hip: token rows per workgroup of the tiled / small-K kernel
WS_K, WS_TN, WS_NW = 320, 160, 8          # linear.hip: the weight-stationary kernel
FBD, FBS, FBK, MAX_TILES_PER_WG = 128, 256, 64, 16   # ff.hip
_PINS = {
    "linear.hip": [
        "constexpr int TM = 128, NT = 256;",
        "constexpr int WS_K = 320, WS_TN = 160, WS_LDW = WS_K + 8;",
        "#define VTM_WS_WAVES 8",
        "if (K == WS_K && N % WS_TN == 0 && (ldo & 7) == 0 && (obs & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&",
        "int64_t bpw = vtm::cdiv(RB * halves * B, (int64_t)vtm::device_cus() * WS_NW);",
        "const int64_t spans = vtm::cdiv(RB, WS_NW * bpw);",
        "const int tn = (N % 160 == 0) ? 160 : 128;",
        "if (K % 320 == 0) {",
        "if (transposed) VTM_LIN_TN(true, 160, 80, true); else VTM_LIN_TN(false, 160, 80, true);",
        "if (transposed) VTM_LIN_TN(true, 32, 32, false); else VTM_LIN_TN(false, 32, 32, false);",
        "const bool vec_ok = ((ldo & 7) == 0) && ((reinterpret_cast<uintptr_t>(ob) & 15) == 0);",
        "const bool vec4_ok = ((ldo & 3) == 0) && ((reinterpret_cast<uintptr_t>(ob) & 7) == 0);",
    ],
    "ff.hip": [
        "constexpr int FBD = 128;", "constexpr int FBS = 256;", "constexpr int FBK = 64;",
        "constexpr int MAX_TILES_PER_WG = 16;",
        "const int ns_tiles = (int)vtm::cdiv(n, FBS), nd_tiles = (int)vtm::cdiv(Nw, FBD);",
        "const int max_patch = (int64_t)16 * FBS * K * 2 <= (3 << 20) ? 16 : 8;",
        "const int tiles_per_xcd = (int)vtm::cdiv(total_src_tiles, 8);",
        "const int patches_per_xcd = (int)vtm::cdiv(tiles_per_xcd, max_patch);",
        "const int patch_tiles = (int)vtm::cdiv(tiles_per_xcd, patches_per_xcd);",
        "const int64_t slots = (int64_t)vtm::device_cus() * 2;",
        # the four lines that decide how many weight tiles one workgroup walks through
        "int64_t nsplit = vtm::cdiv(3 * slots, (int64_t)ns_tiles);",
        "nsplit = std::max<int64_t>(nsplit, vtm::cdiv(nd_tiles, MAX_TILES_PER_WG));",
        "nsplit = std::min<int64_t>(std::max<int64_t>(nsplit, 1), nd_tiles);",
        "const int tiles_per_split = (int)vtm::cdiv(nd_tiles, nsplit);",
    ],
}


def _pinned(fname):
    """The tests' precondition: the dispatch conditions of `fname` still read as restated here."""
    with open(os.path.join(CSRC, fname)) as f:
        src = f.read()
    for text in _PINS[fname]:
        assert text in src, f"{fname} no longer contains {text!r}: re-derive the shapes of this file from the new condition"


def _cdiv(a, b):
    return -(-a // b)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rows_kernel(K, N, ldo, obs, base_aligned=True):
    """(family, output channels per workgroup) that linear.hip's launch() picks."""
    _pinned("linear.hip")
    if K == WS_K and N % WS_TN == 0 and ldo % 8 == 0 and obs % 8 == 0 and base_aligned:
        return "ws", WS_TN
    return ("tiled" if K % 320 == 0 else "small"), (160 if N % 160 == 0 else 128)


def _ws_blocks_per_wave(n, N, B):
    _pinned("linear.hip")
    return max(1, _cdiv(_cdiv(n, 32) * (N // WS_TN) * B, _cus() * WS_NW))


def _panel_plan(n, Nw, K):
    """launch_panel_gemm's work split for n token rows x Nw weight rows, from the restated lines."""
    _pinned("ff.hip")
    ns_tiles, nd_tiles = _cdiv(n, FBS), _cdiv(Nw, FBD)
    max_patch = 16 if 16 * FBS * K * 2 <= (3 << 20) else 8
    tiles_per_xcd = _cdiv(ns_tiles, 8)
    patch_tiles = _cdiv(tiles_per_xcd, _cdiv(tiles_per_xcd, max_patch))
    slots = _cus() * 2
    nsplit = _cdiv(3 * slots, ns_tiles)
    nsplit = max(nsplit, _cdiv(nd_tiles, MAX_TILES_PER_WG))
    nsplit = min(max(nsplit, 1), nd_tiles)
    return SimpleNamespace(ns_tiles=ns_tiles, nd_tiles=nd_tiles, max_patch=max_patch, patch_tiles=patch_tiles,
                           tiles_per_split=_cdiv(nd_tiles, nsplit))


def _smallest_n(pred):
    """The smallest n = 256 m + 3 for which pred(n) holds (pred is monotone in n)."""
    m = next(m for m in range(1, 4096) if pred(256 * m + 3))
    assert m == 1 or not pred(256 * (m - 1) + 3)
    return 256 * m + 3


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _same(got, want):
    return same_bits(got, want) | ((got == 0) & (want == 0))


def _assert_same(got, want, tag):
    ok = _same(got, want)
    if not bool(ok.all()):
        at = (~ok).nonzero()[0].tolist()
        raise AssertionError(f"{tag}: {int((~ok).sum())} of {ok.numel()} elements differ, first at {at}: "
                             f"got {got[tuple(at)].item()}, want {want[tuple(at)].item()}")


def _assert_exact_range(z, dtype, tag):
    """§1's condition, on the reference alone: every result is an integer that the format holds."""
    assert float(z.abs().max()) <= EXACT_INT_MAX[IDS[dtype]], (tag, float(z.abs().max()))


# ---------------------------------------------------------------------------------------------------
# vtm_linear_rows: operands, maps, reference
# ---------------------------------------------------------------------------------------------------
MAPS = ("rows", "both", "rows2", "id")     # one-level map, two-level map, rows2 alone, identity


class _Rows:
    """Integer operands of one (dtype, K, N): tokens and weights in {-1, 0, 1} (weights times `wscale`), bias in [-8, 8]."""

    def __init__(self, dtype, B, P0, P1, K, N, seed, wscale=1):
        self.g = g = _gen(seed)
        self.dtype, self.B, self.P0, self.P1, self.K, self.N = dtype, B, P0, P1, K, N
        self.x0 = int_uniform((B, P0, K), -1, 1, dtype, g)
        self.x1 = int_uniform((B, P1, K), -1, 1, dtype, g)
        self.W = int_uniform((N, K), -1, 1, dtype, g) * wscale
        self.bias = int_uniform((N,), -8, 8, dtype, g)

    def maps(self, kind, use_x1, n):
        """(rows, rows2, composed pool ids (B, n) int64)."""
        B, P, g = self.B, self.P0 + (self.P1 if use_x1 else 0), self.g
        ri = lambda hi, shape: torch.randint(0, hi, shape, generator=g, device=DEV, dtype=torch.int32)
        if kind == "rows":
            rows = ri(P, (B, n))
            return rows, None, rows.long()
        if kind == "both":
            M = n + 13
            rows, rows2 = ri(P, (B, M)), ri(M, (B, n))
            return rows, rows2, torch.gather(rows.long(), 1, rows2.long())
        if kind == "rows2":
            rows2 = ri(P, (B, n))
            return None, rows2, rows2.long()
        assert n <= P
        return None, None, torch.arange(n, device=DEV).expand(B, n)

    def sums(self, idx, use_x1):
        """(B, n, N) float64: the gathered rows times W^T."""
        pool = torch.cat([self.x0, self.x1], dim=1) if use_x1 else self.x0
        a = torch.gather(pool, 1, idx[..., None].expand(-1, -1, self.K))
        return a.double() @ self.W.double().T

    def run(self, L, kind, use_x1, n, transposed, with_bias, **kw):
        """-> (what the library returned, float64 sums + bias (B, n, N))."""
        rows, rows2, idx = self.maps(kind, use_x1, n)
        y = L.linear_rows(self.x0, self.x1 if use_x1 else None, rows, rows2, n, self.W, self.bias if with_bias else None,
                          transposed=transposed, **kw)
        z = self.sums(idx, use_x1)
        return y, (z + self.bias.double() if with_bias else z)


def _valid(y, n, N, transposed):
    """The valid (B, n, N) part of a linear_rows result of either layout."""
    return y[:, :N, :n].transpose(1, 2) if transposed else y[:, :n, :N]


def _check_allocated(y, z, n, N, transposed, dtype, tag):
    """A result the wrapper allocated (n padded to 8, the padding zero) against the exact reference z."""
    B = z.shape[0]
    n8 = _cdiv(n, 8) * 8
    assert y.shape == ((B, N, n8) if transposed else (B, n8, N)) and y.dtype == dtype, tag
    _assert_exact_range(z, dtype, tag)
    _assert_same(_valid(y, n, N, transposed), z.to(dtype), tag)
    assert not bool((y[:, :, n:] if transposed else y[:, n:]).any()), (tag, "padding")


def _rows_exact(L, ops, ns, family, big=()):
    """Every n x layout x map kind, with and without x1 / bias (the large `big` sizes: x1 and bias alternate)."""
    K, N, dtype = ops.K, ops.N, ops.dtype
    flip = itertools.cycle((False, True, True, False, True))
    for n in tuple(ns) + tuple(big):
        for transposed, kind in itertools.product((False, True), MAPS):
            for use_x1 in ((next(flip),) if n in big else (False, True)):
                if kind == "id" and not use_x1 and n > ops.P0:
                    continue
                ldo = _cdiv(n, 8) * 8 if transposed else N
                assert _rows_kernel(K, N, ldo, ldo * (N if transposed else _cdiv(n, 8) * 8))[0] == family
                with_bias = next(flip)
                y, z = ops.run(L, kind, use_x1, n, transposed, with_bias)
                _check_allocated(y, z, n, N, transposed, dtype,
                                 f"{family} K={K} N={N} n={n} {'T' if transposed else 'R'} {kind} x1={use_x1} bias={with_bias}")


# ---------------------------------------------------------------------------------------------------
# 1. exact integers: vtm_linear_rows
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (160, 320, 640))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_rows_exact_weight_stationary(L, dtype, N):
    """linear_rows_ws_kernel: n around the 32-token block, and the smallest n that gives every wave two blocks (B = 2, so
    that q / spans and the 8-per-XCD slot arithmetic see a second sample) plus 5: a ragged last block."""
    B, halves = 2, N // WS_TN
    n_two = 32 * ((_cus() * WS_NW) // (halves * B)) + 1
    assert _ws_blocks_per_wave(n_two, N, B) == 2 and _ws_blocks_per_wave(n_two - 1, N, B) == 1
    n_big = n_two + 5
    ops = _Rows(dtype, B, n_big, 97, WS_K, N, seed=N)
    _rows_exact(L, ops, (1, 31, 32, 33, 257), "ws", big=(n_big,))


TILED_SHAPES = [(640, 160), (1280, 320), (640, 96), (320, 192), (1280, 136), (640, 100), (640, 37)]


@pytest.mark.parametrize("K,N", TILED_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_rows_exact_tiled(L, dtype, K, N):
    """linear_rows_kernel<160, 80, true, TN>: TN = 160 and 128, a ragged last channel tile, N % 8 != 0 and N % 4 != 0 (the
    partial 8-element pieces of the staged store; N % 8 != 0 also makes ldo % 8 != 0 token-major: the scalar stores), n around
    the 128-token tile and over more than two of them."""
    assert _rows_kernel(K, N, N, 8 * N)[1] == (160 if N % 160 == 0 else 128)
    ops = _Rows(dtype, 2, 307, 110, K, N, seed=K + N)
    _rows_exact(L, ops, (1, 127, 128, 129, 300), "tiled")


@pytest.mark.parametrize("N", (160, 320))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_rows_exact_tiled_k320_through_an_unaligned_view(L, dtype, N):
    """K = 320 with whole 160-channel halves reaches the tiled kernel only when the output rows are not 16-byte aligned: an
    `out` view with ldo % 8 != 0 (which is also the staged path's scalar store with nothing ragged about N)."""
    B, K = 2, WS_K
    ops = _Rows(dtype, B, 307, 110, K, N, seed=3 * N)
    for n, transposed, kind in itertools.product((1, 127, 129, 300), (False, True), MAPS):
        rows_, cols = (N, n) if transposed else (n, N)
        ldo = cols + 3 if (cols + 3) % 8 else cols + 1
        buf = sentinel_filled((B, rows_ + 1, ldo), dtype)
        assert _rows_kernel(K, N, ldo, buf.stride(0)) == ("tiled", 160)
        y, z = ops.run(L, kind, True, n, transposed, True, out=buf[:, :rows_, :cols])
        assert y.data_ptr() == buf.data_ptr()
        tag = f"K=320 N={N} n={n} {'T' if transposed else 'R'} {kind} ldo={ldo}"
        _assert_exact_range(z, dtype, tag)
        _assert_same(_valid(buf, n, N, transposed), z.to(dtype), tag)
        assert bool(is_sentinel(buf[:, rows_:]).all()) and bool(is_sentinel(buf[:, :, cols:]).all()), tag


@pytest.mark.parametrize("K", (32, 64, 96, 352))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_rows_exact_small_k(L, dtype, K):
    """linear_rows_kernel<32, 32, false, TN>: one chunk, an even and two odd chunk counts (the PAIRS = false tail), N below a
    tile, ragged in 4 and in 8, whole tiles of 128 and 160, and two tiles."""
    for N in (8, 37, 128, 160, 200):
        ops = _Rows(dtype, 2, 307, 110, K, N, seed=K + N)
        _rows_exact(L, ops, (1, 127, 128, 129, 300), "small")


# ---------------------------------------------------------------------------------------------------
# panel GEMM: operands and references
# ---------------------------------------------------------------------------------------------------
def _panel_valid(p, n, C):
    """Rows < n of a panel tensor (C / 8, rows_pad, 8) as (n, C)."""
    return p[:, :n].permute(1, 0, 2).reshape(n, C)


def _geglu_pack(L, w, b, D):
    """W1 (2 D, K) = [value rows; gate rows] and its fp32 bias in the tile order vtm_ff_geglu reads (include/vidtome_hip.h)."""
    t = torch.arange(D // 64, device=DEV)[:, None] * 64 + torch.arange(64, device=DEV)[None, :]
    order = torch.cat([t, t + D], dim=1).reshape(-1)
    return L.to_panels(w, order.to(torch.int32)), b[order].contiguous()


def _gelu64(g):
    return 0.5 * g * torch.special.erfc(-g / math.sqrt(2.0))


def _rn(z, dtype):
    """Round float64 values once to the format, back in float64."""
    return z.to(dtype).double()


PANEL_KT = (1, 2, 3, 4, 5, 20)           # K / 64: every prologue / tail stage of the pipelined loop; 20 is past max_patch's 384
PANEL_N = (1, 255, 256, 257, 2305)       # token rows; 2305 -> ns_tiles = 10 > 8 -> patch_tiles = 2
GATE_SHIFT = 130                         # added to the gate bias: every gate an integer in [10, 250]


@pytest.mark.parametrize("kt", PANEL_KT)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_linear_panels_exact(L, dtype, kt):
    """vtm_linear_panels on integers, every bias / residual combination; half of the calls take both operands as row ranges
    of larger panel tensors (whose other rows then sit where a whole operand has its zero padding)."""
    K, n_max, N_max, r0, w0 = 64 * kt, PANEL_N[-1], 2176, 3, 5
    assert _panel_plan(n_max, N_max, K).patch_tiles == 2
    assert _panel_plan(n_max, N_max, K).max_patch == (16 if K <= 384 else 8)
    g = _gen(kt)
    x = int_uniform((n_max + FBS, K), -1, 1, dtype, g)          # + a tile: a row range at r0 stays inside the tensor
    w = int_uniform((N_max + w0, K), -1, 1, dtype, g)
    bias = int_uniform((N_max,), -8, 8, torch.float32, g)
    resid = int_uniform((n_max, N_max), -16, 16, dtype, g)
    S = x.double() @ w.double().T
    xp_all, wp_all = L.to_panels(x), L.to_panels(w)
    assert r0 + _cdiv(n_max, FBS) * FBS <= xp_all.shape[1] and w0 + _cdiv(N_max, FBD) * FBD <= wp_all.shape[1]
    flip = itertools.cycle((False, True, True))
    for n, N in itertools.product(PANEL_N, (8, 128, 136, 2176)):
        for hb, hr in itertools.product((False, True), repeat=2):
            if next(flip):
                xp, wp, z = xp_all[:, r0:], wp_all[:, w0:], S[r0:r0 + n, w0:w0 + N]
            else:
                xp, wp, z = L.to_panels(x[:n]), L.to_panels(w[:N]), S[:n, :N]
            b, r = (bias[:N].contiguous() if hb else None), (resid[:n, :N].contiguous() if hr else None)
            y = L.linear_panels(xp, n, wp, N, b, r)
            z = z + b.double() if hb else z
            tag = f"K={K} n={n} N={N} bias={hb} resid={hr}"
            _assert_exact_range(z, dtype, tag)
            want = z.to(dtype)
            if hr:
                _assert_exact_range(z + r.double(), dtype, tag)
                want = (want.double() + r.double()).to(dtype)
            assert y.shape == (n, N)
            _assert_same(y, want, tag)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_linear_panels_swapped_operands(L, dtype):
    """V^T = W X^T: the weight as the "token" operand, one sample's token rows (n padded to 8) as the "weight", into a
    preallocated view with a longer row."""
    for K, N, n in ((64, 8, 1), (320, 136, 255), (192, 320, 257), (1280, 128, 1001)):
        g = _gen(K + n)
        x, w = int_uniform((n, K), -1, 1, dtype, g), int_uniform((N, K), -1, 1, dtype, g)
        xp, wp = L.to_panels(x), L.to_panels(w)
        n8 = _cdiv(n, 8) * 8
        yt = sentinel_filled((N + 2, L.panel_rows(n) + 8), dtype)
        L.linear_panels(wp, N, xp, n8, None, out=yt)
        z = w.double() @ x.double().T
        _assert_exact_range(z, dtype, (K, N, n))
        _assert_same(yt[:N, :n], z.to(dtype), f"swapped K={K} N={N} n={n}")
        assert not bool(yt[:N, n:n8].any())                       # the zero padding rows of the token panels
        assert bool(is_sentinel(yt[N:]).all()) and bool(is_sentinel(yt[:, n8:]).all())


def _compare_in_row_chunks(got, x, w, epilogue, tag, rows=8192):
    """got (n, ..) against epilogue(float64 x[i0:i1] @ w^T) -> the expected 16-bit rows, on the device, a chunk of rows at a
    time (the float64 form of the largest result would take 6.4 GB)."""
    wd = w.double().T.contiguous()
    for i0 in range(0, x.shape[0], rows):
        i1 = min(i0 + rows, x.shape[0])
        want = epilogue(x[i0:i1].double() @ wd, i0, i1)
        _assert_same(got[i0:i1], want, f"{tag} rows {i0}..{i1}")


def _multi_tile_cases():
    """(name, Nw, K, n, check on the plan): the smallest n = 256 m + 3 at which a workgroup walks through 2 / 16 weight tiles
    of Nw = 10240 weight rows, a 17-tile weight (N = 2176) with two tiles per workgroup, and the same past max_patch's K = 384
    with more than 8 token tiles per XCD (the only place where the 16 -> 8 switch changes patch_tiles)."""
    t = lambda Nw, K, want: _smallest_n(lambda n: _panel_plan(n, Nw, K).tiles_per_split >= want)
    return [("2 tiles", 10240, 64, t(10240, 64, 2), lambda p: p.tiles_per_split == 2),
            ("16 tiles", 10240, 64, t(10240, 64, 16), lambda p: p.tiles_per_split == MAX_TILES_PER_WG),
            ("17-tile weight", 2176, 64, t(2176, 64, 2), lambda p: p.nd_tiles == 17 and p.tiles_per_split >= 2),
            ("17-tile weight, K = 448", 2176, 448, max(t(2176, 448, 2), 8 * 8 * FBS + 3),
             lambda p: p.tiles_per_split >= 2 and p.max_patch == 8 and p.patch_tiles < _cdiv(p.ns_tiles, 8) <= 16)]


@pytest.mark.parametrize("case", range(4), ids=["2-tiles", "16-tiles", "17-tile-weight", "17-tile-weight-K448"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_linear_panels_several_weight_tiles_per_workgroup(L, dtype, case):
    """The loop over several weight tiles inside one workgroup: the epilogue between tiles inside the pipelined k-loop, the
    (jt - jt0) FBD bias slice, the MAX_TILES_PER_WG cap.  Sizes derived from the launcher's formula for this device's CU
    count (256 CUs: n = 4867, 78595, 24323, 24323)."""
    name, N, K, n, holds = _multi_tile_cases()[case]
    plan = _panel_plan(n, N, K)
    assert holds(plan), (name, n, vars(plan))
    print(f"\n[panel GEMM] {name}: {_cus()} CUs -> n = {n}, N = {N}, K = {K}, plan {vars(plan)}")
    g = _gen(case)
    x, w = int_uniform((n, K), -1, 1, dtype, g), int_uniform((N, K), -1, 1, dtype, g)
    bias = int_uniform((N,), -8, 8, torch.float32, g)
    y = L.linear_panels(L.to_panels(x), n, L.to_panels(w), N, bias)

    def epilogue(s, i0, i1):
        z = s + bias.double()
        _assert_exact_range(z, dtype, name)
        return z.to(dtype)
    _compare_in_row_chunks(y, x, w, epilogue, f"{name} n={n}")


def _geglu_reference(s, b, D, dtype, exact):
    """The chain include/vidtome_hip.h states for vtm_ff_geglu, from the float64 sums s (n, 2 D) = [value | gate] and the bias
    b (2 D): RN(RN(value) * RN(gelu(RN(gate)))).  `exact`: §1's conditions are asserted (value a held integer, every gate an
    integer in [10, 250] -- there gelu(g) rounds back to g, so the product is that of two integers, rounded once)."""
    z = s + b.double()
    v, gt = z[:, :D], z[:, D:]
    if exact:
        _assert_exact_range(v, dtype, "geglu value")
        assert float(gt.min()) >= 10 and float(gt.max()) <= 250 and bool((gt == gt.round()).all())
        assert bool((_rn(_gelu64(gt), dtype) == gt).all())        # gelu(g) rounds back to g: 1.5e-7 g is far below half an ulp
    h = _rn(_gelu64(_rn(gt, dtype)), dtype)
    return (_rn(v, dtype) * h).to(dtype)                          # the float64 product of two 16-bit values is exact


@pytest.mark.parametrize("kt", PANEL_KT)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_ff_geglu_exact(L, dtype, kt):
    """vtm_ff_geglu on integers: value * gelu(gate) with every gate shifted to an integer in [10, 250]."""
    K, n_max, D_max = 64 * kt, PANEL_N[-1], 5120
    g = _gen(100 + kt)
    x = int_uniform((n_max, K), -1, 1, dtype, g)
    w = int_uniform((2 * D_max, K), -1, 1, dtype, g)
    if K > 640:
        # 12 million gate sums of 1280 uniform products (deviation 24) reach past +-130, outside the [10, 250] that the
        # shift allows inside bf16's integers: half of the gate weights are zeroed here (deviation 17: 112 is 6.6 of them)
        w[D_max:] *= int_uniform((D_max, K), 0, 1, dtype, g)
    b = int_uniform((2 * D_max,), -8, 8, torch.float32, g)
    b[D_max:] += GATE_SHIFT
    S = x.double() @ w.double().T
    for D in (64, 192, 1280, 5120):
        sel = torch.cat([torch.arange(D, device=DEV), D_max + torch.arange(D, device=DEV)])
        wp, bp = _geglu_pack(L, w[sel].contiguous(), b[sel], D)
        for n in PANEL_N:
            hp = L.ff_geglu(L.to_panels(x[:n]), n, wp, D, bp)
            assert hp.shape == (D // 8, L.panel_rows(n), 8)
            want = _geglu_reference(S[:n][:, sel], b[sel], D, dtype, exact=True)
            _assert_same(_panel_valid(hp, n, D), want, f"geglu K={K} D={D} n={n}")


@pytest.mark.parametrize("tiles", (2, 16))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_ff_geglu_several_weight_tiles_per_workgroup(L, dtype, tiles):
    """D = 5120 (2 D = 10240 packed weight rows, 80 tiles) at the token counts that make a workgroup walk through 2 and 16 of
    them."""
    D, K = 5120, 64
    n = _smallest_n(lambda n_: _panel_plan(n_, 2 * D, K).tiles_per_split >= tiles)
    assert _panel_plan(n, 2 * D, K).tiles_per_split == tiles
    g = _gen(200 + tiles)
    x = int_uniform((n, K), -1, 1, dtype, g)
    w = int_uniform((2 * D, K), -1, 1, dtype, g)
    b = int_uniform((2 * D,), -8, 8, torch.float32, g)
    b[D:] += GATE_SHIFT
    wp, bp = _geglu_pack(L, w, b, D)
    hp = L.ff_geglu(L.to_panels(x), n, wp, D, bp)
    got = _panel_valid(hp, n, D)
    _compare_in_row_chunks(got, x, w, lambda s, i0, i1: _geglu_reference(s, b, D, dtype, exact=True), f"geglu {tiles} tiles n={n}")


# ---------------------------------------------------------------------------------------------------
# 2. rounding order: integers beyond the exact range
# ---------------------------------------------------------------------------------------------------
# weight scales: sums become multiples of 64 / 8 (fp16 / bf16) whose tails reach the binades where the spacing is 2 ... 8, so
# that sum + bias is no value of the format there; at eight times that most of the result lies in those binades
WSCALE = {F16: (64, 512), BF16: (8, 64)}
MIN_INEXACT = (0.0, 0.2)                 # share of the results that a rounding changes, at least (measured on the reference)
TOP = {F16: 2048.0, BF16: 256.0}         # the first integer whose successor the format does not hold


def _inexact_share(z, dtype):
    return float((_rn(z, dtype) != z).double().mean())


@pytest.mark.parametrize("big", (0, 1), ids=["scale", "scale-x8"])
@pytest.mark.parametrize("K,N", [(320, 320), (640, 100), (96, 37)], ids=["ws", "tiled", "small-k"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_rows_rounding_order(L, dtype, K, N, big):
    """vtm_linear_rows = RN(sum + bias): one rounding of the exact fp32 value.  Planted element (token 5, channel 2 of sample 0):
    sum = TOP + 1, bias = 1 -> TOP + 2 is a value; rounding the sum first would give RN(TOP + 1) + 1 -> TOP."""
    B, n, top = 2, 129, TOP[dtype]
    ops = _Rows(dtype, B, n, 0, K, N, seed=K, wscale=WSCALE[dtype][big])
    ops.x0[0, 5] = 0
    ops.x0[0, 5, :2] = 1
    ops.W[2] = 0
    ops.W[2, 0], ops.W[2, 1], ops.bias[2] = top, 1, 1
    for transposed in (False, True):
        y, z = ops.run(L, "id", False, n, transposed, True)
        want, other = z.to(dtype), (_rn(z - ops.bias.double(), dtype) + ops.bias.double()).to(dtype)
        assert z[0, 5, 2] == top + 2 and want[0, 5, 2] == top + 2 and other[0, 5, 2] == top
        assert _inexact_share(z, dtype) > MIN_INEXACT[big]       # the rounding is exercised all over the result
        _assert_same(_valid(y, n, N, transposed), want, f"rows rounding K={K} N={N} T={transposed}")


@pytest.mark.parametrize("big", (0, 1), ids=["scale", "scale-x8"])
@pytest.mark.parametrize("kt", (1, 5, 20))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_linear_panels_rounding_order(L, dtype, kt, big):
    """vtm_linear_panels = RN(RN(sum + bias) + resid).  Planted element (token 5, channel 2): sum = TOP, bias = 1, resid = 1:
    RN(TOP + 1) = TOP, RN(TOP + 1) = TOP; a single rounding of TOP + 2 gives TOP + 2."""
    K, n, N, top = 64 * kt, 257, 136, TOP[dtype]
    g = _gen(300 + kt)
    x = int_uniform((n, K), -1, 1, dtype, g)
    w = int_uniform((N, K), -1, 1, dtype, g) * WSCALE[dtype][big]
    bias = int_uniform((N,), -8, 8, torch.float32, g)
    resid = int_uniform((n, N), -16, 16, dtype, g)
    x[5] = 0
    x[5, 0] = 1
    w[2] = 0
    w[2, 0], bias[2], resid[5, 2] = top, 1, 1
    y = L.linear_panels(L.to_panels(x), n, L.to_panels(w), N, bias, resid)
    z = x.double() @ w.double().T + bias.double()
    want, single = (_rn(z, dtype) + resid.double()).to(dtype), (z + resid.double()).to(dtype)
    assert z[5, 2] == top + 1 and want[5, 2] == top and single[5, 2] == top + 2
    assert min(_inexact_share(z, dtype), _inexact_share(_rn(z, dtype) + resid.double(), dtype)) > MIN_INEXACT[big]
    _assert_same(y, want, f"panels rounding K={K}")


# (value weight scale, gate weight scale, gate bias: lowest, highest).  bf16 holds both sides scaled at once.  In fp16 a product
# of two values past 2048 overflows, so the sides take turns: values past 2048 meet gates of 10 ... 14 (the gate's weights are
# zero: the bias alone), gates past 2048 meet the unscaled values.
GEGLU_ROUNDING = [(BF16, 64, 8, 504, 520), (F16, 256, 0, 10, 14), (F16, 1, 8, 2296, 2312)]


@pytest.mark.parametrize("dtype,sv,sg,glo,ghi", GEGLU_ROUNDING, ids=["bf16-both", "fp16-value", "fp16-gate"])
def test_ff_geglu_rounding_order(L, dtype, sv, sg, glo, ghi):
    """vtm_ff_geglu = RN(RN(sum_v + b_v) * RN(gelu(RN(sum_g + b_g)))), gates kept large and positive (gelu(g) == g in fp32, so
    the chain is bitwise).  Planted element (token 5, channel 2): value TOP + 1 -> TOP, gate 10: TOP * 10 is a value, while the
    unrounded (TOP + 1) * 10 rounds 16 higher."""
    K, n, D, top = 64, 257, 192, TOP[dtype]
    g = _gen(400 + sv + sg)
    x = int_uniform((n, K), -1, 1, dtype, g)
    w = int_uniform((2 * D, K), -1, 1, dtype, g)
    w[:D] *= sv
    w[D:] *= sg
    b = int_uniform((2 * D,), -8, 8, torch.float32, g)
    b[D:] = int_uniform((D,), glo, ghi, torch.float32, g)
    x[5] = 0
    x[5, 0] = 1
    w[2], w[D + 2] = 0, 0
    w[2, 0], b[2], b[D + 2] = top, 1, 10
    wp, bp = _geglu_pack(L, w, b, D)
    hp = L.ff_geglu(L.to_panels(x), n, wp, D, bp)
    s = x.double() @ w.double().T
    z = s + b.double()
    want = _geglu_reference(s, b, D, dtype, exact=False)
    single = (z[:, :D] * _gelu64(z[:, D:])).to(dtype)
    assert z[5, 2] == top + 1 and z[5, D + 2] == 10 and want[5, 2] == top * 10 and single[5, 2] == top * 10 + 16
    assert float(z[:, D:].min()) >= 10                            # gelu(g) == g to far below the last bit of fp32
    assert _inexact_share(z[:, :D] if sv > 1 else z[:, D:], dtype) > 0.03
    assert float(torch.isfinite(want.float()).double().mean()) > 0.9
    _assert_same(_panel_valid(hp, n, D), want, f"geglu rounding {IDS[dtype]} sv={sv} sg={sg}")


# ---------------------------------------------------------------------------------------------------
# 3. writes nothing it must not
# ---------------------------------------------------------------------------------------------------
# (elements into the buffer, ldo - row length, out_batch_stride - rows * ldo)
LAYOUTS = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (4, 0, 0), (8, 0, 0), (0, 1, 0), (0, 3, 0), (0, 8, 0), (0, 0, 3), (0, 8, 4),
           (2, 3, 1), (4, 4, 4), (8, 8, 8),
           # aligned rows that end past a ragged N (ldo % 8 == 0 for N = 100 and for N = 37): the vector path's partial pieces
           (0, 4, 0), (8, 4, 0), (8, 3, 0)]
POISON_SHAPES = [("ws", 320, 160, 33), ("tiled", 640, 100, 33), ("tiled", 640, 37, 129), ("small", 32, 37, 33),
                 ("small", 96, 8, 129), ("small", 64, 128, 33)]


@pytest.mark.parametrize("family,K,N,n", POISON_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_rows_poison(L, dtype, family, K, N, n):
    """Every layout of `out`: offsets of 1, 2, 4, 8 elements into a larger buffer, ldo beyond the row by 1, 3, 8, a sample
    stride that is no multiple of 8 -- both output layouts, every map kind.  The whole buffer is compared: the valid elements
    equal §1's reference bit for bit, every other element (rows >= n, columns >= N, the gaps between samples, the ends of the
    buffer) still holds the sentinel.  (K = 320, N = 160 is the weight-stationary kernel in the aligned layouts and the tiled
    kernel in the others.)"""
    B = 2
    ops = _Rows(dtype, B, n + 4, 9, K, N, seed=K + N + n)
    kinds = itertools.cycle(MAPS)
    seen = set()
    for transposed, (off, dl, ds) in itertools.product((False, True), LAYOUTS):
        rows_, cols = (N, n) if transposed else (n, N)
        ldo = cols + dl
        obs = (rows_ + 2) * ldo + ds
        flat = sentinel_filled((off + B * obs + 16,), dtype)
        view = flat.as_strided((B, rows_, cols), (obs, ldo, 1), off)
        seen.add(_rows_kernel(K, N, ldo, obs, base_aligned=off % 8 == 0)[0])
        kind = next(kinds)
        y, z = ops.run(L, kind, True, n, transposed, True, out=view)
        tag = f"{family} K={K} N={N} n={n} {'T' if transposed else 'R'} {kind} off={off} ldo={ldo} obs={obs}"
        _assert_exact_range(z, dtype, tag)
        want = sentinel_filled(flat.shape, dtype)
        want.as_strided((B, rows_, cols), (obs, ldo, 1), off).copy_(z.transpose(1, 2) if transposed else z)
        _assert_same(flat, want, tag)
    assert family in seen and seen <= {family, "tiled"}, seen


@pytest.mark.parametrize("K,N", [(320, 160), (640, 37), (32, 37)], ids=["ws", "tiled", "small-k"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_rows_pad_to(L, dtype, K, N):
    """Results the wrapper allocates: pad_to = 8 (zero padding) and pad_to = 1 -- channel-major with an odd n that is ldo = n
    odd, every row at another alignment.  The block the allocator hands out was filled with NaN patterns just before."""
    B, n = 2, 33
    ops = _Rows(dtype, B, n, 5, K, N, seed=K + N)
    for transposed, pad_to, kind in itertools.product((False, True), (1, 8), ("rows", "id")):
        torch.full((B * N * 40,), -1, dtype=torch.int16, device=DEV)     # freed at once: the next torch.empty finds it
        y, z = ops.run(L, kind, True, n, transposed, True, pad_to=pad_to)
        n_pad = _cdiv(n, pad_to) * pad_to
        tag = f"K={K} N={N} T={transposed} pad_to={pad_to} {kind}"
        assert y.shape == ((B, N, n_pad) if transposed else (B, n_pad, N)), tag
        _assert_exact_range(z, dtype, tag)
        _assert_same(_valid(y, n, N, transposed), z.to(dtype), tag)
        assert not bool((y[:, :, n:] if transposed else y[:, n:]).any()), tag


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_linear_panels_poison(L, dtype):
    """vtm_linear_panels into a view with ldo = N + 8 of a buffer with rows to spare."""
    for K, N, n in ((64, 8, 1), (128, 136, 257), (320, 128, 255)):
        g = _gen(K + N)
        x, w = int_uniform((n, K), -1, 1, dtype, g), int_uniform((N, K), -1, 1, dtype, g)
        bias = int_uniform((N,), -8, 8, torch.float32, g)
        buf = sentinel_filled((n + 3, N + 8), dtype)
        L.linear_panels(L.to_panels(x), n, L.to_panels(w), N, bias, out=buf[:, :N])
        z = x.double() @ w.double().T + bias.double()
        _assert_exact_range(z, dtype, (K, N, n))
        want = sentinel_filled(buf.shape, dtype)
        want[:n, :N] = z.to(dtype)
        _assert_same(buf, want, f"panels poison K={K} N={N} n={n}")


# ---------------------------------------------------------------------------------------------------
# 4. per-element bound against float64 on realistic data
# ---------------------------------------------------------------------------------------------------
def _realistic_tokens(shape, dtype, g, smin=-12, smax=12):
    """Gaussian rows, row i scaled by 2 ** s_i with s_i uniform in [smin, smax]; the last rows: two of the format's
    subnormals, one of zeros, one mixing a subnormal half with a normal half."""
    n, K = shape[-2:]
    x = torch.randn(shape, generator=g, device=DEV, dtype=torch.float64)
    s = torch.randint(smin, smax + 1, shape[:-1] + (1,), generator=g, device=DEV)
    x = torch.ldexp(x, s)
    if n >= 8:
        tiny = -16 if dtype == F16 else -128                      # below 2 ** -14 / 2 ** -126: subnormal in the format
        x[..., n - 4:n - 2, :] = torch.ldexp(torch.randn(shape[:-2] + (2, K), generator=g, device=DEV, dtype=torch.float64),
                                             torch.tensor(tiny, device=DEV))
        x[..., n - 2, :] = 0
        x[..., n - 1, :K // 2] = torch.ldexp(x[..., n - 1, :K // 2], (tiny - s[..., n - 1, :]))
    return x.to(dtype)


def _gamma(a, w, bias):
    """2 K 2^-24 (sum |a_k w_k| + |bias|): K fp32 accumulation steps, the factor 2 for a non-RN accumulate inside the MFMA."""
    K = a.shape[-1]
    t = a.double().abs() @ w.double().abs().T
    if bias is not None:
        t = t + bias.double().abs()
    return 2.0 * K * 2.0 ** -24 * t


def _report(name, dtype, err, bound, record):
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"\n[gemm16 float64 bound] {name} {IDS[dtype]}: worst err / bound = {ratio:.3f}")
    record.append((name, IDS[dtype], ratio))
    return ratio


FP16_MAX = 65504.0


@pytest.mark.parametrize("family,K,N", [("ws", 320, 320), ("tiled", 640, 96), ("small", 96, 200)], ids=["ws", "tiled", "small-k"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_rows_vs_float64(L, dtype, family, K, N):
    """vtm_linear_rows on Gaussian tokens over 24 binades, weights N(0, 1 / K): per element
    |got - ref| <= 1/2 ulp(|ref| + gamma) + gamma against the float64 matmul of the same 16-bit operands.
    Measured worst err / bound (MI355X): DESIGN.md 4.4."""
    B, n = 2, 300
    g = _gen(K + N)
    x0 = _realistic_tokens((B, n, K), dtype, g)
    w = (torch.randn(N, K, generator=g, device=DEV) * K ** -0.5).to(dtype)
    bias = torch.randn(N, generator=g, device=DEV).to(dtype)
    ref = x0.double() @ w.double().T + bias.double()
    gam = _gamma(x0, w, bias)
    bound = rounding_bound(ref, gam, dtype)
    if dtype == F16:
        assert float((ref.abs() + bound).max()) < FP16_MAX
    worst = []
    for transposed in (False, True):
        assert _rows_kernel(K, N, _cdiv(n, 8) * 8 if transposed else N, 8 * N)[0] == family
        y = L.linear_rows(x0, None, None, None, n, w, bias, transposed=transposed)
        err = (_valid(y, n, N, transposed).double() - ref).abs()
        ratio = _report(f"linear_rows {family} {'T' if transposed else 'R'}", dtype, err, bound, worst)
        assert ratio <= 1.0, (family, transposed, ratio)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_linear_panels_vs_float64(L, dtype):
    """vtm_linear_panels, plain and with the residual chain RN(RN(sum + bias) + resid): the first rounding's bound e1 goes
    through the fp32 add (relative 2^-24) and the second rounding, e2 = e1 + 2^-24 (|t| + e1), bound = 1/2 ulp(|t| + e2) + e2."""
    K, N, n = 320, 136, 300
    g = _gen(7)
    x = _realistic_tokens((n, K), dtype, g)
    w = (torch.randn(N, K, generator=g, device=DEV) * K ** -0.5).to(dtype)
    bias = torch.randn(N, generator=g, device=DEV)
    resid = (x[:, :N].double() * 0.5).to(dtype)                   # of the rows' own magnitude, like the block's residual
    z1 = x.double() @ w.double().T + bias.double()
    e1 = rounding_bound(z1, _gamma(x, w, bias), dtype)
    t = z1 + resid.double()
    e2 = e1 + 2.0 ** -24 * (t.abs() + e1)
    b2 = rounding_bound(t, e2, dtype)
    if dtype == F16:
        assert float((z1.abs() + e1).max()) < FP16_MAX and float((t.abs() + b2).max()) < FP16_MAX
    xp, wp = L.to_panels(x), L.to_panels(w)
    worst = []
    r1 = _report("linear_panels", dtype, (L.linear_panels(xp, n, wp, N, bias).double() - z1).abs(), e1, worst)
    r2 = _report("linear_panels + resid", dtype, (L.linear_panels(xp, n, wp, N, bias, resid).double() - t).abs(), b2, worst)
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_ff_geglu_vs_float64(L, dtype):
    """vtm_ff_geglu against v * gelu(g) in float64, the bound carried through the chain's three roundings:
      ev, eg   the rounded value / gate: 1/2 ulp(|z| + gamma) + gamma
      ep       gelu_erf in fp32 at the rounded gate: Abramowitz & Stegun 7.1.26 is within 1.5e-7 of erfc, and the fp32
               evaluation of e = p t exp2(-x^2 log2 e) (rcp, four fma, two products, the exponent's two roundings scaled by
               x^2, exp2) within (12 + 2 x^2) 2^-24 of it relatively, x^2 = g^2 / 2; then 0.5 g (e | 2 - e): three roundings
      eh       the rounded gelu: |gelu'| <= 1.13 carries eg, then ep, then half a spacing
      product  exact in fp32 (two 11-bit significands); bound = 1/2 ulp(|ref| + e) + e, e = |v| eh + |gelu(g)| ev + ev eh.
    Rows span 2^-12 ... 2^5 so that no fp16 product overflows."""
    K, D, n = 320, 192, 300
    g = _gen(9)
    x = _realistic_tokens((n, K), dtype, g, smin=-12, smax=5)
    w = (torch.randn(2 * D, K, generator=g, device=DEV) * K ** -0.5).to(dtype)
    b = torch.randn(2 * D, generator=g, device=DEV)
    z = x.double() @ w.double().T + b.double()
    gam = _gamma(x, w, b)
    zv, zg = z[:, :D], z[:, D:]
    ev, eg = rounding_bound(zv, gam[:, :D], dtype), rounding_bound(zg, gam[:, D:], dtype)
    G = _gelu64(zg)
    ga = zg.abs() + eg                                            # the largest |rounded gate|
    E = torch.special.erfc((zg.abs() - eg).clamp_min(0) / math.sqrt(2.0))
    ep = 0.5 * ga * (1.5e-7 + (12 + ga * ga) * 2.0 ** -24 * E) + 3 * 2.0 ** -24 * (G.abs() + 1.13 * eg)
    eh = rounding_bound(G, 1.13 * eg + ep, dtype)
    e = zv.abs() * eh + G.abs() * ev + ev * eh
    ref = zv * G
    bound = rounding_bound(ref, e, dtype)
    if dtype == F16:
        assert float((ref.abs() + bound).max()) < FP16_MAX and float((z.abs() + ev.max()).max()) < FP16_MAX
    wp, bp = _geglu_pack(L, w, b, D)
    got = _panel_valid(L.ff_geglu(L.to_panels(x), n, wp, D, bp), n, D).double()
    ratio = _report("ff_geglu", dtype, (got - ref).abs(), bound, [])
    assert ratio <= 1.0, ratio


# ---------------------------------------------------------------------------------------------------
# 5. special values
# ---------------------------------------------------------------------------------------------------
def _special_rows(x):
    """Of a (32, K) integer block, row 7 gets one infinity (an output is +inf, -inf or NaN with its weight's sign), row 9
    three of both signs (inf - inf as well), row 20 a NaN."""
    K = x.shape[-1]
    x[..., 7, 1] = math.inf
    x[..., 9, 1], x[..., 9, K // 2], x[..., 9, K - 3] = math.inf, -math.inf, math.inf
    x[..., 20, K - 1] = math.nan
    return x


@pytest.mark.parametrize("K,N", [(320, 160), (640, 100), (96, 37)], ids=["ws", "tiled", "small-k"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_rows_inf_and_nan_rows(L, dtype, K, N):
    """Two token rows with infinities and one with a NaN inside a 32-row integer block: those output rows as torch
    computes them on the CPU (which elements are NaN, the signs of the infinities), every other row still §1's bits."""
    n = 32
    ops = _Rows(dtype, 1, n, 0, K, N, seed=K)
    _special_rows(ops.x0)
    want = (ops.x0.cpu().double() @ ops.W.cpu().double().T + ops.bias.cpu().double()).to(dtype).to(DEV)
    assert bool(want[0, 7].isinf().any()) and bool(want[0, 7].isnan().any()) and bool(want[0, 20].isnan().all())
    assert bool(torch.isfinite(want[0, :7].float()).all())
    for transposed in (False, True):
        y = L.linear_rows(ops.x0, None, None, None, n, ops.W, ops.bias, transposed=transposed)
        _assert_same(_valid(y, n, N, transposed), want, f"special rows K={K} N={N} T={transposed}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_panels_inf_and_nan_rows(L, dtype):
    """The same through vtm_linear_panels (bias and residual) and vtm_ff_geglu (gates of the finite rows in [10, 250])."""
    K, N, D, n = 128, 136, 64, 32
    g = _gen(11)
    x = _special_rows(int_uniform((n, K), -1, 1, dtype, g))
    w = int_uniform((N, K), -1, 1, dtype, g)
    bias = int_uniform((N,), -8, 8, torch.float32, g)
    resid = int_uniform((n, N), -16, 16, dtype, g)
    z = (x.cpu().double() @ w.cpu().double().T + bias.cpu().double()).to(dtype)
    want = (z.double() + resid.cpu().double()).to(dtype).to(DEV)
    assert bool(want[7].isinf().any()) and bool(want[7].isnan().any()) and bool(want[20].isnan().all())
    _assert_same(L.linear_panels(L.to_panels(x), n, L.to_panels(w), N, bias, resid), want, "panels special rows")

    w1 = int_uniform((2 * D, K), -1, 1, dtype, g)
    b1 = int_uniform((2 * D,), -8, 8, torch.float32, g)
    b1[D:] += GATE_SHIFT
    p = (x.cpu().double() @ w1.cpu().double().T + b1.cpu().double()).to(dtype)
    # gelu in its float64 erfc form: gelu(+inf) = +inf, gelu(-inf) = -inf * 0 = NaN (torch's vectorised CPU gelu returns
    # NaN at +inf as well, which is not the function's value there)
    h = _rn(_gelu64(p[:, D:].double()), dtype)
    want = (p[:, :D].double() * h).to(dtype).to(DEV)
    assert bool(want[7].isinf().any()) and bool(want[20].isnan().all())
    wp, bp = _geglu_pack(L, w1, b1, D)
    _assert_same(_panel_valid(L.ff_geglu(L.to_panels(x), n, wp, D, bp), n, D), want, "geglu special rows")
