"""GPU tests of the merge closures' reduce modes (vtm_merge_reduce, gather.hip; run with -m gpu on an MI355X) beyond the sizes of
tests/golden/modes.npz (N <= 96 tokens, at most 8 members per destination row, one workgroup, the smallest sort), and one of
vtm_gather_panels.

Reference: plain torch on the CPU, from the same tensors copied to the host (helpers.scatter_reduce_reference):
    dst.scatter_reduce(-2, dst_idx[..., None].expand(-1, -1, C).long(), src, reduce=mode, include_self=True)
with dst = x[b, dst_rows], src = x[b, src_rows] -- the operation that the library's contract names (include/vidtome_hip.h,
vtm_merge_reduce).  Every comparison is of bit patterns, a NaN equal to a NaN whatever its payload.  The result buffer is
filled with 0xFF bytes before each call and the rows outside [out_row0, out_row0 + Nd) must still hold them afterwards.

Signed zeros under amax / amin: torch's CPU kernel keeps the accumulator on a tie, so of +0 and -0 the one that came first
stays -- for both operand orders, at C = 8 and at C = 64, in all three dtypes (test_signed_zeros asserts that on the
reference before it uses it).  The kernel is held to that choice bitwise; zeros are NOT compared by value anywhere here.

Thread count of the CPU reference: for an index that is an expanded (stride-0) view torch reduces every destination row
by itself, its sources in index order, whatever torch.get_num_threads() says (checked at 1 and 8 threads on every shape
below: identical bits).  No shape had to be dropped.

condition                                                       source                reached by
--------------------------------------------------------------  --------------------  ------------------------------------------
B Nd C/8 > 256: more than one block, ragged last block          gather.hip:113-114    test_multi_block_launch (17 blocks at C = 24)
C = 8: one chunk per row (torch: its narrow-row path, C < 16)   gather.hip:112,115    test_multi_block_launch[C8..], test_sort_variants
C = 320, 1280: 40 / 160 chunks per row                          gather.hip:115        test_multi_block_launch[C320.. / C1280..]
src_rows / dst_rows are not the identity                        gather.hip:123,128    every case (rows are random permutations)
"mean": count beyond the dtype's exact integers                 gather.hip:143,147    test_member_counts_around_the_exact_limit
a segment's sources are folded in index order                   gather.hip:127-128,   test_summation_order
                                                                _lib.py:486-488
bisection: first / last row, rows without a source, one         gather.hip:117-121,   test_segment_edges
  segment of all r pairs, Nd = 1, r = 1                          127
r = 0: no sort, dst rows returned unchanged                     _lib.py:489-490       test_segment_edges[no_pairs-..]
sort: one segment | several | several tiles per segment         sort.hip:168-172      test_sort_variants (r = 256 | 257, 16384 | 16385)
out_row0 > 0, rows behind out_row0 + Nd                         gather.hip:142        test_output_placement (every other case: 1, 1)
NaN, +-inf, +-0, denormals, largest finite value                gather.hip:133-137    test_special_values, test_signed_zeros
the closures: out_row0 = Ns - r, rows through a_idx / b_idx     merge.py:272-283      test_closure_path
gather_panels: rows | rows + rows2 | identity, two-part pool,   ff.hip:360-366        test_gather_panels
  zero padding rows
"""
import functools
import math
import os

import pytest
import torch

from helpers import MEMBER_COUNTS, REDUCE_MODES, interleaved_destinations, reduce_tokens, same_bits, scatter_reduce_reference
from test_gpu_dispatch_variants import _bits, _poison, _random_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F32, F16, BF16]
IDS = {F32: "fp32", F16: "fp16", BF16: "bf16"}
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vidtome_amd", "csrc")
BLOCK = 256                          # threads per block of merge_reduce_kernel, 8 channels per thread
EXACT_COUNT = {F32: 1 << 24, F16: 2048, BF16: 256}       # the largest count below which every integer is representable
_PINS = {
    "gather.hip": ["const int64_t chunks = C / 8;", "if (idx >= B * Nd * chunks) return;",
                   "const dim3 grid((unsigned)vtm::cdiv(total, 256)), block(256);"],
    "sort.hip": ["constexpr int T = 256;", "const int64_t tiles = vtm::cdiv(n, T);",
                 "int64_t tps = vtm::cdiv(tiles, 64);", "g.nseg = (int)vtm::cdiv(tiles, tps);"],
}


def _pinned(fname):
    """The tests' precondition: the launch geometry of `fname` still reads as the shapes below assume."""
    with open(os.path.join(CSRC, fname)) as f:
        src = f.read()
    for text in _PINS[fname]:
        assert text in src, f"{fname} no longer contains {text!r}: re-derive the shapes of this test from the new code"


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _i32(t):
    return t.to(torch.int32).contiguous()


def _run(L, x, src_rows, dst_rows, dst_idx, mode, out_row0=1, spare=1):
    """L.merge_reduce on the device copies of CPU operands, into a poisoned buffer with `out_row0` rows in front of the Nd
    result rows and `spare` behind; returns the Nd rows on the CPU."""
    B, _, C = x.shape
    Nd = dst_rows.shape[1]
    rows = out_row0 + Nd + spare
    out = torch.full((B, rows, C * x.element_size()), 0xFF, dtype=torch.uint8, device=DEV).view(x.dtype)
    assert out.shape == (B, rows, C)
    res = L.merge_reduce(x.to(DEV), src_rows.to(DEV), dst_rows.to(DEV), dst_idx.to(DEV), mode, out, out_row0)
    assert res is out
    got = out.cpu()
    outside = torch.cat([got[:, :out_row0], got[:, out_row0 + Nd:]], dim=1).contiguous().view(torch.uint8)
    assert bool((outside == 0xFF).all()), f"{mode}: rows outside [{out_row0}, {out_row0 + Nd}) were written"
    return got[:, out_row0:out_row0 + Nd]


def _check(L, x, src_rows, dst_rows, dst_idx, mode, tag, **placement):
    """The kernel against torch's CPU scatter_reduce on the same operands: bit for bit; the differing elements are counted
    per destination row before the assertion."""
    want = scatter_reduce_reference(x, src_rows, dst_rows, dst_idx, mode)
    got = _run(L, x, src_rows, dst_rows, dst_idx, mode, **placement)
    same = same_bits(got, want)
    if not bool(same.all()):
        members = 1 + torch.stack([torch.bincount(d.long(), minlength=dst_rows.shape[1]) for d in dst_idx])
        bad = (~same).sum(-1)
        rows = [(b, j, int(members[b, j]), int(bad[b, j])) for b, j in bad.nonzero().tolist()[:12]]
        print(f"\n[merge_reduce] {tag} {mode}: {int(bad.sum())} of {same.numel()} elements differ; (sample, row, members, "
              f"differing channels of {x.shape[-1]}): {rows}")
    assert bool(same.all()), (tag, mode, int((~same).sum()))


@functools.lru_cache(maxsize=2)
def _random_case(B, N, Nd, r, C, dtype, tokens_for):
    """Random pairs: dst_idx uniform and unsorted, dst_rows / src_rows disjoint pieces of a random permutation of the N
    token rows of every sample."""
    g = torch.Generator().manual_seed(N + Nd + r + C)
    x = reduce_tokens((B, N, C), dtype, N + C, tokens_for)
    perm = torch.stack([torch.randperm(N, generator=g) for _ in range(B)])
    dst_rows, src_rows = _i32(perm[:, :Nd]), _i32(perm[:, Nd:Nd + r])
    dst_idx = _i32(torch.randint(0, Nd, (B, r), generator=g))
    assert Nd + r <= N and not torch.equal(dst_rows[0], torch.arange(Nd, dtype=torch.int32))
    assert r < 2 or bool((dst_idx[:, 1:] < dst_idx[:, :-1]).any())           # unsorted
    return x, src_rows, dst_rows, dst_idx


def _tokens_for(mode):
    return "prod" if mode == "prod" else "sum"


# ---------------------------------------------------------------------------------------------------
# 1. more than one workgroup
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", REDUCE_MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("C,Nd,r", [(24, 700, 5000), (8, 700, 5000), (320, 700, 5000), (1280, 200, 1300)],
                         ids=["C24-17_blocks", "C8-one_chunk_per_row", "C320", "C1280"])
def test_multi_block_launch(L, C, Nd, r, dtype, mode):
    """B = 2, thousands of pairs on hundreds of rows: threads of one row lie in different waves and blocks, every one runs
    its own bisection over 5000 (1300) sorted pairs.  C = 24: 4200 threads = 16 full blocks + 104 threads."""
    _pinned("gather.hip")
    B = 2
    threads = B * Nd * (C // 8)
    blocks = -(-threads // BLOCK)
    assert blocks > 1 and B * r * C <= 3_500_000
    if C == 24:
        assert blocks == 17 and threads % BLOCK == 104
    if C == 8:
        assert C // 8 == 1 and C < 16
    x, src_rows, dst_rows, dst_idx = _random_case(B, Nd + r + 13, Nd, r, C, dtype, _tokens_for(mode))
    _check(L, x, src_rows, dst_rows, dst_idx, mode, f"multi-block C={C} {IDS[dtype]}")


# ---------------------------------------------------------------------------------------------------
# 2. member counts around the largest exactly representable one
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", REDUCE_MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_member_counts_around_the_exact_limit(L, dtype, mode):
    """One call whose destination rows have the member counts of helpers.MEMBER_COUNTS (fp16: .. 2047 - 2051, 2501, 4099;
    bf16: .. 255 - 259, 301, 2501), C = 64, the pairs of all rows shuffled into one another.  torch holds the count of
    "mean" in the tensors' dtype: 2049 members of an fp16 row divide by 2048, 2051 by 2052.

    Before the fix of this rule (the kernel divided by the fp32 count) this test failed for mean-fp16 and mean-bf16, at
    exactly the rows above 2048 / 256 members."""
    counts = MEMBER_COUNTS[IDS[dtype]]
    lim = EXACT_COUNT[dtype]
    held = [float(torch.tensor(float(c)).to(dtype)) == c for c in counts]              # counts that the dtype represents
    if dtype == F32:
        assert all(held)
    else:
        assert {lim - 1, lim, lim + 1, lim + 2, lim + 3} <= set(counts) and not all(held)
    C, Nd = 64, len(counts)
    dst_idx = interleaved_destinations(counts, seed=Nd)
    r = dst_idx.shape[1]
    assert r == sum(counts) - Nd and r * C <= 3_500_000
    x = reduce_tokens((1, Nd + r, C), dtype, 21, _tokens_for(mode))
    perm = torch.randperm(Nd + r, generator=torch.Generator().manual_seed(22))[None]
    _check(L, x, _i32(perm[:, Nd:]), _i32(perm[:, :Nd]), dst_idx, mode, f"member counts {IDS[dtype]}")


# ---------------------------------------------------------------------------------------------------
# 3. summation order
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F16], ids=IDS.get)
def test_summation_order(L, dtype):
    """600 sources on one row (and 120 on its two neighbours, shuffled in between): magnitudes 10 ** U(-3, 3), every value
    once with each sign and in random order, so that the row's sum is what the roundings of the partial sums leave of a
    total that cancels -- it depends on the order in the last bits of fp32, which a result rounded to fp16 still shows
    because it is small.  Precondition (on the CPU reference alone): the same pairs fed in reversed index order change at
    least 10 % of that row's sums.  A sort or a kernel that loses index order inside a segment fails here."""
    C, Nd, half = 64, 3, 300
    g = torch.Generator().manual_seed(31)
    mag = torch.pow(10.0, torch.rand(half, C, generator=g) * 6 - 3)
    mag = mag * (torch.randint(0, 2, (half, C), generator=g) * 2 - 1)
    heavy = torch.cat([mag, -mag])[torch.randperm(2 * half, generator=g)].to(dtype)            # exact negations, shuffled
    light = reduce_tokens((120, C), dtype, 32, "sum")
    selfs = (torch.pow(10.0, torch.rand(Nd, C, generator=g) * 6 - 3)).to(dtype)
    place = torch.randperm(720, generator=g)                       # pair i sits at index place[i]
    dst_idx = torch.empty(720, dtype=torch.int32)
    dst_idx[place[:600]] = 1
    dst_idx[place[600:]] = torch.tensor([0, 2], dtype=torch.int32).repeat(60)
    src = torch.empty(720, C, dtype=dtype)
    src[place[:600]], src[place[600:]] = heavy, light
    x = torch.cat([selfs, src])[None].contiguous()
    dst_rows, src_rows, dst_idx = _i32(torch.arange(Nd)[None]), _i32(Nd + torch.arange(720)[None]), dst_idx[None]
    assert int((dst_idx == 1).sum()) >= 500
    fwd = scatter_reduce_reference(x, src_rows, dst_rows, dst_idx, "sum")
    rev = scatter_reduce_reference(x, src_rows.flip(1), dst_rows, dst_idx.flip(1), "sum")
    changed = int((~same_bits(fwd, rev))[0, 1].sum())
    print(f"\n[merge_reduce] summation order {IDS[dtype]}: reversed order changes {changed} of {C} sums")
    assert changed >= math.ceil(0.1 * C), changed
    for mode in ("sum", "mean"):
        _check(L, x, src_rows, dst_rows, dst_idx, mode, f"summation order {IDS[dtype]}")


# ---------------------------------------------------------------------------------------------------
# 4. bisection and segment edges
# ---------------------------------------------------------------------------------------------------
def _edge_case(name):
    """(Nd, dst_idx (B, r)) of an edge configuration, B = 2 (the second sample: the same pairs in reversed order)."""
    g = torch.Generator().manual_seed(41)
    if name == "ends_and_gap":         # rows 0 and Nd - 1 hit, rows 6 .. 29 without a source
        Nd = 40
        pool = torch.tensor([0, Nd - 1, 1, 2, 3, 4, 5, 30, 31, 32, 33, 34, 35, 36, 37, 38])
        d = pool[torch.randint(0, len(pool), (50,), generator=g)]
        d[7], d[20] = 0, Nd - 1
        hit = torch.bincount(d, minlength=Nd)
        assert hit[0] > 0 and hit[Nd - 1] > 0 and not hit[6:30].any()
    elif name == "single_destination":  # all r pairs on one row: every other row's bisection ends at 0 or at r
        Nd, d = 9, torch.full((300,), 4)
    elif name == "one_row":
        Nd, d = 1, torch.zeros(20, dtype=torch.int64)
    elif name == "one_pair":
        Nd, d = 5, torch.tensor([3])
    else:
        assert name == "no_pairs"
        Nd, d = 5, torch.zeros(0, dtype=torch.int64)
    return Nd, _i32(torch.stack([d, d.flip(0)]))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("name", ["ends_and_gap", "single_destination", "one_row", "one_pair", "no_pairs"])
def test_segment_edges(L, name, dtype):
    C, B = 16, 2
    Nd, dst_idx = _edge_case(name)
    r = dst_idx.shape[1]
    N = Nd + r + 3
    perm = torch.stack([torch.randperm(N, generator=torch.Generator().manual_seed(42 + b)) for b in range(B)])
    dst_rows, src_rows = _i32(perm[:, :Nd]), _i32(perm[:, Nd:Nd + r])
    assert src_rows.shape == (B, r) and dst_idx.shape == (B, r)
    for mode in REDUCE_MODES:
        x = reduce_tokens((B, N, C), dtype, 43, _tokens_for(mode))
        if r == 0:                  # nothing to fold: the dst rows come back as they are, "mean" included (x / 1)
            got = _run(L, x, src_rows, dst_rows, dst_idx, mode)
            assert torch.equal(_bits(got), _bits(x[torch.arange(B)[:, None], dst_rows.long()])), mode
        _check(L, x, src_rows, dst_rows, dst_idx, mode, f"{name} {IDS[dtype]}")


# ---------------------------------------------------------------------------------------------------
# 5. the host side's sort by destination, at every size where vtm_sort_desc changes shape
# ---------------------------------------------------------------------------------------------------
def _sort_geometry(n):
    """(segments per row, 256-key tiles per segment) of vtm_sort_desc: make_geo of sort.hip restated."""
    _pinned("sort.hip")
    tiles = -(-n // 256)
    tps = max(1, -(-tiles // 64))
    return -(-tiles // tps), tps


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("r,geometry", [(256, (1, 1)), (257, (2, 1)), (16384, (64, 1)), (16385, (33, 2))])
def test_sort_variants(L, r, geometry, dtype):
    """The pairs are sorted by destination with the library's radix sort (_lib.merge_reduce -> sort_desc): one workgroup per
    sample up to 256 pairs, one workgroup per 256-key tile up to 64 tiles, several tiles per workgroup beyond (the sizes
    that test_sort_desc's parameter list marks as 16384 | 16385).  C = 8 and B = 2; 300 rows, so a row has about r / 300
    sources whose order the sort must keep."""
    assert _sort_geometry(r) == geometry
    B, C, Nd = 2, 8, 300
    for mode in REDUCE_MODES:
        x, src_rows, dst_rows, dst_idx = _random_case(B, Nd + r + 5, Nd, r, C, dtype, _tokens_for(mode))
        _check(L, x, src_rows, dst_rows, dst_idx, mode, f"sort r={r} {IDS[dtype]}")


# ---------------------------------------------------------------------------------------------------
# 6. output placement
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_output_placement(L, dtype):
    """B = 3, out_row0 = 37 and 11 spare rows behind the result: exactly rows [37, 37 + Nd) of every sample are written."""
    B, C, Nd, r = 3, 40, 29, 200
    for mode in REDUCE_MODES:
        x, src_rows, dst_rows, dst_idx = _random_case(B, Nd + r + 7, Nd, r, C, dtype, _tokens_for(mode))
        _check(L, x, src_rows, dst_rows, dst_idx, mode, f"placement {IDS[dtype]}", out_row0=37, spare=11)


# ---------------------------------------------------------------------------------------------------
# 7. special values
# ---------------------------------------------------------------------------------------------------
def _special_sequences(dtype):
    """Scenarios [self, source 1, source 2, source 3], one per channel."""
    fi = torch.finfo(dtype)
    big, tiny = fi.max, fi.smallest_normal
    den = tiny * fi.eps                          # the smallest denormal
    dmax = tiny - den                            # the largest denormal
    nan, inf = math.nan, math.inf
    seqs = [
        [1.0, inf, -inf, 2.0], [inf, -inf, 1.0, 1.0], [-inf, 3.0, inf, -inf], [inf, inf, 2.0, -1.0],      # inf + -inf
        [big, big, 2.0, 0.5], [big, 2.0, big, -big], [-big, big, big, 0.5], [big, -big, big, -big],       # overflow, largest finite
        [big, big, 1.0, 1.0], [-big, -big, -big, -big], [big, 1.0, -1.0, 0.5],
        [0.0, inf, 1.0, 1.0], [inf, 2.0, 0.0, 1.0], [-inf, -0.0, 2.0, 3.0], [2.0, 0.0, -inf, 0.5],        # 0 * inf
        [1.0, nan, 2.0, 3.0], [1.0, 2.0, nan, 3.0], [1.0, 2.0, 3.0, nan], [nan, 1.0, 2.0, 3.0],           # NaN first, middle, last, self
        [inf, nan, -inf, 1.0], [-inf, 5.0, nan, inf], [nan, nan, nan, nan], [3.0, inf, -1.0, nan],
        [0.0, -0.0, 0.0, -0.0], [-0.0, 0.0, -0.0, 0.0], [-0.0, -0.0, -0.0, -0.0], [-0.0, -0.0, 1.0, -1.0],
        [den, den, den, den], [dmax, dmax, -den, den], [den, 0.5, 0.5, 0.5], [tiny, -dmax, 0.5, 0.25],    # denormals
        [-den, den, -0.0, 0.0], [dmax, den, 2.0, 0.5], [tiny, tiny, tiny, tiny], [den, -dmax, tiny, -tiny],
        [big, den, -big, den], [1.0, -1.0, den, -den], [inf, den, 0.0, -den], [-0.0, den, -den, 0.0],
        [dmax, 1.0, 1.0, 1.0],
    ]
    assert len(seqs) % 8 == 0
    return torch.tensor(seqs, dtype=torch.float64).to(dtype)        # (C, 4): every value is representable in dtype


@pytest.mark.parametrize("mode", REDUCE_MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_special_values(L, dtype, mode):
    """NaN, +-inf, +-0, denormals of the dtype and its largest finite value in self rows and sources: inf + -inf, a product
    that overflows, 0 * inf, amax / amin through a NaN in the first, middle and last position of a segment.  Row 0 folds
    its three sources in the order listed, row 1 the same sources in reversed order; the pairs of the two rows alternate."""
    seq = _special_sequences(dtype)                                  # (C, 4)
    C = seq.shape[0]
    fi = torch.finfo(dtype)
    assert seq.isnan().any() and seq.isinf().any() and bool((seq == fi.max).any())
    assert bool(((seq != 0) & (seq.abs() < fi.smallest_normal)).any())       # denormals survived the conversion
    # x rows: 0, 1 = the two self rows; 2, 3, 4 = sources 1, 2, 3
    x = torch.stack([seq[:, 0], seq[:, 0], seq[:, 1], seq[:, 2], seq[:, 3]])[None].contiguous()
    dst_rows = _i32(torch.tensor([[0, 1]]))
    src_rows = _i32(torch.tensor([[2, 4, 3, 3, 4, 2]]))
    dst_idx = _i32(torch.tensor([[0, 1, 0, 1, 0, 1]]))
    _check(L, x, src_rows, dst_rows, dst_idx, mode, f"special values {IDS[dtype]}")


@pytest.mark.parametrize("mode", REDUCE_MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_signed_zeros(L, dtype, mode):
    """Every sequence of +0 / -0 over a self row and three sources (16 rows), at C = 8 and C = 64.  Precondition on the
    reference: under amax and amin torch returns the self row's zero for every sequence at both widths (the accumulator
    stays on a tie), so its choice depends on neither the width nor the operand order and the kernel is held to it bit for
    bit.  (The device's fmaxf / fminf order -0 below +0 and would return the other zero in half of the rows.)"""
    signs = torch.tensor([[(k >> p) & 1 for p in range(4)] for k in range(16)])           # (16 rows, 4 members)
    zeros = torch.where(signs.bool(), -0.0, 0.0)
    for C in (8, 64):
        x = torch.cat([zeros[:, 0], zeros[:, 1], zeros[:, 2], zeros[:, 3]])[None, :, None].expand(1, 64, C).to(dtype).contiguous()
        dst_rows = _i32(torch.arange(16)[None])
        # keep a row's sources in their listed order (source 1, 2, 3) while mixing the rows: pairs sorted by source number,
        # rows shuffled inside every source number
        mix = torch.cat([k * 16 + torch.randperm(16, generator=torch.Generator().manual_seed(C + k)) for k in range(3)])
        src_rows, dst_idx = _i32(16 + mix[None]), _i32((mix % 16)[None])
        if mode in ("amax", "amin"):
            want = scatter_reduce_reference(x, src_rows, dst_rows, dst_idx, mode)
            assert torch.equal(_bits(want), _bits(x[:, :16])), "torch no longer keeps the accumulator's zero"
        _check(L, x, src_rows, dst_rows, dst_idx, mode, f"signed zeros C={C} {IDS[dtype]}")


# ---------------------------------------------------------------------------------------------------
# 8. through the closures
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted_level(L):
    """bipartite_soft_matching_randframe on B = 2, 16 global + 4 frames of 32 x 32 tokens, C = 16, ratio 0.9: positions
    0 .. 799 of EVERY frame hold one and the same token, so whichever frame is drawn as dst, 2400 src tokens are exact
    copies of a dst token and all of them pick its first copy (equal scores: lowest index).  The planted token has positive
    channels only and every other token negative ones, so no other token picks it: that row has 2401 members, a count that
    neither fp16 (2400 | 2402) nor bf16 (2400 | 2416) holds."""
    from vidtome_amd import merge
    B, F, T, C, unm_pre = 2, 4, 32 * 32, 16, 16
    g = torch.Generator().manual_seed(51)
    x = -0.1 - torch.randn(B, unm_pre + F * T, C, generator=g).abs()
    token = 0.1 + torch.randn(B, 1, 1, C, generator=g).abs()
    x[:, unm_pre:].view(B, F, T, C)[:, :, :800] = token
    m, u, info = merge.bipartite_soft_matching_randframe(x.to(DEV), F, 0.9, unm_pre, torch.Generator().manual_seed(52), 4, False)
    idx = {n: info[n].cpu().long() for n in ("unm_idx", "src_idx", "dst_idx", "a_idx", "b_idx")}
    Ns = idx["a_idx"].numel()
    r = idx["src_idx"].shape[1]
    assert Ns == 3 * T and r == int(Ns * 0.9) and idx["unm_idx"].shape[1] == Ns - r > 0
    members = [1 + int(torch.bincount(d).max()) for d in idx["dst_idx"]]
    print(f"\n[merge_reduce] closure path: largest member counts {members}")
    assert int(torch.bincount(idx["dst_idx"][0]).max()) >= 2049, "the planted copies did not land on one destination"
    for dt in (F16, BF16):
        assert all(float(torch.tensor(float(c)).to(dt)) != c for c in members), (members, "representable in", dt)
    return m, idx, x.shape


@pytest.mark.parametrize("mode", REDUCE_MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_closure_path(L, planted_level, dtype, mode):
    """merge(y, mode=...) of a level with more than 2048 sources on one destination and out_row0 = Ns - r = 308 equals
    cat([unm, scatter_reduce]) built on the CPU from the indices the library returned.  y is not the metric: random tokens
    of helpers.reduce_tokens, so that the sums round."""
    m, idx, shape = planted_level
    B = shape[0]
    y = reduce_tokens(shape, dtype, 53, _tokens_for(mode))
    bi = torch.arange(B)[:, None]
    src_rows = idx["a_idx"][idx["src_idx"]]
    dst_rows = idx["b_idx"][None].expand(B, -1)
    want = torch.cat([y[bi, idx["a_idx"][idx["unm_idx"]]],
                      scatter_reduce_reference(y, src_rows, dst_rows, idx["dst_idx"], mode)], dim=1)
    _poison(want.numel() * want.element_size())
    got = m(y.to(DEV), mode=mode).cpu()
    same = same_bits(got, want)
    assert bool(same.all()), (IDS[dtype], mode, int((~same).sum()), "rows", (~same).any(-1).nonzero()[:8].tolist())


# ---------------------------------------------------------------------------------------------------
# 9. gather_panels
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maps", ["rows", "rows_and_rows2", "identity"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=IDS.get)
def test_gather_panels(L, dtype, maps):
    """vtm_gather_panels == torch.gather on the pool [x0 | x1] rearranged to (C / 8, B n_pad, 8), over random bit patterns:
    B = 3, n = 300 (n_pad = 512: 212 zero padding rows per sample), P0 = 200 < n so that the identity crosses into x1."""
    B, C, n, P0, P1, M = 3, 64, 300, 200, 150, 400
    g = torch.Generator(device=DEV).manual_seed(61)
    x0, x1 = _random_bits((B, P0, C), dtype, g), _random_bits((B, P1, C), dtype, g)
    rows = torch.randint(0, P0 + P1, (B, M), device=DEV, generator=g).to(torch.int32)
    rows[:, :4] = torch.tensor([0, P0 - 1, P0, P0 + P1 - 1], dtype=torch.int32, device=DEV)       # the pool's edges
    rows2 = torch.randint(0, M, (B, n), device=DEV, generator=g).to(torch.int32)
    rows2[:, :6] = torch.tensor([0, 1, 2, 3, M - 1, n], dtype=torch.int32, device=DEV)
    n_pad = L.panel_rows(n)
    assert n_pad == 512 and n <= P0 + P1 and P0 < n
    p = torch.arange(n, device=DEV).expand(B, n)
    if maps == "rows_and_rows2":
        p = rows.long().gather(1, rows2.long())
    elif maps == "rows":
        p = rows[:, :n].long()
    pool = torch.cat([_bits(x0), _bits(x1)], dim=1)
    sel = pool.gather(1, p[..., None].expand(B, n, C))
    want = torch.zeros(B, n_pad, C, dtype=torch.int16, device=DEV)
    want[:, :n] = sel
    want = want.view(B * n_pad, C // 8, 8).permute(1, 0, 2)
    _poison(want.numel() * 2)
    out = L.gather_panels(x0, x1, rows if maps != "identity" else None, rows2 if maps == "rows_and_rows2" else None, n)
    assert out.shape == (C // 8, B * n_pad, 8) and out.dtype == dtype
    assert torch.equal(_bits(out), want)
    assert not _bits(out).view(C // 8, B, n_pad, 8)[:, :, n:].any()
