"""CPU tests of the receptive-field matchers: the bitwise restatement of tests/rf_common.py against the reference's recorded runs
(tests/golden/rf.npz), the host's threshold function, the C-ABI surface of vtm_match_masked, and the argument rules of
bipartite_soft_matching_random2d_hier / _2f that need no GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import rf_common as rf
from helpers import load_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = load_cases("rf.npz")


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


@pytest.mark.parametrize("n", range(len(rf.CASES)))
def test_restatement_equals_the_fixture(oracle, n):
    """Indices: src / dst exactly, unm as a set with the same node_max bits position by position (tie-aware: the reference's
    argsort is not stable, and the rows whose maximum is a masked 0 are one large group of equal keys).  Merged rows through
    the same permutation (rf_common.canonical), every stored closure result included."""
    c = CASES[n]
    assert tuple(c[k] for k in rf.FIELDS) == rf.CASES[n] and len(CASES) == len(rf.CASES)
    x = rf.build_inputs(c, c["seed"])
    rf.assert_stored(c, "x", x)
    coord = rf.build_coord(c) if c["with_coord"] else None
    a_idx, b_idx = rf.partition_hier(c, c["randf"]) if c["fn"] == "hier" else rf.partition_2f(c)
    assert np.array_equal(a_idx, c["a_idx"]) and np.array_equal(b_idx, c["b_idx"])
    lv = rf.restate(oracle, x, a_idx, b_idx, c["ratio"], c["adhere_src"], coord, c["rec_field"])
    assert np.array_equal(lv["src_idx"], c["src_idx"]) and np.array_equal(lv["dst_idx"], c["dst_idx"])
    assert np.array_equal(np.sort(lv["unm_idx"], -1), np.sort(c["unm_idx"], -1))
    nm = np.broadcast_to(np.atleast_2d(lv["node_max"]), (c["B"], len(a_idx)))
    same = np.take_along_axis(nm, lv["unm_idx"], 1).view(np.uint32) == np.take_along_axis(nm, c["unm_idx"].astype(np.int64), 1).view(np.uint32)
    assert same.all()
    if n in (0, 1, 7, 8):        # "zero wins, first masked column": a good part of the rows
        zero = nm == 0
        assert zero.mean() > 0.2
        ni = np.broadcast_to(np.atleast_2d(lv["node_idx"]), nm.shape)
        mask = rf.mask_of(coord[:, a_idx], coord[:, b_idx], c["rec_field"])
        if not c["adhere_src"]:
            assert np.array_equal(ni[zero], mask.argmax(-1)[zero])
    first = c["fn"] == "2f"
    N = rf.tokens(c)
    canon = lambda t, ui=lv["unm_idx"]: rf.canonical(t, ui)
    merged = rf.merge_restated(oracle, x, a_idx, b_idx, lv, "replace")
    rf.assert_stored(c, "replace", canon(merged))
    for mode in ("mean", "sum"):
        rf.assert_stored(c, mode, canon(rf.merge_restated(oracle, x, a_idx, b_idx, lv, mode, first)))
    full = rf.unmerge_restated(merged, a_idx, b_idx, lv, N)
    s = rf.src_len_2f(c)
    if first:
        rf.assert_stored(c, "unmerged0", full[:, :s])
        rf.assert_stored(c, "unmerged1", full[:, s:])
    else:
        rf.assert_stored(c, "unmerged", full)
    zero_un = rf.unmerge_restated(merged, a_idx, b_idx, lv, N, unm_modi="zero")
    rf.assert_stored(c, "zero_unmerged", zero_un[:, :s] if first else zero_un)
    sel = [1, 0]
    bm = rf.merge_restated(oracle, x[sel], a_idx, b_idx, lv, "replace", first, sel)
    rf.assert_stored(c, "bsel_replace", canon(bm, lv["unm_idx"][sel]))
    rf.assert_stored(c, "bsel_mean", canon(rf.merge_restated(oracle, x[sel], a_idx, b_idx, lv, "mean", first, sel), lv["unm_idx"][sel]))
    bu = rf.unmerge_restated(bm, a_idx, b_idx, lv, N, sel)
    rf.assert_stored(c, "bsel_unmerged", bu[:, :s] if first else bu)
    rf.assert_stored(c, "bsel_int_replace", canon(rf.merge_restated(oracle, x[1:2], a_idx, b_idx, lv, "replace", first, 1),
                                                  lv["unm_idx"][1:2]))


def test_2f_folds_the_first_src_rows_not_the_matched_ones(oracle):
    """merge.py:718 is commented out: the fixture's "mean" rows are those of the first r src rows, and differ from the fold of
    the matched rows (what every other matcher does)."""
    n = 9
    c = CASES[n]
    x, coord = rf.build_inputs(c, c["seed"]), rf.build_coord(c)
    a_idx, b_idx = rf.partition_2f(c)
    lv = {k: c[k].astype(np.int64) for k in ("unm_idx", "src_idx", "dst_idx")}
    rf.assert_stored(c, "mean", rf.canonical(rf.merge_restated(oracle, x, a_idx, b_idx, lv, "mean", True), lv["unm_idx"]))
    with pytest.raises(AssertionError):
        rf.assert_stored(c, "mean", rf.canonical(rf.merge_restated(oracle, x, a_idx, b_idx, lv, "mean", False), lv["unm_idx"]))


REC_SWEEP = ([float(i) for i in range(0, 70)] + [i + 0.5 for i in range(0, 70)] +
             [math.sqrt(k) for k in (2, 3, 5, 7, 8, 10, 1000, 12345)] + [math.pi, math.e, 1 / 3, 0.1, 1e-3, 1e-20, 1e-30, 2047.9,
                                                                          2896.3, 1e9, 1e18, 1.8e19, 1.9e19, 3e38])


def test_threshold_is_the_largest_fp32_whose_sqrt_is_within_the_field():
    """mask_threshold against numpy's correctly rounded fp32 sqrt, at the threshold and at its upper neighbour; the field is
    compared in fp32, as torch compares an fp32 tensor with a Python number."""
    from vidtome_amd import _lib
    fmax = np.finfo(np.float32).max
    for rec in REC_SWEEP:
        T = _lib.mask_threshold(rec)
        r32 = np.float32(rec)
        t = np.float32(T)
        assert float(t) == T and T >= 0, rec                       # an fp32 value
        assert np.sqrt(t) <= r32, rec
        if t < fmax:
            up = np.nextafter(t, np.float32(np.inf))
            assert not np.sqrt(up) <= r32, rec
        if t > 0:
            assert np.sqrt(np.nextafter(t, np.float32(0))) <= r32, rec
    # exact squares: s = 4 is inside a field of 2, s = 5 is not; sqrt(8) = 2.828.. against the field 2.8284271 (fp32 of sqrt 8)
    assert _lib.mask_threshold(2) >= 4 and _lib.mask_threshold(2) < 5
    assert _lib.mask_threshold(0) == 0.0 and _lib.mask_threshold(-0.0) == 0.0
    for rec in (-1, -1e-30, -math.inf):
        assert _lib.mask_threshold(rec) == -math.inf                # every pair is masked, s = 0 included
    assert _lib.mask_threshold(math.inf) == math.inf and _lib.mask_threshold(math.nan) == math.inf   # none is
    assert _lib.mask_threshold(1e39) == math.inf                    # fl32(1e39) = inf
    # agreement with torch on exact distances at the boundary, rounded-up and rounded-down fields included
    for rec in (math.sqrt(2), math.sqrt(5), math.sqrt(8), math.pi, 2.0, 2.5):
        s = torch.arange(0, 64, dtype=torch.float32)
        assert torch.equal(s.sqrt() > rec, s > _lib.mask_threshold(rec)), rec


def test_header_exports_and_bindings_agree(built):
    from vidtome_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    lib = ctypes.CDLL(built)
    for name in ("vtm_match_masked", "vtm_match_masked_ws_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in _lib.exported_symbols(), name
    assert re.search(r"#define VTM_ABI_VERSION 2\b", hdr) and _lib.lib().vtm_version() == _lib.ABI_VERSION == 2
    # the binding's argument list is the header's
    decl = re.search(r"int vtm_match_masked\((.*?)\);", hdr, re.S).group(1)
    assert len(decl.split(",")) == len(_lib._SIGNATURES["vtm_match_masked"][0]) == 19
    ws = _lib.lib().vtm_match_masked_ws_bytes
    assert ws(2, 3072, 1024) == 2 * (12 + 8) * 32 and ws(1, 256, 256) == 3 * 32 and ws(0, 256, 256) == 0


def test_argument_checks_answer_einval_without_a_launch(built):
    """Every check comes before the first HIP call, so they can be exercised without a GPU (pointers are never followed)."""
    from vidtome_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    good = dict(a=p, b=p, B=2, Ns=300, Nd=200, Ns_pad=512, Nd_pad=256, C_pad=32, align=0, coord=p, Bc=2, P=500, a_rows=p, b_rows=p,
                T=4.0, ws=p, ws_bytes=L.vtm_match_masked_ws_bytes(2, 512, 256), best=p, stream=None)
    bad = [dict(a=None), dict(b=None), dict(best=None), dict(coord=None), dict(a_rows=None), dict(b_rows=None), dict(ws=None),
           dict(B=0), dict(Ns=0), dict(Nd=-1), dict(Ns_pad=256), dict(Ns_pad=384), dict(Nd_pad=128), dict(Nd_pad=320),
           dict(C_pad=0), dict(C_pad=48), dict(Bc=3), dict(Bc=0), dict(P=0), dict(P=1 << 31), dict(T=math.nan),
           dict(coord=p + 4), dict(ws=p + 8), dict(B=1 << 30, Bc=1 << 30)]
    for change in bad:
        args = dict(good, **change)
        assert L.vtm_match_masked(*args.values()) == -1, change                                   # VTM_EINVAL
        assert b"vtm_match_masked" in L.vtm_last_error(), change
    assert L.vtm_match_masked(*dict(good, ws_bytes=good["ws_bytes"] - 1).values()) == -3          # VTM_EWORKSPACE


def test_ratio_zero_returns_the_two_tuple_before_any_draw():
    from vidtome_amd import merge
    x = torch.zeros(2, 64, 8)                       # never looked at: merge.py:181-182 / 599-600 return first
    gen = torch.Generator().manual_seed(3)
    state = gen.get_state().clone()
    for ratio in (0, 0.0, -0.5):
        assert merge.bipartite_soft_matching_random2d_hier(x, 4, ratio, 0, gen) == (merge.do_nothing, merge.do_nothing)
        assert merge.bipartite_soft_matching_2f(x, 48, ratio, False) == (merge.do_nothing, merge.do_nothing)
    assert torch.equal(gen.get_state(), state)
    assert merge.do_nothing(x, mode="mean", b_select=0) is x


def test_more_than_four_coordinate_components_raise():
    from vidtome_amd import merge
    metric = torch.zeros(2, 64, 8)
    for c in (5, 8):
        with pytest.raises(ValueError, match="components"):
            merge._coord_pool(torch.zeros(2, 64, c), metric)
    with pytest.raises(ValueError):
        merge._coord_pool(torch.zeros(2, 63, 2), metric)
    with pytest.raises(ValueError):
        merge._coord_pool(torch.zeros(3, 64, 2), metric)
    pool = merge._coord_pool(torch.arange(2 * 64 * 3, dtype=torch.float64).reshape(2, 64, 3), metric)
    assert pool.shape == (2, 64, 4) and pool.dtype == torch.float32 and not pool[..., 3].any() and pool[1, 63, 2] == 383


def test_the_new_functions_mirror_the_reference_signatures():
    import inspect
    from vidtome_amd import merge
    h = inspect.signature(merge.bipartite_soft_matching_random2d_hier).parameters
    assert list(h) == ["metric", "frame_num", "ratio", "unm_pre", "generator", "target_stride", "adhere_src", "merge_mode", "scores",
                       "coord", "rec_field"]
    assert (h["target_stride"].default, h["adhere_src"].default, h["merge_mode"].default, h["rec_field"].default) == (4, False, "replace", 2)
    f = inspect.signature(merge.bipartite_soft_matching_2f).parameters
    assert list(f) == ["metric", "src_len", "ratio", "adhere_src", "merge_mode", "scores", "coord", "rec_field", "unmerge_chunk"]
    assert (f["merge_mode"].default, f["rec_field"].default, f["unmerge_chunk"].default) == ("replace", 2, 0)
