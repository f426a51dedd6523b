"""bipartite_soft_matching_random2d (vidtome/merge.py:467-579) without a GPU: the fixtures of tests/golden/random2d.npz
against a plain-numpy restatement of the 2-D partition, and the parts of the public function that run before any kernel.

The order of a_idx / b_idx.  The reference splits the tokens with an argsort of a buffer that holds -1 at dst and 0 at src
tokens: all keys of a side are equal, and torch's CPU argsort is not stable, so the order inside each side is whatever its
sort leaves.  The library's order is the stable one, ascending token index.  In ALL 6 of the 6 fixture cases the recorded
order is not the ascending one (the no_rand case and the case without src tokens included), so every case is compared
through the permutation that maps one order to the other, which is asserted to reorder only within src and within dst."""
import numpy as np
import pytest
import torch

import random2d_common as rc
from helpers import load_cases, scatter_reduce_reference

CASES = load_cases("random2d.npz")


def test_fixture_holds_the_cases_of_the_list():
    assert len(CASES) == len(rc.CASES) == 6
    for c, spec in zip(CASES, rc.CASES):
        assert (c["h"], c["w"], c["sx"], c["sy"], c["r"], c["B"], c["C"], bool(c["no_rand"])) == spec
        hsy, wsx = c["h"] // c["sy"], c["w"] // c["sx"]
        assert c["draws"].shape == (hsy * wsx,) and c["draws"].min() >= 0 and c["draws"].max() < c["sx"] * c["sy"]
        Ns = c["h"] * c["w"] - hsy * wsx
        r = min(Ns, c["r"])                                                  # merge.py:542
        assert c["src_idx"].shape == c["dst_idx"].shape == (c["B"], r) and c["unm_idx"].shape == (c["B"], Ns - r)


@pytest.mark.parametrize("n", range(len(rc.CASES)))
def test_partition_restatement_equals_the_reference_lists(n):
    c = CASES[n]
    a, b = rc.partition_2d(c["h"], c["w"], c["sx"], c["sy"], None if c["no_rand"] else c["draws"])
    assert np.all(np.diff(a) > 0) and np.all(np.diff(b) > 0)
    assert set(a) == set(c["a_idx"].tolist()) and set(b) == set(c["b_idx"].tolist())
    assert len(a) == len(c["a_idx"]) and len(b) == len(c["b_idx"]) and len(a) + len(b) == c["h"] * c["w"]
    if np.array_equal(np.sort(c["a_idx"]), c["a_idx"]) and np.array_equal(np.sort(c["b_idx"]), c["b_idx"]):
        assert np.array_equal(a, c["a_idx"]) and np.array_equal(b, c["b_idx"])      # (none of the recorded cases)
    v = rc.stable_view(c)                 # asserts that the permutation reorders within src and within dst only
    assert np.array_equal(a[v["pa"]], c["a_idx"]) and np.array_equal(b[v["pb"]], c["b_idx"])
    # one dst token per cell, inside its cell; the rows / columns behind the last whole cell are src
    hsy, wsx = c["h"] // c["sy"], c["w"] // c["sx"]
    y, x = b // c["w"], b % c["w"]
    assert np.array_equal(np.sort((y // c["sy"]) * wsx + x // c["sx"]), np.arange(hsy * wsx))
    assert y.max() < hsy * c["sy"] and x.max() < wsx * c["sx"]
    if c["no_rand"]:
        assert np.all(y % c["sy"] == 0) and np.all(x % c["sx"] == 0)


@pytest.mark.parametrize("n", range(len(rc.CASES)))
def test_fixture_results_follow_from_the_stable_indices(n):
    """What the GPU tests hold the library to: the reference's index arrays renumbered into the ascending lists give, with
    torch's CPU scatter_reduce, the recorded `merge(x)` -- its dst part permuted back, every bit -- and the recorded
    `unmerge(merge(x))` as it is.  (The sources of a dst row are folded in similarity-rank order under either numbering.)"""
    c = CASES[n]
    v = rc.stable_view(c)
    x = torch.from_numpy(rc.case_inputs(c))
    B = x.shape[0]
    a, b = torch.from_numpy(v["a_idx"]), torch.from_numpy(v["b_idx"])
    unm, src, dst = (torch.from_numpy(v[k]) for k in ("unm_idx", "src_idx", "dst_idx"))
    bi = torch.arange(B)[:, None]
    merged = {}
    for mode in ("mean", "amax"):
        red = scatter_reduce_reference(x, a[src], b.expand(B, -1), dst, mode)
        merged[mode] = torch.cat([x[bi, a[unm]], red], 1)
        rc.assert_stored(c, mode, rc.in_reference_order(merged[mode].numpy(), v["pb"]))
    U = unm.shape[1]
    out = torch.zeros_like(x)                                                # merge.py:562-577
    out[bi, b.expand(B, -1)] = merged["mean"][:, U:]
    out[bi, a[unm]] = merged["mean"][:, :U]
    out[bi, a[src]] = merged["mean"][:, U:][bi, dst]
    rc.assert_stored(c, "unmerged", out.numpy())


def test_nonpositive_r_returns_do_nothing_without_a_draw():
    from vidtome_amd import merge
    gen = torch.Generator().manual_seed(5)
    before = gen.get_state().clone()
    x = torch.randn(1, 64, 8)              # (a CPU tensor: the early-out comes before any device work, as in the reference)
    for r in (0, -3):
        m, u = merge.bipartite_soft_matching_random2d(x, 8, 8, 2, 2, r, generator=gen)
        assert m is merge.do_nothing and u is merge.do_nothing
        assert m(x) is x and m(x, mode="mean") is x and u(x) is x
    assert torch.equal(gen.get_state(), before)


def test_metric_rules_are_those_of_the_other_matchers():
    from vidtome_amd import merge
    gen = torch.Generator().manual_seed(5)
    before = gen.get_state().clone()
    with pytest.raises(RuntimeError, match="GPU only"):
        merge.bipartite_soft_matching_random2d(torch.randn(1, 64, 8), 8, 8, 2, 2, 4, generator=gen)
    with pytest.raises(ValueError, match="B, N, C"):
        merge.bipartite_soft_matching_random2d(torch.randn(64, 8), 8, 8, 2, 2, 4, generator=gen)
    assert torch.equal(gen.get_state(), before)


def test_signature_is_the_reference_one():
    import inspect
    from vidtome_amd import merge
    sig = inspect.signature(merge.bipartite_soft_matching_random2d)
    assert list(sig.parameters) == ["metric", "w", "h", "sx", "sy", "r", "no_rand", "generator"]
    assert sig.parameters["no_rand"].default is False and sig.parameters["generator"].default is None
