"""bipartite_soft_matching_random2d on the GPU (run with -m gpu on an MI355X): vtm_partition_2d against the plain-numpy
restatement of the partition, and the public function against the reference's recorded run (tests/golden/random2d.npz).

The reference's a_idx / b_idx come out of an unstable argsort of equal keys; the library's are in ascending token order
(include/vidtome_hip.h).  So the recorded unm / src / dst_idx are renumbered into the ascending lists and the dst part of
the recorded `merge(x)` is read through the same permutation (random2d_common.stable_view / in_reference_order;
tests/test_random2d_host.py shows on the CPU that this is exactly what the recorded indices give).  tests/helpers.py has no
tie-aware comparison of its own; the one here restates test_gpu_parity._tie_aware_equal for a level that is never aligned."""
import functools

import numpy as np
import pytest
import torch

import random2d_common as rc
from helpers import REDUCE_MODES, load_cases, same_bits, scatter_reduce_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CASES = load_cases("random2d.npz")
ALL = range(len(rc.CASES))

# (h, w, sx, sy) beyond the fixture's: one cell column / row / cell, cell rows of more than one 256-token chunk, rows and
# columns behind the last whole cell (less and more than one workgroup of them), 128 x 128 in 2 x 2 cells and as one cell row
EXTRA_GEOMETRIES = [(8, 8, 8, 2), (8, 8, 2, 8), (20, 20, 2, 20), (20, 20, 20, 20), (13, 7, 3, 5), (33, 40, 3, 2), (70, 9, 2, 3),
                    (7, 300, 4, 4), (5, 1, 1, 1), (1, 9, 2, 1), (128, 128, 2, 2), (128, 128, 4, 128)]


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _partition(L, h, w, sx, sy, draws):
    d = None if draws is None else torch.from_numpy(np.asarray(draws, np.int32)).to(DEV)
    a, b = L.partition_2d(DEV, h, w, sx, sy, d)
    return a.cpu().numpy(), b.cpu().numpy()


@pytest.mark.parametrize("n", ALL)
def test_partition_2d_equals_the_restatement_on_the_fixture_cases(L, n):
    c = CASES[n]
    draws = None if c["no_rand"] else c["draws"]
    a, b = _partition(L, c["h"], c["w"], c["sx"], c["sy"], draws)
    ea, eb = rc.partition_2d(c["h"], c["w"], c["sx"], c["sy"], draws)
    assert a.dtype == b.dtype == np.int32 and np.array_equal(a, ea) and np.array_equal(b, eb)


@pytest.mark.parametrize("geometry", EXTRA_GEOMETRIES)
def test_partition_2d_equals_the_restatement_on_other_geometries(L, geometry):
    h, w, sx, sy = geometry
    rng = np.random.default_rng(h * 1000 + w * 10 + sx)
    cells = (h // sy) * (w // sx)
    for draws in (None, rng.integers(0, sx * sy, size=cells), np.full(cells, sx * sy - 1)):
        a, b = _partition(L, h, w, sx, sy, draws)
        ea, eb = rc.partition_2d(h, w, sx, sy, draws)
        assert np.array_equal(a, ea) and np.array_equal(b, eb), (geometry, draws is None)
    # a draw outside [0, sx * sy) counts modulo the cell size (every cell keeps exactly one dst token)
    draws = rng.integers(0, sx * sy, size=cells)
    a, b = _partition(L, h, w, sx, sy, draws + 3 * sx * sy)
    ea, eb = rc.partition_2d(h, w, sx, sy, draws)
    assert np.array_equal(a, ea) and np.array_equal(b, eb), geometry


def test_partition_2d_refuses_bad_arguments_and_leaves_the_outputs_alone(L):
    h, w = 8, 8
    a = torch.full((h * w,), -7, dtype=torch.int32, device=DEV)
    b = torch.full((h * w,), -7, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    fn = L.lib().vtm_partition_2d
    bad = [(h, w, 0, 2, b.data_ptr(), a.data_ptr()), (h, w, 2, 0, b.data_ptr(), a.data_ptr()),
           (h, w, -1, 2, b.data_ptr(), a.data_ptr()), (h, w, 2, -2, b.data_ptr(), a.data_ptr()),
           (h, w, w + 1, 2, b.data_ptr(), a.data_ptr()), (h, w, 2, h + 1, b.data_ptr(), a.data_ptr()),
           (0, w, 2, 2, b.data_ptr(), a.data_ptr()), (h, w, 2, 2, None, a.data_ptr()), (h, w, 2, 2, b.data_ptr(), None)]
    for hh, ww, sx, sy, bp, ap in bad:
        assert fn(hh, ww, sx, sy, None, bp, ap, stream) == -1, (hh, ww, sx, sy, bp is None, ap is None)      # VTM_EINVAL
        assert b"vtm_partition_2d" in L.lib().vtm_last_error()
    torch.cuda.synchronize()
    assert bool((a == -7).all()) and bool((b == -7).all())
    with pytest.raises(ValueError):
        L.partition_2d(DEV, h, w, w + 1, 2, None)
    # without src tokens there is no a_idx to write: a null pointer is then fine
    assert fn(h, w, 1, 1, None, b.data_ptr(), None, stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(b.cpu().numpy(), np.arange(h * w))


@functools.lru_cache(maxsize=None)
def _run(n):
    """One call of the public function per fixture case, shared by the tests below."""
    from vidtome_amd import merge
    c = CASES[n]
    x = torch.from_numpy(rc.case_inputs(c)).to(DEV)
    gen = torch.Generator().manual_seed(int(c["seed"]))
    m, u = merge.bipartite_soft_matching_random2d(x, c["w"], c["h"], c["sx"], c["sy"], c["r"], no_rand=bool(c["no_rand"]),
                                                  generator=gen)
    return c, rc.stable_view(c), x, m, u, gen.get_state().clone()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("n", ALL)
def test_indices_equal_the_reference_run(L, n):
    """a_idx / b_idx exactly; unm / src / dst_idx exactly except inside groups of exactly equal node_max, where the canonical
    order is the stable one (the suite's tie rule, tests/test_oracle_golden.py)."""
    c, v, x, m, u, _ = _run(n)
    level = m.level
    assert u.level is level and level.r == min(level.Ns, c["r"]) and level.Ns == len(v["a_idx"]) and level.Nd == len(v["b_idx"])
    assert np.array_equal(level.a_pos.cpu().numpy(), v["a_idx"]) and np.array_equal(level.b_pos.cpu().numpy(), v["b_idx"])
    got = {k: getattr(level, k).cpu().numpy() for k in ("unm_idx", "src_idx", "dst_idx")}
    for k in got:
        assert got[k].shape == v[k].shape and got[k].dtype == np.int32, k
    if all(np.array_equal(got[k], v[k]) for k in got):
        return
    nm, ni = L.decode_best(level.best)
    nm, ni = nm.cpu().numpy(), ni.cpu().numpy()
    for b in range(c["B"]):
        assert np.array_equal(_bits(nm[b][v["src_idx"][b]]), _bits(nm[b][got["src_idx"][b]]))
        assert np.array_equal(_bits(nm[b][v["unm_idx"][b]]), _bits(nm[b][got["unm_idx"][b]]))
        assert np.array_equal(np.sort(np.concatenate([got["src_idx"][b], got["unm_idx"][b]])), np.arange(level.Ns))
        assert np.array_equal(ni[b][v["src_idx"][b]], v["dst_idx"][b])
        assert np.array_equal(ni[b][got["src_idx"][b]], got["dst_idx"][b])


@pytest.mark.parametrize("n", ALL)
def test_merge_and_unmerge_equal_the_reference_run_in_fp32(n):
    c, v, x, m, u, _ = _run(n)
    merged = m(x)                                                            # mode="mean" by default (merge.py:552)
    assert merged.shape == (c["B"], c["h"] * c["w"] - min(len(v["a_idx"]), c["r"]), c["C"])
    rc.assert_stored(c, "mean", rc.in_reference_order(merged.cpu().numpy(), v["pb"]))
    assert torch.equal(m(x, mode="mean"), merged)
    rc.assert_stored(c, "amax", rc.in_reference_order(m(x, mode="amax").cpu().numpy(), v["pb"]))
    rc.assert_stored(c, "unmerged", u(merged).cpu().numpy())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("n", ALL)
def test_merge_of_16_bit_tokens_equals_torch_scatter_reduce(n, dtype):
    """The closures take tokens of another dtype than the metric's; every mode then equals torch's CPU scatter_reduce on the
    level's own indices bit for bit (the contract of vtm_merge_reduce), and unmerge is a pure row copy."""
    c, v, x, m, u, _ = _run(n)
    level = m.level
    xl = x.to(dtype)
    xc = xl.cpu()
    B = xc.shape[0]
    a, b = level.a_pos.cpu().long(), level.b_pos.cpu().long()
    unm, src, dst = level.unm_idx.cpu().long(), level.src_idx.cpu().long(), level.dst_idx.cpu().long()
    bi = torch.arange(B)[:, None]
    for mode in REDUCE_MODES:
        want = torch.cat([xc[bi, a[unm]], scatter_reduce_reference(xc, a[src], b.expand(B, -1), dst, mode)], 1)
        got = m(xl, mode=mode).cpu()
        assert bool(same_bits(got, want).all()), (mode, int((~same_bits(got, want)).sum()))
    merged = m(xl)
    U = unm.shape[1]
    want = torch.zeros_like(xc)
    mc = merged.cpu()
    want[bi, b.expand(B, -1)] = mc[:, U:]
    want[bi, a[unm]] = mc[:, :U]
    want[bi, a[src]] = mc[:, U:][bi, dst]
    assert bool(same_bits(u(merged).cpu(), want).all())


@pytest.mark.parametrize("n", ALL)
def test_generator_state_is_that_after_the_single_draw(n):
    c, _, _, _, _, state = _run(n)
    gen = torch.Generator().manual_seed(int(c["seed"]))
    if not c["no_rand"]:
        hsy, wsx = c["h"] // c["sy"], c["w"] // c["sx"]
        draws = torch.randint(c["sy"] * c["sx"], size=(hsy, wsx, 1), generator=gen)            # merge.py:500-501
        assert np.array_equal(draws.reshape(-1).numpy(), c["draws"])
    assert torch.equal(state, gen.get_state())


def test_merge_takes_scatter_reduce_modes_only():
    _, _, x, m, _, _ = _run(0)
    for mode in ("replace", "median", None):
        with pytest.raises(ValueError):
            m(x, mode=mode)
