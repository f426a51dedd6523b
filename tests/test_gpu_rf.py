"""The receptive-field matchers on the GPU (run with -m gpu on an MI355X): bipartite_soft_matching_random2d_hier / _2f against
the reference's recorded runs (tests/golden/rf.npz), and vtm_match_masked through the C ABI against the bitwise restatement of
tests/rf_common.py, with the dead-tile skip on and off and against vtm_match.

Run as a script (`python tests/test_gpu_rf.py out.npz`) this file is the fresh child process of the skip on / off comparison: it
computes the packed keys of SKIP_CASES under whatever environment it was started with and writes them to `out.npz`."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    _T = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(_T), _T, os.path.join(_T, "golden")]
import rf_common as rf  # noqa: E402
from helpers import load_cases  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CASES = load_cases("rf.npz")
ALL = range(len(rf.CASES))
REC_FIELDS = (0.5, 2, 1e9, -1)          # 1e9: nothing masked; -1: everything


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---- 1. the public functions against the reference's recorded runs ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _run(n):
    from vidtome_amd import merge
    c = CASES[n]
    assert tuple(c[k] for k in rf.FIELDS) == rf.CASES[n], n
    xn = rf.build_inputs(c, c["seed"])
    rf.assert_stored(c, "x", xn)
    x = torch.from_numpy(xn).to(DEV)
    coord = torch.from_numpy(rf.build_coord(c)).to(DEV) if c["with_coord"] else None
    gen = torch.Generator().manual_seed(int(c["seed"]))
    if c["fn"] == "hier":
        res = merge.bipartite_soft_matching_random2d_hier(x, c["F"], c["ratio"], c["unm_pre"], gen, rf.TARGET_STRIDE,
                                                          bool(c["adhere_src"]), coord=coord, rec_field=c["rec_field"])
        res = {0: res}
    else:
        res = {k: merge.bipartite_soft_matching_2f(x, rf.src_len_2f(c), c["ratio"], bool(c["adhere_src"]), coord=coord,
                                                   rec_field=c["rec_field"], unmerge_chunk=k) for k in (0, 1)}
    return c, x, res, gen.get_state().clone()


@pytest.mark.parametrize("n", ALL)
def test_indices_equal_the_reference_run(L, n):
    """a_idx / b_idx / src_idx / dst_idx exactly (the fixture's merged rows have pairwise different node_max); unm_idx as a set,
    and with the same node_max bits position by position: inside the group of rows whose maximum is a masked 0 the reference's
    unstable argsort and the library's stable one may order differently."""
    c, x, res, state = _run(n)
    for m, u, ret in res.values():
        level = ret["level"]
        assert ret["unm_num"] == level.unm_num == c["unm_idx"].shape[1] and level.r == c["src_idx"].shape[1]
        got = {k: ret[k].cpu().numpy() for k in rf.IDX}
        for k in rf.IDX:
            assert got[k].dtype == np.int32 and got[k].shape == c[k].shape, k
        for k in ("a_idx", "b_idx", "src_idx", "dst_idx"):
            assert np.array_equal(got[k], c[k]), k
        assert np.array_equal(np.sort(got["unm_idx"], -1), np.sort(c["unm_idx"], -1))
        nm = L.decode_best(level.best)[0].cpu().numpy()
        nm = np.broadcast_to(nm, (c["B"], nm.shape[1]))
        assert np.array_equal(_bits(np.take_along_axis(nm, got["unm_idx"].astype(np.int64), 1)),
                              _bits(np.take_along_axis(nm, c["unm_idx"].astype(np.int64), 1)))
    if c["fn"] == "hier":        # the single draw of merge.py:198 was made on the caller's generator
        gen = torch.Generator().manual_seed(int(c["seed"]))
        assert int(torch.randint(0, min(rf.TARGET_STRIDE, c["F"]), [1], generator=gen)) == c["randf"]
        assert torch.equal(state, gen.get_state())


@pytest.mark.parametrize("n", ALL)
def test_closures_equal_the_reference_run(n):
    c, x, res, _ = _run(n)
    m, u, ret = res[0]
    unm = ret["unm_idx"].cpu().numpy()
    canon = lambda t, ui=unm: rf.canonical(t.cpu().numpy(), ui)
    merged = m(x)                                                      # merge_mode="replace"
    assert merged.shape == (c["B"], rf.tokens(c) - c["src_idx"].shape[1], c["C"])
    rf.assert_stored(c, "replace", canon(merged))
    assert torch.equal(m(x, mode="replace"), merged)
    for mode in ("mean", "sum"):                                       # 2f: the first r src rows are folded (merge.py:718)
        rf.assert_stored(c, mode, canon(m(x, mode=mode)))
    if c["fn"] == "hier":
        rf.assert_stored(c, "unmerged", u(merged).cpu().numpy())
    else:
        for k in (0, 1):
            rf.assert_stored(c, f"unmerged{k}", res[k][1](merged).cpu().numpy())
    rf.assert_stored(c, "zero_unmerged", u(merged, unm_modi="zero").cpu().numpy())
    assert torch.equal(u(merged, unm_modi="other"), u(merged))         # only "zero" means anything (merge.py:326-328)
    sel = [1, 0]
    xs = x[sel].contiguous()
    bm = m(xs, b_select=sel)
    rf.assert_stored(c, "bsel_replace", canon(bm, unm[sel]))
    rf.assert_stored(c, "bsel_mean", canon(m(xs, mode="mean", b_select=sel), unm[sel]))
    rf.assert_stored(c, "bsel_unmerged", u(bm, b_select=sel).cpu().numpy())
    rf.assert_stored(c, "bsel_int_replace", canon(m(x[1:2].contiguous(), b_select=1), unm[1:2]))


def test_merge_closure_with_a_default_mode(L):
    """merge_mode= of the constructor is the mode of merge(x) (merge.py:301 / 719)."""
    from vidtome_amd import merge
    c, x, res, _ = _run(0)
    coord = torch.from_numpy(rf.build_coord(c)).to(DEV)
    m, _, _ = merge.bipartite_soft_matching_random2d_hier(x, c["F"], c["ratio"], 0, torch.Generator().manual_seed(int(c["seed"])),
                                                          rf.TARGET_STRIDE, False, "mean", None, coord, c["rec_field"])
    assert torch.equal(m(x), res[0][0](x, mode="mean"))


@pytest.mark.parametrize("n", [0, 1, 9])
def test_one_coordinate_set_serves_every_sample(n):
    """coord of shape (1, N, c): the pool's batch stride is 0; the fixture's samples share their coordinates, so nothing changes."""
    from vidtome_amd import merge
    c, x, res, _ = _run(n)
    coord = torch.from_numpy(rf.build_coord(c)[:1]).to(DEV)
    if c["fn"] == "hier":
        _, _, ret = merge.bipartite_soft_matching_random2d_hier(x, c["F"], c["ratio"], c["unm_pre"],
                                                                torch.Generator().manual_seed(int(c["seed"])), rf.TARGET_STRIDE,
                                                                bool(c["adhere_src"]), coord=coord, rec_field=c["rec_field"])
    else:
        _, _, ret = merge.bipartite_soft_matching_2f(x, rf.src_len_2f(c), c["ratio"], bool(c["adhere_src"]), coord=coord,
                                                     rec_field=c["rec_field"])
    assert torch.equal(ret["level"].best, res[0][2]["level"].best)
    for k in rf.IDX:
        assert torch.equal(ret[k], res[0][2][k]), k


# ---- 2. vtm_match_masked through the C ABI against the bitwise restatement ----------------------------------------------------
def _geometry(side, F=4):
    """F frames of side x side tokens, frame 1 is dst (merge.py:200 with randf = 1): a_rows are not one run of rows."""
    c = {"F": F, "h": side, "w": side, "unm_pre": 0, "B": 2}
    a_idx, b_idx = rf.partition_hier(c, 1)
    return c, a_idx, b_idx


@functools.lru_cache(maxsize=None)
def _problem(side, C, special=None):
    """x, coord, the row lists and the oracle-bit score matrix of one shape, shared by every (align, rec_field) of it."""
    from oracle import oracle
    oracle.build()
    c, a_idx, b_idx = _geometry(side)
    c["C"], c["corr"] = C, 0.5
    x = rf.build_inputs(c, 4242 + side + C)
    coord = rf.build_coord(c)
    if special == "nan_coord":       # a src and a dst token without a position: their pairs are unmasked (NaN > x is false)
        coord[0, a_idx[5], 0] = np.nan
        coord[1, b_idx[130], 1] = np.nan
    elif special == "nan_row":       # a src and a dst token of NaNs: NaN where unmasked, 0 where masked
        x[0, a_idx[300]] = np.nan
        x[1, b_idx[77], 3] = np.nan
    elif special == "shuffled":      # coordinates in random row order: every tile's box is the whole frame
        rng = np.random.default_rng(5)
        coord = np.stack([coord[b][rng.permutation(coord.shape[1])] for b in range(coord.shape[0])])
    S = rf.score_bits(oracle, oracle.normalize_gather(x, a_idx[None]), oracle.normalize_gather(x, b_idx[None]))
    S.setflags(write=False)
    return x, coord, a_idx, b_idx, S


def _device_problem(L, x, coord, a_idx, b_idx):
    B = x.shape[0]
    xd = torch.from_numpy(x).to(DEV)
    pool = torch.zeros((B, x.shape[1], 4), dtype=torch.float32, device=DEV)
    pool[:, :, :coord.shape[2]] = torch.from_numpy(coord).to(DEV)
    rows = [torch.from_numpy(np.broadcast_to(i.astype(np.int32), (B, len(i))).copy()).to(DEV) for i in (a_idx, b_idx)]
    a_op, _ = L.normalize_gather(xd, None, rows[0])
    b_op, _ = L.normalize_gather(xd, None, rows[1])
    return a_op, b_op, pool, rows[0], rows[1]


def _masked(L, dp, Ns, Nd, align, rec_field):
    """One raw vtm_match_masked call -> the packed keys (int64 bits) on the host."""
    a_op, b_op, pool, a_rows, b_rows = dp
    B = a_op.shape[0]
    Ns_pad, Nd_pad, C_pad = a_op.shape[3], b_op.shape[3], a_op.shape[1] * 8
    nbytes = L.lib().vtm_match_masked_ws_bytes(B, Ns_pad, Nd_pad)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    best = torch.empty((1 if align else B, Ns), dtype=torch.int64, device=DEV)
    rc = L.lib().vtm_match_masked(a_op.data_ptr(), b_op.data_ptr(), B, Ns, Nd, Ns_pad, Nd_pad, C_pad, int(align), pool.data_ptr(),
                                  pool.shape[0], pool.shape[1], a_rows.data_ptr(), b_rows.data_ptr(), L.mask_threshold(rec_field),
                                  ws.data_ptr(), nbytes, best.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.lib().vtm_last_error()
    torch.cuda.synchronize()
    return best


def _check_against_restatement(L, side, C, align, rec_field, special=None):
    x, coord, a_idx, b_idx, S = _problem(side, C, special)
    best = _masked(L, _device_problem(L, x, coord, a_idx, b_idx), len(a_idx), len(b_idx), align, rec_field)
    nm, ni = (t.cpu().numpy() for t in L.decode_best(best))
    Sm = np.where(rf.mask_of(coord[:, a_idx], coord[:, b_idx], rec_field), np.float32(0), S)
    want_nm, want_ni = (np.atleast_2d(t) for t in rf.row_max(Sm, align))
    assert nm.shape == want_nm.shape
    assert np.array_equal(ni, want_ni), (int((ni != want_ni).sum()), ni.size)
    assert np.array_equal(_bits(nm), _bits(want_nm)) or np.array_equal(np.isnan(nm), np.isnan(want_nm)) and \
        np.array_equal(_bits(nm)[~np.isnan(nm)], _bits(want_nm)[~np.isnan(nm)])
    return want_nm


@pytest.mark.parametrize("rec_field", REC_FIELDS)
@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("side", [20, 32])
def test_match_masked_equals_the_restatement(L, side, C, align, rec_field):
    """20 x 20: Nd = 400 = 4 dst tiles and Ns = 1200 = 5 src tiles, the last of each partial.  32 x 32: Nd = 1024 = 8 dst tiles
    (one split of 8 K-steps at C = 32, two at C = 64), 12 src tiles, at rec_field = 2 about half the tile pairs dead."""
    nm = _check_against_restatement(L, side, C, align, rec_field)
    if rec_field == -1:
        assert not nm.any()
    if rec_field == 0.5:        # one unmasked score per row and sample: where it is negative the maximum is a masked zero
        assert 0 < (nm == 0).mean() < 1


def test_match_masked_equals_the_restatement_at_320_channels(L):
    _check_against_restatement(L, 20, 320, 0, 2)


@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("special", ["nan_coord", "nan_row"])
def test_match_masked_with_nan_coordinates_and_nan_tokens(L, special, align):
    nm = _check_against_restatement(L, 20, 32, align, 2, special)
    if special == "nan_row":
        assert np.isnan(nm).any()


# ---- 3. the dead-tile skip changes no bit -------------------------------------------------------------------------------------
SKIP_CASES = [(C, special, align, rec_field) for C in (32, 64) for special in (None, "shuffled") for align in (0, 1)
              for rec_field in (0.5, 2)]


def _skip_keys(L):
    out = {}
    for C, special, align, rec_field in SKIP_CASES:
        x, coord, a_idx, b_idx, _ = _problem_inputs(32, C, special)
        out[f"{C}/{special}/{align}/{rec_field}"] = _masked(L, _device_problem(L, x, coord, a_idx, b_idx), len(a_idx), len(b_idx),
                                                            align, rec_field).cpu().numpy()
    return out


def _problem_inputs(side, C, special):
    """_problem without the score matrix (the child process needs none)."""
    c, a_idx, b_idx = _geometry(side)
    c["C"], c["corr"] = C, 0.5
    x, coord = rf.build_inputs(c, 4242 + side + C), rf.build_coord(c)
    if special == "shuffled":
        rng = np.random.default_rng(5)
        coord = np.stack([coord[b][rng.permutation(coord.shape[1])] for b in range(coord.shape[0])])
    return x, coord, a_idx, b_idx, None


def test_box_skip_on_and_off_give_the_same_bits(L, tmp_path):
    """The 32 x 32 shapes (C = 32 and 64) in (frame, position) order, where about half the tiles are dead at rec_field = 2 and most at 0.5, and
    with the coordinates in random row order, where none is: this process (skip on) against a fresh child started with
    VTM_DEBUG_NOBOXSKIP=1 (the hook is read once per process)."""
    assert not os.environ.get("VTM_DEBUG_NOBOXSKIP")
    mine = _skip_keys(L)
    out = str(tmp_path / "noskip.npz")
    env = dict(os.environ, VTM_DEBUG_NOBOXSKIP="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    theirs = np.load(out)
    assert sorted(theirs.files) == sorted(mine)
    for k in mine:
        assert np.array_equal(mine[k], theirs[k]), k
    # ... and the ordered cases are the ones test 2 holds to the restatement; the shuffled ones are held to it here
    for C in (32, 64):
        _check_against_restatement(L, 32, C, C == 64, 2, "shuffled")


# ---- 4. nothing masked: vtm_match ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("side,C", [(20, 32), (32, 64), (20, 320)])
def test_nothing_masked_equals_vtm_match_bit_for_bit(L, side, C, align):
    x, coord, a_idx, b_idx, _ = _problem_inputs(side, C, None)
    dp = _device_problem(L, x, coord, a_idx, b_idx)
    got = _masked(L, dp, len(a_idx), len(b_idx), align, 1e9)
    want = L.match(dp[0], dp[1], len(a_idx), len(b_idx), bool(align))
    assert torch.equal(got, want)


def test_python_wrapper_checks_its_arguments(L):
    from vidtome_amd import merge
    c, x, _, _ = _run(0)
    coord5 = torch.zeros((c["B"], x.shape[1], 5), device=DEV)
    with pytest.raises(ValueError):
        merge.bipartite_soft_matching_random2d_hier(x, c["F"], .5, 0, torch.Generator().manual_seed(1), coord=coord5)
    with pytest.raises(ValueError):
        merge.bipartite_soft_matching_2f(x, 192, .5, False, coord=coord5)
    with pytest.raises(ValueError):
        merge.bipartite_soft_matching_2f(x, 192, .5, False, coord=coord5[:, :7, :2])


if __name__ == "__main__":
    from vidtome_amd import _lib as _L
    _L.lib()
    np.savez(sys.argv[1], **_skip_keys(_L))
