#!/usr/bin/env python3
"""The reference's receptive-field matchers, `bipartite_soft_matching_random2d_hier` (vidtome/merge.py:162-340) and
`bipartite_soft_matching_2f` (merge.py:582-767) -> tests/golden/rf.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rf.py [reference root]     (needs the reference tree)

Only vidtome/merge.py of the reference is loaded.  For every case of tests/rf_common.py the fixture holds the seed, the frame
draw, the reference's index arrays (read out of the closure cells), `merge(x)` in the replace, "mean" and "sum" modes,
`unmerge` (2f: both chunks), and the `b_select` / `unm_modi` results.  Merged rows are stored with the unm part in ascending
src-index order (rf_common.canonical).  Screening, per case, another seed on failure:
  * fp32 and fp64 runs of the reference give the same src / dst indices and the same unm set, and in fp64 any two node_max
    are more than rounding apart or both exactly 0 (masked), as are the two best scores of every merged row (whose best is an
    unmasked score);
  * ASSERTED on the reference's own fp32 values: no group of exactly equal node_max straddles position r -- otherwise the
    reference's src / unm sets would not be defined by the reference alone (its argsort is not stable)."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import rf_common as rf  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
_spec = importlib.util.spec_from_file_location("ref_vidtome_merge", os.path.join(REF, "vidtome", "merge.py"))
ref_merge = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref_merge)
torch.set_grad_enabled(False)


def cells(fn):
    out = {n: c.cell_contents for n, c in zip(fn.__code__.co_freevars, fn.__closure__)}
    if "split" in out:
        out.update(cells(out["split"]))
    return out


def call(c, x, coord, seed, dtype, chunk=0):
    co = None if coord is None else torch.from_numpy(coord).to(dtype)
    xt = torch.from_numpy(x).to(dtype)
    if c["fn"] == "hier":
        m, u, ret = ref_merge.bipartite_soft_matching_random2d_hier(
            xt, c["F"], c["ratio"], c["unm_pre"], torch.Generator().manual_seed(seed), rf.TARGET_STRIDE, c["adhere_src"],
            coord=co, rec_field=c["rec_field"])
    else:
        m, u, ret = ref_merge.bipartite_soft_matching_2f(xt, rf.src_len_2f(c), c["ratio"], c["adhere_src"], coord=co,
                                                         rec_field=c["rec_field"], unmerge_chunk=chunk)
    cl = cells(m)
    idx = {"a_idx": cl["a_idx"][0, :, 0].numpy(), "b_idx": cl["b_idx"][0, :, 0].numpy()}
    idx.update({k: cl[k][..., 0].numpy().copy() for k in ("unm_idx", "src_idx", "dst_idx")})
    return m, u, ret, idx


def node_max_of(c, x, coord, idx, dtype):
    """node_max and the masked score matrix as the reference computes them (merge.py:229-252) in ``dtype``."""
    xt = torch.from_numpy(x).to(dtype)
    xt = xt / xt.norm(dim=-1, keepdim=True)
    a, b = xt[:, idx["a_idx"]], xt[:, idx["b_idx"]]
    scores = a @ b.transpose(-1, -2)
    if coord is not None:
        co = torch.from_numpy(coord).to(dtype)
        sc, dc = co[:, idx["a_idx"]], co[:, idx["b_idx"]]
        scores[torch.norm(sc[:, :, None, :] - dc[:, None, :, :], dim=-1) > c["rec_field"]] = 0
    if c["adhere_src"]:
        scores = torch.cat([*scores], dim=-1)
    return scores.max(dim=-1)[0].numpy(), scores.numpy()


def screened(c, x, coord, i32, i64):
    if not all(np.array_equal(i32[k], i64[k]) for k in ("a_idx", "b_idx", "src_idx", "dst_idx")):
        return False
    if not np.array_equal(np.sort(i32["unm_idx"], -1), np.sort(i64["unm_idx"], -1)):
        return False
    nm, S = node_max_of(c, x, coord, i64, torch.float64)
    nm, S = np.atleast_2d(nm), (S[None] if S.ndim == 2 else S)
    r = i64["src_idx"].shape[1]
    top = -np.sort(-nm, axis=-1)
    both_zero = (top[:, :-1] == 0) & (top[:, 1:] == 0)            # the rows whose maximum is a masked 0: exactly equal
    if not ((np.abs(np.diff(top, axis=-1)) >= rf.MARGIN) | both_zero).all():
        return False
    for b in range(nm.shape[0]):
        rows = S[b][i64["src_idx"][b]]
        two = -np.sort(-rows, axis=-1)[:, :2]
        if (two[:, 0] - two[:, 1]).min() < rf.MARGIN or two[:, 0].min() < rf.MARGIN:
            return False
    return True


def main():
    out = {}
    for n in range(len(rf.CASES)):
        c = rf.case_dict(n)
        for attempt in range(2000):
            seed = 9100 + 37 * n + attempt
            x = rf.build_inputs(c, seed)
            coord = rf.build_coord(c) if c["with_coord"] else None
            m32, u32, ret, i32 = call(c, x, coord, seed, torch.float32)
            _, _, _, i64 = call(c, x, coord, seed, torch.float64)
            if screened(c, x, coord, i32, i64):
                break
        else:
            raise RuntimeError(f"case {n} could not be screened")
        # the tie condition, on the reference's own fp32 values
        nm32 = np.atleast_2d(node_max_of(c, x, coord, i32, torch.float32)[0])
        r, Ns = i32["src_idx"].shape[1], len(i32["a_idx"])
        assert 0 < r < Ns
        srt = -np.sort(-nm32, axis=-1)
        assert (srt[:, r - 1] > srt[:, r]).all(), f"case {n}: a group of equal node_max straddles position r"
        assert (np.diff(srt[:, :r + 1], axis=-1) < 0).all(), f"case {n}: equal node_max among the merged rows"
        if c["fn"] == "hier":
            randf = int(torch.randint(0, min(rf.TARGET_STRIDE, c["F"]), [1], generator=torch.Generator().manual_seed(seed)))
            ea, eb = rf.partition_hier(c, randf)
        else:
            randf = -1
            ea, eb = rf.partition_2f(c)
        assert np.array_equal(i32["a_idx"], ea) and np.array_equal(i32["b_idx"], eb)
        assert ret["unm_num"] == Ns - r
        out.update({f"{n}/{k}": v for k, v in c.items()})
        out.update({f"{n}/seed": seed, f"{n}/randf": randf})
        for k in rf.IDX:
            out[f"{n}/{k}"] = i32[k].astype(np.int32)
        xt = torch.from_numpy(x)
        rf.store(out, f"{n}/x", x)
        merged = m32(xt)
        zero_masked = 0 if coord is None else int((nm32 == 0).sum())
        rf.store(out, f"{n}/replace", rf.canonical(merged.numpy(), i32["unm_idx"]))
        for mode in ("mean", "sum"):
            rf.store(out, f"{n}/{mode}", rf.canonical(m32(xt, mode=mode).numpy(), i32["unm_idx"]))
        if c["fn"] == "hier":
            rf.store(out, f"{n}/unmerged", u32(merged).numpy())
        else:
            for chunk in (0, 1):
                _, u, _, ic = call(c, x, coord, seed, torch.float32, chunk)
                assert all(np.array_equal(ic[k], i32[k]) for k in rf.IDX)
                rf.store(out, f"{n}/unmerged{chunk}", u(merged).numpy())
        rf.store(out, f"{n}/zero_unmerged", u32(merged, unm_modi="zero").numpy())
        sel = [1, 0]
        bm = m32(xt[sel], b_select=sel)
        rf.store(out, f"{n}/bsel_replace", rf.canonical(bm.numpy(), i32["unm_idx"][sel]))
        rf.store(out, f"{n}/bsel_mean", rf.canonical(m32(xt[sel], mode="mean", b_select=sel).numpy(), i32["unm_idx"][sel]))
        rf.store(out, f"{n}/bsel_unmerged", u32(bm, b_select=sel).numpy())
        rf.store(out, f"{n}/bsel_int_replace", rf.canonical(m32(xt[1:2], b_select=1).numpy(), i32["unm_idx"][1:2]))
        print(f"case {n}: {rf.CASES[n]} N={rf.tokens(c)} Ns={Ns} r={r} randf={randf} rows whose maximum is a masked 0: "
              f"{zero_masked} of {nm32.size} (attempt {attempt})", flush=True)
    out["n_cases"] = np.array(len(rf.CASES))
    path = os.path.join(HERE, "rf.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
