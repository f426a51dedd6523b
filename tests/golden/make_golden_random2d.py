#!/usr/bin/env python3
"""The reference's per-frame 2-D matcher, `bipartite_soft_matching_random2d` (vidtome/merge.py:467-579) -> tests/golden/random2d.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_random2d.py     (build container only: imports /root/reference)

For every case of tests/random2d_common.py the fixture holds the cell draws, the reference's index arrays (read out of the
closure cells, in the reference's own order), `merge(x)` in "mean" and "amax" mode and `unmerge(merge(x))`.  The inputs are
planted on the partition the draws give (random2d_common.build_inputs) and screened like the other fixtures: fp32 and fp64
runs of the reference give the same indices and the best cosines are separated by more than rounding.  Arrays above
random2d_common.FULL_BYTES are stored as a sha256 of their fp32 bytes plus a few sampled rows (as planted*.npz do); so are
the inputs, which the tests rebuild from the seed."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (imports the reference)
import random2d_common as rc  # noqa: E402

ref_merge = mg.ref_merge


def store(out, key, arr, row_axis=1):
    arr = np.ascontiguousarray(arr)
    if arr.nbytes <= rc.FULL_BYTES:
        out[key] = arr
        return
    rows = rc.sample_rows(arr.shape[row_axis])
    out[key + "_sha256"] = rc.sha(arr)
    out[key + "_rows"] = np.take(arr, rows, axis=row_axis)


def run(x, w, h, sx, sy, r, no_rand, seed, dtype):
    m, u = ref_merge.bipartite_soft_matching_random2d(x.to(dtype), w, h, sx, sy, r, no_rand=no_rand,
                                                      generator=mg.fork_generator(seed))
    c = mg.cells(m)
    idx = {"a_idx": mg.np64(c["a_idx"])[0, :, 0], "b_idx": mg.np64(c["b_idx"])[0, :, 0]}
    idx.update({k: mg.np64(c[k])[..., 0] for k in ("unm_idx", "src_idx", "dst_idx")})
    return m, u, idx


def main():
    out = {}
    for n, (h, w, sx, sy, r, B, C, no_rand) in enumerate(rc.CASES):
        hsy, wsx = h // sy, w // sx
        for attempt in range(50):
            seed = 7000 + 31 * n + attempt
            draws = None
            if not no_rand:      # the reference's single draw (merge.py:500-501) on a generator forked like the blocks' are
                draws = torch.randint(sy * sx, size=(hsy, wsx, 1), generator=mg.fork_generator(seed)).numpy().reshape(-1)
            a_idx, b_idx = rc.partition_2d(h, w, sx, sy, draws)
            x = torch.from_numpy(rc.build_inputs(h, w, B, C, a_idx, b_idx, seed))
            m32, u32, i32 = run(x, w, h, sx, sy, r, no_rand, seed, torch.float32)
            _, _, i64 = run(x, w, h, sx, sy, r, no_rand, seed, torch.float64)
            assert np.array_equal(np.sort(i32["a_idx"]), a_idx) and np.array_equal(np.sort(i32["b_idx"]), b_idx)
            g1, g2 = (1.0, 1.0) if len(a_idx) == 0 else mg.margins(x, torch.from_numpy(i32["a_idx"]),
                                                                    torch.from_numpy(i32["b_idx"]), False)
            if all(np.array_equal(i32[k], i64[k]) for k in rc.IDX) and min(g1, g2) >= mg.MARGIN:
                break
        else:
            raise RuntimeError(f"case {n} could not be screened")
        out.update({f"{n}/h": h, f"{n}/w": w, f"{n}/sx": sx, f"{n}/sy": sy, f"{n}/r": r, f"{n}/B": B, f"{n}/C": C,
                    f"{n}/no_rand": no_rand, f"{n}/seed": seed,
                    f"{n}/draws": np.zeros(hsy * wsx, np.int32) if draws is None else draws.astype(np.int32)})
        for k in rc.IDX:
            out[f"{n}/{k}"] = i32[k].astype(np.int32)
        store(out, f"{n}/x", x.numpy())
        merged = m32(x)
        assert np.array_equal(merged.numpy(), m32(x, mode="mean").numpy())      # (the default mode)
        store(out, f"{n}/mean", merged.numpy())
        store(out, f"{n}/amax", m32(x, mode="amax").numpy())
        store(out, f"{n}/unmerged", u32(merged).numpy())
        asc = bool(np.array_equal(i32["a_idx"], a_idx) and np.array_equal(i32["b_idx"], b_idx))
        print(f"case {n}: {h} x {w} stride ({sx}, {sy}) B={B} C={C} Ns={len(a_idx)} Nd={len(b_idx)} r={i32['src_idx'].shape[1]} "
              f"a_idx / b_idx ascending: {asc} margins {g1:.2e} {g2:.2e} (attempt {attempt})", flush=True)
    out["n_cases"] = np.array(len(rc.CASES))
    path = os.path.join(HERE, "random2d.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
