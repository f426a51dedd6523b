#!/usr/bin/env python3
"""What PnP feature injection costs on the resnet it patches: one JSON line, also written to profiles/pnp_conv.json.

    python tools/pnp_conv_block.py [--reps 20] [--warmup 5] [--out profiles/pnp_conv.json]

* resnet_call: one call of up_blocks[1].resnets[1] at the cfg-3 size (B = 48, 2560 -> 1280 channels, 16 x 16, fp16,
  num_inputs = 3) at an injecting and at a non-injecting timestep, for "all_rows" (a torch closure that does what the
  reference's does: the main branch for every row with separate ops, the copies, the residual, the division) and "fused"
  (the closure of vidtome_amd.pnp.register_conv_control), plus "source_only_torch" (this project's plain-torch fallback:
  the source-only branch without the kernels).  Device events, median and [min, max] of --reps after --warmup, the
  variants alternating; the fused and all-rows outputs are compared at the timed size.
* groupnorm_silu: vtm_groupnorm_silu alone against F.silu(F.group_norm(...)) at both norm sizes (C = 2560 and 1280, 32
  groups, 16 x 16) for the 48 rows of a non-injecting and the 16 rows of an injecting call, with the bytes moved (one
  read and one write of the tensor) over the time.
* closure_errors: per fixture case (tests/golden/pnp_conv.npz) and dtype, the max abs error of the fused closure and of
  the plain-torch fallback against the reference's recorded fp32 output (the figures tests/test_gpu_pnp_conv.py bounds).
One process; run it under a time limit.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import pnp_conv_standin as st  # noqa: E402
from vidtome_amd import _lib, pnp  # noqa: E402

DEV = "cuda"
SIZES = (32, 2560, 1280, 1280)          # groups, channels in, channels out, time-embedding width
B, NUM_INPUTS, SIDE = 48, 3, 16


def event_ms(fns, reps, warmup):
    """Median and [min, max] ms per variant, the variants alternating inside every repetition."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e))
    return {k: {"ms": round(statistics.median(v), 4), "spread_ms": [round(min(v), 4), round(max(v), 4)], "reps": reps}
            for k, v in times.items()}


def all_rows_forward(resnet, x, temb, inject):
    """The closure as the reference states it: every row through the main branch, then the copies (pnp_utils.py:146-155)."""
    h = pnp._main_branch_torch(resnet, x, temb, None)
    if inject:
        sbs = x.shape[0] // NUM_INPUTS
        h[sbs:2 * sbs] = h[:sbs]
        h[2 * sbs:3 * sbs] = h[:sbs]
    return (resnet.conv_shortcut(x) + h) / resnet.output_scale_factor


def resnet_call(reps, warmup):
    resnet = st.StandinResnet(shortcut=True, sizes=SIZES).eval().to(device=DEV, dtype=torch.float16)
    pnp.register_conv_control(st.model_around(resnet), list(st.SCHEDULE), NUM_INPUTS)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(B, SIZES[1], SIDE, SIDE, generator=gen).to(device=DEV, dtype=torch.float16)
    temb = torch.randn(B, SIZES[3], generator=gen).to(device=DEV, dtype=torch.float16)
    out = {}
    route = pnp._fused_route
    for label, t in (("injecting", st.SCHEDULE[0]), ("non_injecting", 500)):
        resnet.t = t
        inject = st.injects(t)

        def torch_route():
            pnp._fused_route = lambda module, x: False
            try:
                return resnet.forward(x, temb)
            finally:
                pnp._fused_route = route

        with torch.no_grad():
            fns = {"all_rows": lambda: all_rows_forward(resnet, x, temb, inject), "fused": lambda: resnet.forward(x, temb),
                   "source_only_torch": torch_route}
            res = event_ms(fns, reps, warmup)
            ref, got = fns["all_rows"]().double(), fns["fused"]().double()
        res["fused_vs_all_rows_max_abs"] = float((ref - got).abs().max())
        res["out_max_abs"] = float(ref.abs().max())
        out[label] = res
    return out


def groupnorm_alone(reps, warmup):
    out = {}
    for C in (SIZES[1], SIZES[2]):
        for rows in (B, B // NUM_INPUTS):
            gen = torch.Generator().manual_seed(C + rows)
            x = torch.randn(rows, C, SIDE, SIDE, generator=gen).to(device=DEV, dtype=torch.float16)
            gamma, beta = (torch.randn(C, generator=gen).to(device=DEV, dtype=torch.float16) for _ in range(2))
            with torch.no_grad():
                res = event_ms({"vtm_groupnorm_silu": lambda: _lib.groupnorm_silu(x, SIZES[0], gamma, beta, 1e-5),
                                "torch_group_norm_silu": lambda: F.silu(F.group_norm(x, SIZES[0], gamma, beta, 1e-5))}, reps, warmup)
            nbytes = 2 * x.numel() * x.element_size()
            res["bytes_read_plus_written"] = nbytes
            res["vtm_TB_per_s"] = round(nbytes / (res["vtm_groupnorm_silu"]["ms"] * 1e-3) / 1e12, 3)
            out[f"C{C}_rows{rows}"] = res
    return out


def closure_errors():
    z = np.load(os.path.join(ROOT, "tests", "golden", "pnp_conv.npz"), allow_pickle=False)
    out = {}
    for dt, dtype in (("fp32", torch.float32), ("fp16", torch.float16)):
        for n, case in enumerate(st.CASES):
            r = st.closure_errors(n, z, dtype, DEV)
            out[f"{n}_{dt}"] = dict(zip(st.FIELDS, case), **r, bound=2 * r["e_module"] + r["ulp"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_conv.json"))
    ap.add_argument("--norm-only", action="store_true",
                    help="only the groupnorm_silu part, printed and not written (A/B of library variants: VIDTOME_HIP_LIB)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pnp_conv_block.py measures on the GPU; none is visible")
    if args.norm_only:
        print(json.dumps({k: [v["vtm_groupnorm_silu"]["ms"], v["vtm_groupnorm_silu"]["spread_ms"], v["torch_group_norm_silu"]["ms"]]
                          for k, v in groupnorm_alone(args.reps, args.warmup).items()}))
        return
    result = {
        "what": "resnet_call: ms per call of the PnP-patched resnet at the cfg-3 size (B = 48, 2560 -> 1280 channels, 16x16, "
                "fp16, num_inputs = 3); groupnorm_silu: ms per launch at both norm sizes; device events, median and "
                "[min, max] of --reps after --warmup, variants alternating; closure_errors: max abs error against the "
                "reference's recorded fp32 outputs, bound = 2 e_module + ulp",
        "device": torch.cuda.get_device_name(0),
        "closure_errors": closure_errors(),
        "groupnorm_silu": groupnorm_alone(args.reps, args.warmup),
        "resnet_call": resnet_call(args.reps, args.warmup),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
