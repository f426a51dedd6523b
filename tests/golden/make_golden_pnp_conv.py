#!/usr/bin/env python3
"""The reference's `register_conv_control` (utils/pnp_utils.py:108-172) on the stand-in resnet of tests/pnp_conv_standin.py,
fp32 on the CPU -> tests/golden/pnp_conv.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pnp_conv.py [reference root]     (needs the reference tree)

Only utils/pnp_utils.py of the reference is loaded.  The fixture holds the stand-in's weights (w1/...: with conv_shortcut,
w0/...: without), the inputs per (B, variant) (x/..., temb/...), and per case of pnp_conv_standin.CASES its fields and the
output of the reference's closure."""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import pnp_conv_standin as st  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
_spec = importlib.util.spec_from_file_location("ref_pnp_utils", os.path.join(REF, "utils", "pnp_utils.py"))
ref_pnp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref_pnp)
torch.set_grad_enabled(False)


def main():
    out = {"n_cases": np.int64(len(st.CASES))}
    for shortcut in (False, True):
        for name, p in st.StandinResnet(shortcut=shortcut).named_parameters():
            out[f"w{int(shortcut)}/{name}"] = p.detach().numpy().copy()
    for i, case in enumerate(st.CASES):
        num_inputs, B, t, shortcut, scale = case
        resnet = st.StandinResnet(shortcut=shortcut, scale=scale).eval()
        model = st.model_around(resnet)
        with contextlib.redirect_stdout(io.StringIO()):     # the reference prints a banner
            ref_pnp.register_conv_control(model, list(st.SCHEDULE), num_inputs)
        resnet.t = t
        x, temb = st.inputs(B, shortcut)
        out[f"x/B{B}s{int(shortcut)}"], out[f"temb/B{B}s{int(shortcut)}"] = x.numpy(), temb.numpy()
        y = resnet.forward(x.clone(), temb.clone())
        plain = st.StandinResnet.forward(resnet, x, temb)
        assert torch.equal(y, plain) != st.injects(t), case      # the injection changes the result exactly when it is due
        for k, v in zip(st.FIELDS, case):
            out[f"{i}/{k}"] = np.asarray(v)
        out[f"{i}/out"] = y.numpy().astype(np.float32)
    path = os.path.join(HERE, "pnp_conv.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
