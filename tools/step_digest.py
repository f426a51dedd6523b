"""Digest of what the caller-side step kernels compute, for a bit-for-bit A/B of two built libraries under ONE host layer: one
line per call -- case name, then the sha256 of every output.

    VIDTOME_HIP_LIB=<libvidtome_hip.so> python tools/step_digest.py [--out FILE]

Two runs compare with `diff`: every input is seeded on the CPU, every output buffer is preset, and a case depends on no other.

Cases (the smallest shapes at which each path of csrc/step_core.h and its users can go wrong):
  guided/* solver/*   fp32 / fp16 / bf16 x the three prediction types x rescale 0 / 0.7 x 3 frames scattered into a 7-frame
               video (4, 0, 2) or an ascending run (2, 3, 4) x E = 140 (element accesses, a short last chunk), 256, 8203 (more
               than one chunk per lane of the per-frame workgroup, ragged); every output asked for.  guided: two groups,
               sigma != 0 with noise.  solver: three groups with a weight of 0, g_ref = 1 (not the last), both history terms,
               h_out a buffer of its own.
  */offset     a base pointer one element off a 16-byte boundary with E a multiple of the chunk (element accesses)
  */inplace    out is x
  guided/groups=1|3, guided/sigma=0
  solver/h_out=h2, solver/no history (c_h1 = c_h2 = 0), solver/noise (c_noise != 0)
  */grid cap   one elementwise launch beyond the grid cap: 17 fp32 frames of 4 x 256 x 256
  sag/*        sag_degrade under the three prediction types, (2, 4, 8, 8), r = 2, with the mask
  lds/*        one call past the 64 KB of dynamic LDS that need the opt-in: sag_degrade on one 96 x 96 plane, semantic_guidance
               on one 120 x 120 plane, freeu on 2 x 8192 planes, groupnorm_silu on one fp32 group of 16400 elements, linear_rows
               in its weight-stationary form (K = 320, which opts in at every size)"""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda"
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
PREDS = {"epsilon": 0, "v": 1, "sample": 2}
FRAMES = 7
COEF = dict(sqrt_alpha=0.8366600275039673, sqrt_beta=0.5477225575051661)


def sha(t):
    if t is None:
        return "-"
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:24]


def draw(shape, dtype, seed, offset=0):
    """Seeded N(0, 1) on the device; ``offset`` elements behind the start of its allocation."""
    g = torch.Generator().manual_seed(seed)
    n = 1
    for s in shape:
        n *= s
    flat = torch.empty(n + offset, dtype=dtype, device=DEV)
    flat[offset:] = torch.randn(n, generator=g).to(dtype)
    return flat[offset:].view(shape)


def guided(_lib, dtype, pred, rescale, ids, E, seed, groups=2, sigma=0.3, offset=0, inplace=False, frames=FRAMES):
    F = frames if ids is None else len(ids)
    x = draw((frames, E), dtype, seed, offset)
    mo = draw((groups * F, E), dtype, seed + 1)
    noise = draw((F, E), dtype, seed + 2) if sigma else None
    out = x if inplace else torch.zeros_like(x)
    res = _lib.guided_step(x, mo, COEF["sqrt_alpha"], COEF["sqrt_beta"], 0.9, 0.4, sigma, groups=groups, frame_ids=ids,
                           pred_type=pred, guidance=7.5, rescale=rescale if groups >= 2 else 0.0, noise=noise, out=out,
                           want_eps=True, want_x0=True)
    return [sha(t) for t in res]


def solver(_lib, dtype, pred, rescale, ids, E, seed, weights=(0.0, -6.5, 7.5), g_ref=1, c_h=(0.35, -0.15), c_noise=0.0,
           offset=0, inplace=False, h_out_is_h2=False, frames=FRAMES):
    F = frames if ids is None else len(ids)
    x = draw((frames, E), dtype, seed, offset)
    mo = draw((len(weights) * F, E), dtype, seed + 1)
    noise = draw((F, E), dtype, seed + 2) if c_noise else None
    h1, h2 = draw((frames, E), torch.float32, seed + 3), draw((frames, E), torch.float32, seed + 4)
    h_out = h2 if h_out_is_h2 else torch.zeros_like(h1)
    out = x if inplace else torch.zeros_like(x)
    res = _lib.solver_step(x, mo, weights, COEF["sqrt_alpha"], COEF["sqrt_beta"], 0.7, 0.9, c_h[0], c_h[1], c_noise,
                           h1=h1 if c_h[0] else None, h2=h2 if c_h[1] or h_out_is_h2 else None, h_out=h_out, g_ref=g_ref,
                           frame_ids=ids, pred_type=pred, rescale=rescale, noise=noise, out=out, want_eps=True, want_x0=True)
    return [sha(t) for t in res] + [sha(h_out)]


def sag(_lib, dtype, pred, shape, seed, r=2):
    F, C, H, W = shape
    x, mo = draw(shape, dtype, seed), draw(shape, dtype, seed + 1)
    h_m, w_m = max(H // 4, 1), max(W // 4, 1)
    mass = draw((F, h_m * w_m), torch.float32, seed + 2).abs()
    out, mask = _lib.sag_degrade(x, mo, mass, h_m, w_m, COEF["sqrt_alpha"], COEF["sqrt_beta"], _lib.gaussian_taps(r, 1.5),
                                 threshold=0.6, pred_type=pred, want_mask=True)
    return [sha(out), sha(mask)]


def semantic(_lib, dtype, shape, seed):
    F, C, H, W = shape
    mo = draw((3 * F, C, H, W), dtype, seed)
    momentum = draw((F, C, H, W), torch.float32, seed + 1)
    out, masks = _lib.semantic_guidance(mo, 3, 0, 1, 7.5, [2], [5.0], [0.9], [1.0], [0.4], [_lib.SEGA_CHANNEL],
                                        momentum=momentum, mom_scale=0.3, mom_beta=0.6, mom_apply=True, want_masks=True)
    return [sha(out), sha(masks), sha(momentum)]


def cases(_lib):
    seed = 1000
    for who, fn in (("guided", guided), ("solver", solver)):
        for dname, dtype in DTYPES.items():
            for pname, pred in PREDS.items():
                for rescale in (0.0, 0.7):
                    for ids in ([4, 0, 2], list(range(2, 5))):
                        for E in (140, 256, 1024 * 8 + 8 + 3):
                            seed += 10
                            yield f"{who}/{dname} {pname} rescale={rescale} ids={ids} E={E}", \
                                (lambda fn=fn, a=(dtype, pred, rescale, ids, E, seed): fn(_lib, *a))
        for dname, dtype in DTYPES.items():
            for rescale in (0.0, 0.7):
                seed += 10
                tail = f"{dname} rescale={rescale}"
                a = (dtype, PREDS["v"], rescale, [4, 0, 2], 256, seed)
                yield f"{who}/offset {tail}", (lambda fn=fn, a=a: fn(_lib, *a, offset=1))
                yield f"{who}/inplace {tail}", (lambda fn=fn, a=a: fn(_lib, *a, inplace=True))
                if who == "guided":
                    yield f"guided/groups=1 {tail}", (lambda a=a: guided(_lib, *a, groups=1))
                    yield f"guided/groups=3 {tail}", (lambda a=a: guided(_lib, *a, groups=3))
                    yield f"guided/sigma=0 {tail}", (lambda a=a: guided(_lib, *a, sigma=0.0))
                else:
                    yield f"solver/h_out=h2 {tail}", (lambda a=a: solver(_lib, *a, h_out_is_h2=True))
                    yield f"solver/no history {tail}", (lambda a=a: solver(_lib, *a, c_h=(0.0, 0.0)))
                    yield f"solver/noise {tail}", (lambda a=a: solver(_lib, *a, c_noise=0.25))
        big = (torch.float32, PREDS["v"], 0.0, None, 4 * 256 * 256, 77)
        yield f"{who}/grid cap fp32 17 x 262144", (lambda fn=fn: fn(_lib, *big, frames=17))
    for dname, dtype in DTYPES.items():
        for pname, pred in PREDS.items():
            seed += 10
            yield f"sag/{dname} {pname} (2, 4, 8, 8) r=2", (lambda a=(dtype, pred, (2, 4, 8, 8), seed): sag(_lib, *a))
    for dname, dtype in DTYPES.items():
        seed += 10
        yield f"lds/sag_degrade {dname} 96 x 96", (lambda a=(dtype, PREDS["epsilon"], (1, 1, 96, 96), seed): sag(_lib, *a))
        yield f"lds/semantic_guidance {dname} 120 x 120", (lambda a=(dtype, (1, 1, 120, 120), seed): semantic(_lib, *a))
        yield f"lds/freeu {dname} 2 x 8192", \
            (lambda a=((1, 3, 2, 8192), dtype, seed): [sha(_lib.freeu(draw(*a), 2, 1.2, 0.9))])
        if dtype != torch.float32:               # (fp32 tokens go through linear_f32)
            yield f"lds/linear_rows {dname} K=320 N=160 n=40", \
                (lambda d=dtype, s=seed: [sha(_lib.linear_rows(draw((1, 40, 320), d, s), None, None, None, 40,
                                                               draw((160, 320), d, s + 1), draw((160,), d, s + 2)))])
    yield "lds/groupnorm_silu fp32 one group of 16400", \
        (lambda: [sha(_lib.groupnorm_silu(draw((1, 1, 20, 820), torch.float32, 5), 1, draw((1,), torch.float32, 6),
                                          draw((1,), torch.float32, 7), 1e-5))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vidtome_amd import _lib
    lines = []
    for name, run in cases(_lib):
        lines.append(f"{name}   " + " ".join(run()))
        print(lines[-1], flush=True)
    torch.cuda.synchronize()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
