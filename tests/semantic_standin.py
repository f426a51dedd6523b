"""Restatements of vtm_semantic_guidance (include/vidtome_hip.h) for tests/test_semantic_host.py and
tests/test_gpu_semantic.py.

``masks`` is the mask path in numpy fp32, operation for operation as the contract writes it: one fp32 subtraction, one fp32
product, |.|, the channel sum ascending from 0 in fp32, np.sort for the ranks (NaNs last: the highest ranks), and the double
formula for thr.  numpy rounds every fp32 operation to nearest and contracts nothing, so the result is what the kernel must
produce bit for bit.

``reference`` evaluates the values in float64 from the same masks and returns each with the magnitude sum A of its terms,
every term expanded down to the inputs (the ``hold`` scheme of test_gpu_guided_step.py / test_gpu_solver_step.py).

``diffusers_masks`` restates the mask of Diffusers' SemanticStableDiffusionPipeline in torch: torch.quantile on
|g|.flatten(2) in fp32, then ``>=``."""
import math

import numpy as np
import torch

CHANNEL, SUM, REGION, CHANNEL_REGION, SUM_REGION = range(5)
MODE_NAMES = {CHANNEL: "channel", SUM: "sum", REGION: "region", CHANNEL_REGION: "channel+region", SUM_REGION: "sum+region"}


def rank(q, P):
    """(rank_lo, rank_frac): pos = q (P - 1) in double."""
    pos = float(q) * (P - 1)
    lo = min(int(math.floor(pos)), P - 1)
    return lo, pos - lo


def exact_rank_q(lo, P):
    """A q strictly inside (0, 1) whose rank_frac is exactly 0 with rank_lo == lo, or None when lo / (P - 1) does not hit."""
    q = lo / (P - 1)
    return q if rank(q, P) == (lo, 0.0) and 0.0 < q < 1.0 else None


def threshold(pop, lo, frac):
    """thr of one population (1-D fp32): exact order statistics, the double formula, one rounding to fp32."""
    srt = np.sort(np.asarray(pop, dtype=np.float32))
    a_lo, a_hi = np.float64(srt[lo]), np.float64(srt[min(lo + 1, srt.size - 1)])
    with np.errstate(invalid="ignore", over="ignore"):
        return np.float32(a_lo + np.float64(frac) * (a_hi - a_lo))


def edit_terms(mo, g_uncond, group, scale):
    """g_e in fp32: mo (groups, F, C, H, W) fp32 (the inputs converted exactly)."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = (mo[group] - mo[g_uncond]).astype(np.float32)
        return (np.float32(scale) * d).astype(np.float32)


def masks(mo, g_uncond, concepts, regions=None):
    """{e: bool (F, C, H, W)} for the concepts with a non-zero weight.  mo: (groups, F, C, H, W) fp32; concepts: a list of
    dicts with group, scale, q, w_apply, w_acc, mode; regions: (E, F, H, W) of 0 / 1 or None.  Also returns {e: thr array}
    ((F, C) for the channel modes, (F,) for the sum modes)."""
    mo = np.asarray(mo, dtype=np.float32)
    _, F, C, H, W = mo.shape
    P = H * W
    out, thrs = {}, {}
    for e, c in enumerate(concepts):
        if np.float32(c["w_apply"]) == 0 and np.float32(c["w_acc"]) == 0:
            continue
        mode = c["mode"]
        on = np.ones((F, C, H, W), dtype=bool)
        if mode != REGION:
            a = np.abs(edit_terms(mo, g_uncond, c["group"], c["scale"]))
            lo, frac = rank(c["q"], P)
            if mode in (SUM, SUM_REGION):
                acc = np.zeros((F, H, W), dtype=np.float32)
                with np.errstate(invalid="ignore", over="ignore"):
                    for ch in range(C):
                        acc = (acc + a[:, ch]).astype(np.float32)
                thr = np.array([threshold(acc[f].ravel(), lo, frac) for f in range(F)], dtype=np.float32)
                with np.errstate(invalid="ignore"):
                    on = np.broadcast_to((acc >= thr[:, None, None])[:, None], (F, C, H, W)).copy()
            else:
                thr = np.array([[threshold(a[f, ch].ravel(), lo, frac) for ch in range(C)] for f in range(F)], dtype=np.float32)
                with np.errstate(invalid="ignore"):
                    on = a >= thr[:, :, None, None]
            thrs[e] = thr
        if mode >= REGION:
            on = on & (np.asarray(regions)[e] != 0)[:, None]
        out[e] = on
    return out, thrs


def reference(mo, M, g_uncond, g_cond, s, concepts, nu=None, mom_scale=0.0, mom_beta=0.0, mom_apply=False):
    """The values in float64.  mo: (groups, F, C, H, W) float64; M: ``masks``' dict; nu: the chunk's momentum rows
    (F, C, H, W) float64 or None.  Returns (m, A_m, nu', A_nu): A_* the sums of the absolute values of the terms, each term
    expanded to the inputs."""
    u = mo[g_uncond]
    m, A = u.copy(), np.abs(u)
    if g_cond >= 0:
        m, A = m + s * (mo[g_cond] - u), A + abs(s) * (np.abs(mo[g_cond]) + np.abs(u))
    acc, A_acc = np.zeros_like(u), np.zeros_like(u)
    for e, c in enumerate(concepts):
        if e not in M:
            continue
        g = np.where(M[e], c["scale"] * (mo[c["group"]] - u), 0.0)
        Ag = np.where(M[e], abs(c["scale"]) * (np.abs(mo[c["group"]]) + np.abs(u)), 0.0)
        if np.float32(c["w_apply"]) != 0:
            m, A = m + c["w_apply"] * g, A + abs(c["w_apply"]) * Ag
        if np.float32(c["w_acc"]) != 0:
            acc, A_acc = acc + c["w_acc"] * g, A_acc + abs(c["w_acc"]) * Ag
    if nu is None:
        return m, A, None, None
    if mom_apply:
        m, A = m + mom_scale * nu, A + np.abs(mom_scale * nu)
    return m, A, mom_beta * nu + (1.0 - mom_beta) * acc, np.abs(mom_beta * nu) + abs(1.0 - mom_beta) * A_acc


def diffusers_masks(g, q):
    """Diffusers' SEGA mask of the fp32 edit terms g (F, C, H, W), a torch tensor: ``|g| >= quantile(|g|.flatten(2), q)``
    per (frame, channel) plane.  Returns (mask bool (F, C, H, W), thr (F, C))."""
    a = torch.abs(g).to(torch.float32)
    thr = torch.quantile(a.flatten(start_dim=2), float(q), dim=2, keepdim=False)
    return a >= thr[:, :, None, None], thr
