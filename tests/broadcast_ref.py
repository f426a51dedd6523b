"""Restatements the attention-broadcast tests compare against (tests/test_broadcast_host.py, tests/test_gpu_broadcast.py):
the schedule rule written out once more, independently of vidtome_amd/broadcast.py, and the two one-line torch forms of the
kernels' arithmetic."""
import torch

MANTISSA = {torch.float16: 10, torch.bfloat16: 7, torch.float32: 23}
MIN_EXP = {torch.float16: -14, torch.bfloat16: -126, torch.float32: -126}


def delta(h_after, h_before):
    """What vtm_residual_record stores: the fp32 difference, rounded once."""
    return (h_after.float() - h_before.float()).to(h_after.dtype)


def replay(h, *deltas):
    """What vtm_residual_replay writes: one fp32 sum and one rounding per delta, in order."""
    for d in deltas:
        h = (h.float() + d.float()).to(h.dtype)
    return h


def record_into(cache, h_in, h_out, ids):
    """``cache`` (G, num_frames, ...) after a record of the group-major batch (G Fg, ...): a copy with the rows ``ids`` (None:
    all, in order) replaced."""
    G, nf = cache.shape[:2]
    ids = list(range(nf)) if ids is None else list(ids)
    out = cache.clone()
    d = delta(h_out, h_in).view(G, len(ids), *cache.shape[2:])
    out[:, ids] = d
    return out


def replay_from(h, ids, *caches):
    """The replay of the group-major batch ``h`` (G Fg, ...) from whole-video caches (G, num_frames, ...)."""
    G, nf = caches[0].shape[:2]
    ids = list(range(nf)) if ids is None else list(ids)
    return replay(h, *[c[:, ids].reshape(h.shape) for c in caches])


def ulp(x, dtype):
    """The spacing of ``dtype`` at magnitude x (float64 tensor), no smaller than the subnormal spacing."""
    _, e = torch.frexp(x.abs().double().clamp_min(2.0 ** (MIN_EXP[dtype] - 1)))     # |x| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), (e - 1).clamp_min(MIN_EXP[dtype]) - MANTISSA[dtype])


def reuse(i, timesteps, every, window):
    """The issue's rule, term by term."""
    if every is None or i <= 0:
        return False
    lo, hi = window
    inside = timesteps[i] > lo and timesteps[i] < hi
    return inside and (i % every) != 0


def mode(i, timesteps, every, window):
    if reuse(i, timesteps, every, window):
        return "reuse"
    if i + 1 < len(timesteps) and reuse(i + 1, timesteps, every, window):
        return "record"
    return "compute"
