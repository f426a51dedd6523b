"""A restatement of the frame-keyed noise contract (include/vidtome_hip.h, "Frame-keyed noise") for the tests: Philox4x32-10 in
vectorised numpy uint64 arithmetic (every product is formed in 64 bits and cut), the counter layout, and the Box-Muller
transform in float64.  It shares no code with csrc/philox.h."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)

# counter | key -> output.  The first and the third are the vectors published with Random123 (kat_vectors, philox4x32 10).
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)

# the seeds and sizes the GPU tests use, so the CPU test can show that the restatement alone meets their thresholds
DIST_SEED, DIST_F, DIST_E, DIST_STEP = 0x5EED0123456789AB, 16, 65536, 7
MAX_ABS = 5.7683


def philox(counters, k0, k1):
    """counters (n, 4) of uint32 values -> (n, 4) uint32 outputs under the key (k0, k1)."""
    c = np.asarray(counters, dtype=np.uint64) & MASK
    c0, c1, c2, c3 = (c[:, j].copy() for j in range(4))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # < 2^64: no wrap
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def key_of(seed):
    return seed & 0xFFFFFFFF, seed >> 32


def counters_of(E, frames, step, tag):
    """The counters of every quad of the given frames at one step: (F * ceil(E / 4), 4), frame-major."""
    quads = (E + 3) // 4
    frames = np.asarray(frames, dtype=np.uint64)
    c = np.empty((len(frames), quads, 4), dtype=np.uint64)
    c[:, :, 0] = np.arange(quads, dtype=np.uint64)[None, :]
    c[:, :, 1] = frames[:, None]
    c[:, :, 2] = step
    c[:, :, 3] = tag
    return c.reshape(-1, 4)


def normals_of(bits):
    """(n, 4) uint32 outputs -> (n, 4) float64 normals: u1 and u2 are the contract's exact fp32 values, everything after
    them is float64."""
    o = bits.astype(np.uint64)
    z = np.empty(o.shape, dtype=np.float64)
    for a, b in ((0, 1), (2, 3)):
        u1 = ((o[:, a] >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
        u2 = (o[:, b] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        z[:, a], z[:, b] = r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)
        # cospi / sinpi are exact at the quarter turns; cos(pi / 2) in float64 is 6e-17, below every floor used here
    return z


def normal(seed, tag, step, frames, E, steps=1):
    """(steps, F, E) float64: what FrameNoise(seed, tag).normal(shape of E elements, step, frames, steps=steps) must hold."""
    frames = list(frames)
    quads = (E + 3) // 4
    out = np.empty((steps, len(frames), E), dtype=np.float64)
    for s in range(steps):
        z = normals_of(philox(counters_of(E, frames, (step + s) & 0xFFFFFFFF, tag), *key_of(seed)))
        out[s] = z.reshape(len(frames), quads * 4)[:, :E]          # element e: normal e & 3 of quad e >> 2
    return out


def moments(z, by_frame, by_step=None):
    """What the distribution tests look at: mean, variance, max |z| of z, the largest sample correlation of consecutive rows
    of by_frame (F, E), and of by_step (S, E) when given."""
    def corr(rows):
        rows = np.asarray(rows, dtype=np.float64)
        return max(abs(np.corrcoef(rows[k], rows[k + 1])[0, 1]) for k in range(len(rows) - 1))
    z = np.asarray(z, dtype=np.float64)
    return dict(mean=float(z.mean()), var=float(z.var()), max_abs=float(np.abs(z).max()), frame_corr=float(corr(by_frame)),
                step_corr=float(corr(by_step)) if by_step is not None else 0.0)


def thresholds(n, E):
    """5-sigma CLT conditions for n values, correlations over E pairs."""
    return dict(mean=5.0 / np.sqrt(n), var=5.0 * np.sqrt(2.0 / n), max_abs=MAX_ABS, frame_corr=5.0 / np.sqrt(E),
                step_corr=5.0 / np.sqrt(E))


def meets(m, t):
    return (abs(m["mean"]) <= t["mean"] and abs(m["var"] - 1.0) <= t["var"] and m["max_abs"] <= t["max_abs"]
            and m["frame_corr"] <= t["frame_corr"] and m["step_corr"] <= t["step_corr"])
