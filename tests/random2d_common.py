"""Reference-free pieces shared by tests/golden/make_golden_random2d.py and the random2d tests: the case list, a plain-numpy
restatement of the 2-D partition (vidtome/merge.py:493-528) in its stable order, and the seeded inputs."""
import numpy as np

from inputs import planted_inputs

# (h, w, sx, sy, r, B, C, no_rand)
CASES = [
    (8, 8, 2, 2, 24, 2, 32, False),
    (8, 8, 2, 2, 24, 1, 32, True),
    (9, 11, 2, 2, 30, 2, 64, False),          # not divisible in either axis
    (16, 16, 4, 2, 10 ** 6, 1, 320, False),   # r clamps to Ns
    (6, 10, 1, 1, 5, 1, 32, False),           # every token is dst, Ns = 0
    (64, 64, 2, 2, 1536, 2, 320, False),      # the largest: stored as hashes + sampled rows
]
IDX = ("a_idx", "b_idx", "unm_idx", "src_idx", "dst_idx")
FULL_BYTES = 64 << 10        # arrays up to this size are stored whole, larger ones as sha256 + SAMPLE_ROWS rows
SAMPLE_ROWS = 16


def partition_2d(h, w, sx, sy, draws):
    """-> (a_idx, b_idx) int64, both ascending.  ``draws``: hsy * wsx integers in [0, sx * sy), or None for no_rand.  Cell
    (i, j) with draw d marks token (i * sy + d // sx, j * sx + d % sx) as dst; every other token is src."""
    hsy, wsx = h // sy, w // sx
    d = np.zeros((hsy, wsx), np.int64) if draws is None else np.asarray(draws, np.int64).reshape(hsy, wsx)
    i, j = np.meshgrid(np.arange(hsy), np.arange(wsx), indexing="ij")
    is_dst = np.zeros((h, w), bool)
    is_dst[i * sy + d // sx, j * sx + d % sx] = True
    flat = is_dst.reshape(-1)
    return np.flatnonzero(~flat), np.flatnonzero(flat)


def sample_rows(n):
    """The rows of an (.., n, C) array a hashed fixture also stores in full."""
    return np.unique(np.linspace(0, n - 1, min(n, SAMPLE_ROWS)).astype(np.int64))


def sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=np.float32)).tobytes()).hexdigest()


def build_inputs(h, w, B, C, a_idx, b_idx, seed):
    """x (B, h * w, C) fp32 whose src / dst rows under the partition are a planted matching (inputs.planted_inputs: strictly
    spaced best cosines, so indices do not hang on rounding).  Without src tokens: plain seeded Gaussians."""
    if len(a_idx) == 0:
        return np.random.default_rng(seed).standard_normal((B, h * w, C)).astype(np.float32)
    a, b = planted_inputs(len(a_idx), len(b_idx), C, seed, B)
    x = np.empty((B, h * w, C), np.float32)
    x[:, a_idx] = a
    x[:, b_idx] = b
    return x


def stable_view(c):
    """A fixture case seen in the stable order.  The reference takes a_idx / b_idx from an argsort of a buffer of equal
    keys (-1 at dst, 0 at src tokens), which torch's CPU sort returns in no particular order; its unm / src / dst_idx
    count positions of THOSE lists.  -> the ascending lists, the permutations pa / pb (position in the reference's list ->
    position in the ascending one: a[pa] = a_ref, b[pb] = b_ref) and the three index arrays renumbered through them."""
    a_ref, b_ref = c["a_idx"].astype(np.int64), c["b_idx"].astype(np.int64)
    a, b = partition_2d(int(c["h"]), int(c["w"]), int(c["sx"]), int(c["sy"]), None if c["no_rand"] else c["draws"])
    assert len(a) == len(a_ref) and len(b) == len(b_ref)
    pa, pb = np.searchsorted(a, a_ref), np.searchsorted(b, b_ref)
    # the permutation only reorders within src and within dst: each list holds the same tokens, each exactly once
    assert np.array_equal(a[pa], a_ref) and np.array_equal(np.sort(pa), np.arange(len(a)))
    assert np.array_equal(b[pb], b_ref) and np.array_equal(np.sort(pb), np.arange(len(b)))
    return {"a_idx": a, "b_idx": b, "pa": pa, "pb": pb, "unm_idx": pa[c["unm_idx"].astype(np.int64)],
            "src_idx": pa[c["src_idx"].astype(np.int64)], "dst_idx": pb[c["dst_idx"].astype(np.int64)]}


def in_reference_order(merged, pb):
    """`cat([unm, dst])` computed on the ascending lists -> the same rows with the dst part in the reference's b_idx order
    (the unm part is in similarity-rank order either way)."""
    U = merged.shape[1] - len(pb)
    return np.concatenate([merged[:, :U], merged[:, U + pb]], axis=1)


def case_inputs(c):
    """x (B, h * w, C) fp32 of a fixture case, rebuilt from its seed and checked against what the fixture stores of it."""
    a, b = partition_2d(int(c["h"]), int(c["w"]), int(c["sx"]), int(c["sy"]), None if c["no_rand"] else c["draws"])
    x = build_inputs(int(c["h"]), int(c["w"]), int(c["B"]), int(c["C"]), a, b, int(c["seed"]))
    assert_stored(c, "x", x)
    return x


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_stored(c, key, got):
    """``got`` (fp32) equals the fixture's array ``key`` bit for bit: the whole array, or its sha256 and sampled rows."""
    got = np.asarray(got)
    assert got.dtype == np.float32, got.dtype
    if key in c:
        assert got.shape == c[key].shape, (key, got.shape, c[key].shape)
        assert np.array_equal(_bits(got), _bits(c[key])), key
        return
    rows = sample_rows(got.shape[1])
    assert np.array_equal(_bits(got[:, rows]), _bits(c[key + "_rows"])), key
    assert sha(got) == str(c[key + "_sha256"]), key
