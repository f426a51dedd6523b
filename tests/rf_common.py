"""Reference-free pieces shared by tests/golden/make_golden_rf.py and the receptive-field tests (test_rf_host.py,
test_gpu_rf.py): the case lists, the seeded inputs and coordinates, and a BITWISE restatement of the masked matching of
bipartite_soft_matching_random2d_hier / _2f (vidtome/merge.py:162-340, 582-767) on the oracle's score bits.

The restatement gets the score matrix in the oracle's bits -- one ``oracle.match(a, b[:, j:j+1])`` call per dst column over
``oracle.normalize_gather`` rows: the row maximum over a single column IS the score, in the canonical k-ascending fmaf
chain -- and then states the mask, the first-index maximum and the canonical stable sort in numpy."""
import hashlib

import numpy as np

TARGET_STRIDE = 4
# (F, h, w, B, C, ratio, rec_field, corr, adhere_src, unm_pre, with_coord)
HIER_CASES = [
    (4, 8, 8, 2, 32, .25, .5, 0., False, 0, True),      # about half the rows: a masked 0 is the maximum, first masked column
    (4, 8, 8, 2, 32, .25, .5, 0., True, 0, True),
    (4, 8, 8, 2, 32, .5, 2, 0., False, 0, True),
    (4, 16, 16, 2, 64, .5, 2, 1., False, 0, True),
    (5, 9, 11, 2, 64, .5, 1.5, .3, False, 0, True),
    (4, 8, 8, 2, 32, .5, 2, 0., False, 24, True),       # unm_pre > 0: 24 tokens in front, appended to dst
    (4, 8, 8, 2, 32, .5, 2, 0., False, 0, False),       # coord=None: the unmasked level
]
# the same geometries through bipartite_soft_matching_2f, src = the first F - 1 frames; every case stores both unmerge chunks
F2_CASES = [c[:9] + (0, True) for c in HIER_CASES[:5]] + [(4, 8, 8, 2, 32, .5, 2, 0., False, 0, False)]
CASES = [("hier",) + c for c in HIER_CASES] + [("2f",) + c for c in F2_CASES]
FIELDS = ("fn", "F", "h", "w", "B", "C", "ratio", "rec_field", "corr", "adhere_src", "unm_pre", "with_coord")
IDX = ("a_idx", "b_idx", "unm_idx", "src_idx", "dst_idx")
FULL_BYTES = 12 << 10        # arrays up to this size are stored whole, larger ones as sha256 + SAMPLE_ROWS rows
SAMPLE_ROWS = 6
MARGIN = 1e-6                # as tests/golden/make_golden.py: >= ~16 ulp of a cosine near 1


def case_dict(n):
    return dict(zip(FIELDS, CASES[n]))


def tokens(c):
    return c["unm_pre"] + c["F"] * c["h"] * c["w"]


def src_len_2f(c):
    return (c["F"] - 1) * c["h"] * c["w"]


def build_inputs(c, seed):
    """x (B, N, C) fp32 = corr * base(position) + N(0, 1): frames of one clip share a per-position component."""
    rng = np.random.default_rng(seed)
    hw, N = c["h"] * c["w"], tokens(c)
    base = rng.standard_normal((hw, c["C"]))
    pos = grid_position(c)
    x = c["corr"] * base[pos][None] + rng.standard_normal((c["B"], N, c["C"]))
    return x.astype(np.float32)


def grid_position(c):
    """Position in the h x w frame of every token: the unm_pre tokens in front take positions 0, 1, ..."""
    hw = c["h"] * c["w"]
    return np.concatenate([np.arange(c["unm_pre"]) % hw, np.tile(np.arange(hw), c["F"])])


def build_coord(c):
    """(B, N, 2) fp32: the (y, x) grid, repeated per frame."""
    pos = grid_position(c)
    yx = np.stack([pos // c["w"], pos % c["w"]], -1).astype(np.float32)
    return np.broadcast_to(yx[None], (c["B"],) + yx.shape).copy()


def partition_hier(c, randf):
    """a_idx, b_idx of merge.py:197-206."""
    N, unm_pre = tokens(c), c["unm_pre"]
    nf = (N - unm_pre) // c["F"]
    idx = np.arange(N - unm_pre)
    sel = (idx // nf) % min(TARGET_STRIDE, c["F"]) == randf
    return idx[~sel] + unm_pre, np.concatenate([idx[sel] + unm_pre, np.arange(unm_pre)])


def partition_2f(c):
    N, s = tokens(c), src_len_2f(c)
    return np.arange(s), np.arange(s, N)


# ---- storage: whole, or sha256 + sampled rows ------------------------------------------------------------------------------
def sample_rows(n):
    return np.unique(np.linspace(0, n - 1, min(n, SAMPLE_ROWS)).astype(np.int64))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=np.float32)).tobytes()).hexdigest()


def store(out, key, arr):
    arr = np.ascontiguousarray(arr, dtype=np.float32)
    if arr.nbytes <= FULL_BYTES:
        out[key] = arr
        return
    out[key + "_sha256"] = sha(arr)
    out[key + "_rows"] = arr[:, sample_rows(arr.shape[1])]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_stored(c, key, got):
    """``got`` (fp32) equals the fixture's array ``key`` bit for bit: the whole array, or its sha256 and sampled rows."""
    got = np.asarray(got)
    assert got.dtype == np.float32, (key, got.dtype)
    if key in c:
        assert got.shape == c[key].shape, (key, got.shape, c[key].shape)
        assert np.array_equal(_bits(got), _bits(c[key])), key
        return
    assert np.array_equal(_bits(got[:, sample_rows(got.shape[1])]), _bits(c[key + "_rows"])), key
    assert sha(got) == str(c[key + "_sha256"]), key


def canonical(merged, unm_idx):
    """``cat([unm, dst])`` with the unm part in ascending src-index order.  The reference's argsort is not stable, so INSIDE a
    group of exactly equal node_max (the rows whose maximum is a masked 0) its order is no property of the inputs; the group
    never straddles position r in a fixture case, so it only permutes unm rows."""
    U = unm_idx.shape[1]
    order = np.argsort(unm_idx, axis=1, kind="stable")
    out = merged.copy()
    out[:, :U] = np.take_along_axis(merged[:, :U], order[:, :, None], axis=1)
    return out


# ---- the bitwise restatement -----------------------------------------------------------------------------------------------
def score_bits(oracle, a, b):
    """(B, Ns, Nd) fp32 scores in the oracle's bits (a, b: oracle.normalize_gather rows)."""
    S = np.empty((a.shape[0], a.shape[1], b.shape[1]), np.float32)
    for j in range(b.shape[1]):
        S[:, :, j] = oracle.match(a, b[:, j:j + 1])[0]
    return S


def mask_of(src_coord, dst_coord, rec_field):
    """merge.py:235: ``torch.norm(src[:, :, None] - dst[:, None], dim=-1) > rec_field`` in fp32 (the Python number is compared
    in the tensor's dtype); components summed in ascending order."""
    s = np.zeros(src_coord.shape[:2] + dst_coord.shape[1:2], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(src_coord.shape[2]):
            d = src_coord[:, :, None, k].astype(np.float32) - dst_coord[:, None, :, k].astype(np.float32)
            s = s + d * d
        return np.sqrt(s) > np.float32(rec_field)


def orderable(v):
    """The monotone fp32 -> uint32 map of the packed keys (NaN largest, -0 == +0)."""
    u = (np.asarray(v, np.float32) + np.float32(0)).view(np.uint32)
    o = np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)
    return np.where(np.isnan(v), np.uint32(0xffffffff), o)


def row_max(S, align):
    """torch's max over the last axis (largest value, first index, first NaN wins); aligned: the samples' score matrices side
    by side on the dst axis first (merge.py:251-252).  -> node_max, node_idx of shape (B, Ns) or (Ns,)."""
    if align:
        S = np.concatenate(list(S), axis=-1)
    key = orderable(S)
    idx = key.argmax(-1)                       # first of the largest keys
    return np.take_along_axis(S, idx[..., None], -1)[..., 0], idx.astype(np.int64)


def sort_desc(node_max):
    """The canonical argsort(descending): stable, NaN first."""
    return np.argsort(~orderable(node_max), axis=-1, kind="stable")


def restate(oracle, x, a_idx, b_idx, ratio, align, coord=None, rec_field=None, S=None):
    """The level of merge.py:228-282 / 641-699 -> dict(node_max, node_idx, unm_idx, src_idx, dst_idx), indices (B, .) int64."""
    B = x.shape[0]
    if S is None:
        S = score_bits(oracle, oracle.normalize_gather(x, a_idx[None]), oracle.normalize_gather(x, b_idx[None]))
    if coord is not None:
        S = np.where(mask_of(coord[:, a_idx], coord[:, b_idx], rec_field), np.float32(0), S)
    Ns, Nd = len(a_idx), len(b_idx)
    r = min(Ns, int(Ns * ratio))
    node_max, node_idx = row_max(S, align)
    edge = sort_desc(node_max)
    if align:
        unm, src = edge[r:], edge[:r]
        dst = node_idx[src] % Nd
        unm, src, dst = (np.broadcast_to(t, (B,) + t.shape).copy() for t in (unm, src, dst))
    else:
        unm, src = edge[:, r:], edge[:, :r]
        dst = np.take_along_axis(node_idx, src, axis=1)
    return {"node_max": node_max, "node_idx": node_idx, "unm_idx": unm, "src_idx": src, "dst_idx": dst}


def merge_restated(oracle, x, a_idx, b_idx, lv, mode, first_rows=False, b_select=None):
    """merge(x, mode, b_select) of merge.py:289-314 / 706-732 on restated indices.  ``first_rows``: 2f folds src rows
    0 .. r - 1 (merge.py:718 is commented out).  x holds one row per selected sample."""
    pick = (lambda t: t) if b_select is None else (lambda t: t[np.atleast_1d(b_select)])
    unm_idx, src_idx, dst_idx = pick(lv["unm_idx"]), pick(lv["src_idx"]), pick(lv["dst_idx"])
    src, dst = x[:, a_idx], x[:, b_idx]
    unm = np.take_along_axis(src, unm_idx[:, :, None], axis=1)
    if mode != "replace":
        r = src_idx.shape[1]
        s = src[:, :r] if first_rows else np.take_along_axis(src, src_idx[:, :, None], axis=1)
        acc, cnt = oracle.scatter_reduce(dst, dst_idx, s.astype(np.float32), mode)
        dst = acc / cnt[:, :, None] if mode == "mean" else acc
    return np.concatenate([unm, dst.astype(np.float32)], axis=1)


def unmerge_restated(y, a_idx, b_idx, lv, N, b_select=None, unm_modi=None):
    """unmerge(y, b_select, unm_modi) of merge.py:316-337 / 734-764 (the full N rows)."""
    pick = (lambda t: t) if b_select is None else (lambda t: t[np.atleast_1d(b_select)])
    unm_idx, src_idx, dst_idx = pick(lv["unm_idx"]), pick(lv["src_idx"]), pick(lv["dst_idx"])
    U = unm_idx.shape[1]
    unm, dst = y[:, :U], y[:, U:]
    if unm_modi == "zero":
        unm = np.zeros_like(unm)
    out = np.zeros((y.shape[0], N, y.shape[2]), y.dtype)
    bi = np.arange(y.shape[0])[:, None]
    out[:, b_idx] = dst
    out[bi, a_idx[unm_idx]] = unm
    out[bi, a_idx[src_idx]] = np.take_along_axis(dst, dst_idx[:, :, None], axis=1)
    return out
