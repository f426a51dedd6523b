"""Frame-keyed noise on the GPU (vtm_philox_bits, vtm_frame_noise, the keyed steps, FrameNoise): the bits against the numpy
restatement (tests/frame_noise_ref.py) exactly, the fp32 normals against its float64 transform of the same bits, and the
properties the feature exists for -- a frame's noise is the same under any chunking, and a keyed step equals the tensor-noise
step on vtm_frame_noise's output BIT FOR BIT.

The value bound, per element:  |z - ref| <= 2^-20 |ref| + 2^-40, i.e. 8 ulp relative.  It is derived, not measured: HIP documents
logf at 1 ulp, sinpif / cospif at 1 - 2 ulp, sqrtf correctly rounded; z = sqrtf(-2 logf(u1)) * cospif(2 u2) with u1, u2 and the
two products by 2 exact.  logf's relative error e_l becomes e_l / 2 under the square root (<= 1 ulp), plus the root's own
rounding (0.5), the trigonometric factor (<= 2) and the final product (0.5): <= 4 ulp, so 8 leaves a factor of two.  The floor
covers cospif's exact zeros, where float64 cos(pi / 2) r is 4e-16.  The worst observed error / bound is printed (run with -s)."""
import numpy as np
import pytest
import torch

import frame_noise_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F32, F16, BF16]
IDS = {F32: "fp32", F16: "fp16", BF16: "bf16"}
SEED = R.DIST_SEED
N_FRAMES = 12


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def _same(a, b):
    """Bit for bit (a NaN equals itself, -0 differs from +0)."""
    assert a.shape == b.shape and a.dtype == b.dtype
    view = torch.int32 if a.dtype == F32 else torch.int16
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def _alphas():
    """Stable Diffusion's schedule: scaled-linear betas 0.00085 .. 0.012 over 1000 steps."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def _timesteps(n):
    return ((np.arange(n) * (1000 // n))[::-1] + 1).tolist()


def _sde(order, n=20, **kw):
    from vidtome_amd import GuidedDPMSolver
    return GuidedDPMSolver(_alphas(), _timesteps(n), algorithm_type="sde-dpmsolver++", solver_order=order, **kw)


def _ddim(n=20, **kw):
    from vidtome_amd import GuidedDDIM
    return GuidedDDIM(_alphas(), _timesteps(n), eta=1.0, **kw)


def _randn(shape, dtype, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)


# ---------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------
def test_philox_bits_equal_the_restatement(L):
    def device(counters, seed):
        c = torch.from_numpy(np.ascontiguousarray(counters, dtype=np.uint32).view(np.int32)).to(DEV)
        return L.philox_bits(c, seed).cpu().numpy().view(np.uint32)
    for counter, key, want in R.KNOWN_ANSWERS:
        assert tuple(int(v) for v in device([counter], key[0] | key[1] << 32)[0]) == want, (counter, key)
    rng = np.random.default_rng(11)
    c = rng.integers(0, 2 ** 32, size=(4096, 4), dtype=np.uint64)
    c[:64, 1], c[32:96, 2] = 2 ** 31 - 1, 2 ** 32 - 1                    # frame = 2^31 - 1, step = 2^32 - 1, and both
    seed = 0xFEDCBA9876543210
    assert np.array_equal(device(c, seed), R.philox(c, *R.key_of(seed)))


# ---------------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------------
VALUE_CASES = {
    # shape (E), frame_ids (host | "device"), steps, offset of out in its allocation (elements)
    "E105-unsorted-ids-S3": ((3, 5, 7), [7, 2, 9], "host", 3, 0),       # partial last quad, element stores
    "E1028-device-ids": ((4, 257), [11, 0, 5, 6], "device", 1, 0),       # quad stores, more than one block
    "E1028-misaligned": ((4, 257), [3, 4, 5], "host", 2, 1),             # an ascending run (frame0), element stores
    "E16384-F1": ((4, 64, 64), [2 ** 31 - 1], "host", 1, 0),             # one frame, the largest row there is
    "E16384-no-ids": ((4, 64, 64), None, "host", 1, 0),
    # element stores of enough values (32 770) that some fp32 normals lie on a 16-bit rounding tie (one in 2^13 for fp16)
    "E16385-element": ((5, 29, 113), [6, 1], "host", 1, 0),
}


def _draw(noise, shape, step, ids, where, steps, dtype, offset=0, n_frames=N_FRAMES):
    E = int(np.prod(shape))
    F = n_frames if ids is None else len(ids)
    out = None
    if offset:
        base = torch.zeros(steps * F * E + offset, dtype=dtype, device=DEV)
        out = base[offset:].view((steps, F) + tuple(shape))
    frame_ids = torch.tensor(ids, dtype=torch.int32, device=DEV) if (where == "device" and ids is not None) else ids
    return noise.normal(shape, step, frame_ids=frame_ids, n_frames=n_frames if ids is None else None, steps=steps,
                        dtype=dtype, out=out)


@pytest.mark.parametrize("case", list(VALUE_CASES))
def test_fp32_values_against_the_float64_restatement(case):
    from vidtome_amd import FrameNoise
    shape, ids, where, steps, offset = VALUE_CASES[case]
    E, step, tag = int(np.prod(shape)), 2 ** 32 - steps, 1               # the last steps there are
    z = _draw(FrameNoise(SEED), shape, step, ids, where, steps, F32, offset).cpu().numpy().astype(np.float64)
    ref = R.normal(SEED, tag, step, range(N_FRAMES) if ids is None else ids, E, steps=steps)
    z = z.reshape(ref.shape)
    bound = 2.0 ** -20 * np.abs(ref) + 2.0 ** -40
    worst = float((np.abs(z - ref) / bound).max())
    print(f"frame_noise fp32 {case}: worst error / bound = {worst:.3f}, max |z| = {np.abs(z).max():.4f}")
    assert np.all(np.abs(z - ref) <= bound), worst


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", ["E105-unsorted-ids-S3", "E1028-device-ids", "E1028-misaligned", "E16385-element",
                                  "E16384-no-ids"])
def test_16_bit_output_is_the_fp32_output_rounded_once(case, dtype):
    from vidtome_amd import FrameNoise
    shape, ids, where, steps, offset = VALUE_CASES[case]
    wide = _draw(FrameNoise(SEED), shape, 5, ids, where, steps, F32, offset)
    if case.startswith("E1638") and dtype == F16:                       # the case is there for the ties: it has some
        assert int((wide.view(torch.int32) & 0x1FFF == 0x1000).sum()) > 0
    assert _same(_draw(FrameNoise(SEED), shape, 5, ids, where, steps, dtype, offset), wide.to(dtype))


def test_rows_are_addressed_by_frame_step_tag_and_seed():
    from vidtome_amd import FrameNoise, noise
    shape, n = (3, 5, 7), FrameNoise(SEED)
    whole = n.normal(shape, 4, n_frames=N_FRAMES, steps=2)
    chunk = n.normal(shape, 4, frame_ids=[7, 2, 9], n_frames=N_FRAMES, steps=2)
    assert _same(chunk, whole[:, [7, 2, 9]])
    assert _same(n.normal(shape, 5, frame_ids=[7, 2, 9])[0], whole[1, [7, 2, 9]])            # step 5 is step 4's second
    assert _same(n.normal(shape, 4, frame_ids=[8, 9, 10])[0], whole[0, 8:11])                # an ascending run: a row offset
    base = whole[0, 7]
    for other in (whole[1, 7], whole[0, 8], n.with_tag(noise.LEVELS).normal(shape, 4, frame_ids=[7])[0, 0],
                  n.with_tag(noise.USER_TAG).normal(shape, 4, frame_ids=[7])[0, 0],
                  FrameNoise(SEED + 1).normal(shape, 4, frame_ids=[7])[0, 0],
                  FrameNoise(SEED + 2 ** 32).normal(shape, 4, frame_ids=[7])[0, 0]):
        assert not bool((other == base).any())


def test_distribution():
    """n = 2^20 values (F = 16, E = 65536) at a fixed seed: 5-sigma CLT conditions on the mean, the variance and the correlation
    of consecutive frames and steps, and the construction's bound on |z|.  tests/test_frame_noise_host.py shows that the
    float64 restatement meets all of them at this seed."""
    from vidtome_amd import FrameNoise
    z = FrameNoise(SEED).normal((4, 128, 128), R.DIST_STEP, n_frames=R.DIST_F, steps=2).double().cpu().numpy()
    z = z.reshape(2, R.DIST_F, R.DIST_E)
    m, t = R.moments(z[0], z[0], z[:, 0]), R.thresholds(R.DIST_F * R.DIST_E, R.DIST_E)
    print("frame_noise distribution:", m, "thresholds:", t)
    assert abs(m["mean"]) <= t["mean"] and abs(m["var"] - 1.0) <= t["var"] and m["max_abs"] <= 5.7683
    assert m["frame_corr"] <= t["frame_corr"] and m["step_corr"] <= t["step_corr"]


# ---------------------------------------------------------------------------------------------------
# keyed steps, fused against stored noise
# ---------------------------------------------------------------------------------------------------
SAMPLERS = {
    "ddim": lambda: _ddim(),
    "ddim-rescale": lambda: _ddim(guidance_rescale=0.7),
    "sde1": lambda: _sde(1),
    "sde2": lambda: _sde(2),
    "sde2-rescale": lambda: _sde(2, guidance_rescale=0.7),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
@pytest.mark.parametrize("shape", [(3, 5, 7), (4, 16, 16)], ids=["E105", "E1024"])
@pytest.mark.parametrize("name", list(SAMPLERS))
def test_keyed_step_equals_the_step_on_stored_noise(name, shape, dtype):
    """Two steps (the second is the solver's second-order one), two groups, for an unsorted chunk, an ascending run (a row
    offset: frame0) and the whole video: x', the history and eps / x0 bit for bit."""
    from vidtome_amd import FrameNoise
    n_frames, noise = 7, FrameNoise(SEED)
    for ids in ([5, 0, 3], [2, 3, 4], None):
        F = n_frames if ids is None else len(ids)
        keyed, stored = SAMPLERS[name](), SAMPLERS[name]()
        xk = _randn((n_frames,) + shape, dtype, 1)
        xs = xk.clone()
        for i in (0, 1):
            mo = _randn((2 * F,) + shape, dtype, 10 + i)
            z = noise.normal(shape, i, frame_ids=ids, n_frames=n_frames, dtype=dtype)[0]
            got = keyed.step(xk, mo, i, frame_ids=ids, noise=noise, out=xk, want=("eps", "x0"))
            want = stored.step(xs, mo, i, frame_ids=ids, noise=z, out=xs, want=("eps", "x0"))
            for g, w, what in zip(got, want, ("x'", "eps", "x0")):
                assert _same(g, w), (ids, i, what)
            for hk, hs in zip(getattr(keyed, "history", ()), getattr(stored, "history", ())):
                rows = slice(None) if ids is None else ids
                assert _same(hk[rows], hs[rows]), (ids, i, "history")
        assert not _same(xk, _randn((n_frames,) + shape, dtype, 1))


# ---------------------------------------------------------------------------------------------------
# chunking invariance
# ---------------------------------------------------------------------------------------------------
def _model(x, chunk):
    """A stand-in UNet that is a function of each frame alone: (uncond, cond), group-major."""
    rows = (x if chunk is None else x[chunk]).float()
    return torch.cat([0.5 * rows, torch.sin(1.3 * rows)]).to(x.dtype)


def _run(make, cuts, streams=None, steps=3, dtype=F16):
    """Three steps over a 12-frame video cut into ``cuts`` (lists of frame indices), each cut on its own stream when
    ``streams``; returns (latents, history)."""
    from vidtome_amd import FrameNoise
    sampler, noise = make(), FrameNoise(SEED)
    x = _randn((N_FRAMES, 4, 16, 16), dtype, 3)
    x_next = torch.empty_like(x)
    if hasattr(sampler, "prepare"):
        sampler.prepare(x)
    main = torch.cuda.current_stream()
    for i in range(steps):
        for k, chunk in enumerate(cuts):
            if streams:
                streams[k].wait_stream(main)
                with torch.cuda.stream(streams[k]):
                    sampler.step(x, _model(x, chunk), i, frame_ids=chunk, noise=noise, out=x_next)
            else:
                sampler.step(x, _model(x, chunk), i, frame_ids=chunk, noise=noise, out=x_next)
        for s in streams or ():
            main.wait_stream(s)
        x, x_next = x_next, x
    torch.cuda.synchronize()
    return x, list(getattr(sampler, "history", ()))


@pytest.mark.parametrize("name", ["sde2", "ddim"])
def test_stochastic_sampling_does_not_depend_on_the_chunking(name):
    whole = _run(SAMPLERS[name], [None])
    cuts = [list(range(0, 5)), list(range(5, 8)), list(range(8, 12))]
    shuffled = [[11, 8, 10, 9], [6, 5, 7], [2, 4, 0, 3, 1]]
    two = [[0, 2, 4, 6, 8, 10], [1, 3, 5, 7, 9, 11]]
    runs = {"chunks": _run(SAMPLERS[name], cuts), "reversed-shuffled": _run(SAMPLERS[name], shuffled),
            "two-streams": _run(SAMPLERS[name], two, streams=[torch.cuda.Stream(), torch.cuda.Stream()])}
    assert bool(torch.isfinite(whole[0]).all()) and len(whole[1]) == (1 if name == "sde2" else 0)
    for how, (x, history) in runs.items():
        assert _same(x, whole[0]), how
        for h, w in zip(history, whole[1]):
            assert _same(h, w), how


# ---------------------------------------------------------------------------------------------------
# inversion
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, F32], ids=["fp16", "fp32"])
def test_keyed_noise_levels_do_not_depend_on_the_videos_length(dtype):
    from vidtome_amd import EditFriendlyInversion, FrameNoise
    x0 = _randn((N_FRAMES, 3, 5, 7), dtype, 4)
    noise = FrameNoise(SEED)
    long = EditFriendlyInversion(_sde(2, n=4)).noise_levels(x0, noise=noise)
    short = EditFriendlyInversion(_sde(2, n=4)).noise_levels(x0[:6].contiguous(), noise=noise)
    assert long.shape == (5, N_FRAMES, 3, 5, 7) and _same(short, long[:, :6]) and _same(long[4], x0)
    # the levels are sqrt(a_k) x0 + sqrt(1 - a_k) z with z the LEVELS-tagged noise of level k, rounded once
    from vidtome_amd import noise as N
    z = noise.with_tag(N.LEVELS).normal((3, 5, 7), 0, n_frames=N_FRAMES, steps=4, dtype=dtype)
    assert not _same(z, noise.normal((3, 5, 7), 0, n_frames=N_FRAMES, steps=4, dtype=dtype))
    coef = EditFriendlyInversion(_sde(2, n=4)).level_coefficients()
    for k, (sa, sb) in enumerate(coef):
        want = (np.float32(sa) * x0.float() + np.float32(sb) * z[k].float()).to(dtype)
        assert _same(long[k], want), k


def test_stored_inversion_noise_still_reproduces_the_keyed_levels():
    """The inversion over keyed levels, then sampling with ``inv.noise[i]``: every level bit for bit."""
    from vidtome_amd import EditFriendlyInversion, FrameNoise
    n, dtype, chunks = 4, F16, [[4, 0, 2], [1, 3, 5]]
    x0 = _randn((6, 4, 16, 16), dtype, 5)
    solver = _sde(2, n=n)
    inv = EditFriendlyInversion(solver)
    levels = inv.noise_levels(x0, noise=FrameNoise(SEED))
    outs = {}
    for i in range(n):
        for c, chunk in enumerate(chunks):
            outs[i, c] = _randn((2 * len(chunk), 4, 16, 16), dtype, 100 + 10 * i + c)
            inv.step(levels, outs[i, c], i, frame_ids=chunk)
    edit = _sde(2, n=n)
    x = levels[0].clone()
    for i in range(n):
        for c, chunk in enumerate(chunks):
            edit.step(x, outs[i, c], i, frame_ids=chunk, noise=inv.noise[i][chunk])
        if i < n - 1:                                                    # (the last step lands on alphas_cumprod = 1)
            assert _same(x, levels[i + 1]), i
