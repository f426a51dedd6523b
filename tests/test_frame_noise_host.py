"""CPU tests of frame-keyed noise (vidtome_amd.noise.FrameNoise, vtm_frame_noise, vtm_philox_bits, the keyed steps): the
numpy restatement (tests/frame_noise_ref.py) against the published known answers, csrc/philox.h's integer core compiled as host
C++ against the restatement, the counter layout, the moments of the restatement at the GPU test's own seed and size (so its
thresholds are known to hold for the reference alone), the C-ABI surface, and every argument error -- raised by the Python
layers before the library is entered, and returned by the library before any launch."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import frame_noise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vidtome_amd", "csrc")
EINVAL = -1      # include/vidtome_hip.h VTM_EINVAL


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """csrc/philox.h as host C++ (tests/philox_probe.cpp): (counters (n, 4), seed) -> (outputs (n, 4), key)."""
    from vidtome_amd import build
    so = tmp_path_factory.mktemp("philox") / "philox_probe.so"
    subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC,
                    os.path.join(ROOT, "tests", "philox_probe.cpp"), "-o", str(so)], check=True)
    fn = ctypes.CDLL(str(so)).philox_probe
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = None

    def run(counters, seed):
        c = np.ascontiguousarray(counters, dtype=np.uint32)
        out, key = np.empty_like(c), np.empty(2, dtype=np.uint32)
        fn(c.ctypes.data, c.shape[0], seed, out.ctypes.data, key.ctypes.data)
        return out, tuple(int(k) for k in key)
    return run


# ---------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------
def test_restatement_gives_the_known_answers():
    for counter, key, want in R.KNOWN_ANSWERS:
        assert tuple(int(v) for v in R.philox([counter], *key)[0]) == want, (counter, key)


def test_host_core_equals_the_restatement(probe):
    """The header's integer core, compiled for the host: the known answers (their keys as 64-bit seeds) and 4096 random
    counters with the corners frame = 2^31 - 1 and step = 2^32 - 1 under a 64-bit seed."""
    for counter, key, want in R.KNOWN_ANSWERS:
        out, k = probe([counter], key[0] | key[1] << 32)
        assert k == key and tuple(int(v) for v in out[0]) == want
    rng = np.random.default_rng(11)
    c = rng.integers(0, 2 ** 32, size=(4096, 4), dtype=np.uint64)
    c[:64, 1], c[32:96, 2] = 2 ** 31 - 1, 2 ** 32 - 1
    seed = 0xFEDCBA9876543210
    out, k = probe(c, seed)
    assert k == R.key_of(seed) == (0x76543210, 0xFEDCBA98)
    assert np.array_equal(out, R.philox(c, *k))


def test_counter_layout():
    """Element e is normal e & 3 of quad e >> 2 of its frame; a frame whose E is no multiple of 4 drops the tail of its last
    quad; the frame, the step and the tag are counter words 1, 2, 3; a seed >= 2^32 reaches the second key word."""
    seed, tag, step, frames = 0x1234567800000005, 1, 9, [7, 2, 9]
    for E in (1, 3, 4, 105, 1028):
        z = R.normal(seed, tag, step, frames, E)
        assert z.shape == (1, 3, E)
        for f, frame in enumerate(frames):
            for e in (0, E // 2, E - 1):
                one = R.normals_of(R.philox([(e >> 2, frame, step, tag)], seed & 0xFFFFFFFF, seed >> 32))[0]
                assert z[0, f, e] == one[e & 3], (E, frame, e)
    # a longer frame extends a shorter one; steps and frames are independent words
    assert np.array_equal(R.normal(seed, tag, step, frames, 105)[0, :, :100], R.normal(seed, tag, step, frames, 100)[0])
    assert np.array_equal(R.normal(seed, tag, step, frames, 64, steps=3)[2], R.normal(seed, tag, step + 2, frames, 64)[0])
    assert np.array_equal(R.normal(seed, tag, step, frames, 64)[0, 1], R.normal(seed, tag, step, [2], 64)[0, 0])
    base = R.normal(seed, tag, step, [4], 64)
    for other in (R.normal(seed + 2 ** 32, tag, step, [4], 64), R.normal(seed + 1, tag, step, [4], 64),
                  R.normal(seed, tag + 1, step, [4], 64), R.normal(seed, tag, step + 1, [4], 64),
                  R.normal(seed, tag, step, [5], 64)):
        assert not np.any(other == base)
    assert R.key_of(2 ** 32) == (0, 1) and R.key_of(2 ** 64 - 1) == (0xFFFFFFFF, 0xFFFFFFFF)


def test_transform_bounds():
    """u1 in [2^-24, 1 - 2^-24] and u2 in [0, 1 - 2^-24]: |z| <= sqrt(48 ln 2) at the corner outputs."""
    corners = np.array([[0, 0, 0xFFFFFFFF, 0xFFFFFFFF], [0x1FF, 0x80000000, 0xFFFFFE00, 0x40000000]], dtype=np.uint32)
    z = R.normals_of(corners)
    assert np.all(np.isfinite(z)) and np.abs(z).max() <= np.sqrt(48 * np.log(2)) < R.MAX_ABS
    assert z[0, 0] == np.sqrt(48 * np.log(2)) and z[0, 1] == 0.0          # u1 = 2^-24, u2 = 0: the largest normal there is
    assert abs(z[1, 0] + np.sqrt(48 * np.log(2))) < 1e-12                  # u2 = 1/2: its negative


def test_restatement_meets_the_gpu_tests_thresholds():
    """The GPU test's distribution conditions (5-sigma CLT, n = 2^20) at its own seed, frames and steps, for the float64
    restatement: what the device then has to meet is met by the reference alone."""
    z = R.normal(R.DIST_SEED, 1, R.DIST_STEP, range(R.DIST_F), R.DIST_E, steps=2)
    m = R.moments(z[0], z[0], z[:, 0])
    t = R.thresholds(R.DIST_F * R.DIST_E, R.DIST_E)
    print("restatement:", m, "thresholds:", t)
    assert z[0].size == 2 ** 20 and R.meets(m, t), (m, t)


# ---------------------------------------------------------------------------------------------------
# the C ABI surface
# ---------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_exports(built):
    import vidtome_amd
    from vidtome_amd import _lib, build, noise
    hdr = open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    so = ctypes.CDLL(built)
    for name, count in (("vtm_frame_noise", 11), ("vtm_philox_bits", 5), ("vtm_guided_step_keyed", 25),
                        ("vtm_solver_step_keyed", 29)):
        decl = re.search(r"int %s\((.*?)\);" % name, hdr, re.S)
        assert decl and len(decl.group(1).split(",")) == len(_lib._SIGNATURES[name][0]) == count, name
        assert hasattr(so, name) and name in _lib.exported_symbols()

    def names(export):
        return [a.split()[-1].lstrip("*") for a in re.search(r"int %s\((.*?)\);" % export, hdr, re.S).group(1).split(",")]
    # the tensor forms' arguments with the key in place of the noise pointer
    for export in ("vtm_guided_step", "vtm_solver_step"):
        tensor, keyed = names(export), names(export + "_keyed")
        at = tensor.index("noise")
        assert keyed == tensor[:at] + ["seed", "step", "tag", "frame0"] + tensor[at + 1:], export
    doc = hdr[hdr.index("Frame-keyed noise --"):hdr.index("int vtm_frame_noise(")]
    for word in ("Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "(seed & 0xffffffff, seed >> 32)",
                 "(e >> 2, frame, step, tag)", "e & 3", "cospif", "sinpif", "5.7682", "rounded ONCE", "VTM_EINVAL"):
        assert word in doc, word
    for c_name, value in (("VTM_NOISE_INIT", noise.INIT), ("VTM_NOISE_STEP", noise.STEP), ("VTM_NOISE_LEVELS", noise.LEVELS),
                          ("VTM_NOISE_USER", noise.USER_TAG)):
        assert re.search(r"^#define %s\s+%d\b" % (c_name, value), hdr, re.M), c_name
    assert (noise.INIT, noise.STEP, noise.LEVELS, noise.USER_TAG) == (0, 1, 2, 16)
    assert re.search(r"#define VTM_ABI_VERSION 2\b", hdr) and _lib.lib().vtm_version() == _lib.ABI_VERSION == 2     # additive
    assert "frame_noise.hip" in build.SOURCES and callable(_lib.frame_noise) and callable(_lib.philox_bits)
    assert vidtome_amd.FrameNoise is noise.FrameNoise and "FrameNoise" in vidtome_amd.__all__
    # one generator: the sources that draw noise take it from philox.h and restate none of it
    for src in ("frame_noise.hip", "guided_step.hip", "solver_step.hip", "step_core.h"):
        text = open(os.path.join(CSRC, src)).read()
        assert "0xD2511F53" not in text and "logf" not in text, src
    assert "-ffast-math" not in build.FLAGS and "-fno-fast-math" in build.FLAGS


def test_kernels_use_no_scratch(built):
    """The noise kernel (3 dtypes x (quad | element) stores), the bits kernel, and the keyed forms of the two step kernels (2
    kernels x 3 dtypes x (16-byte | element) accesses each): no scratch memory and no spilled vector register -- nothing of a
    kernel's state lives in memory.  Scalar registers: the tensor-noise step kernels sit at 93 .. 101 of the 102 there are, so
    csrc/philox.h pins the key schedule to vector registers.  That pin is held to: the noise kernels and every 16-byte-access
    keyed step kernel (the path a latent frame takes) spill no scalar; an element-access one may park scalars in the lanes of
    ONE vector register (fewer than 64), which costs a lane read per use and no memory traffic."""
    from vidtome_amd import build
    lib = os.path.dirname(built)
    noise = build.kernel_resources(os.path.join(lib, "frame_noise.o"))
    assert len([k for k in noise if "frame_noise_kernel" in k]) == 6 and len([k for k in noise if "philox_bits" in k]) == 1
    keyed = {}
    for obj in ("guided_step.o", "solver_step.o"):
        res = {k: v for k, v in build.kernel_resources(os.path.join(lib, obj)).items() if "_keyed_" in k}
        assert len(res) == 12, sorted(res)
        keyed.update(res)
    for name, r in {**noise, **keyed}.items():
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
    for name, r in noise.items():
        assert r["sgpr_spill_count"] == 0, (name, r)
    for name, r in keyed.items():
        vec = re.search(r"Lb([01])E", name).group(1) == "1"               # the kernels' <T, VEC> template arguments
        assert r["sgpr_spill_count"] == 0 if vec else r["sgpr_spill_count"] < 64, (name, r)
    assert sum(re.search(r"Lb([01])E", k).group(1) == "1" for k in keyed) == 12


def test_library_refuses_before_any_launch(built):
    """VTM_EINVAL comes back before anything is launched, so no GPU is needed to see it (the pointers are never followed)."""
    from vidtome_amd import _lib
    L = _lib.lib()
    p = 1 << 20                                                            # a non-null, 16-byte aligned address
    ok = dict(out=p, dtype=0, S=1, F=2, E=8, ids=None, frame0=0, seed=1, step0=0, tag=1)
    for change, word in ((dict(dtype=3), "dtype"), (dict(out=None), "out is required"), (dict(E=0), "bad sizes"),
                         (dict(S=-1), "bad sizes"), (dict(F=(1 << 20) + 1), "bad sizes"), (dict(frame0=-1), "frame0"),
                         (dict(frame0=1 << 31), "frame0"), (dict(E=(1 << 34) + 1), "quad index"),
                         (dict(S=1 << 20, F=1 << 20, E=4), "exceed one launch")):
        a = dict(ok, **change)
        rc = L.vtm_frame_noise(a["out"], a["dtype"], a["S"], a["F"], a["E"], a["ids"], a["frame0"], a["seed"], a["step0"], a["tag"],
                               None)
        assert rc == EINVAL and word in L.vtm_last_error().decode(), (change, L.vtm_last_error())
    assert L.vtm_frame_noise(p, 0, 0, 2, 8, None, 0, 1, 0, 1, None) == 0 and L.vtm_frame_noise(p, 0, 1, 0, 8, None, 0, 1, 0, 1, None) == 0
    for args, word in (((None, 4, 1, p), "required"), ((p, 4, 1, None), "required"), ((p, -1, 1, p), "n = -1"),
                       ((p + 4, 4, 1, p), "aligned"), ((p, 4, 1, p + 8), "aligned")):
        assert L.vtm_philox_bits(*args, None) == EINVAL and word in L.vtm_last_error().decode(), args
    assert L.vtm_philox_bits(p, 0, 1, p, None) == 0

    w = (ctypes.c_float * 2)(-6.5, 7.5)

    def guided(frame0=0, E=8, sigma=0.5, pred=0, x_out=p):
        return L.vtm_guided_step_keyed(p, p, 1, 0, 1, frame0, 1, 2, E, 2, 0, 1, None, pred, 7.5, 0.0, 0.9, 0.4, 0.95, 0.3, sigma,
                                       x_out, None, None, None)

    def solver(frame0=0, E=8, c_noise=0.5, pred=0, c_h1=0.0):
        return L.vtm_solver_step_keyed(p, p, 1, 0, 1, frame0, None, None, 1, 2, E, 2, w, 1, None, pred, 0.0, 0.9, 0.4, 0.95, 0.3,
                                       c_h1, 0.0, c_noise, p, None, None, None, None)
    for call, who in ((guided, "vtm_guided_step_keyed"), (solver, "vtm_solver_step_keyed")):
        for kw, word in ((dict(frame0=-1), "frame0"), (dict(frame0=1 << 31), "frame0"), (dict(E=(1 << 34) + 4), "quad index"),
                         (dict(pred=3), "pred_type"), (dict(E=0), "bad sizes")):
            assert call(**kw) == EINVAL, (who, kw)
            msg = L.vtm_last_error().decode()
            assert msg.startswith(who + ":") and word in msg, (who, kw, msg)
    assert guided(x_out=None) == EINVAL and "no output" in L.vtm_last_error().decode()
    assert solver(c_h1=0.1) == EINVAL and "c_h1 != 0 needs h1" in L.vtm_last_error().decode()


# ---------------------------------------------------------------------------------------------------
# refusals of the Python layers
# ---------------------------------------------------------------------------------------------------
@pytest.fixture()
def no_library(monkeypatch):
    """The Python layers must refuse before the library is entered: entering it fails the test."""
    from vidtome_amd import _lib

    def entered():
        raise AssertionError("the library was entered")
    monkeypatch.setattr(_lib, "lib", entered)
    return _lib


def test_frame_noise_argument_errors(no_library):
    from vidtome_amd import FrameNoise, noise
    for args, err in (((-1,), ValueError), ((2 ** 64,), ValueError), ((1.5,), TypeError), (("7",), TypeError),
                      ((1, 3), ValueError), ((1, 15), ValueError), ((1, -1), ValueError), ((1, 2 ** 32), ValueError),
                      ((1, 2.0), TypeError)):
        with pytest.raises(err):
            FrameNoise(*args)
    n = FrameNoise(2 ** 64 - 1, noise.USER_TAG)
    assert n.key(5) == (2 ** 64 - 1, 5, 16) and FrameNoise(3).key(0) == (3, 0, noise.STEP)
    assert n.with_tag(noise.LEVELS).key(1) == (2 ** 64 - 1, 1, 2) and FrameNoise(np.int64(4), np.int32(0)).key(np.int64(2)) == (4, 2, 0)
    for step, err in ((-1, ValueError), (2 ** 32, ValueError), (0.5, TypeError)):
        with pytest.raises(err):
            n.key(step)
    cpu = torch.empty(1, 3, 4, 2, 2)
    for kw, err, word in ((dict(shape=(), n_frames=3), ValueError, "shape"),
                          (dict(shape=(4, 0, 2), n_frames=3), ValueError, "shape"),
                          (dict(shape=(4, 2.5), n_frames=3), TypeError, "shape"),
                          (dict(shape=(4, 2, 2)), ValueError, "n_frames"),
                          (dict(shape=(4, 2, 2), n_frames=-1), ValueError, "n_frames"),
                          (dict(shape=(4, 2, 2), n_frames=3, steps=-1), ValueError, "steps"),
                          (dict(shape=(4, 2, 2), n_frames=3, step=2 ** 32 - 1, steps=2), ValueError, "leave"),
                          (dict(shape=(4, 2, 2), n_frames=3, dtype=torch.float64), RuntimeError, "dtype"),
                          (dict(shape=(4, 2, 2), n_frames=3, device="cpu"), RuntimeError, "no CPU path"),
                          (dict(shape=(4, 2, 2), n_frames=3, out=cpu), RuntimeError, "must live on the GPU"),
                          (dict(shape=(4, 2, 2), n_frames=2, out=cpu), RuntimeError, "out must be a"),
                          (dict(shape=(4, 2, 2), n_frames=3, out=cpu.double()), RuntimeError, "fp16 / bf16 / fp32"),
                          (dict(shape=(4, 2, 2), n_frames=3, out=cpu.transpose(3, 4)), RuntimeError, "contiguous|GPU"),
                          (dict(shape=(4, 2, 2), frame_ids=[0, 1, 1], out=cpu), RuntimeError, "twice"),
                          (dict(shape=(4, 2, 2), frame_ids=[0, 1, 5], n_frames=5, out=cpu), RuntimeError, "outside"),
                          (dict(shape=(4, 2, 2), frame_ids=[0, -1, 2], out=cpu), RuntimeError, "outside"),
                          (dict(shape=(4, 2, 2), frame_ids=[0, 1.5, 2], out=cpu), RuntimeError, "integers")):
        kw = dict(dict(step=0), **kw)
        with pytest.raises(err, match=word):
            n.normal(kw.pop("shape"), kw.pop("step"), **kw)
    for kw, word in ((dict(n_frames=2), "n_frames = 2"), (dict(frame_ids=[0, 1]), "2 frame_ids")):       # the wrapper itself
        with pytest.raises(RuntimeError, match=word):
            no_library.frame_noise(cpu, 1, 0, 1, **kw)


def _ddim(**kw):
    from vidtome_amd import GuidedDDIM
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    return GuidedDDIM(torch.cumprod(1.0 - betas, dim=0), list(range(981, -1, -20)), **kw)


def _sde(**kw):
    from vidtome_amd import GuidedDPMSolver
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    return GuidedDPMSolver(torch.cumprod(1.0 - betas, dim=0), list(range(951, 0, -50)), algorithm_type="sde-dpmsolver++", **kw)


def test_sampler_and_inversion_argument_errors(no_library):
    from vidtome_amd import EditFriendlyInversion, FrameNoise
    L = no_library
    x, mo = torch.zeros(7, 4, 2, 2), torch.zeros(6, 4, 2, 2)
    g = torch.Generator()
    for sampler in (_ddim(eta=1.0), _sde()):
        with pytest.raises(ValueError, match="generator"):
            sampler.step(x, mo, 0, frame_ids=[4, 0, 2], noise=FrameNoise(1), generator=g)
        with pytest.raises(RuntimeError, match="must live on the GPU"):              # a CPU tensor: no fallback, keyed or not
            sampler.step(x, mo, 0, frame_ids=[4, 0, 2], noise=FrameNoise(1))
        with pytest.raises(IndexError):
            sampler.step(x, mo, 99, frame_ids=[4, 0, 2], noise=FrameNoise(1))
        with pytest.raises(RuntimeError, match="noise must be"):                       # anything else is taken for a tensor
            sampler.step(x, mo, 0, frame_ids=[4, 0, 2], noise=(1, 0, 1))
    for key, word in (((1, 2), "three integers"), ((1, 0.5, 1), "three integers"), ((-1, 0, 1), "outside"),
                      ((1, 2 ** 32, 1), "outside"), ((1, 0, 2 ** 32), "outside")):
        with pytest.raises(RuntimeError, match=word):
            L.guided_step(x, mo, 0.9, 0.4, 0.95, 0.3, 0.2, frame_ids=[4, 0, 2], key=key)
        with pytest.raises(RuntimeError, match=word):
            L.solver_step(x, mo, (-6.5, 7.5), 0.9, 0.4, 0.95, 0.3, c_noise=0.2, frame_ids=[4, 0, 2], key=key)
    with pytest.raises(RuntimeError, match="both a noise tensor and a noise key"):
        L.guided_step(x, mo, 0.9, 0.4, 0.95, 0.3, 0.2, frame_ids=[4, 0, 2], noise=torch.zeros(3, 4, 2, 2), key=(1, 0, 1))
    with pytest.raises(RuntimeError, match="sigma != 0 needs noise"):                  # without a key the tensor is still required
        L.guided_step(x, mo, 0.9, 0.4, 0.95, 0.3, 0.2, frame_ids=[4, 0, 2])
    with pytest.raises(RuntimeError, match="counters must be"):
        L.philox_bits(torch.zeros(4, 3, dtype=torch.int32), 1)
    inv = EditFriendlyInversion(_sde())
    with pytest.raises(TypeError, match="FrameNoise"):
        inv.noise_levels(x, noise=torch.zeros(3))
    with pytest.raises(ValueError, match="generator"):
        inv.noise_levels(x, generator=g, noise=FrameNoise(1))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        inv.noise_levels(x, noise=FrameNoise(1))
