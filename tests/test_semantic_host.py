"""CPU tests of semantic guidance: the C-ABI surface of vtm_semantic_guidance (declaration, export, argument count, constants,
resources), every VTM_EINVAL path without a launch, the binding's and the host module's own checks, ``schedule``, and the
contract's mask against Diffusers' torch.quantile chain (tests/semantic_standin.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import semantic_standin as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NAME = "vtm_semantic_guidance"


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


def _header():
    return open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()


def test_header_declares_the_entry_and_the_version_stays(built):
    from vidtome_amd import _lib, build
    import vidtome_amd
    hdr = _header()
    decl = re.search(r"^int " + NAME + r"\(([^;]*)\);", hdr, re.M)
    assert decl and hasattr(ctypes.CDLL(built), NAME) and NAME in _lib.exported_symbols()
    argtypes, restype = _lib._SIGNATURES[NAME]
    assert len(decl.group(1).split(",")) == len(argtypes) == 28 and restype is ctypes.c_int
    assert "#define VTM_ABI_VERSION 2" in hdr and _lib.lib().vtm_version() == _lib.ABI_VERSION == 2
    assert "semantic.hip" in build.SOURCES and callable(_lib.semantic_guidance)
    for c_name, value in (("VTM_SEGA_MAX_CONCEPTS", _lib.SEGA_MAX_CONCEPTS), ("VTM_SEGA_MAX_PLANE", _lib.SEGA_MAX_PLANE),
                          ("VTM_SEGA_CHANNEL", _lib.SEGA_CHANNEL), ("VTM_SEGA_SUM", _lib.SEGA_SUM),
                          ("VTM_SEGA_REGION", _lib.SEGA_REGION), ("VTM_SEGA_CHANNEL_REGION", _lib.SEGA_CHANNEL_REGION),
                          ("VTM_SEGA_SUM_REGION", _lib.SEGA_SUM_REGION), ("VTM_SOLVER_MAX_GROUPS", _lib.SOLVER_MAX_GROUPS)):
        assert re.search(r"^#define " + c_name + r" (\d+)\b", hdr, re.M).group(1) == str(value), c_name
    assert (_lib.SEGA_MAX_CONCEPTS, _lib.SEGA_MAX_PLANE) == (6, 16384) and 2 + _lib.SEGA_MAX_CONCEPTS <= _lib.SOLVER_MAX_GROUPS
    assert {"EditConcept", "SemanticGuidance"} <= set(vidtome_amd.__all__)
    from vidtome_amd.semantic import MASK_MODES
    assert MASK_MODES == {v: k for k, v in S.MODE_NAMES.items()}


def test_kernel_uses_no_scratch(built):
    """profiles/semantic_resources.txt: no scratch and no spills in any of the three instantiations; the fixed part of the
    LDS is dynamic (histogram, selection words, thresholds, then the population)."""
    from vidtome_amd import build
    res = build.kernel_resources(os.path.join(os.path.dirname(built), "semantic.o"))
    kernels = {k: v for k, v in res.items() if "semantic_kernel" in k}
    assert len(kernels) == 3 == len(res), sorted(res)
    for k, v in kernels.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
        assert v["vgpr_count"] <= 128, (k, v)


def test_einval_paths_answer_without_a_launch(built):
    """No GPU here: a call that got as far as a launch would fail differently (VTM_ELAUNCH) or crash on the fake pointers."""
    from vidtome_amd import _lib
    L = _lib.lib()
    MO, OUT, REG, MOM, MASK = 0x100000, 0x900000, 0xA00000, 0xB00000, 0xC00000
    i32, f32, f64 = ctypes.c_int32 * 6, ctypes.c_float * 6, ctypes.c_double * 6
    ok = dict(mo=MO, dtype=_lib.VTM_F16, F=2, C=4, H=8, W=8, groups=4, gu=0, gc=1, s=7.5, E=2, group=[2, 3], scale=[5.0, -5.0],
              lo=[10, 63], frac=[0.5, 0.0], wa=[1.0, 0.0], wc=[1.0, 1.0], mode=[0, 1], regions=None, mom=MOM, n_rows=2,
              ids=None, ms=0.1, mb=0.4, ma=1, out=OUT, mask=MASK)

    def call(**kw):
        a = dict(ok, **kw)
        pad = lambda v: list(v) + [0] * (6 - len(v))
        arr = lambda t, v: None if v is None else t(*pad(v))
        return L.vtm_semantic_guidance(a["mo"], a["dtype"], a["F"], a["C"], a["H"], a["W"], a["groups"], a["gu"], a["gc"], a["s"],
                                       a["E"], arr(i32, a["group"]), arr(f32, a["scale"]), arr(i32, a["lo"]), arr(f64, a["frac"]),
                                       arr(f32, a["wa"]), arr(f32, a["wc"]), arr(i32, a["mode"]), a["regions"], a["mom"],
                                       a["n_rows"], a["ids"], a["ms"], a["mb"], a["ma"], a["out"], a["mask"], None)
    nan, inf = float("nan"), float("inf")
    bad = [dict(mo=None), dict(out=None), dict(dtype=9), dict(F=-1), dict(F=(1 << 20) + 1), dict(C=0), dict(H=0), dict(W=0),
           dict(H=128, W=129), dict(H=16385, W=1), dict(E=7), dict(E=-1), dict(groups=0), dict(groups=9), dict(gu=4), dict(gu=-1),
           dict(gc=4), dict(gc=-2), dict(group=[2, 4]), dict(group=[-1, 3]), dict(group=None), dict(scale=None), dict(lo=None),
           dict(frac=None), dict(wa=None), dict(wc=None), dict(mode=None), dict(mode=[0, 5]), dict(mode=[-1, 0]),
           dict(lo=[64, 0]), dict(lo=[-1, 0]), dict(frac=[1.0, 0.0]), dict(frac=[-0.1, 0.0]), dict(frac=[nan, 0.0]),
           dict(wa=[inf, 0.0]), dict(wc=[nan, 1.0]), dict(s=nan), dict(ms=inf), dict(mb=nan), dict(ma=2), dict(ma=-1),
           dict(mode=[3, 1]), dict(mode=[0, 2]), dict(mode=[0, 4]),                     # a region mode, regions NULL
           dict(n_rows=1), dict(ids=0xD00000, n_rows=0),
           dict(out=MO), dict(out=MO + 4 * 2 * 4 * 64 * 2 - 2), dict(out=MO - 2 * 4 * 64 * 2 + 2)]   # out overlaps model_out
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert _lib.lib().vtm_last_error(), kw
    # F == 0 is fine and launches nothing; a weight-0 concept may name a region without regions
    assert call(F=0, n_rows=0) == 0
    assert call(F=0, n_rows=0, mode=[0, 2], wc=[1.0, 0.0]) == 0
    assert call(F=0, n_rows=0, E=0, group=None, scale=None, lo=None, frac=None, wa=None, wc=None, mode=None) == 0
    # the quantile's ranks are not read for the region mode
    assert call(F=0, n_rows=0, mode=[0, 2], lo=[0, 999], regions=REG) == 0


def test_sega_rank_is_the_contracts(built):
    from vidtome_amd import _lib
    for P in (1, 2, 35, 64, 480, 4096, 16384):
        for q in (0.0, 0.5, 0.9, 0.95, 0.999, 1.0, 1 / 3):
            lo, frac = _lib.sega_rank(q, P)
            assert (lo, frac) == S.rank(q, P) and 0 <= lo <= P - 1 and 0.0 <= frac < 1.0
            assert lo + frac == q * (P - 1)
        assert _lib.sega_rank(1.0, P) == (P - 1, 0.0) and _lib.sega_rank(0.0, P) == (0, 0.0)
    for q in (-0.1, 1.1, float("nan")):
        with pytest.raises(RuntimeError, match="quantile"):
            _lib.sega_rank(q, 64)


def test_schedule_warmup_cooldown_and_momentum():
    from vidtome_amd import EditConcept, SemanticGuidance
    a = EditConcept(scale=5.0, warmup=3, cooldown=8, weight=0.5)
    b = EditConcept(scale=4.0, reverse=True, warmup=5, cooldown=None, weight=2.0, mask="sum")
    sg = SemanticGuidance([a, b], guidance_scale=7.5)
    assert sg.groups == 4 and SemanticGuidance([a], cfg=False).groups == 2 and SemanticGuidance([]).groups == 2
    assert a.signed_scale == 5.0 and b.signed_scale == -4.0
    for i in range(12):
        app, acc, mom = sg.schedule(i)
        assert acc == [0.5 if i < 8 else 0.0, 2.0]                     # accumulates while i < cooldown
        assert app == [0.5 if 3 <= i < 8 else 0.0, 2.0 if i >= 5 else 0.0]     # applied while warmup <= i < cooldown
        assert mom is (i >= 5)                                         # once EVERY concept is past its warm-up
    assert SemanticGuidance([]).schedule(3) == ([], [], False)
    with pytest.raises(IndexError):
        sg.schedule(-1)
    for kw in (dict(mask="pixel"), dict(threshold=1.5), dict(threshold=-0.1), dict(scale=-1.0), dict(scale=float("nan")),
               dict(weight=float("inf")), dict(warmup=-1), dict(cooldown=-2)):
        with pytest.raises(ValueError):
            EditConcept(**kw)
    with pytest.raises(ValueError, match="at most 6"):
        SemanticGuidance([a] * 7)
    with pytest.raises(TypeError):
        SemanticGuidance([dict(scale=1.0)])
    with pytest.raises(RuntimeError, match="prepare"):
        sg.combine(torch.zeros(4, 4, 8, 8), 0)
    with pytest.raises(RuntimeError, match="GPU"):
        sg.prepare(torch.zeros(1, 4, 8, 8))


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: the binding's checks run, and a launch would be caught by the test."""
    @property
    def is_cuda(self):
        return True


def test_binding_raises_before_any_launch(built, monkeypatch):
    from vidtome_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the binding reached the library"))
    F16 = torch.float16

    def call(shape=(8, 4, 8, 8), groups=4, gu=0, gc=1, group=(2, 3), scale=(5.0, 5.0), q=(0.9, 0.5), wa=(1.0, 1.0), wc=(1.0, 1.0),
             mode=(0, 1), dtype=F16, **kw):
        mo = torch.zeros(shape, dtype=dtype).as_subclass(_FakeCuda)
        return _lib.semantic_guidance(mo, groups, gu, gc, 7.5, list(group), list(scale), list(q), list(wa), list(wc), list(mode), **kw)
    cases = [
        (dict(shape=(8, 4, 128, 129)), "plane"),                                        # P > 16384
        (dict(shape=(8, 4, 8, 8), group=(2,) * 7, scale=(1.0,) * 7, q=(0.5,) * 7, wa=(1.0,) * 7, wc=(1.0,) * 7, mode=(0,) * 7,
              groups=8), "concepts"),                                                   # E > 6
        (dict(q=(1.5, 0.5)), "quantiles"), (dict(q=(0.9, -0.01)), "quantiles"), (dict(q=(float("nan"), 0.5)), "quantiles"),
        (dict(mode=(3, 1)), "regions"), (dict(mode=(0, 2)), "regions"), (dict(mode=(4, 1)), "regions"),
        (dict(mode=(0, 2), regions=torch.zeros(2, 2, 8, 4, dtype=torch.uint8)), "regions"),
        (dict(mode=(0, 2), regions=torch.zeros(2, 2, 8, 8)), "regions"),
        (dict(groups=3), "groups"),                                                     # 8 samples are not 3 groups of frames
        (dict(groups=9, shape=(9, 4, 8, 8)), "groups"), (dict(group=(2, 4)), "group index"), (dict(gu=4), "group index"),
        (dict(gc=-2), "group index"), (dict(frame_ids=[0, 1, 2]), "frames"),           # 3 rows for a chunk of 2 frames
        (dict(mode=(0, 7)), "mode"), (dict(wa=(float("inf"), 1.0)), "finite"), (dict(scale=(1.0,)), "per-concept"),
        (dict(dtype=torch.float64), "fp16 / bf16 / fp32"), (dict(shape=(8, 4, 64)), "fp16 / bf16 / fp32"),
        (dict(momentum=torch.zeros(2, 4, 8, 8, dtype=F16)), "momentum"), (dict(momentum=torch.zeros(2, 4, 8, 4)), "momentum"),
        (dict(momentum=torch.zeros(5, 4, 8, 8), frame_ids=[0, 5]), "frame_ids"),
        (dict(out=torch.zeros(2, 4, 8, 8)), "out must be"), (dict(out=torch.zeros(3, 4, 8, 8, dtype=F16)), "out must be"),
    ]
    for kw, match in cases:
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    # overlapping out: a view of model_out's own storage
    mo = torch.zeros((8, 4, 8, 8), dtype=F16).as_subclass(_FakeCuda)
    with pytest.raises(RuntimeError, match="overlaps"):
        _lib.semantic_guidance(mo, 4, 0, 1, 7.5, [2, 3], [5.0, 5.0], [0.9, 0.5], [1.0, 1.0], [1.0, 1.0], [0, 1], out=mo[2:4])
    # a CPU tensor is refused: there is no torch fallback
    with pytest.raises(RuntimeError, match="GPU"):
        _lib.semantic_guidance(torch.zeros((8, 4, 8, 8), dtype=F16), 4, 0, 1, 7.5, [2, 3], [5.0, 5.0], [0.9, 0.5], [1.0, 1.0],
                               [1.0, 1.0], [0, 1])


@pytest.mark.parametrize("P", [35, 64, 480, 4096, 16384])
def test_contract_masks_equal_diffusers_quantile_chain(P):
    """On N(0, 1)-scaled fp32 planes the contract's mask (exact order statistics, the double formula) equals the mask of
    Diffusers' chain (torch.quantile's fp32 lerp on |g|.flatten(2), then >=) exactly.  The two thresholds differ by what
    torch's fp32 arithmetic costs, and are held to that: torch forms pos = fp32(q) * (P - 1) in fp32, off by at most
    2 (P - 1) 2^-24 from the double pos, which moves a piecewise-linear interpolant by at most that times the largest gap
    between the neighbouring order statistics (ranks lo - 1 .. lo + 2); its lerp a + w (b - a) rounds three times and the
    contract's formula once, 4 * 2^-24 a_hi together.  The relative difference is printed: at most a few 1e-6, the largest
    at q = 0.999 of P = 16384, where pos = 16366.6 has an fp32 spacing of 1e-3 and the tail's gaps are wide."""
    H, W = {35: (5, 7), 64: (8, 8), 480: (24, 20), 4096: (64, 64), 16384: (128, 128)}[P]
    gen = torch.Generator().manual_seed(1000 + P)
    F, C = 2, 4
    mo = (torch.randn((2, F, C, H, W), generator=gen) * 1.3).numpy()
    for q in (0.0, 0.5, 0.9, 0.95, 0.999, 1.0):
        concept = dict(group=1, scale=5.0, q=q, w_apply=1.0, w_acc=1.0, mode=S.CHANNEL)
        M, thrs = S.masks(mo, 0, [concept])
        ref_mask, ref_thr = S.diffusers_masks(torch.from_numpy(S.edit_terms(mo, 0, 1, 5.0)), q)
        rel = np.abs(thrs[0].astype(np.float64) - ref_thr.double().numpy()) / ref_thr.double().numpy()
        print(f"[semantic] P = {P} q = {q}: worst relative thr difference {rel.max():.3e}, "
              f"kept {M[0].mean():.4f} of the plane")
        srt = np.sort(np.abs(S.edit_terms(mo, 0, 1, 5.0)).reshape(F, C, P), axis=2).astype(np.float64)
        lo = S.rank(q, P)[0]
        near = srt[:, :, max(lo - 1, 0):min(lo + 3, P)]
        gap = np.diff(near, axis=2).max(axis=2) if near.shape[2] > 1 else np.zeros((F, C))
        bound = 2 * (P - 1) * 2.0 ** -24 * gap + 4 * 2.0 ** -24 * near[:, :, -1]
        assert (np.abs(thrs[0].astype(np.float64) - ref_thr.double().numpy()) <= bound).all(), (P, q, rel.max())
        assert np.array_equal(M[0], ref_mask.numpy()), (P, q, int((M[0] != ref_mask.numpy()).sum()))
        kept = M[0].reshape(F, C, P).sum(axis=2)
        assert (kept >= P - S.rank(q, P)[0] - 1).all() and (kept <= P - S.rank(q, P)[0]).all()


def test_standin_sum_mode_region_and_nan_rules():
    gen = torch.Generator().manual_seed(7)
    mo = torch.randn((3, 1, 4, 6, 6), generator=gen).numpy()
    reg = (torch.rand((2, 1, 6, 6), generator=gen) > 0.5).to(torch.uint8).numpy()
    cs = [dict(group=1, scale=3.0, q=0.75, w_apply=1.0, w_acc=0.0, mode=S.SUM_REGION),
          dict(group=2, scale=-2.0, q=0.5, w_apply=0.0, w_acc=1.0, mode=S.REGION)]
    M, thrs = S.masks(mo, 0, cs, reg)
    assert all((M[0][:, ch] == M[0][:, 0]).all() for ch in range(4)) and thrs[0].shape == (1,)     # one mask per frame
    assert not (M[0][:, 0] & (reg[0] == 0)).any() and np.array_equal(M[1][:, 2], reg[1] != 0) and 1 not in thrs
    # a NaN ranks last: it is never selected, and a quantile that lands on it selects nothing
    mo[1, 0, 0, 0, 0] = np.nan
    c = dict(group=1, scale=3.0, q=0.5, w_apply=1.0, w_acc=1.0, mode=S.CHANNEL)
    M, _ = S.masks(mo, 0, [c])
    assert not M[0][0, 0, 0, 0] and M[0][0, 0].sum() > 0
    M, _ = S.masks(mo, 0, [dict(c, q=1.0)])
    assert M[0][0, 0].sum() == 0 and M[0][0, 1].sum() >= 1
    # a concept of weight 0 is absent
    assert S.masks(mo, 0, [dict(c, w_apply=0.0, w_acc=0.0)])[0] == {}
