"""CPU tests of merge_mlp (the feed-forward on the merged local tokens): the C-ABI surface of vtm_layernorm_gather, every
argument error it returns before any launch, ``patch.ff_route`` on stand-in blocks (no GPU: the tokens only pretend to be on
one), the plan slots, how the block forward hands this forward's plan to the feed-forward, and that ``remove_patch`` drops the
opt-in."""
import ctypes
import os
import re

import pytest
import torch

import standin
from test_masked_cross_host import FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1      # include/vidtome_hip.h VTM_EINVAL
NAME = "vtm_layernorm_gather"
C, HEADS, B, F, N = 64, 2, 2, 4, 16
F16, F32 = torch.float16, torch.float32


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


def test_header_declares_and_lib_binds_the_export(built):
    from vidtome_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    decl = re.search(r"int vtm_layernorm_gather\((.*?)\);", hdr, re.S)
    assert decl, "not declared"
    params = [p.strip() for p in decl.group(1).split(",")]
    argtypes, restype = _lib._SIGNATURES[NAME]
    assert len(params) == len(argtypes) == 13 and restype is ctypes.c_int
    # parameter by parameter: pointers, int64 sizes, the int dtype, the float eps
    for p, t in zip(params, argtypes):
        want = (ctypes.c_void_p if "*" in p or p.startswith("vtm_stream_t") else ctypes.c_int64 if p.startswith("int64_t")
                else ctypes.c_float if p.startswith("float") else ctypes.c_int)
        assert t is want, (p, t)
    assert [p.split()[-1].lstrip("*") for p in params] == ["x", "gamma", "beta", "dtype", "B", "L", "C", "rows", "n", "eps",
                                                            "out", "panel_rows", "stream"]
    doc = hdr[hdr.index("vtm_layernorm_gather --"):decl.start()]
    for word in ("patch.py:187", "merge.py:119-133", "NOT range-checked", "BIT-EQUAL", "vtm_panel_rows(B * n)", "VTM_EINVAL"):
        assert word in doc, word
    # additive: the ABI version stays
    assert re.search(r"#define VTM_ABI_VERSION 2\b", hdr) and _lib.lib().vtm_version() == _lib.ABI_VERSION == 2
    assert hasattr(ctypes.CDLL(built), NAME) and NAME in _lib.exported_symbols()
    assert "layernorm.hip" in build.SOURCES and callable(_lib.layernorm_gather)


def test_gather_kernels_do_not_spill(built):
    """Both kernel families x 3 dtypes x streaming or not, with the map (last template argument true): no scratch, no
    spilled register, and no more than 128 VGPRs (the occupancy step of the kernels without the map)."""
    from vidtome_amd import build
    res = build.kernel_resources(os.path.join(os.path.dirname(built), "layernorm.o"))
    # (mangled template arguments <T, NCH | LPR, R, NT, G>: ... Lb<NT>E Lb<G>E E)
    gathered = {k: v for k, v in res.items() if re.search(r"layernorm(_rows)?_kernel.*Lb[01]ELb1EEEv", k)}
    assert len(gathered) == 42, sorted(res)
    for name, r in gathered.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r["vgpr_count"] <= 128, (name, r)


# ---------------------------------------------------------------------------------------------------
# argument errors: returned before anything is launched, so they can be provoked without a GPU (the pointers are never read)
# ---------------------------------------------------------------------------------------------------
P = 0x1000      # a non-NULL "pointer"


def _call(x=P, gamma=P, beta=P, dtype=1, b=3, l=100, c=320, rows=P, n=37, eps=1e-5, out=P, panel_rows=None):
    from vidtome_amd import _lib
    lib = _lib.lib()
    if panel_rows is None:
        panel_rows = lib.vtm_panel_rows(b * n)
    rc = lib.vtm_layernorm_gather(x, gamma, beta, dtype, b, l, c, rows, n, eps, out, panel_rows, None)
    return rc, (lib.vtm_last_error() or b"").decode()


BAD = {
    "x NULL": dict(x=None),
    "rows NULL": dict(rows=None),
    "out NULL": dict(out=None),
    "C not a multiple of 8": dict(c=324),
    "C = 0": dict(c=0),
    "C above 2048": dict(c=2056),
    "unknown dtype": dict(dtype=7),
    "negative dtype": dict(dtype=-1),
    "panel_rows below the rows": dict(panel_rows=104),
    "panel_rows of another row count": dict(panel_rows=512),
    "panel_rows negative": dict(panel_rows=-256),
    "fp32 panels": dict(dtype=0),
    "negative n": dict(n=-1, panel_rows=0),
    "B beyond the grid": dict(b=65536, panel_rows=0),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_argument_errors_return_einval_and_name_the_call(built, what):
    from vidtome_amd import _lib
    assert _lib.lib().vtm_panel_rows(3 * 37) == 256
    rc, msg = _call(**BAD[what])
    assert rc == EINVAL, (what, rc, msg)
    assert msg.startswith(NAME + ":"), msg


def test_nothing_to_do_is_ok(built):
    assert _call(n=0, panel_rows=0)[0] == 0 and _call(b=0, panel_rows=0)[0] == 0


def test_wrapper_refuses_operands_before_the_library(built):
    from vidtome_amd import _lib
    x = torch.zeros(2, 10, 64, dtype=F16)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        _lib.layernorm_gather(x, torch.zeros(2, 4, dtype=torch.int32), None, None, 1e-5)
    xf = x.as_subclass(FakeCuda)
    for rows in (torch.zeros(2, 4, dtype=torch.int64), torch.zeros(3, 4, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="rows"):
            _lib.layernorm_gather(xf, rows.as_subclass(FakeCuda), None, None, 1e-5)


# ---------------------------------------------------------------------------------------------------
# ff_route
# ---------------------------------------------------------------------------------------------------
class OtherNorm(torch.nn.LayerNorm):
    """Computes a LayerNorm, but is not the class the fused path reads."""


class PlainFF(torch.nn.Module):
    """A feed-forward that is not the GEGLU one."""

    def __init__(self, c):
        super().__init__()
        self.net = torch.nn.ModuleList([torch.nn.Linear(c, c)])

    def forward(self, x):
        return self.net[0](x)


def _patched(dtype=F16, **kw):
    import vidtome_amd
    unet = standin.StandInUNet(C, HEADS, full=True, cond_dim=32).to(dtype)
    vidtome_amd.apply_patch(unet, batch_size=B, **kw)
    return unet, list(unet.blocks())[-1]


def _tokens(dtype=F16, cuda=True):
    t = torch.zeros(B * F, N, C, dtype=dtype)
    return t.as_subclass(FakeCuda) if cuda else t


def _plan(local=True):
    from vidtome_amd import patch as vpatch
    plan = vpatch.MergePlan()
    plan.fsize, plan.L = F, F * N
    if local:
        plan.keep = torch.zeros(B, 40, dtype=torch.int32)
        plan.inv_local = torch.zeros(B, F * N, dtype=torch.int32)
    return plan


def test_plan_has_the_two_slots_empty():
    from vidtome_amd import patch as vpatch
    plan = vpatch.MergePlan()
    assert plan.keep is None and plan.inv_local is None
    assert "keep" in vpatch.MergePlan.__slots__ and "inv_local" in vpatch.MergePlan.__slots__


def test_route_is_plain_without_the_flag_a_local_map_or_with_ada_zero(built):
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    unet, blk = _patched()
    x = _tokens()
    assert vpatch.fused_ff_ok(blk.norm3, blk.ff, x)
    assert vpatch.ff_route(blk, x, _plan()) == "panels"                    # flag unset
    vidtome_amd.update_patch(unet, merge_mlp=False)
    assert vpatch.ff_route(blk, x, _plan()) == "panels"
    vidtome_amd.update_patch(unet, merge_mlp=1)                            # the opt-in is True itself, like fp32_projections
    assert vpatch.ff_route(blk, x, _plan()) == "panels"
    vidtome_amd.update_patch(unet, merge_mlp=True)
    assert vpatch.ff_route(blk, x, _plan()) == "merged-panels"
    assert vpatch.ff_route(blk, x, None) == "panels"                       # a site that does not merge: no plan
    assert vpatch.ff_route(blk, x, _plan(local=False)) == "panels"         # single-frame chunk, local_merge_ratio <= 0
    half = _plan()
    half.inv_local = None
    assert vpatch.ff_route(blk, x, half) == "panels"
    blk.use_ada_layer_norm_zero = True
    assert vpatch.ff_route(blk, x, _plan()) == "module"
    blk.use_ada_layer_norm_zero = False
    blk.use_ada_layer_norm = True                                          # AdaLayerNorm keeps a plain norm3
    assert vpatch.ff_route(blk, x, _plan()) == "merged-panels"


@pytest.mark.parametrize("what", ["fp32 model", "FF_MODE = blas", "not a GEGLU ff", "a non-plain norm3", "fp32 ff in an fp16 block",
                                  "bf16"])
def test_route_follows_fused_ff_ok(built, monkeypatch, what):
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    dtype = {"fp32 model": F32, "bf16": torch.bfloat16}.get(what, F16)
    unet, blk = _patched(dtype)
    vidtome_amd.update_patch(unet, merge_mlp=True)
    if what == "FF_MODE = blas":
        monkeypatch.setattr(vpatch, "FF_MODE", "blas")
    elif what == "not a GEGLU ff":
        blk.ff = PlainFF(C).to(dtype)
    elif what == "a non-plain norm3":
        blk.norm3 = OtherNorm(C).to(dtype)
    elif what == "fp32 ff in an fp16 block":
        blk.ff.float()
    x = _tokens(dtype)
    want = "merged-panels" if what == "bf16" else "merged"
    assert vpatch.fused_ff_ok(blk.norm3, blk.ff, x) == (want == "merged-panels")
    assert vpatch.ff_route(blk, x, _plan()) == want


def test_route_launches_nothing(built, monkeypatch):
    """Every wrapper of the library is replaced by one that fails: ff_route still answers."""
    import vidtome_amd
    from vidtome_amd import _lib, patch as vpatch
    unet, blk = _patched()
    vidtome_amd.update_patch(unet, merge_mlp=True)

    def boom(*a, **k):
        raise AssertionError("ff_route called into the library")
    for name in ("layernorm_gather", "layernorm", "layernorm_panels", "gather_rows", "unmerge_add", "ff_geglu", "linear_panels",
                 "to_panels", "geglu"):
        monkeypatch.setattr(_lib, name, boom)
    assert vpatch.ff_route(blk, _tokens(), _plan()) == "merged-panels"
    monkeypatch.setattr(vpatch, "FF_MODE", "blas")
    assert vpatch.ff_route(blk, _tokens(), _plan()) == "merged"


# ---------------------------------------------------------------------------------------------------
# the block forward: the plan of THIS forward reaches the feed-forward on a local, nothing is kept on the module
# ---------------------------------------------------------------------------------------------------
def _stub_forward(monkeypatch, blk, seen):
    from vidtome_amd import patch as vpatch

    def segment(block, hs, *a, **kw):
        seen["segment_kw"] = dict(kw)
        if "plan_to" in kw:
            seen["plan"] = _plan()
            kw["plan_to"].append(seen["plan"])
        return hs

    def merged(block, hs, plan, route):
        seen["merged"] = (plan, route)
        return hs + 1

    monkeypatch.setattr(vpatch, "self_attention_segment", segment)
    monkeypatch.setattr(vpatch, "merged_feed_forward_residual", merged)
    monkeypatch.setattr(vpatch, "norm_feed_forward_residual", lambda norm, ff, hs: hs + 2)
    blk.attn2 = None


def test_forward_hands_this_forwards_plan_to_the_feed_forward(built, monkeypatch):
    import vidtome_amd
    unet, blk = _patched()
    seen = {}
    _stub_forward(monkeypatch, blk, seen)
    x = _tokens()
    # flag unset: the segment is called as before (no new keyword), the feed-forward is today's
    assert torch.equal(blk(x), x + 2) and seen["segment_kw"] == {} and "merged" not in seen
    before = set(blk.__dict__)
    vidtome_amd.update_patch(unet, merge_mlp=True)
    y = blk(x)
    assert torch.equal(y, x + 1)
    assert seen["merged"][0] is seen["plan"] and seen["merged"][1] == "merged-panels"
    # nothing of the forward stays on the module: only the opt-in itself was added
    assert set(blk.__dict__) - before == {"merge_mlp"}
    first = seen["plan"]
    blk(x)
    assert seen["merged"][0] is seen["plan"] and seen["plan"] is not first


def test_remove_patch_drops_the_flag(built):
    import vidtome_amd
    unet, blk = _patched()
    vidtome_amd.update_patch(unet, merge_mlp=True)
    assert all(b.merge_mlp is True for b in unet.blocks())
    vidtome_amd.remove_patch(unet)
    assert not any(hasattr(b, "merge_mlp") for b in unet.blocks())
    vidtome_amd.apply_patch(unet, batch_size=B)
    assert not any(hasattr(b, "merge_mlp") for b in unet.blocks())
    vidtome_amd.update_patch(unet, merge_mlp=True)
    vidtome_amd.apply_patch(unet, batch_size=B)                            # apply_patch removes first: starts without it too
    assert not any(hasattr(b, "merge_mlp") for b in unet.blocks())
    vidtome_amd.remove_patch(unet)
