"""CPU tests of merge_crossattn (attn2 on the merged local tokens, keys routed per frame): the C-ABI surface of
vtm_frame_order and vtm_attention_kv_segments, the argument errors they return before any launch, ``patch.cross_merge_route``
over the table of its conditions on stand-in blocks (no GPU: the tokens only pretend to be on one), how the block forward hands
this forward's plan to attn2, and the life cycle of the opt-in through ``update_patch`` / ``remove_patch`` / ``apply_patch``."""
import ctypes
import os
import re

import pytest
import torch

import standin
from test_masked_cross_host import FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1      # include/vidtome_hip.h VTM_EINVAL
C, HEADS, B, F, N, K, D = 64, 2, 3, 4, 16, 77, 32
F16, F32 = torch.float16, torch.float32
NAMES = {"vtm_frame_order": ["keep", "Ml", "inv_local", "B", "F", "N", "ws", "ws_bytes", "keep_sorted", "inv_sorted", "seg_off",
                             "stream"],
         "vtm_attention_kv_segments": ["q", "ldq", "k", "ldk", "vt", "ldvt", "out", "ldo", "dtype", "rows_total", "seg_off",
                                       "n_seg", "max_seg_rows", "h", "Mk", "Mkp", "d", "scale", "stream"]}


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


@pytest.mark.parametrize("name", sorted(NAMES))
def test_header_declares_and_lib_binds_the_exports(built, name):
    from vidtome_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    decl = re.search(r"int %s\((.*?)\);" % name, hdr, re.S)
    assert decl, "not declared"
    params = [p.strip() for p in decl.group(1).split(",")]
    argtypes, restype = _lib._SIGNATURES[name]
    assert len(params) == len(argtypes) == len(NAMES[name]) and restype is ctypes.c_int
    for p, t in zip(params, argtypes):
        want = (ctypes.c_void_p if "*" in p or p.startswith("vtm_stream_t") else ctypes.c_int64 if p.startswith("int64_t")
                else ctypes.c_size_t if p.startswith("size_t") else ctypes.c_float if p.startswith("float") else ctypes.c_int)
        assert t is want, (p, t)
    assert [p.split()[-1].lstrip("*") for p in params] == NAMES[name]
    doc = hdr[hdr.index(name + " --"):decl.start()]
    for word in ("vidtome/patch.py:171-185", "VTM_EINVAL", "DEVICE"):
        assert word in doc, word
    # additive: the ABI version stays
    assert re.search(r"#define VTM_ABI_VERSION 2\b", hdr) and _lib.lib().vtm_version() == _lib.ABI_VERSION == 2
    assert hasattr(ctypes.CDLL(built), name) and name in _lib.exported_symbols()
    assert "frame_order.hip" in build.SOURCES and "attention_segments.hip" in build.SOURCES
    assert callable(_lib.frame_order) and callable(_lib.attention_kv_segments)


def test_frame_order_workspace_size(built):
    from vidtome_amd import _lib
    assert "size_t vtm_frame_order_ws_bytes(" in open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    ws = _lib.lib().vtm_frame_order_ws_bytes
    assert ws(3, 4, 24) >= 3 * 4 * 24 * 4 and ws(0, 4, 24) == 0 and ws(3, 0, 24) == 0 and ws(3, 4, -1) == 0


def test_segments_kernels_do_not_spill(built):
    """Every head dim x fp16 / bf16: no scratch, no spilled register, the LDS of the per-key-bias kernel."""
    from vidtome_amd import build
    res = build.kernel_resources(os.path.join(os.path.dirname(built), "attention_segments.o"))
    seg = {k: v for k, v in res.items() if "attention_segments_kernel" in k}
    bias = {k: v for k, v in build.kernel_resources(os.path.join(os.path.dirname(built), "attention_bias.o")).items()
            if "attention_bias_kernel" in k}
    assert len(seg) == 18 == len(bias), sorted(res)
    for name, r in seg.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
    assert sorted(r["group_segment_fixed_size"] for r in seg.values()) == sorted(r["group_segment_fixed_size"]
                                                                                 for r in bias.values())


# ---------------------------------------------------------------------------------------------------
# argument errors: returned before anything is launched, so they can be provoked without a GPU (the pointers are never read)
# ---------------------------------------------------------------------------------------------------
P = 0x1000      # a non-NULL "pointer"


def _frame_order(keep=P, ml=37, inv=P, b=3, f=4, n=24, ws=P, ws_bytes=1 << 20, ks=P, inv_s=P, seg=P):
    from vidtome_amd import _lib
    lib = _lib.lib()
    rc = lib.vtm_frame_order(keep, ml, inv, b, f, n, ws, ws_bytes, ks, inv_s, seg, None)
    return rc, (lib.vtm_last_error() or b"").decode()


def _segments(q=P, ldq=80, k=P, ldk=80, vt=P, ldvt=80, out=P, ldo=80, dtype=1, rows=1000, off=P, n_seg=12, bound=256, h=2,
              mk=77, mkp=80, d=40, scale=0.158):
    from vidtome_amd import _lib
    lib = _lib.lib()
    rc = lib.vtm_attention_kv_segments(q, ldq, k, ldk, vt, ldvt, out, ldo, dtype, rows, off, n_seg, bound, h, mk, mkp, d, scale,
                                       None)
    return rc, (lib.vtm_last_error() or b"").decode()


BAD_ORDER = {
    "keep NULL": dict(keep=None), "inv_local NULL": dict(inv=None), "ws NULL": dict(ws=None), "keep_sorted NULL": dict(ks=None),
    "inv_sorted NULL": dict(inv_s=None), "seg_off NULL": dict(seg=None), "M_l = 0": dict(ml=0), "M_l above L": dict(ml=97),
    "B = 0": dict(b=0), "F negative": dict(f=-4), "N = 0": dict(n=0), "more than 2^31 rows": dict(f=1 << 16, n=1 << 16),
}
BAD_SEGMENTS = {
    "fp32": dict(dtype=0), "unknown dtype": dict(dtype=7), "q NULL": dict(q=None), "k NULL": dict(k=None), "vt NULL": dict(vt=None),
    "out NULL": dict(out=None), "seg_off NULL": dict(off=None), "no rows": dict(rows=0), "no segments": dict(n_seg=0),
    "bound 0": dict(bound=0), "bound negative": dict(bound=-1), "h = 0": dict(h=0), "Mk = 0": dict(mk=0),
    "Mkp below Mk": dict(mkp=72), "Mkp not a multiple of 8": dict(mk=75, mkp=77, ldvt=80), "head dim 48": dict(d=48, ldq=96,
                                                                                                              ldk=96, ldo=96),
    "scale 0": dict(scale=0.0), "scale inf": dict(scale=float("inf")), "ldq not a multiple of 8": dict(ldq=84),
    "ldq below a row": dict(ldq=72), "ldk not a multiple of 8": dict(ldk=84), "ldvt below Mk": dict(ldvt=72),
    "ldo not a multiple of 4": dict(ldo=82), "ldo below a row": dict(ldo=76), "rows beyond int32": dict(rows=1 << 31),
}


@pytest.mark.parametrize("what", sorted(BAD_ORDER))
def test_frame_order_argument_errors(built, what):
    rc, msg = _frame_order(**BAD_ORDER[what])
    assert rc == EINVAL, (what, rc, msg)
    assert msg.startswith("vtm_frame_order:"), msg


def test_frame_order_workspace_error(built):
    rc, msg = _frame_order(ws_bytes=3 * 4 * 24 * 4 - 1)
    assert rc == -3 and msg.startswith("vtm_frame_order:"), (rc, msg)          # VTM_EWORKSPACE


@pytest.mark.parametrize("what", sorted(BAD_SEGMENTS))
def test_segments_argument_errors(built, what):
    rc, msg = _segments(**BAD_SEGMENTS[what])
    assert rc == EINVAL, (what, rc, msg)
    assert msg.startswith("vtm_attention_kv_segments:") or "head dim" in msg, msg


def test_wrappers_refuse_operands_before_the_library(built):
    from vidtome_amd import _lib
    keep, inv = torch.zeros(B, 5, dtype=torch.int32), torch.zeros(B, F * N, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        _lib.frame_order(keep, inv, F, N)
    fk, fi = keep.as_subclass(FakeCuda), inv.as_subclass(FakeCuda)
    for k2, i2, f2 in ((fk.long(), fi, F), (fk, fi, F + 1), (fk, fi[:2], F), (fk[0], fi, F)):
        with pytest.raises(RuntimeError, match="frame_order takes"):
            _lib.frame_order(k2.as_subclass(FakeCuda), i2.as_subclass(FakeCuda), f2, N)
    q = torch.zeros(10, C, dtype=F32).as_subclass(FakeCuda)
    with pytest.raises(RuntimeError, match="fp16 / bf16"):
        _lib.attention_kv_segments(q, q, q, HEADS, fi, 4, 8, 0.1)


# ---------------------------------------------------------------------------------------------------
# cross_merge_route
# ---------------------------------------------------------------------------------------------------
def _patched(dtype=F16, **kw):
    import vidtome_amd
    unet = standin.StandInUNet(C, HEADS, full=True, cond_dim=D).to(dtype)
    vidtome_amd.apply_patch(unet, batch_size=B, **kw)
    return unet, list(unet.blocks())[-1]


def _tokens(dtype=F16, frames=F):
    return torch.zeros(B * frames, N, C, dtype=dtype).as_subclass(FakeCuda)


def _cond(rows=B * F, dtype=F16):
    return torch.zeros(rows, K, D, dtype=dtype).as_subclass(FakeCuda)


def _plan(local=True):
    from vidtome_amd import patch as vpatch
    plan = vpatch.MergePlan()
    plan.fsize, plan.L = F, F * N
    if local:
        plan.keep = torch.zeros(B, 40, dtype=torch.int32)
        plan.inv_local = torch.zeros(B, F * N, dtype=torch.int32)
    return plan


def test_plan_has_the_frame_order_slot_empty():
    from vidtome_amd import patch as vpatch
    plan = vpatch.MergePlan()
    assert "_frame_order" in vpatch.MergePlan.__slots__ and plan._frame_order is None
    assert plan.frame_order() is None                               # no local level ran: nothing to order, nothing launched


def test_plan_caches_the_frame_order(built, monkeypatch):
    from vidtome_amd import _lib
    calls = []
    monkeypatch.setattr(_lib, "frame_order", lambda keep, inv, f, n: calls.append((keep, inv, f, n)) or ("ks", "inv", "seg"))
    plan = _plan()
    keep, inv = plan.keep, plan.inv_local
    assert plan.frame_order() == ("ks", "inv", "seg") and plan.frame_order() == ("ks", "inv", "seg")
    assert len(calls) == 1 and calls[0][0] is keep and calls[0][1] is inv and calls[0][2:] == (F, N)
    assert plan.keep is keep and plan.inv_local is inv               # merge_mlp keeps using the maps as they are


def _route(blk, x=None, plan="local", route=None, enc="default", mask=None):
    from vidtome_amd import patch as vpatch
    x = _tokens() if x is None else x
    enc = _cond() if isinstance(enc, str) else enc
    plan = _plan() if isinstance(plan, str) else plan
    if route is None:
        route = vpatch.attn2_route(blk, x, enc, mask, {})
    return vpatch.cross_merge_route(blk, x, plan, route, enc, mask)


def test_route_is_merged_panels_on_the_plain_panels_frame(built):
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    unet, blk = _patched()
    x, enc = _tokens(), _cond()
    assert vpatch.attn2_route(blk, x, enc, None, {}) == vpatch.Attn2Route("panels")
    assert _route(blk) == "plain"                                             # flag unset
    for value in (False, 1, "yes"):                                           # only True itself counts
        vidtome_amd.update_patch(unet, merge_crossattn=value)
        assert _route(blk) == "plain"
    vidtome_amd.update_patch(unet, merge_crossattn=True)
    assert _route(blk) == "merged-panels"
    # attn2_route keeps answering what it answered
    assert vpatch.attn2_route(blk, x, enc, None, {}) == vpatch.Attn2Route("panels")
    # bf16 takes it too
    unet16, blk16 = _patched(torch.bfloat16)
    vidtome_amd.update_patch(unet16, merge_crossattn=True)
    assert _route(blk16, x=_tokens(torch.bfloat16), enc=_cond(dtype=torch.bfloat16)) == "merged-panels"


PLAIN = ["no plan", "no local level", "half a map", "blas frame", "f32 frame", "module frame", "IP-Adapter call",
         "AdaLayerNorm block", "encoder_attention_mask", "control registered", "maps registered", "LocalBlend registered",
         "conditioning with one row set", "conditioning with a row set too many", "conditioning is a tuple",
         "2-D conditioning", "another frame count than the plan's", "another token count than the plan's"]


@pytest.mark.parametrize("what", PLAIN)
def test_route_is_plain(built, what):
    import vidtome_amd
    from vidtome_amd import patch as vpatch
    unet, blk = _patched()
    vidtome_amd.update_patch(unet, merge_crossattn=True)
    assert _route(blk) == "merged-panels"
    kw = {}
    if what == "no plan":
        kw["plan"] = None
    elif what == "no local level":
        kw["plan"] = _plan(local=False)
    elif what == "half a map":
        kw["plan"] = _plan()
        kw["plan"].inv_local = None
    elif what.endswith(" frame"):
        kw["route"] = vpatch.Attn2Route(what.split()[0])
    elif what == "IP-Adapter call":
        kw["route"] = vpatch.Attn2Route("panels", object())
    elif what == "AdaLayerNorm block":
        blk.use_ada_layer_norm = True
        kw["route"] = vpatch.Attn2Route("panels")                     # (attn2_route never says so for such a block)
    elif what == "encoder_attention_mask":
        kw["mask"] = torch.zeros(B * F, 1, K, dtype=F16).as_subclass(FakeCuda)
        kw["route"] = vpatch.Attn2Route("panels")
    elif what == "control registered":
        blk.vtm_cross_control = ([981], 4, {}, "block")               # registered; whether this step injects does not matter
    elif what == "maps registered":
        blk.vtm_attention_maps = True
    elif what == "LocalBlend registered":
        blk.vtm_local_blend = (object(), "block")
    elif what == "conditioning with one row set":
        kw["enc"] = _cond(1)
        kw["route"] = vpatch.Attn2Route("panels")
    elif what == "conditioning with a row set too many":
        kw["enc"] = _cond(B * F + 1)
        kw["route"] = vpatch.Attn2Route("panels")
    elif what == "conditioning is a tuple":
        kw["enc"] = (_cond(), [_cond()])
        kw["route"] = vpatch.Attn2Route("panels")
    elif what == "2-D conditioning":
        kw["enc"] = torch.zeros(B * F, D, dtype=F16).as_subclass(FakeCuda)
        kw["route"] = vpatch.Attn2Route("panels")
    elif what == "another frame count than the plan's":
        kw["x"], kw["enc"], kw["route"] = _tokens(frames=2), _cond(B * 2), vpatch.Attn2Route("panels")
    elif what == "another token count than the plan's":
        kw["x"] = torch.zeros(B * F, N + 8, C, dtype=F16).as_subclass(FakeCuda)
        kw["route"] = vpatch.Attn2Route("panels")
    assert _route(blk, **kw) == "plain"


def test_route_launches_nothing(built, monkeypatch):
    """Every wrapper the merged segment uses is replaced by one that fails: cross_merge_route still answers."""
    import vidtome_amd
    from vidtome_amd import _lib
    unet, blk = _patched()
    vidtome_amd.update_patch(unet, merge_crossattn=True)

    def boom(*a, **k):
        raise AssertionError("cross_merge_route called into the library")
    for name in ("frame_order", "layernorm_gather", "layernorm_panels", "linear_panels", "to_panels", "attention_kv_segments",
                 "attention_kv", "unmerge_add", "gather_rows"):
        monkeypatch.setattr(_lib, name, boom)
    assert _route(blk) == "merged-panels"
    assert _route(blk, plan=None) == "plain"


# ---------------------------------------------------------------------------------------------------
# the block forward: the plan of THIS forward reaches attn2 on a local, nothing is kept on the module
# ---------------------------------------------------------------------------------------------------
def _stub_forward(monkeypatch, seen):
    from vidtome_amd import patch as vpatch

    def segment(block, hs, *a, **kw):
        seen["segment_kw"] = dict(kw)
        if "plan_to" in kw:
            seen["plan"] = _plan()
            kw["plan_to"].append(seen["plan"])
        return hs

    def merged(block, hs, enc, plan):
        seen["merged"] = (enc, plan)
        return hs + 1

    monkeypatch.setattr(vpatch, "self_attention_segment", segment)
    monkeypatch.setattr(vpatch, "merged_cross_attention_residual", merged)
    monkeypatch.setattr(vpatch, "norm_cross_attention_residual", lambda norm, attn, hs, enc, *a: hs + 2)
    monkeypatch.setattr(vpatch, "norm_feed_forward_residual", lambda norm, ff, hs: hs + 10)
    monkeypatch.setattr(vpatch, "merged_feed_forward_residual", lambda block, hs, plan, route: hs + 20)


def test_forward_hands_this_forwards_plan_to_attn2(built, monkeypatch):
    import vidtome_amd
    unet, blk = _patched()
    seen = {}
    _stub_forward(monkeypatch, seen)
    x, enc = _tokens(), _cond()
    # flag unset: the segment is called as before (no new keyword), attn2 and the feed-forward are today's
    assert torch.equal(blk(x, encoder_hidden_states=enc), x + 12) and seen["segment_kw"] == {} and "merged" not in seen
    before = set(blk.__dict__)
    vidtome_amd.update_patch(unet, merge_crossattn=True)
    y = blk(x, encoder_hidden_states=enc)
    assert torch.equal(y, x + 11)                                         # merged attn2, today's feed-forward
    assert seen["merged"][0] is enc and seen["merged"][1] is seen["plan"]
    assert set(blk.__dict__) - before == {"merge_crossattn"}              # nothing of the forward stays on the module
    first = seen["plan"]
    blk(x, encoder_hidden_states=enc)
    assert seen["merged"][1] is seen["plan"] and seen["plan"] is not first
    vidtome_amd.update_patch(unet, merge_mlp=True)                         # both: one plan serves attn2 and the feed-forward
    assert torch.equal(blk(x, encoder_hidden_states=enc), x + 21)
    vidtome_amd.update_patch(unet, merge_crossattn=False)                  # merge_mlp alone: attn2 is today's
    assert torch.equal(blk(x, encoder_hidden_states=enc), x + 22)
    # a masked call stays on today's attn2 with the flag set
    vidtome_amd.update_patch(unet, merge_crossattn=True, merge_mlp=False)
    mask = torch.zeros(B * F, 1, K, dtype=F16).as_subclass(FakeCuda)
    assert torch.equal(blk(x, encoder_hidden_states=enc, encoder_attention_mask=mask), x + 12)


def test_flag_life_cycle(built):
    import vidtome_amd
    unet, blk = _patched()
    assert not any(hasattr(b, "merge_crossattn") for b in unet.blocks())
    assert vidtome_amd.update_patch(unet, merge_crossattn=True) is unet
    assert all(b.merge_crossattn is True for b in unet.blocks())
    vidtome_amd.remove_patch(unet)
    assert not any(hasattr(b, "merge_crossattn") for b in unet.blocks())
    vidtome_amd.apply_patch(unet, batch_size=B)
    assert not any(hasattr(b, "merge_crossattn") for b in unet.blocks())
    vidtome_amd.update_patch(unet, merge_crossattn=True, merge_mlp=True)
    vidtome_amd.apply_patch(unet, batch_size=B)                            # apply_patch removes first: starts without it too
    assert not any(hasattr(b, "merge_crossattn") or hasattr(b, "merge_mlp") for b in unet.blocks())
    vidtome_amd.remove_patch(unet)
