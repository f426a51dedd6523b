"""CPU tests of attention broadcast (vidtome_amd/broadcast.py, csrc/broadcast.hip): the schedule against an independent
restatement of the rule, the C ABI surface, the constructor's / set_frames' / the block helper's refusals, what the library
refuses before any launch, and the kernels' resource figures.  The GPU side is tests/test_gpu_broadcast.py."""
import ctypes
import os
import re

import pytest
import torch

import broadcast_ref as R
import standin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vidtome_amd", "csrc")
EXPORTS = {"vtm_residual_record": 10, "vtm_residual_replay": 11, "vtm_residual_replay_layernorm": 17}
T50 = list(range(981, 0, -20))          # 981, 961, ..., 1: 50 steps
T4 = [999, 666, 333, 0]
EVERY = (None, 1, 2, 6)
WINDOWS = ((100, 800), (1000, 2000), (-1, 1001))      # the default, one that contains no step, one that contains every step


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


# ---------------------------------------------------------------------------------------------------
# the schedule
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", WINDOWS, ids=str)
@pytest.mark.parametrize("every", EVERY, ids=str)
@pytest.mark.parametrize("timesteps", [T50, T4], ids=["50steps", "4steps"])
def test_modes_follow_the_rule(timesteps, every, window):
    from vidtome_amd import AttentionBroadcast
    assert len(T50) == 50 and T50[0] == 981 and T50[-1] == 1
    other = 6 if every != 6 else 2
    bc = AttentionBroadcast(timesteps, 3, attn1_every=every, attn2_every=other, attn1_window=window, attn2_window=(100, 800))
    swapped = AttentionBroadcast(torch.tensor(timesteps), 3, attn1_every=other, attn2_every=every, attn1_window=(100, 800),
                                 attn2_window=window)
    n = len(timesteps)
    got = [bc.modes(i) for i in range(n)]
    for i in range(n):
        want = (R.mode(i, timesteps, every, window), R.mode(i, timesteps, other, (100, 800)))
        assert got[i] == want and swapped.modes(i) == want[::-1], (i, got[i], want)
    m = [g[0] for g in got]
    assert m[0] != "reuse"                                                   # nothing is cached at the first step
    if every in (None, 1):
        assert set(m) == {"compute"}                                         # off; every step recomputes
    for i in range(n):
        if m[i] == "record":
            assert i + 1 < n and m[i + 1] == "reuse"                         # a record is always read by the next step
        if m[i] == "reuse":
            assert m[i - 1] in ("record", "reuse")                           # ... and a reuse has one immediately before it
    if window == (1000, 2000):
        assert set(m) == {"compute"}
    if window == (-1, 1001) and every in (2, 6):
        assert [x == "reuse" for x in m] == [i > 0 and i % every != 0 for i in range(n)]
    if timesteps is T50 and every == 2 and window == (100, 800):
        # t = 781 (i = 10) is the first step inside the window, t = 101 (i = 44) the last
        assert m[9] == "compute" and m[10] == "record" and m[11] == "reuse" and m[12] == "record" and m[43] == "reuse"
        assert m[44] == "compute" and set(m[45:]) == {"compute"}
    for bad in (-1, n, 1.5, True):
        with pytest.raises(ValueError, match="does not lie in"):
            bc.modes(bad)


def test_constructor_and_set_frames_refuse():
    from vidtome_amd import AttentionBroadcast
    for kwargs, word in ((dict(timesteps=[]), "non-empty"), (dict(timesteps=[1.0, float("nan")]), "finite"),
                         (dict(num_frames=0), "num_frames"), (dict(attn1_every=0), "attn1_every"),
                         (dict(attn2_every=True), "attn2_every"), (dict(attn1_every=2.5), "attn1_every"),
                         (dict(attn1_window=(800, 100)), "attn1_window"), (dict(attn2_window=(1, 2, 3)), "attn2_window"),
                         (dict(attn2_window=5), "attn2_window"), (dict(attn1_window=(float("nan"), 1)), "attn1_window")):
        args = dict(timesteps=T4, num_frames=4)
        args.update(kwargs)
        with pytest.raises(ValueError, match=word):
            AttentionBroadcast(**args)
    bc = AttentionBroadcast(T4, 5)
    assert bc.every == (2, 6) and bc.windows == ((100.0, 800.0), (100.0, 800.0)) and bc.nbytes() == 0
    for ids in ([], [0, 0], [-1], [5], [1, 2, 5]):
        with pytest.raises(ValueError, match="distinct and lie in 0 .. 4"):
            bc.set_frames(ids)
    bc.set_frames([4, 0, 2])
    bc.set_frames(None)
    with pytest.raises(ValueError, match="does not lie in"):
        bc.set_step(4)
    with pytest.raises(RuntimeError, match="set_step"):
        bc.step_modes("blk")
    bc.set_step(1)
    assert bc.step_modes("blk") == bc.modes(1) == ("reuse", "reuse")
    with pytest.raises(RuntimeError, match="recorded no attn1"):
        bc.cache("blk", "attn1")
    with pytest.raises(ValueError, match="kind"):
        bc.cache("blk", "ff")
    # the chunk: a batch that is no multiple of the frames, hidden states that are not (B F, N, C)
    bc.set_frames([4, 0, 2])
    with pytest.raises(RuntimeError, match="not a multiple of the chunk's 3 frames"):
        bc.replay("blk", ("attn1",), torch.zeros(4, 2, 8))
    with pytest.raises(RuntimeError, match=r"must be \(B F, N, C\)"):
        bc.replay("blk", ("attn1",), torch.zeros(3, 8))
    # a reuse of frames nobody recorded: host bookkeeping alone
    with pytest.raises(RuntimeError, match=r"frames \[0, 2, 4\] were not recorded at step 0"):
        bc.replay("blk", ("attn1",), torch.zeros(6, 2, 8))
    bc.reset()
    with pytest.raises(RuntimeError, match="set_step"):
        bc.step_modes("blk")


# ---------------------------------------------------------------------------------------------------
# registration and the block's helper (nothing is launched)
# ---------------------------------------------------------------------------------------------------
def test_registration_marker_and_the_forward_refusals(built):
    import vidtome_amd
    from vidtome_amd import AttentionBroadcast, patch as vpatch
    unet = standin.StandInUNet(64, 2, full=True, cond_dim=32)
    bc = AttentionBroadcast(T4, 4, attn1_every=2, attn2_every=2, attn1_window=(0, 1000), attn2_window=(0, 1000))
    with pytest.raises(RuntimeError, match="nothing is patched"):
        vidtome_amd.register_attention_broadcast(unet, bc)
    vidtome_amd.apply_patch(unet)
    try:
        with pytest.raises(TypeError, match="AttentionBroadcast"):
            vidtome_amd.register_attention_broadcast(unet, object())
        with pytest.raises(ValueError, match="not patched blocks"):
            vidtome_amd.register_attention_broadcast(unet, bc, blocks=["nope"])
        blocks = list(unet.blocks())
        names = [n for n, m in unet.named_modules() if m in blocks]
        assert vidtome_amd.register_attention_broadcast(unet, bc) == sorted(names)
        assert all(b.__dict__["vtm_broadcast"] == (bc, n) for b, n in zip(blocks, names))
        assert vidtome_amd.register_attention_broadcast(unet, bc, blocks=names[:2]) == sorted(names[:2])
        assert [("vtm_broadcast" in b.__dict__) for b in blocks] == [True, True] + [False] * 7
        blk, name = blocks[0], names[0]
        assert vpatch.broadcast_modes(blocks[2]) == vpatch._NO_BROADCAST == (None, "", "compute", "compute")
        with pytest.raises(RuntimeError, match="set_step"):
            vpatch.broadcast_modes(blk)
        bc.set_step(0)
        assert vpatch.broadcast_modes(blk) == (bc, name, "record", "record")
        bc.set_step(1)
        assert vpatch.broadcast_modes(blk) == (bc, name, "reuse", "reuse")
        # every consumer that would miss a map, with the block's name
        for attr, value, word in (("vtm_attention_maps", True, "attention maps"), ("vtm_local_blend", (object(), name), "LocalBlend"),
                                  ("vtm_cross_control", object(), "cross-attention control"), ("vtm_sag", True, "self-attention guidance")):
            blk.__dict__[attr] = value
            with pytest.raises(RuntimeError, match=re.escape(f"block '{name}'") + ".*" + word):
                vpatch.broadcast_modes(blk)
            bc.set_step(0)
            assert vpatch.broadcast_modes(blk)[2:] == ("record", "record")        # (only a reuse step misses it)
            bc.set_step(1)
            del blk.__dict__[attr]
        for flag in ("use_ada_layer_norm", "use_ada_layer_norm_zero"):
            setattr(blk, flag, True)
            with pytest.raises(RuntimeError, match=re.escape(f"block '{name}'") + ".*AdaLayerNorm"):
                vpatch.broadcast_modes(blk)
            setattr(blk, flag, False)
        attn2, blk.attn2 = blk.attn2, None
        assert vpatch.broadcast_modes(blk)[2:] == ("reuse", "compute")           # no attn2: nothing of it to replay
        blk.attn2 = attn2
        vidtome_amd.unregister_attention_broadcast(unet)
        assert not any("vtm_broadcast" in b.__dict__ for b in blocks)
        vidtome_amd.register_attention_broadcast(unet, bc, blocks=lambda n, b: n == names[3])
        assert [("vtm_broadcast" in b.__dict__) for b in blocks] == [i == 3 for i in range(9)]
    finally:
        vidtome_amd.remove_patch(unet)
    assert not any("vtm_broadcast" in b.__dict__ for b in unet.blocks())
    src = open(os.path.join(ROOT, "vidtome_amd", "patch.py")).read()
    body = src[src.index("def remove_patch"):src.index("def update_patch")]
    assert body.index('pop("vtm_broadcast"') > body.index("pop(pag.MARK")       # added after the existing lines


# ---------------------------------------------------------------------------------------------------
# the C ABI surface
# ---------------------------------------------------------------------------------------------------
def test_header_declares_what_the_binding_lists(built):
    import vidtome_amd
    from vidtome_amd import _lib, broadcast, build
    hdr = open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    declared = re.findall(r"^(?:const char \*|int64_t |size_t |int )(vtm_\w+)\(", hdr, re.M)
    assert sorted(declared) == _lib.exported_symbols() and len(set(declared)) == len(declared)
    so = ctypes.CDLL(built)
    for name, count in EXPORTS.items():
        decl = re.search(r"^int %s\((.*?)\);" % name, hdr, re.S | re.M)
        assert decl and len(decl.group(1).split(",")) == len(_lib._SIGNATURES[name][0]) == count, name
        assert hasattr(so, name)
    assert re.search(r"#define VTM_ABI_VERSION 2\b", hdr) and _lib.lib().vtm_version() == _lib.ABI_VERSION == 2     # additive
    doc = hdr[hdr.index("Attention broadcast --"):hdr.index("int vtm_residual_record(")]
    for word in ("NOT checked", "distinct", "BIT-EQUAL to vtm_layernorm_panels", "C % 64 == 0", "C <= 2048", "out may be h",
                 "cache2 (may be NULL)", "VTM_EINVAL", "intermediate rounding"):
        assert word in doc, word
    assert "broadcast.hip" in build.SOURCES
    for name in ("AttentionBroadcast", "register_attention_broadcast", "unregister_attention_broadcast"):
        assert name in vidtome_amd.__all__ and getattr(vidtome_amd, name) is getattr(broadcast, name)
    for fn in ("residual_record", "residual_replay", "residual_replay_layernorm"):
        assert callable(getattr(_lib, fn))
    # the fused kernel picks its LayerNorm family by layernorm.hip's own condition, and takes the row pieces from the header
    # the LayerNorm kernels take them from
    text = open(os.path.join(CSRC, "broadcast.hip")).read()
    cond = "if (C == 320 || C == 640 || (C == 1280 && rows >= 32768)) {"
    assert cond in text and cond in open(os.path.join(CSRC, "layernorm.hip")).read()
    assert '#include "layernorm_row.h"' in text and "__builtin_nontemporal" not in text and "ld16<true>" not in text
    assert '#include "layernorm_row.h"' in open(os.path.join(CSRC, "layernorm.hip")).read()


def test_kernels_use_no_scratch(built):
    """2 elementwise kernels x 3 dtypes x (16-byte | element) accesses, the fused kernel's wave-per-row family (1 .. 4 pieces
    per lane) and lanes-per-row family (8 / 16 / 32 lanes) x 2 dtypes: no scratch memory, no spilled register, no LDS -- and
    layernorm.o, whose helpers moved to a header, keeps every kernel it had, none with scratch."""
    from vidtome_amd import build
    lib = os.path.dirname(built)
    res = build.kernel_resources(os.path.join(lib, "broadcast.o"))
    count = lambda word: len([k for k in res if word in k])
    assert count("residual_record_kernel") == 6 and count("residual_replay_kernel") == 6
    assert count("replay_layernorm_kernel") == 8 and count("replay_layernorm_rows_kernel") == 6 and len(res) == 26
    for name, r in res.items():
        print(name, r)
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r.get("group_segment_fixed_size", 0) == 0 and r["vgpr_count"] <= 128, (name, r)     # (4 waves per SIMD and more)
    ln = build.kernel_resources(os.path.join(lib, "layernorm.o"))
    assert len(ln) == 84
    assert all(r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 for r in ln.values())


def test_library_refuses_before_any_launch(built):
    """VTM_EINVAL comes back before anything is launched, so no GPU is needed to see it (the pointers are never followed)."""
    from vidtome_amd import _lib
    L = _lib.lib()
    p, q, r, s = (i << 24 for i in (1, 2, 3, 4))                          # non-null, 16-byte aligned, far apart

    def refused(rc, word):
        msg = L.vtm_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg, word)

    ok = dict(h_in=p, h_out=q, cache=r, ids=None, dtype=1, G=2, Fg=3, nf=5, E=64)
    for change, word in ((dict(dtype=3), "unsupported dtype"), (dict(Fg=6), "bad sizes"), (dict(Fg=0), "bad sizes"),
                         (dict(G=0), "bad sizes"), (dict(E=0), "bad sizes"), (dict(cache=None), "are required"),
                         (dict(h_in=None), "are required"), (dict(cache=p + 64), "overlaps"), (dict(cache=q), "overlaps")):
        a = dict(ok, **change)
        refused(L.vtm_residual_record(a["h_in"], a["h_out"], a["cache"], a["ids"], a["dtype"], a["G"], a["Fg"], a["nf"], a["E"],
                                      None), word)
    ok = dict(h=p, c1=q, c2=None, ids=None, dtype=2, G=2, Fg=3, nf=5, E=64, out=r)
    for change, word in ((dict(dtype=-1), "unsupported dtype"), (dict(Fg=6), "bad sizes"), (dict(c1=None), "are required"),
                         (dict(out=None), "are required"), (dict(out=q), "overlaps a cache"), (dict(c2=r), "overlaps a cache"),
                         (dict(out=p + 2), "without being h")):
        a = dict(ok, **change)
        refused(L.vtm_residual_replay(a["h"], a["c1"], a["c2"], a["ids"], a["dtype"], a["G"], a["Fg"], a["nf"], a["E"], a["out"],
                                      None), word)
    rows = 2 * 3 * 7
    ok = dict(h=p, c1=q, c2=None, ids=None, gamma=None, beta=None, dtype=1, G=2, Fg=3, nf=5, N=7, C=64, rows=r, panels=s,
              pr=_lib.panel_rows(rows))
    for change, word in ((dict(dtype=0), "VTM_F16 or VTM_BF16"), (dict(C=72), "multiple of 64"), (dict(C=2112), "multiple of 64"),
                         (dict(N=0), "multiple of 64"), (dict(Fg=6), "bad sizes"), (dict(panels=None), "are required"),
                         (dict(pr=rows), "vtm_panel_rows"), (dict(h=p + 2), "16-byte aligned"), (dict(gamma=p + 8), "16-byte aligned"),
                         (dict(rows=q), "overlaps a cache"), (dict(rows=p + 16), "without being h"),
                         (dict(panels=p), "out_panels overlaps"), (dict(panels=q + 16), "out_panels overlaps")):
        a = dict(ok, **change)
        refused(L.vtm_residual_replay_layernorm(a["h"], a["c1"], a["c2"], a["ids"], a["gamma"], a["beta"], 1e-5, a["dtype"], a["G"],
                                                a["Fg"], a["nf"], a["N"], a["C"], a["rows"], a["panels"], a["pr"], None), word)
