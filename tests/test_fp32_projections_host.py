"""CPU checks of the fp32 projection GEMMs (csrc/linear_f32.hip, `update_patch(model, fp32_projections=True)`): the export
is declared, exported and bound, its argument checks (and vtm_linear_rows' forwarding of VTM_F32) answer without a launch,
the switch reaches every patched block and leaves nothing behind, and every kernel instantiation cross-compiles for gfx950
onto the f32 MFMA with no 16-bit operand, no conversion but the fp16 store's, and no scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "vidtome_amd", "csrc", "linear_f32.hip")


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


def test_export_is_declared_exported_and_bound(built):
    from vidtome_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vidtome_hip.h")).read()
    assert re.search(r"\bint vtm_linear_f32\s*\(", hdr)
    assert "vtm_linear_f32" in _lib.exported_symbols()
    assert hasattr(ctypes.CDLL(built), "vtm_linear_f32")
    assert _lib.lib().vtm_linear_f32.argtypes is not None
    assert _lib.ABI_VERSION == 2 and _lib.lib().vtm_version() == 2
    assert "linear_f32.hip" in __import__("vidtome_amd.build", fromlist=["SOURCES"]).SOURCES


def _f32(L, K=32, N=32, n=1, epi=0, resid=None, out_dtype=0, W=16, transposed=0, ldo=None):
    """vtm_linear_f32 on fake (never dereferenced) pointers: every call here must be refused or finish before a launch."""
    ldo = (n if transposed else (N // 2 if epi == 2 else N)) if ldo is None else ldo
    return L.lib().vtm_linear_f32(16, 64, None, 0, 1, K, None, 0, None, n, W, None, N, epi, resid, 16, out_dtype, ldo,
                                  64 * ldo, transposed, None)


def _err(L):
    msg = L.lib().vtm_last_error()
    return msg.decode() if msg else ""


def test_argument_checks_answer_without_a_launch(built):
    from vidtome_amd import _lib as L
    assert _f32(L, n=0) == 0                                  # nothing to do: no launch
    assert _f32(L, n=0, epi=2, N=64) == 0
    assert _f32(L, n=0, out_dtype=L.VTM_F16, transposed=1) == 0
    assert _f32(L, K=12) < 0 and "K=12" in _err(L)
    assert _f32(L, N=12) < 0 and "N=12" in _err(L)
    assert _f32(L, epi=3) < 0 and "epilogue" in _err(L)
    assert _f32(L, epi=1) < 0 and "resid" in _err(L)        # RESID without resid
    assert _f32(L, epi=2, N=40) < 0 and "GEGLU" in _err(L)  # D = 20 is not a multiple of 8
    assert _f32(L, out_dtype=L.VTM_BF16) < 0 and "out_dtype" in _err(L)
    assert _f32(L, W=20) < 0 and "aligned" in _err(L)
    assert _f32(L, ldo=16) < 0 and "ldo" in _err(L)


def test_linear_rows_forwards_f32(built):
    """vtm_linear_rows no longer rejects VTM_F32: it reaches vtm_linear_f32's own checks (a misaligned weight here), where
    it used to stop at the dtype."""
    from vidtome_amd import _lib as L
    args = dict(x0=16, P0=64, x1=None, P1=0, B=1, K=32, rows=None, rows_ld=0, rows2=None, n=1, b=None, N=32, out=16, ldo=32,
                obs=64 * 32, tr=0, s=None)

    def call(dtype, W):
        a = args
        return L.lib().vtm_linear_rows(a["x0"], a["P0"], a["x1"], a["P1"], dtype, a["B"], a["K"], a["rows"], a["rows_ld"],
                                       a["rows2"], a["n"], W, a["b"], a["N"], a["out"], a["ldo"], a["obs"], a["tr"], a["s"])
    assert call(L.VTM_F32, 20) < 0
    msg = _err(L)
    assert "vtm_linear_f32" in msg and "aligned" in msg and "dtype" not in msg
    assert call(7, 16) < 0 and "dtype" in _err(L)


class _ControlNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from standin import BasicTransformerBlock
        self.blocks = torch.nn.ModuleList([BasicTransformerBlock(16, 2) for _ in range(2)])


class DiffusionPipeline:                          # apply_patch tests class NAMES in the MRO
    def __init__(self, unet):
        self.unet = unet


class StableDiffusionControlNetPipeline(DiffusionPipeline):
    def __init__(self, unet, controlnet):
        self.unet, self.controlnet = unet, controlnet


def _blocks(root):
    return [m for m in root.modules() if m.__class__.__name__ == "ToMeBlock"]


def test_update_patch_reaches_every_patched_block_controlnet_included(built):
    import vidtome_amd
    from standin import StandInUNet
    unet, cn = StandInUNet(16, 2), _ControlNet()
    pipe = StableDiffusionControlNetPipeline(unet, cn)
    vidtome_amd.apply_patch(pipe, include_control=True)
    blocks = _blocks(unet) + _blocks(cn)
    assert len(_blocks(unet)) == 9 and len(_blocks(cn)) == 2
    assert not any(getattr(b, "fp32_projections", False) for b in blocks)    # off unless asked for
    vidtome_amd.update_patch(pipe, fp32_projections=True)
    assert all(b.fp32_projections is True for b in blocks)
    vidtome_amd.update_patch(pipe, fp32_projections=False)
    assert not any(b.fp32_projections for b in blocks)


def test_remove_patch_leaves_no_flag_for_a_later_apply_patch(built):
    import vidtome_amd
    from standin import StandInUNet
    unet = StandInUNet(16, 2)
    vidtome_amd.apply_patch(unet)
    vidtome_amd.update_patch(unet, fp32_projections=True, fp32_attention=True)
    vidtome_amd.remove_patch(unet)
    assert not any("fp32_projections" in m.__dict__ or "fp32_attention" in m.__dict__ for m in unet.modules())
    vidtome_amd.apply_patch(unet)
    assert not any(getattr(b, "fp32_projections", False) for b in _blocks(unet))
    vidtome_amd.remove_patch(unet)


def test_the_switch_is_not_an_apply_patch_argument():
    import inspect
    import vidtome_amd
    assert "fp32_projections" not in inspect.signature(vidtome_amd.apply_patch).parameters


@pytest.fixture(scope="module")
def f32_asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    from vidtome_amd import build
    out = tmp_path_factory.mktemp("asm") / "linear_f32.s"
    flags = [f for f in build.FLAGS if f not in ("-fPIC",)]
    subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", SRC, "-o", str(out)], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return out.read_text()


def _kernel_bodies(asm):
    """{(waves along M, transposed, epilogue, output type): (symbol, assembly)} of every linear_f32_kernel instantiation."""
    out = {}
    lines = asm.splitlines()
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN\S*17linear_f32_kernelILi(\d)ELb(\d)ELi(\d)E(f|6__half)EE\S*):\s*(;.*)?$", l)
        if m:
            end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))   # (several s_endpgm)
            key = (int(m.group(2)), int(m.group(3)), int(m.group(4)), "f16" if m.group(5) == "6__half" else "f32")
            out[key] = (m.group(1), "\n".join(lines[i:end + 1]))
    return out


def test_every_instantiation_runs_on_the_f32_mfma(f32_asm):
    bodies = _kernel_bodies(f32_asm)
    assert len(bodies) == 2 * 2 * 3 * 2                      # tile x orientation x epilogue x output type
    for key, (_, body) in bodies.items():
        assert re.search(r"v_mfma_f32_(32x32x2|16x16x4)_f32", body), key
        assert not re.search(r"v_mfma_\S+_(f16|bf16)\b", body), key
        # the fp16 output is the fp32 value rounded once: no mixed-precision multiply-add folded into the conversion
        assert not re.search(r"v_(fma|mad)_mix", body), key
        cvt = re.search(r"v_cvt_(pk_)?(f16|bf16)_f32|v_cvt_pk_rtz_f16", body)
        if key[3] == "f32":
            assert not cvt, key                              # operands and results stay fp32
        else:
            assert cvt, key                                  # the VTM_F16 output is rounded at the store


def test_no_scratch_in_any_instantiation(f32_asm):
    names = {sym: key for key, (sym, _) in _kernel_bodies(f32_asm).items()}
    assert len(names) == 24
    for sym in names:
        m = re.search(r"\.amdhsa_kernel " + re.escape(sym) + r"\n(.*?)\.end_amdhsa_kernel", f32_asm, re.S)
        assert m, sym
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", m.group(1)), sym
    meta = f32_asm[f32_asm.index("amdhsa.kernels"):]
    seen = 0
    for block in re.split(r"\n  - ", meta):
        nm = re.search(r"\.name:\s+(\S+)", block)
        if nm and nm.group(1) in names:
            seen += 1
            assert re.search(r"\.private_segment_fixed_size:\s+0\b", block), nm.group(1)
            assert re.search(r"\.vgpr_spill_count:\s+0\b", block), nm.group(1)
            assert re.search(r"\.sgpr_spill_count:\s+0\b", block), nm.group(1)
    assert seen == 24
