"""Which projection kernels a patched block call runs, against a literal table of attn1's routes (patch.attn1_route): one
call of the self-attention segment per row -- batch 2, 4 frames, latent 16 x 16 (256 tokens per frame; 64 at the sites that
do not merge), local_merge_ratio 0.5 -- with the vidtome_amd._lib wrappers spied (every spy calls through).  The rows are
built by tools/block_digest.py, whose digest of the same calls is what profiles/patch_routes_bitwise.txt compares."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

# what ran, per route: (wrappers that must have run, wrappers that must not have)
RAN = {
    "rows": ({"linear_rows"}, {"linear_panels", "linear_f32"}),
    "panels": ({"gather_panels", "linear_panels"}, {"linear_rows", "linear_f32"}),
    "panels, un-merged": ({"layernorm_panels", "linear_panels", "transpose_cols"}, {"gather_panels", "linear_rows", "linear_f32"}),
    "f32": ({"linear_f32"}, {"linear_rows", "linear_panels"}),
    "blas": ({"attention"}, {"linear_rows", "linear_panels", "linear_f32"}),
    "module": (set(), {"linear_rows", "linear_panels", "linear_f32", "attention", "attention_kv"}),
}
EXPECTED = {
    "fp16 C=320 heads 8": "rows",
    "fp16 C=64 heads 8": "rows",
    "bf16 C=320": "rows",
    "fp16 C=640": "panels",
    "fp16 C=640 bias on to_v": "blas",
    "fp16 C=480 heads 12": "blas",                  # C % 32 == 0, C % 64 != 0, C > 320
    "fp16 block, fp32 to_out": "blas",
    "fp32 C=320": "blas",
    "fp32 C=320 fp32_projections": "f32",
    "PROJ_MODE=rows C=640": "rows",
    "PROJ_MODE=panels C=320": "panels",
    "PROJ_MODE=blas C=320": "blas",
    "un-merged fp16 C=640": "panels, un-merged",    # unmerged_self_attention_residual
    "un-merged fp16 C=320": "rows",
    "PnP sharing fp16 C=320": "rows",
    "attention_mask given": "module",
}


@pytest.fixture(scope="module")
def digest():
    spec = importlib.util.spec_from_file_location(
        "block_digest", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "block_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_table_names_every_case(digest):
    assert set(EXPECTED) == set(digest.ROUTE_CASES)


@pytest.mark.filterwarnings("ignore:vidtome_amd")
@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_block_call_takes_its_route(digest, case, monkeypatch):
    import vidtome_amd
    from vidtome_amd import _lib
    from vidtome_amd import patch as vpatch
    monkeypatch.setattr(vpatch, "_warned", set())          # (the "blas" rows say once what they are: not this test's trace)
    expected = EXPECTED[case]
    torch.manual_seed(123)
    unet, blk, h, mask, restore = digest.route_case(vidtome_amd, case)
    try:
        assert vpatch.attn1_route(blk, h, None, mask, None) == expected.split(",")[0]
        with torch.no_grad(), digest.Spy(_lib) as spy:
            out = vpatch.self_attention_segment(blk, h, None, mask, None)
        torch.cuda.synchronize()
    finally:
        restore()
    ran, must, must_not = set(spy.calls), *RAN[expected]
    assert must <= ran and not (must_not & ran), (case, expected, spy.calls)
    assert getattr(blk.attn1, "calls", 0) == (1 if expected == "module" else 0)      # attn1's own forward
    assert out.shape == h.shape and out.dtype == h.dtype and bool(torch.isfinite(out).all())
