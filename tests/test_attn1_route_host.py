"""CPU tests of attn1's routing (patch.attn1_route) and of the guard on query rows under PnP shared probabilities
(patch._attn1_params): no GPU, no launch."""
import pytest
import torch

import standin

C, HEADS, B, N = 64, 2, 3, 16


class FakeCuda(torch.Tensor):          # the predicates need x.is_cuda; emulate it without a device
    @property
    def is_cuda(self):
        return True


def _x(dtype=torch.float16, c=C):
    return torch.zeros(B, N, c, dtype=dtype).as_subclass(FakeCuda)


def _block(c=C, heads=HEADS, dtype=torch.float16):
    return standin.BasicTransformerBlock(c, heads).to(dtype)


class Wrapper(torch.nn.Module):
    """A projection wrapper lora.recognise does not know."""

    def __init__(self, lin):
        super().__init__()
        self.inner = lin


def test_routes_of_a_plain_block():
    from vidtome_amd import patch as vpatch
    assert vpatch.attn1_route(_block(), _x()) == "rows"
    assert vpatch.attn1_route(_block(dtype=torch.float32), _x(torch.float32)) == "blas"
    blk = _block(dtype=torch.float32)
    blk.fp32_projections = True
    assert vpatch.attn1_route(blk, _x(torch.float32)) == "f32"


def test_module_route():
    from vidtome_amd import patch as vpatch
    blk, x = _block(), _x()
    assert vpatch.attn1_route(blk, torch.zeros(B, N, C, dtype=torch.float16)) == "module"             # a CPU tensor
    for mask in (torch.zeros(B, 1, N, dtype=torch.float16), torch.ones(B, N, dtype=torch.bool), [[0.0] * N] * B):
        assert vpatch.attn1_route(blk, x, None, mask) == "module"                                      # any non-None mask
    assert vpatch.attn1_route(blk, x, None, None, {"scale": 1.0}) == "module"
    assert vpatch.attn1_route(blk, x, None, None, {"scale": 1.0, "ip_adapter_masks": []}) == "module"
    enc = torch.zeros(B, 77, C, dtype=torch.float16)
    assert vpatch.attn1_route(blk, x, enc) == "rows"                          # conditioning alone: attn1 does not read it
    blk.only_cross_attention = True
    assert vpatch.attn1_route(blk, x, enc) == "module"
    assert vpatch.attn1_route(blk, x) == "rows"
    wrapped = _block()
    wrapped.attn1.to_k = Wrapper(wrapped.attn1.to_k)
    assert vpatch.attn1_route(wrapped, x) == "module"                         # an unrecognised projection wrapper
    assert 24 not in vpatch._HEAD_DIMS
    assert vpatch.attn1_route(_block(48, 2), _x(c=48)) == "module"            # a head dim without a kernel instantiation


def test_region_masks_alone_do_not_change_the_route():
    from vidtome_amd import patch as vpatch
    for blk, x in ((_block(), _x()), (_block(dtype=torch.float32), _x(torch.float32))):
        plain = vpatch.attn1_route(blk, x)
        assert plain != "module"
        assert vpatch.attn1_route(blk, x, None, None, {"ip_adapter_masks": [torch.zeros(1, 1, 4, 4)]}) == plain
        assert vpatch.attn1_route(blk, x, None, None, {}) == plain


def test_unmerged_ok_is_the_panels_route_at_a_site_that_does_not_merge(monkeypatch):
    from vidtome_amd import patch as vpatch
    blk, x = _block(), _x()
    blk._tome_info = {"size": (8, 8), "args": {"max_downsample": 1}}          # 16 tokens of 64: downsample 2
    assert vpatch.attn1_route(blk, x) == "rows" and not vpatch.unmerged_self_attention_ok(blk, x)
    monkeypatch.setattr(vpatch, "PROJ_MODE", "panels")
    assert vpatch.attn1_route(blk, x) == "panels" and vpatch.unmerged_self_attention_ok(blk, x)
    assert vpatch.unmerged_self_attention_ok(blk, x, "panels") and not vpatch.unmerged_self_attention_ok(blk, x, "rows")
    blk._tome_info["args"]["max_downsample"] = 2
    assert not vpatch.unmerged_self_attention_ok(blk, x)                      # the site merges


BODIES = {
    "self_attention": lambda vp, attn, x, q, **kw: vp.self_attention(attn, x, None, q, **kw),
    "self_attention_rows": lambda vp, attn, x, q, **kw: vp.self_attention_rows(attn, x, None, None, q, **kw),
    "self_attention_panels": lambda vp, attn, x, q, **kw: vp.self_attention_panels(attn, x, None, None, q, **kw),
}


@pytest.mark.filterwarnings("ignore:vidtome_amd. attn1 projections")
@pytest.mark.parametrize("body", sorted(BODIES))
def test_query_rows_under_sharing_need_aligned_matching(body, monkeypatch):
    """Three groups share the source group's probabilities: per-sample query rows raise before any library call unless the
    caller says the matching was aligned; then the body goes on to its first launch."""
    from vidtome_amd import _lib
    from vidtome_amd import patch as vpatch
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    monkeypatch.setattr(_lib, "_req", lambda t, name: t)   # (the wrappers' own refusal of CPU operands: the weights are)
    monkeypatch.setattr(vpatch, "_warned", set())          # (the library-GEMM body says once what it is: not this test's trace)
    attn = _block().attn1
    attn.injection_schedule, attn.t, attn.vtm_num_inputs = [981], 981, 3
    assert vpatch._pnp_share_groups(attn) == 3
    q_rows = torch.zeros(B, 8, dtype=torch.int32).as_subclass(FakeCuda)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="aligned"):
            BODIES[body](vpatch, attn, _x(), q_rows)
        with pytest.raises(RuntimeError, match="aligned"):
            BODIES[body](vpatch, attn, _x(), q_rows, aligned=False)
        with pytest.raises(pytest.fail.Exception, match="the library was reached"):
            BODIES[body](vpatch, attn, _x(), q_rows, aligned=True)
        with pytest.raises(pytest.fail.Exception, match="the library was reached"):
            BODIES[body](vpatch, attn, _x(), None)                          # no query rows: nothing to guard
