"""Host tests of tests/first_forward.py (the stage recorder of tests/test_gpu_first_forward.py), on fake wrappers that
return CPU tensors: a fake takes the REAL wrapper's signature (so the table's argument names are the real ones) and builds
its padded result from a restatement, written here by hand, of which part of it is valid:
* one flipped bit inside any stage's valid region changes that stage's digest and nothing else, and first_divergence names it;
* arbitrary bytes in the rows / columns past n, Mq or count change nothing;
* a wrapper the table does not know raises when it is called under ``record``."""
import inspect
import types

import pytest
import torch

import first_forward as FF
from vidtome_amd import _lib as REAL

B, C = 2, 16
f16, f32, i32, i64 = torch.float16, torch.float32, torch.int32, torch.int64


class Ctl:
    pad = 0x00          # the byte every element outside a valid region is made of
    flip = None         # (stage, call index) whose last valid element gets its lowest bit flipped
    calls = None


def _mk(stage, shape, dtype, index=None, counts=None, outside=None):
    """A result tensor: pad bytes everywhere (``outside``: that byte instead -- what the header promises there), then a
    fixed pattern in the valid region ``index`` (a tuple of slices; None: everything), cut to counts[b] entries along
    axis 1 of sample b."""
    n = 1
    for s in shape:
        n *= s
    byte = Ctl.pad if outside is None else outside
    t = torch.full((n * torch.empty((), dtype=dtype).element_size(),), byte, dtype=torch.uint8).view(dtype).reshape(shape).clone()
    mask = torch.zeros(shape, dtype=torch.bool)
    mask[index if index is not None else ...] = True
    if counts is not None:
        for b, c in enumerate(counts):
            mask[b, c:] = False
    k = int(mask.sum())
    vals = (torch.arange(k) % 97 + 1).to(dtype)
    i = Ctl.calls[stage] = Ctl.calls.get(stage, -1) + 1
    if Ctl.flip == (stage, i):
        raw = vals[-1:].clone().view(torch.uint8)
        raw[0] = raw[0] ^ 1
        vals[-1:] = raw.view(dtype)
    t[mask] = vals
    return t


S = slice
COUNTS = [3, 5]
count_t = lambda: torch.tensor(COUNTS, dtype=i32)

# wrapper -> f(bound arguments) -> result, with the valid regions as the recorder's specification states them
SPEC = {
    "normalize_gather": lambda a: (_mk("_lib.normalize_gather.operand", (B, 4, 2, 256, 4), f32, (S(None), S(None), S(None), S(5))),
                                   _mk("_lib.normalize_gather.norms", (B, 5), f32)),
    "match": lambda a: _mk("_lib.match.best", (B, a["Ns"]), i64),
    "match_masked": lambda a: _mk("_lib.match_masked.best", (B, a["Ns"]), i64),
    "match_filtered": lambda a: _mk("_lib.match_filtered.best", (B, 6), i64),
    "decode_best": lambda a: (_mk("_lib.decode_best.max", (B, 6), f32), _mk("_lib.decode_best.argmax", (B, 6), i32)),
    "sort_desc": lambda a: _mk("_lib.sort_desc.perm", (B, 6), i32),
    "partition_local": lambda a: tuple(_mk(f"_lib.partition_local.{n}", s, i32) for n, s in
                                       (("a_pos", (6,)), ("b_pos", (4,)), ("a_rows", (B, 6)), ("b_rows", (B, 4)))),
    "partition_global": lambda a: tuple(_mk(f"_lib.partition_global.{n}", s, i32) for n, s in
                                        (("a_pos", (6,)), ("b_pos", (4,)), ("a_rows", (B, 6)), ("b_rows", (B, 4)))),
    "anchor_pos": lambda a: _mk("_lib.anchor_pos.pos", (B, 6), i32),
    "plan_apply": lambda a: tuple(_mk(f"_lib.plan_apply.{n}", (B, 5), i32) for n in ("new_cur", "inv")) + (None, None, None),
    "compose": lambda a: _mk("_lib.compose.out", (B, a["n"]), i32),
    "anchor_maps": lambda a: tuple(_mk(f"_lib.anchor_maps.{n}", (B, 6), i32) for n in ("loc", "amap", "pos")),
    "gather_rows": lambda a: _mk("_lib.gather_rows.out", (B, 8, C), f16, (S(None), S(a["idx"].shape[1]))),
    "linear_rows": lambda a: _mk("_lib.linear_rows.out", (B, C, 8) if a["transposed"] else (B, 8, C), f16,
                                 (S(None), S(None), S(a["n"])) if a["transposed"] else (S(None), S(a["n"]))),
    "linear_f32": lambda a: _mk("_lib.linear_f32.out", (B, C, 8) if a["transposed"] else (B, 8, C), f32,
                                (S(None), S(None), S(a["n"])) if a["transposed"] else (S(None), S(a["n"]))),
    "attention": lambda a: _mk("_lib.attention.out", (B, 8, C), f16, (S(None), S(a["M"]))),
    "attention_kv": lambda a: _mk("_lib.attention_kv.out", (B, 8, C), f16, (S(None), S(a["Mq"])),
                                  None if a["q_count"] is None else COUNTS),
    "attention_kv_bias": lambda a: _mk("_lib.attention_kv_bias.out", (B, 8, C), f16, (S(None), S(a["Mq"]))),
    "unmerge_add": lambda a: _mk("_lib.unmerge_add.out", (B, 12, C), f16),
    "layernorm": lambda a: _mk("_lib.layernorm.out", (B, 6, C), f16),
    "layernorm_panels": lambda a: _mk("_lib.layernorm_panels.out", (C // 8, 256, 8), f16, (S(None), S(B * 6))),
    "to_panels": lambda a: _mk("_lib.to_panels.out", (C // 8, 256, 8), f16, (S(None), S(10))),
    "gather_panels": lambda a: _mk("_lib.gather_panels.out", (C // 8, B, 256, 8), f16,
                                   (S(None), S(None), S(a["n"]))).view(C // 8, B * 256, 8),
    "linear_panels": lambda a: _mk("_lib.linear_panels.out", (16, 24), f16, (S(a["n"]), S(a["N"]))),
    "ff_geglu": lambda a: _mk("_lib.ff_geglu.out", (4, 256, 8), f16, (S(None), S(a["n"]))),
    "transpose_cols": lambda a: _mk("_lib.transpose_cols.out", (B, C, 8), f16),
    "geglu": lambda a: _mk("_lib.geglu.out", (B, 6, C), f16),
}


def _compact_queries(a):
    # (qc past the count: zero, as the header promises -- the recorder also hashes the whole list)
    qc = _mk("_lib.compact_queries.qc", (B, 6), i32, None, COUNTS, outside=0)
    Ctl.calls["_lib.compact_queries.qc_padded"] = Ctl.calls.get("_lib.compact_queries.qc_padded", -1) + 1
    return qc, _mk("_lib.compact_queries.tmap", (B, 6), i32), count_t()


def _fold_keys(a):
    ks = _mk("_lib.fold_keys.key_sel", (B, 6), i32, None, COUNTS, outside=0)
    return ks, _mk("_lib.fold_keys.k_bias", (B, 8), i32, None, COUNTS), count_t()


SPEC.update(compact_queries=_compact_queries, fold_keys=_fold_keys)


def _fake(name, spec):
    sig = inspect.signature(getattr(REAL, name))

    def fake(*args, **kwargs):
        bound = sig.bind(*args, **kwargs)
        bound.apply_defaults()
        return spec(bound.arguments)
    fake.__signature__ = sig
    fake.__name__ = name
    return fake


def fake_lib():
    lib = types.ModuleType("fake_lib")
    for name, spec in SPEC.items():
        setattr(lib, name, _fake(name, spec))
    lib.panel_rows = REAL.panel_rows                     # host-only: passes through un-recorded
    return lib


def fake_patch(lib):
    """The five functions of vidtome_amd.patch the recorder wraps, as a block forward calls them."""
    p = types.ModuleType("fake_patch")

    def compute_merge(module, x, info, **kw):
        lv = types.SimpleNamespace(**{n: _mk(f"plan.level0.{n}", (B, 5), i64 if n == "best" else i32) for n in FF.LEVEL_TENSORS[:5]},
                                   unm_idx=None, src_idx=None, dst_idx=None)
        gl = types.SimpleNamespace(**{n: _mk(f"plan.global.{n}", (B, 5), i64 if n == "best" else i32) for n in FF.LEVEL_TENSORS})
        plan = types.SimpleNamespace(gather_map=_mk("plan.gather_map", (B, 7), i32), inv=_mk("plan.inv", (B, 12), i32),
                                     q_rows=_mk("plan.q_rows", (B, 6), i32, None, COUNTS), q_count=count_t(),
                                     inv_q=_mk("plan.inv_q", (B, 12), i32), levels=[lv], global_level=gl)
        module.global_tokens = _mk("global_tokens", (B, 6, C), f16)
        module.global_tokens._vtm_pos = _mk("global_tokens._vtm_pos", (B, 6), i32)
        m = lambda t: t
        m.plan = plan
        return m, m, None

    def layer_norm(norm, x):
        return _mk("norm1" if norm == "norm1" else "layer_norm", (B * 2, 6, C), f16)

    def self_attention_segment(block, h):
        p.layer_norm("norm1", h)
        p.compute_merge(block, h, None)
        return _mk("attn1_segment", (B * 2, 6, C), f16)

    def cross(block, h):
        return _mk("attn2_segment", (B * 2, 6, C), f16)

    p.compute_merge, p.layer_norm, p.self_attention_segment = compute_merge, layer_norm, self_attention_segment
    p.norm_cross_attention_residual = p.norm_cross_attention_f32 = cross
    return p


def _drive(lib, p, rec):
    """Every tabled wrapper once (attention_kv, the linears and to_panels in each of their forms), then the block."""
    z = lambda *s, dt=f16: torch.zeros(s, dtype=dt)
    idx = z(B, 5, dt=i32)
    lib.normalize_gather(z(B, 12, C), None, idx)
    lib.match(None, None, 6, 4, False)
    lib.match_masked(None, None, 6, 4, False, None, None, None, 0.0)
    lib.match_filtered(z(B, 12, C), None, idx, idx, False)
    lib.decode_best(None), lib.sort_desc(None)
    lib.partition_local(None, B, 10, 0, 5, 2, 0, "cpu")
    lib.partition_global(idx, 12, 6, True, z(B, 6, dt=i32), 6, None)
    lib.anchor_pos(None, B, 6, 12, 6, None, "cpu")
    lib.plan_apply(None, None, None, None, idx, idx, 3, False, False)
    lib.compose(None, idx, 12)
    lib.anchor_maps(idx, 0, idx, 6, 12, 6, None, True)
    lib.compact_queries(idx, 3, 4), lib.fold_keys(idx, 12, idx, 6, f16)
    lib.gather_rows(z(B, 12, C), None, idx, pad_to=8)
    lib.linear_rows(z(B, 12, C), None, idx, None, 5, None, None)
    lib.linear_rows(z(B, 12, C), None, idx, None, 5, None, None, transposed=True)
    lib.linear_f32(z(B, 12, C), None, idx, None, 5, None, None)
    lib.linear_f32(z(B, 12, C), None, idx, None, 5, None, None, transposed=True)
    lib.attention(None, None, None, 2, 5, 1.0)
    lib.attention_kv(None, None, None, 2, 7, 5, 1.0)
    o = lib.attention_kv(None, None, None, 2, 7, 5, 1.0, q_count=count_t())
    lib.attention_kv_bias(None, None, None, 2, 7, 5, 1.0, None)
    lib.unmerge_add(None, None, None), lib.layernorm(None, None, None, 1e-5)
    lib.layernorm_panels(z(B, 6, C), None, None, 1e-5)
    lib.to_panels(z(10, C)), lib.to_panels(z(4, C), z(10, dt=i32)), lib.to_panels(z(12, C), None, 10)
    lib.gather_panels(z(B, 12, C), None, idx, None, 5)
    lib.linear_panels(None, 9, None, 16, None)
    lib.ff_geglu(None, 9, None, 32, None), lib.transpose_cols(None, 0, C), lib.geglu(None)
    assert lib.panel_rows(5) == 256
    blk = types.SimpleNamespace()
    p.self_attention_segment(blk, None)
    p.layer_norm("norm3", None)
    p.norm_cross_attention_residual(blk, None), p.norm_cross_attention_f32(blk, None)
    rec.tap("block_output", _mk("block_output", (B * 2, 6, C), f16))
    return o


def _run(pad=0x00, flip=None):
    Ctl.pad, Ctl.flip, Ctl.calls = pad, flip, {}
    lib = fake_lib()
    p = fake_patch(lib)
    with FF.record(lib=lib, patch=p) as rec:
        _drive(lib, p, rec)
    assert lib.match.__name__ == "match" and p.compute_merge.__name__ == "compute_merge", "record did not restore"
    return rec


def test_the_table_names_real_wrappers_and_the_fakes_cover_it():
    real = set(FF.wrapper_names(REAL))
    assert set(FF.TABLE) <= real, set(FF.TABLE) - real
    assert set(SPEC) == set(FF.TABLE)
    assert not FF.HOST_ONLY & set(FF.TABLE)
    base = _run()
    stages = {e[0] for e in base}
    for name in FF.TABLE:
        assert any(s.startswith(f"_lib.{name}.") for s in stages), name
    for s in ("plan.gather_map", "plan.inv", "plan.q_rows", "plan.inv_q", "plan.level0.new_cur", "plan.global.dst_idx",
              "global_tokens", "global_tokens._vtm_pos", "norm1", "attn1_segment", "attn2_segment", "block_output"):
        assert s in stages, s
    assert FF.first_divergence(base, _run()) is None and base.nonfinite == []


def test_one_flipped_bit_in_a_valid_region_is_named():
    base = _run()
    keys = [(e[0], e[1]) for e in base]
    assert len(set(keys)) == len(keys) > 70
    for pos, (stage, i) in enumerate(keys):
        if stage.endswith("_padded") or stage in ("_lib.compact_queries.count", "_lib.fold_keys.k_count", "plan.q_count"):
            continue                       # (hashed with the sliced list / a count of the scenario, not a fake tensor)
        got = _run(flip=(stage, i))
        div = FF.first_divergence(base, got)
        assert div is not None, f"a flipped bit in {stage} #{i} went unseen"
        # (the sliced and the whole list of a compacted result are two entries of the same tensor)
        differing = [k for k, (a, b) in enumerate(zip(base, got)) if tuple(a) != tuple(b)]
        assert div[0] == pos and div[1][:2] == (stage, i), (stage, i, div)
        assert all(base[k][0] in (stage, stage + "_padded") for k in differing), (stage, [base[k][0] for k in differing])


@pytest.mark.parametrize("pad", [0xFF, 0x5A])
def test_bytes_outside_the_valid_regions_change_nothing(pad):
    base, got = _run(), _run(pad=pad)
    assert FF.first_divergence(base, got) is None, FF.first_divergence(base, got)
    assert got.nonfinite == []            # (0xFF bytes are NaNs in every float format: none of them is looked at)


def test_rows_behind_a_bounded_attention_follow_its_count():
    """The projection that reads a query-bounded attention output is hashed up to q_count[b] rows per sample too."""
    def run(pad):
        Ctl.pad, Ctl.flip, Ctl.calls = pad, None, {}
        lib = fake_lib()
        lib.linear_rows = _fake("linear_rows", lambda a: _mk("_lib.linear_rows.out", (B, 8, C), f16, (S(None), S(a["n"])),
                                                             COUNTS if a["rows"] is None else None))
        with FF.record(lib=lib, patch=fake_patch(lib)) as rec:
            o = lib.attention_kv(None, None, None, 2, 7, 5, 1.0, q_count=count_t())
            lib.linear_rows(o, None, None, None, 7, None, None)
            lib.linear_rows(o, None, torch.zeros(B, 7, dtype=i32), None, 7, None, None)
        return rec
    assert FF.first_divergence(run(0x00), run(0xFF)) is None


def test_an_untabled_wrapper_raises():
    Ctl.pad, Ctl.flip, Ctl.calls = 0, None, {}
    lib = fake_lib()

    def brand_new(x):
        return x
    lib.brand_new = brand_new
    with pytest.raises(FF.Untabled, match="brand_new"):
        with FF.record(lib=lib, patch=fake_patch(lib)):
            lib.geglu(None)
            lib.brand_new(torch.zeros(2))
    assert lib.brand_new is brand_new
    untabled = set(FF.wrapper_names(REAL)) - set(FF.TABLE)
    assert "attention_kv_sets" in untabled and "position_order" in untabled      # (not on the scenarios' path: they would raise)


def test_first_divergence_reports_a_missing_tail():
    base = _run()
    assert FF.first_divergence(base, base[:-1]) == (len(base) - 1, tuple(base[-1]), None)
