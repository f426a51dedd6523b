"""A stage recorder for the patched block (tests/test_first_forward_host.py, tests/test_gpu_first_forward.py,
tests/first_forward_child.py): ``record`` wraps the Python-level stages of vidtome_amd.patch and the vidtome_amd._lib
wrappers of the patched path and leaves, per call, the sha256 of the bytes of every result's VALID REGION -- padded results
are sliced with the call's own arguments first (rows < n, < Mq, < count[b], ...), so bytes nobody may read are not reported.
Two runs of the same work are then compared stage by stage (``first_divergence``).

Nothing here synchronises the host with the device while the recorded work runs: a tap keeps a device-side copy of what it
will hash (stream-ordered behind the launch that wrote it) and the digests are taken when ``record`` ends."""
import contextlib
import hashlib
import inspect

import torch

# functions of vidtome_amd._lib that launch nothing: not stages
HOST_ONLY = {"exported_symbols", "lib", "release_workspaces", "dtype_code", "pad_rows", "pad_k", "panel_rows", "partition_counts",
             "mask_threshold", "guided_step_chunk"}


class Untabled(RuntimeError):
    """A _lib wrapper ran under ``record`` that the table below has no entry for."""


class Recording(list):
    """[(stage, call index, shape, dtype, sha256 hex)] in call order; ``nonfinite``: the stages whose valid region holds a
    NaN or an infinity; ``result``: what ``fn`` returned."""

    def __init__(self):
        super().__init__()
        self.nonfinite = []
        self.result = None
        self._pending = []
        self._counts = {}
        self.keep_names = set()     # stages whose valid region is also kept as a CPU tensor: tensors[(stage, call index)]
        self.tensors = {}
        self.bounded = {}           # data_ptr of a query-bounded attention output -> its q_count
        self.keep = []

    def tap(self, stage, tensor, valid=None, count=None):
        """Keep ``tensor`` (None: nothing) for stage ``stage``.  ``valid`` slices the copy to its valid region; ``count``
        (B,) int: only the first count[b] entries along axis 1 of sample b are valid."""
        if tensor is None:
            return
        i = self._counts[stage] = self._counts.get(stage, -1) + 1
        t = tensor.detach()
        if valid is not None:
            t = valid(t)
        self._pending.append((stage, i, t.clone(), None if count is None else count.detach().clone()))

    def finish(self):
        for stage, i, t, count in self._pending:
            t = t.cpu()
            if count is not None:
                count = [int(c) for c in count.cpu().reshape(-1)]
                if len(count) == 1 and t.shape[0] != 1:
                    count = count * t.shape[0]
                t = torch.cat([t[b, :max(0, min(c, t.shape[1]))].reshape(-1) for b, c in enumerate(count)])
            t = t.contiguous()
            if stage in self.keep_names:
                self.tensors[(stage, i)] = t
            if t.is_floating_point() and not bool(torch.isfinite(t).all()):
                self.nonfinite.append((stage, i))
            raw = t.reshape(-1).view(torch.uint8).numpy().tobytes()
            self.append((stage, i, tuple(t.shape), str(t.dtype), hashlib.sha256(raw).hexdigest()))
        self._pending, self.keep, self.bounded = [], [], {}
        return self


# ---------------------------------------------------------------------------------------------------------------------
# the table: wrapper name -> f(bound arguments, result) -> [(sub-stage, tensor, valid-region slicer or None, count or None)]
# ---------------------------------------------------------------------------------------------------------------------
def _rows(n):
    return lambda t: t[:, :n]


def _cols(n):
    return lambda t: t[:, :, :n]


def _whole(*names):
    def f(a, res):
        res = res if isinstance(res, (tuple, list)) else (res,)
        return [(n, t, None, None) for n, t in zip(names, res)]
    return f


def _normalize_gather(a, res):
    n = a["rows"].shape[1]
    return [("operand", res[0], lambda t: t[:, :, :, :n], None), ("norms", res[1], _rows(n), None)]


def _match_filtered(a, res):
    return [("best", res[0] if a["want_flag"] else res, None, None)]      # (the flags are counters of the launch plan)


def _compact_queries(a, res):
    qc, tmap, count = res
    # (the header also promises zeros past the count, and the projections gather through every entry: "qc_padded")
    return [("qc", qc, None, count), ("qc_padded", qc, None, None), ("tmap", tmap, None, None), ("count", count, None, None)]


def _fold_keys(a, res):
    key_sel, k_bias, k_count = res
    return [("key_sel", key_sel, None, k_count), ("key_sel_padded", key_sel, None, None), ("k_bias", k_bias, None, k_count),
            ("k_count", k_count, None, None)]


def _gather_rows(a, res):
    return [("out", res, _rows(a["idx"].shape[1]), None)]


def _linear(a, res):
    """rows < n (columns < n when transposed).  Behind a query-bounded attention call the rows past q_count[b] of its
    output are undefined, and so are the same rows of the row-wise projection that reads it: they are not hashed either."""
    if a["transposed"]:
        return [("out", res, _cols(a["n"]), None)]
    count = a["__rec__"].bounded.get(a["x0"].data_ptr()) if a["rows"] is None and a["rows2"] is None else None
    return [("out", res, _rows(a["n"]), count)]


def _attention(a, res):
    return [("out", res, _rows(a["M"]), None)]


def _attention_kv(a, res):
    if a.get("q_count") is not None:
        a["__rec__"].bounded[res.data_ptr()] = a["q_count"]
        a["__rec__"].keep.append(res)              # (the address stays this tensor's while the recording lasts)
    return [("out", res, _rows(a["Mq"]), a.get("q_count"))]


def _layernorm_panels(a, res):
    x = a["x"]
    return [("out", res, _rows(x.numel() // x.shape[-1]), None)]


def _to_panels(a, res):
    x, order = a["x"], a["order"]
    n = x.numel() // x.shape[-1] if order is None else order.numel()
    return [("out", res, _rows(n if a["rows"] is None else a["rows"]), None)]


def _gather_panels(a, res):
    B, n = a["x0"].shape[0], a["n"]
    return [("out", res, lambda t: t.view(t.shape[0], B, t.shape[1] // B, 8)[:, :, :n], None)]


def _linear_panels(a, res):
    n, N = a["n"], a["N"]
    return [("out", res, lambda t: t[:n, :N], None)]


def _ff_geglu(a, res):
    return [("out", res, _rows(a["n"]), None)]


TABLE = {
    "normalize_gather": _normalize_gather,
    "match": _whole("best"),
    "match_masked": _whole("best"),
    "match_filtered": _match_filtered,
    "decode_best": _whole("max", "argmax"),
    "sort_desc": _whole("perm"),
    "partition_local": _whole("a_pos", "b_pos", "a_rows", "b_rows"),
    # (not its seed_table: several dst rows hold one token position and "whichever write lands last is as good as any
    # other", csrc/plan.hip -- it differs from run to run by design and only seeds the matcher, whose result is hashed)
    "partition_global": _whole("a_pos", "b_pos", "a_rows", "b_rows"),
    "anchor_pos": _whole("pos"),
    "plan_apply": _whole("new_cur", "inv", "unm_idx", "src_idx", "dst_idx"),
    "compose": _whole("out"),
    "anchor_maps": _whole("loc", "amap", "pos"),
    "compact_queries": _compact_queries,
    "fold_keys": _fold_keys,
    "gather_rows": _gather_rows,
    "linear_rows": _linear,
    "linear_f32": _linear,
    "attention": _attention,
    "attention_kv": _attention_kv,
    "attention_kv_bias": _attention_kv,
    "unmerge_add": _whole("out"),
    "layernorm": _whole("out"),
    "layernorm_panels": _layernorm_panels,
    "to_panels": _to_panels,
    "gather_panels": _gather_panels,
    "linear_panels": _linear_panels,
    "ff_geglu": _ff_geglu,
    "transpose_cols": _whole("out"),       # (the header promises zero fill: all of it)
    "geglu": _whole("out"),
}


def wrapper_names(lib):
    """The launching wrappers of ``lib``: its public functions apart from the host-only helpers."""
    return sorted(n for n, f in vars(lib).items()
                  if not n.startswith("_") and inspect.isfunction(f) and n not in HOST_ONLY)


def _tapped(rec, name, fn):
    entry = TABLE.get(name)
    sig = inspect.signature(fn)

    def call(*args, **kwargs):
        if entry is None:
            raise Untabled(f"first_forward.TABLE has no entry for _lib.{name}: a stage would go unrecorded")
        res = fn(*args, **kwargs)
        bound = sig.bind(*args, **kwargs)
        bound.apply_defaults()
        bound.arguments["__rec__"] = rec
        for sub, t, valid, count in entry(bound.arguments, res):
            rec.tap(f"_lib.{name}.{sub}", t, valid, count)
        return res
    call.__wrapped__ = fn
    return call


# ---------------------------------------------------------------------------------------------------------------------
# the Python-level stages of vidtome_amd.patch
# ---------------------------------------------------------------------------------------------------------------------
LEVEL_TENSORS = ("new_cur", "inv", "a_pos", "b_pos", "best", "unm_idx", "src_idx", "dst_idx")


def tap_plan(rec, plan, module):
    """The MergePlan of one compute_merge call and the anchors it left on ``module``."""
    if plan is None:
        return
    rec.tap("plan.gather_map", plan.gather_map)
    rec.tap("plan.inv", plan.inv)
    rec.tap("plan.q_rows", plan.q_rows, None, plan.q_count)
    rec.tap("plan.q_count", plan.q_count)
    rec.tap("plan.inv_q", plan.inv_q)
    for i, lv in enumerate(list(plan.levels) + ([plan.global_level] if plan.global_level is not None else [])):
        which = "global" if lv is plan.global_level else f"level{i}"
        for n in LEVEL_TENSORS:
            rec.tap(f"plan.{which}.{n}", getattr(lv, n, None))
    gt = getattr(module, "global_tokens", None)
    rec.tap("global_tokens", gt)
    rec.tap("global_tokens._vtm_pos", getattr(gt, "_vtm_pos", None) if gt is not None else None)


def _patch_taps(rec, patch):
    state = {"in_attn1": False, "norm1_seen": False}
    orig = {n: getattr(patch, n) for n in ("compute_merge", "layer_norm", "self_attention_segment",
                                           "norm_cross_attention_residual", "norm_cross_attention_f32")}

    def compute_merge(module, x, info, *a, **kw):
        res = orig["compute_merge"](module, x, info, *a, **kw)
        tap_plan(rec, getattr(res[0], "plan", None), module)
        return res

    def layer_norm(norm, x):
        y = orig["layer_norm"](norm, x)
        first = state["in_attn1"] and not state["norm1_seen"]
        state["norm1_seen"] = state["norm1_seen"] or first
        rec.tap("norm1" if first else "layer_norm", y)
        return y

    def self_attention_segment(*a, **kw):
        state["in_attn1"], state["norm1_seen"] = True, False
        try:
            y = orig["self_attention_segment"](*a, **kw)
        finally:
            state["in_attn1"] = False
        rec.tap("attn1_segment", y)                 # = norm2's input
        return y

    def cross(name):
        def f(*a, **kw):
            y = orig[name](*a, **kw)
            rec.tap("attn2_segment", y)
            return y
        return f

    new = {"compute_merge": compute_merge, "layer_norm": layer_norm, "self_attention_segment": self_attention_segment,
           "norm_cross_attention_residual": cross("norm_cross_attention_residual"),
           "norm_cross_attention_f32": cross("norm_cross_attention_f32")}
    return orig, new


@contextlib.contextmanager
def record(fn=None, lib=None, patch=None):
    """``with record() as rec: ...`` -- or ``with record(fn) as rec`` (``fn()`` runs inside, its value is ``rec.result``) --
    records the work done inside; ``rec`` is complete when the block ends.  ``rec.tap(name, tensor)`` adds a stage by hand
    (the block output).  ``lib`` / ``patch``: the modules to wrap (vidtome_amd._lib / vidtome_amd.patch; the host tests pass
    fakes).  Every launching wrapper of ``lib`` is wrapped: one the table does not know raises ``Untabled`` when called."""
    if lib is None:
        from vidtome_amd import _lib as lib
    if patch is None:
        from vidtome_amd import patch
    rec = Recording()
    saved_lib = {n: getattr(lib, n) for n in wrapper_names(lib)}
    saved_patch, new_patch = _patch_taps(rec, patch)
    try:
        for n, f in saved_lib.items():
            setattr(lib, n, _tapped(rec, n, f))
        for n, f in new_patch.items():
            setattr(patch, n, f)
        if fn is not None:
            rec.result = fn()
        yield rec
    finally:
        for n, f in saved_lib.items():
            setattr(lib, n, f)
        for n, f in saved_patch.items():
            setattr(patch, n, f)
    rec.finish()


def first_divergence(a, b):
    """The first stage whose digests differ: (position, entry of a, entry of b) -- an entry is None where one list has
    ended -- or None when the lists are equal."""
    for i in range(max(len(a), len(b))):
        ea = tuple(a[i]) if i < len(a) else None
        eb = tuple(b[i]) if i < len(b) else None
        if ea != eb:
            return i, ea, eb
    return None


# ---------------------------------------------------------------------------------------------------------------------
# the scenarios of tests/test_gpu_first_forward.py and its child process
# ---------------------------------------------------------------------------------------------------------------------
# id -> (C, dtype name, latent, frames per sample, chunks, fp32 opt-ins)
SCENARIOS = {
    "s9": (320, "float16", (8, 8), 2, 1, False),        # DESIGN.md section 9's own
    "odd": (320, "float16", (9, 5), 2, 1, False),       # 45 tokens per frame: pad rows / pad key columns exist
    "chain": (320, "float16", (8, 8), 4, 3, False),     # global level, anchors, compacted live queries, folded keys
    "c640": (640, "float16", (8, 8), 2, 1, False),      # panel-GEMM route
    "bf16": (320, "bfloat16", (8, 8), 2, 1, False),
    "f32": (320, "float32", (8, 8), 2, 1, True),        # linear_f32, attention_f32
}
GLOBAL_RAND = (0.5, 0.0, 1.0)                            # per chunk, as tests/test_gpu_lora.py's _run
KEEP = ("norm1", "attn1_segment", "block_output")


def scenario_inputs(name, device, chunk=0):
    """Tokens (B F, N, C) and conditioning (B F, 77, 768) of one chunk: attention_maps_standin.inputs' seeds (70 + chunk)."""
    import attention_maps_standin as AM
    C, dt, latent, frames, _, _ = SCENARIOS[name]
    dtype = getattr(torch, dt)
    g = torch.Generator().manual_seed(70 + chunk)
    h = torch.randn(AM.B * frames, latent[0] * latent[1], C, generator=g).to(device=device, dtype=dtype)
    cond = torch.randn(AM.B * frames, AM.COND, AM.COND_DIM, generator=g).to(device=device, dtype=dtype)
    return h, cond


def run_scenario(name, device="cuda", keep=()):
    """One patch -> forward(s) -> remove_patch round of scenario ``name`` on a fresh block under ``record``: the Recording
    (``rec.unet``: the un-patched model, ``rec.args``: the patch arguments it ran with)."""
    import attention_maps_standin as AM
    import vidtome_amd
    C, dt, latent, frames, chunks, f32 = SCENARIOS[name]
    unet = AM.patched(C, getattr(torch, dt), device, latent=latent)
    if f32:
        vidtome_amd.update_patch(unet, fp32_attention=True, fp32_projections=True)
    try:
        with record() as rec, torch.no_grad():
            rec.keep_names = set(keep)
            torch.manual_seed(123)
            for ck in range(chunks):
                if chunks > 1:
                    unet._tome_info["args"]["global_rand"] = GLOBAL_RAND[ck % 3]
                h, cond = scenario_inputs(name, device, ck)
                rec.tap("block_output", unet.blocks[0](h, encoder_hidden_states=cond))
        rec.args = dict(unet._tome_info["args"])
    finally:
        vidtome_amd.remove_patch(unet)
    rec.unet = unet
    return rec


# ---------------------------------------------------------------------------------------------------------------------
# which side is right: the float64 restatement of tests/test_gpu_odd_tokens.py over the oracle's merge
# ---------------------------------------------------------------------------------------------------------------------
TOL = {"float16": 1e-3, "bfloat16": 8e-3}              # tests/test_gpu_odd_tokens.py: a segment ...
BLOCK_TOL = {"float16": 2e-3, "bfloat16": 8e-3}        # ... and the whole block, of the output scale


def reference_ratios(name, rec):
    """(norm1, norm2's input, block output) of the first forward of ``rec`` (run with keep=KEEP) against float64, each as
    max |got - ref| / max(1, |ref|max).  Operands as the device holds them, every intermediate rounded where the module path
    rounds it; the merge is the oracle's, computed from the recorded norm1 output (the matcher of a 16-bit model sees the
    rounded rows), so wrong merge indices show as a large error."""
    import torch.nn.functional as F
    from oracle import oracle
    C, dt, latent, frames, _, _ = SCENARIOS[name]
    dtype = getattr(torch, dt)
    blk = rec.unet.blocks[0].cpu()
    rd = lambda t: t.to(dtype).double()
    w = lambda m: m.weight.detach().double()
    lin = lambda m, x: rd(x @ w(m).T + (0 if m.bias is None else m.bias.detach().double()))
    ln = lambda n, x: rd(F.layer_norm(x, x.shape[-1:], n.weight.detach().double(), n.bias.detach().double(), n.eps))

    def att(a, q, k, v):
        sh = lambda t: t.view(t.shape[0], t.shape[1], a.heads, -1).transpose(1, 2)
        s = sh(q) @ sh(k).transpose(-1, -2) * a.scale
        return (torch.softmax(s, dim=-1) @ sh(v)).transpose(1, 2).reshape(q.shape)

    def ratio(got, ref):
        g = got.double()
        assert bool(torch.isfinite(g).all())
        return float((g - ref).abs().max()) / max(1.0, float(ref.abs().max()))

    h, cond = scenario_inputs(name, "cpu")
    x, c = h.double(), cond.double()
    got1, got_a, got_o = (rec.tensors[(n, 0)] for n in KEEP)
    r1 = ratio(got1, ln(blk.norm1, x))
    torch.manual_seed(123)
    draws = oracle.RandomDraws.from_torch_generator(torch.Generator().set_state(torch.get_rng_state()))
    m_o, u_o, merged, _ = oracle.compute_merge(got1.float().numpy(), latent, rec.args, draws, {"global_tokens": None})
    a = blk.attn1
    xm = torch.from_numpy(merged).double()
    y = lin(a.to_out[0], rd(att(a, lin(a.to_q, xm), lin(a.to_k, xm), lin(a.to_v, xm))))
    x2 = torch.from_numpy(u_o(y.float().numpy())).double() + x            # (an unmerge of 16-bit values: exact in fp32)
    ra = ratio(got_a, x2)
    a, x2 = blk.attn2, rd(x2)
    x3 = lin(a.to_out[0], rd(att(a, lin(a.to_q, ln(blk.norm2, x2)), lin(a.to_k, c), lin(a.to_v, c)))) + x2
    x3 = rd(x3)
    value, gate = lin(blk.ff.net[0].proj, ln(blk.norm3, x3)).chunk(2, dim=-1)
    out = lin(blk.ff.net[2], rd(value * F.gelu(gate))) + x3
    return r1, ra, ratio(got_o, out)
