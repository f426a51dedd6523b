"""A process's first patched forward against its later ones, stage by stage (run with -m gpu on an MI355X).

Every kernel test hands its kernel freshly written operands, so none of them sees a result that depends on the HISTORY of the
memory the library is given (about 70 torch.empty sites: workspaces, padded outputs, panel rows past n, V^T pad columns) or
on one-time process state.  Here the whole patched block runs under tests/first_forward.py's recorder, which hashes the
valid region of every stage's result, and the digest lists are compared
(a) between the first three patch -> forward -> remove_patch rounds of a freshly started process, and
(b) between three runs in this process whose every allocation comes out of allocator cache filled with 0x00000000,
    0xFFFFFFFF (NaN in every float format, -1 as an index) and 0x00003C00 (fp16 (1.0, 0.0), a denormal fp32, index 15360);
(c) the first round's norm1 output, norm2 input and block output are held to the float64 restatement of
    tests/test_gpu_odd_tokens.py over the oracle's merge, at that file's bars (1e-3 of the output scale for a segment,
    2e-3 for the whole block, fp16)."""
import functools
import gc
import json
import os
import subprocess
import sys

import pytest
import torch

import first_forward as FF

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "first_forward_child.py")
CHILD_SCENARIOS = ("s9", "odd", "chain")
FILLS = (0x00000000, 0xFFFFFFFF, 0x00003C00)
MB = 1 << 20
SMALL_BLOCK, LARGE_BLOCK = MB, 20 * MB          # torch's caching allocator: requests <= 1 MB come from the small pool
SWEEP = {"small": (MB, 256 << 10, 64 << 10, 16 << 10, 4 << 10, 512), "large": (20 * MB, 8 * MB, 2 * MB, MB + 512)}


def _describe(div):
    if div is None:
        return "equal"
    i, a, b = div
    return f"first divergence at entry {i}: {a} against {b}"


# ---------------------------------------------------------------------------------------------------
# (a), (c): a fresh child process
# ---------------------------------------------------------------------------------------------------
FF_CHILD_TIMEOUT = 240       # (the child's own watchdog ends it first)


@functools.lru_cache(maxsize=None)
def _child(name):
    """One child per scenario (they run one after another), shared by the tests that read its line."""
    p = subprocess.run([sys.executable, CHILD, name], capture_output=True, text=True, timeout=FF_CHILD_TIMEOUT)
    assert p.returncode == 0, f"child {name} ended with status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("FIRST_FORWARD ")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0][len("FIRST_FORWARD "):])


@pytest.mark.parametrize("name", CHILD_SCENARIOS)
def test_first_forward_of_a_process_equals_its_later_ones(name):
    got = _child(name)
    r0, r1, r2 = ([tuple(map(lambda v: tuple(v) if isinstance(v, list) else v, e)) for e in r] for r in got["runs"])
    assert len(r0) > 30, "the recorder saw too few stages"
    print(f"first forward {name}: {len(r0)} stages; run 0 / run 1: {_describe(FF.first_divergence(r0, r1))}; "
          f"run 1 / run 2: {_describe(FF.first_divergence(r1, r2))}")
    assert got["nonfinite"] == [[], [], []], got["nonfinite"]
    assert FF.first_divergence(r1, r2) is None, "later runs differ: " + _describe(FF.first_divergence(r1, r2))
    assert FF.first_divergence(r0, r1) is None, "the first forward differs: " + _describe(FF.first_divergence(r0, r1))


@pytest.mark.parametrize("name", ("s9", "odd"))
def test_first_forward_is_the_float64_restatements(name):
    r1, ra, ro = _child(name)["ratios"]
    dt = FF.SCENARIOS[name][1]
    print(f"first forward {name} against float64: norm1 {r1:.3e}, norm2's input {ra:.3e} (bar {FF.TOL[dt]:.0e}), "
          f"block output {ro:.3e} (bar {FF.BLOCK_TOL[dt]:.0e})")
    assert r1 < FF.TOL[dt], r1
    assert ra < FF.TOL[dt], ra
    assert ro < FF.BLOCK_TOL[dt], ro


# ---------------------------------------------------------------------------------------------------
# (b): independence from what allocated memory held
# ---------------------------------------------------------------------------------------------------
# (stage, dtype) pairs a scenario exists for: the part of the path its row of the table names
_16 = lambda dt: [("_lib.match_filtered.best", "torch.int64"), ("_lib.linear_rows.out", dt), ("_lib.attention.out", dt),
                  ("_lib.unmerge_add.out", dt), ("_lib.layernorm_panels.out", dt), ("_lib.attention_kv.out", dt),
                  ("_lib.ff_geglu.out", dt), ("attn1_segment", dt), ("attn2_segment", dt), ("block_output", dt)]
REACHES = {
    "s9": _16("torch.float16"),
    "odd": _16("torch.float16"),
    "bf16": _16("torch.bfloat16"),
    "chain": _16("torch.float16") + [("_lib.partition_global.a_rows", "torch.int32"), ("_lib.anchor_maps.amap", "torch.int32"),
                                     ("_lib.compact_queries.qc", "torch.int32"), ("_lib.fold_keys.key_sel", "torch.int32"),
                                     ("plan.global.new_cur", "torch.int32"), ("plan.q_rows", "torch.int32"),
                                     ("global_tokens._vtm_pos", "torch.int32")],
    "c640": [("_lib.gather_panels.out", "torch.float16"), ("_lib.linear_panels.out", "torch.float16"),
             ("_lib.attention.out", "torch.float16"), ("_lib.to_panels.out", "torch.float16")],
    "f32": [("_lib.linear_f32.out", "torch.float32"), ("_lib.attention.out", "torch.float32"),      # (the fp32 core)
            ("_lib.attention_kv.out", "torch.float32"), ("_lib.layernorm.out", "torch.float32")],
}


def _signed(word):
    return word - (1 << 32) if word >= 1 << 31 else word


def _poison(word, peak):
    """Fill and free blocks of both allocator pools: at least 2 x ``peak`` bytes per pool, then every cached fragment a
    request of 512 B (small pool) / 1 MB + 512 B (large pool) or more can still be served from -- blocks of falling size
    are taken until the allocator has to reserve new memory for one."""
    held = []
    take = lambda nbytes: held.append(torch.empty((nbytes // 4,), dtype=torch.int32, device=DEV))
    for _ in range(max(2, -(-2 * peak // SMALL_BLOCK))):
        take(SMALL_BLOCK)
    for _ in range(max(2, -(-2 * peak // LARGE_BLOCK))):
        take(LARGE_BLOCK)
    for pool in ("small", "large"):
        for nbytes in SWEEP[pool]:
            for _ in range(4096):
                before = torch.cuda.memory_reserved()
                take(nbytes)
                if torch.cuda.memory_reserved() != before:
                    # a new segment: the block goes back and the segment with it (empty_cache releases the wholly free
                    # segments), or what is left of it would be handed out later as it came from the driver
                    del held[-1]
                    torch.cuda.empty_cache()
                    assert torch.cuda.memory_reserved() <= before
                    break
            else:
                raise AssertionError(f"the cache still serves {nbytes}-byte requests after 4096 of them")
    for t in held:
        t.fill_(_signed(word))
    total = sum(t.numel() * 4 for t in held)
    del held, t
    torch.cuda.synchronize()
    return total


def _poisoned_run(name, word, peak):
    import vidtome_amd  # noqa: F401
    gc.collect()
    _poison(word, peak)
    # the conditions that keep the comparison from passing vacuously: what the allocator hands out next IS the fill ...
    for nbytes in (4096, 4 * MB):
        probe = torch.empty((nbytes // 4,), dtype=torch.int32, device=DEV)
        assert bool((probe == _signed(word)).all()), f"a {nbytes}-byte allocation does not read back as {word:#010x}"
        del probe
    reserved = torch.cuda.memory_reserved()
    rec = FF.run_scenario(name, DEV)
    torch.cuda.synchronize()
    # ... and the forward was handed nothing else
    assert torch.cuda.memory_reserved() == reserved, \
        f"the forward took fresh memory: {torch.cuda.memory_reserved()} bytes reserved against {reserved}"
    del rec.unet
    return rec


@pytest.mark.parametrize("name", sorted(FF.SCENARIOS))
def test_forward_does_not_depend_on_what_its_memory_held(name):
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()                               # (what earlier tests left cached need not be swept)
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    dry = FF.run_scenario(name, DEV)                       # (remove_patch inside: release_workspaces)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del dry.unet
    assert peak > 0 and len(dry) > 30
    seen = {(e[0], e[3]) for e in dry}
    missing = [s for s in REACHES[name] if s not in seen]
    assert not missing, f"scenario {name} does not reach {missing}"
    recs = []
    for word in FILLS:                                     # in this order: an uninitialised index is -1 before it is 15360
        rec = _poisoned_run(name, word, peak)
        assert rec.nonfinite == [], f"fill {word:#010x}: non-finite values at {rec.nonfinite}"
        if recs:
            div = FF.first_divergence(recs[0], rec)
            print(f"poisoned forward {name}: fill {FILLS[0]:#010x} / {word:#010x}: {_describe(div)}")
            assert div is None, f"fill {FILLS[0]:#010x} against {word:#010x}: " + _describe(div)
        recs.append(rec)
    div = FF.first_divergence(dry, recs[0])
    print(f"poisoned forward {name}: {len(dry)} stages, peak {peak} bytes; un-poisoned / {FILLS[0]:#010x}: {_describe(div)}")
    assert div is None, "the un-poisoned run differs from the zero-filled one: " + _describe(div)
