"""CPU test of the operand contract of the attention side exports (vtm_attention_kv_sets / _sets_masked / _sets_src,
vtm_attention_kv_bias, vtm_attention_kv_segments, vtm_attention_probs, vtm_attention_word_map, vtm_attention_key_mass): every
rejection's return code AND whole message, against tests/golden/attention_contract.json.  One table of valid calls on fake
pointers, one list of single-argument violations applied to every export that has the argument and checks it.  Nothing here
gets as far as a launch: every entry is answered VTM_EINVAL by the host checks.

The golden file is a recording of the library's answers (``python tests/test_attention_contract_host.py`` rewrites it from
the built library): a change of any message, or of which check answers first, shows up as a diff of that file."""
import ctypes
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "attention_contract.json")
EINVAL = -1
F16, F32 = 1, 0
INF, NAN = float("inf"), float("nan")

# fake operands: 8 heads of 40 channels, 2 samples of 64 query rows and 64 keys
Q, K, VT, OUT, QSRC, BIAS, W, MASK, ROWS, SEG, WS = (0x10000 * i for i in range(1, 12))
_QKV = dict(q=Q, ldq=320, k=K, ldk=320, vt=VT, ldvt=64, out=OUT, ldo=320)
_SETS = dict(_QKV, dtype=F16, B=2, h=8, Mq=64, Mqp=64, Mkp=64, d=40, scale=40 ** -0.5, n_sets=2, set_start=[0, 32],
             set_len=[32, 32], set_weight=[1.0, 0.5])
_SETS_ARGS = ("q", "ldq", "k", "ldk", "vt", "ldvt", "out", "ldo", "dtype", "B", "h", "Mq", "Mqp", "Mkp", "d", "scale", "n_sets",
              "set_start", "set_len", "set_weight")
_SETS_PTRS = ("q", "k", "vt", "out", "set_start", "set_len", "set_weight")
_MAP = dict(q=Q, ldq=320, k=K, ldk=320, out=OUT, ldo=64, dtype=F16, B=2, h=8, Mq=64, Mqp=64, Mk=64, Mkp=64, d=40,
            scale=40 ** -0.5)
_NO_ROW_BOUND = {"ldq=312", "ldk=312"}     # the planned families take the caller's word that a row holds h * d channels

# export -> args: the C parameters in order (the stream, always last, is null); ok: a call every check accepts; ptrs: the
# pointers that must not be null; aligned: {pointer: an offset that breaks the alignment the export asks of it}; skip: the
# violations of the list below that this export does not check; extra: (label, overrides) of its own
EXPORTS = {
    "vtm_attention_kv_sets": dict(args=_SETS_ARGS, ok=_SETS, ptrs=_SETS_PTRS, aligned={}, skip=_NO_ROW_BOUND, extra=[]),
    "vtm_attention_kv_sets_masked": dict(
        args=_SETS_ARGS + ("set_mask", "mask", "ld_mask", "mask_batch_stride"),
        ok=dict(_SETS, set_mask=[0, -1], mask=MASK, ld_mask=64, mask_batch_stride=64), ptrs=_SETS_PTRS + ("set_mask", "mask"),
        aligned={}, skip=_NO_ROW_BOUND,
        extra=[("set_mask=[0,2]", dict(set_mask=[0, 2])), ("set_mask=[-2,0]", dict(set_mask=[-2, 0])),
               ("ld_mask=63", dict(ld_mask=63)), ("mask_batch_stride=1", dict(mask_batch_stride=1)),
               ("mask_batch_stride=63", dict(mask_batch_stride=63))]),
    "vtm_attention_kv_sets_src": dict(
        args=("q", "ldq", "q_src", "ldq_src", "Mqp_src") + _SETS_ARGS[2:] + ("set_src",),
        ok=dict(_SETS, q_src=QSRC, ldq_src=320, Mqp_src=64, set_src=[0, 1]), ptrs=_SETS_PTRS + ("set_src", "q_src"),
        aligned={"q_src": 8}, skip=_NO_ROW_BOUND,
        extra=[("set_src=[0,2]", dict(set_src=[0, 2])), ("set_src=[-1,1]", dict(set_src=[-1, 1])),
               ("ldq_src=324", dict(ldq_src=324)), ("ldq_src=312", dict(ldq_src=312)), ("Mqp_src=63", dict(Mqp_src=63))]),
    "vtm_attention_kv_bias": dict(
        args=("q", "ldq", "k", "ldk", "vt", "ldvt", "out", "ldo", "dtype", "B", "h", "Mq", "Mqp", "Mk", "Mkp", "d", "scale",
              "bias", "ld_bias", "bias_batch_stride"),
        ok=dict(_QKV, dtype=F16, B=2, h=8, Mq=64, Mqp=64, Mk=64, Mkp=64, d=40, scale=40 ** -0.5, bias=BIAS, ld_bias=64,
                bias_batch_stride=64),
        ptrs=("q", "k", "vt", "out", "bias"), aligned={}, skip=_NO_ROW_BOUND,
        extra=[("Mkp%8", dict(Mkp=68)), ("ldvt<Mk", dict(ldvt=56))]),
    "vtm_attention_kv_segments": dict(
        args=("q", "ldq", "k", "ldk", "vt", "ldvt", "out", "ldo", "dtype", "rows_total", "seg_off", "n_seg", "max_seg_rows", "h",
              "Mk", "Mkp", "d", "scale"),
        ok=dict(_QKV, dtype=F16, rows_total=128, seg_off=SEG, n_seg=2, max_seg_rows=64, h=8, Mk=64, Mkp=64, d=40,
                scale=40 ** -0.5),
        ptrs=("q", "k", "vt", "out", "seg_off"), aligned={}, skip=set(),
        extra=[("Mkp%8", dict(Mkp=68)), ("ldvt<Mk", dict(ldvt=56)), ("ldo=312", dict(ldo=312)),
               ("rows_total=2^31", dict(rows_total=1 << 31))]),
    "vtm_attention_probs": dict(
        args=("q", "ldq", "k", "ldk", "out", "ldo", "dtype", "B", "h", "Mq", "Mqp", "Mk", "Mkp", "d", "scale", "bias", "ld_bias",
              "bias_batch_stride"),
        ok=dict(_MAP, bias=BIAS, ld_bias=64, bias_batch_stride=64), ptrs=("q", "k", "out"),
        aligned={"q": 8, "k": 2, "out": 2}, skip={"ldo=322"},
        extra=[("Mk=257", dict(Mk=257, Mkp=257)), ("h=41", dict(h=41)), ("ldo=63", dict(ldo=63)), ("B=2^31", dict(B=1 << 31))]),
    "vtm_attention_word_map": dict(
        args=("q", "ldq", "k", "ldk", "dtype", "B", "h", "Mq", "Mqp", "Mk", "Mkp", "d", "scale", "bias", "ld_bias",
              "bias_batch_stride", "weights", "ld_w", "w_batch_stride", "out", "ldo", "out_rows", "accumulate"),
        ok=dict(_MAP, bias=BIAS, ld_bias=64, bias_batch_stride=64, weights=W, ld_w=64, w_batch_stride=64, out_rows=ROWS,
                accumulate=1),
        ptrs=("q", "k", "weights", "out"), aligned={"q": 8, "k": 2, "out": 2, "weights": 2, "out_rows": 4}, skip={"ldo=322"},
        extra=[("Mk=257", dict(Mk=257, Mkp=257)), ("h=2^20", dict(h=1 << 20)), ("ldo=63", dict(ldo=63)),
               ("B=2^31", dict(B=1 << 31)), ("ld_w=63", dict(ld_w=63)), ("w_batch_stride=1", dict(w_batch_stride=1)),
               ("w_batch_stride=63", dict(w_batch_stride=63))]),
    "vtm_attention_key_mass": dict(
        args=("q", "ldq", "k", "ldk", "out", "ldo", "dtype", "B", "h", "Mq", "Mqp", "Mk", "Mkp", "d", "scale", "ws", "ws_bytes"),
        ok=dict(_MAP, ws=None, ws_bytes=0), ptrs=("q", "k", "out"), aligned={"q": 8, "k": 2, "out": 2}, skip={"ldo=322"},
        extra=[("Mk=4097", dict(Mk=4097, Mkp=4097)), ("Mq=65537", dict(Mq=65537, Mqp=65537)), ("h=2^20", dict(h=1 << 20)),
               ("ldo=63", dict(ldo=63)), ("B=2^31", dict(B=1 << 31)), ("B=65536", dict(B=65536)),
               ("ws=null", dict(Mq=129, Mqp=129)),
               ("ws short", dict(Mq=129, Mqp=129, ws=WS, ws_bytes=2 * 2 * 64 * 4 - 1)),
               ("ws+2", dict(Mq=129, Mqp=129, ws=WS + 2, ws_bytes=1 << 20))]),
}

# one argument wrong at a time (the operands above otherwise); an entry goes to every export that has all its arguments
VIOLATIONS = [(f"{s}=0", {s: 0}) for s in ("B", "h", "Mq", "Mk", "Mkp", "d", "rows_total", "n_seg", "max_seg_rows")] + [
    ("Mqp<Mq", dict(Mqp=63)), ("Mkp<Mk", dict(Mk=64, Mkp=56)),
    ("scale=0", dict(scale=0.0)), ("scale<0", dict(scale=-1.0)), ("scale=inf", dict(scale=INF)), ("scale=nan", dict(scale=NAN)),
    ("dtype=fp32", dict(dtype=F32)), ("dtype=9", dict(dtype=9)),
    ("ldq=324", dict(ldq=324)), ("ldk=324", dict(ldk=324)), ("ldvt=68", dict(ldvt=68)), ("ldo=322", dict(ldo=322)),
    ("ldq=312", dict(ldq=312)), ("ldk=312", dict(ldk=312)),
    ("ldk=2^24", dict(ldk=1 << 24)), ("ldvt=2^25", dict(ldvt=1 << 25)),                 # the 2 GiB slice bound
    ("ld_bias=63", dict(ld_bias=63)), ("bias_batch_stride=1", dict(bias_batch_stride=1)),
    ("bias_batch_stride=63", dict(bias_batch_stride=63)),
    ("n_sets=0", dict(n_sets=0)), ("n_sets=9", dict(n_sets=9)), ("set_start=4", dict(set_start=[4, 32])),
    ("set_start<0", dict(set_start=[-8, 32])), ("set_len=0", dict(set_len=[32, 0])),
    ("set beyond Mkp", dict(set_len=[32, 40])), ("set beyond ldvt", dict(ldvt=56, set_len=[32, 32])),
    ("set_weight=inf", dict(set_weight=[1.0, INF])), ("set_weight=nan", dict(set_weight=[NAN, 0.5])),
    ("d=24", dict(d=24)),                                                               # a head dim no kernel is built for
]
_ARRAYS = {"set_start": ctypes.c_int64, "set_len": ctypes.c_int64, "set_weight": ctypes.c_float, "set_mask": ctypes.c_int,
           "set_src": ctypes.c_int}


def entries():
    """[(key, export, overrides)] in a fixed order."""
    out = []
    for name, spec in EXPORTS.items():
        ok = spec["ok"]
        assert set(spec["args"]) == set(ok), name
        cases = [(f"{p}=null", {p: None}) for p in spec["ptrs"]]
        cases += [(f"{p}+{off}", {p: ok[p] + off}) for p, off in spec["aligned"].items()]
        cases += [(label, kw) for label, kw in VIOLATIONS if set(kw) <= set(ok) and label not in spec["skip"]]
        cases += spec["extra"]
        assert len({label for label, _ in cases}) == len(cases), name
        out += [(f"{name}|{label}", name, kw) for label, kw in cases]
    return out


def call(L, name, kw):
    """(return code, message) of export `name` on its valid operands with `kw` on top."""
    spec = EXPORTS[name]
    a = dict(spec["ok"], **kw)
    argv = []
    for n in spec["args"]:
        v = a[n]
        if n in _ARRAYS and v is not None:
            v = (_ARRAYS[n] * 9)(*(list(v) + [0] * (9 - len(v))))
        argv.append(v)
    rc = getattr(L, name)(*argv, None)
    return rc, (L.vtm_last_error() or b"").decode()


@pytest.fixture(scope="module")
def built():
    from vidtome_amd import build
    return build.build()


def test_every_rejection_keeps_its_code_and_message(built):
    from vidtome_amd import _lib
    L = _lib.lib()
    golden = json.load(open(GOLDEN))
    todo = entries()
    assert sorted(golden) == sorted(key for key, _, _ in todo)       # the table and the recording name the same cases
    assert all(rc == EINVAL and msg for rc, msg in golden.values())  # (nothing recorded ever reached a launch)
    wrong = []
    for key, name, kw in todo:
        got = call(L, name, kw)
        if list(got) != golden[key]:
            wrong.append((key, got, golden[key]))
    assert not wrong, wrong


def test_the_cases_cover_every_export(built):
    per = {}
    for key, name, _ in entries():
        per.setdefault(name, []).append(key.split("|", 1)[1])
    assert set(per) == set(EXPORTS) and all(len(v) >= 30 for v in per.values()), {k: len(v) for k, v in per.items()}
    for name, labels in per.items():   # what every one of them checks
        for label in ("q=null", "k=null", "out=null", "d=0", "h=0", "scale=nan", "dtype=fp32", "dtype=9", "ldq=324", "ldk=2^24",
                      "d=24"):
            assert label in labels, (name, label)


if __name__ == "__main__":   # record
    sys.path.insert(0, ROOT)
    from vidtome_amd import _lib
    L = _lib.lib()
    rec = {}
    for key, name, kw in entries():
        rc, msg = call(L, name, kw)
        assert rc == EINVAL and msg, (key, rc, msg)   # a case that is not rejected must not be in the table
        rec[key] = [rc, msg]
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(rec), "entries ->", GOLDEN)
