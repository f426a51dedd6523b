"""What the receptive-field mask costs and what the dead-tile skip saves: vtm_match_masked against vtm_match, one JSON line.

    python tools/rf_match.py [--reps 30] [--out profiles/rf_match.json]

F = 4 frames of 64 x 64 tokens, C = 320, B = 2, frame 1 is dst (Ns = 12288, Nd = 4096 per sample: 48 x 32 tiles), tokens in
(frame, position) order with the (y, x) grid as coordinates, rec_field in {2, 8, 1e9 (nothing masked)}.  Per field, event-timed
on the same operands, the variants interleaved repetition by repetition so they share the clock:
  masked   vtm_match_masked (box pre-pass + kernel)
  plain    vtm_match -- the kernel as it was before the mask, the same code object in the same process
once with the dead-tile skip on and once with VTM_DEBUG_NOBOXSKIP=1; the hook is read once per process, so each setting runs in
a fresh child process of this tool (the parent never opens the GPU).  Before timing, each child checks that the masked keys at
rec_field = 1e9 equal vtm_match's, and reports a checksum of the keys per field, which the parent compares between the two
settings.  Reports median and min / max in microseconds and the share of masked pairs; nothing is asserted about the times."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REC_FIELDS = (2, 8, 1e9)
F, SIDE, C, B = 4, 64, 320, 2


def _timed(variants, warmup, reps):
    import torch
    times = {k: [] for k in variants}
    for rep in range(warmup + reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    return {k: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
            for k, v in times.items()}


def child(args):
    import torch
    from vidtome_amd import _lib
    dev = torch.device("cuda")
    hw, N = SIDE * SIDE, F * SIDE * SIDE
    g = torch.Generator().manual_seed(11)
    base = torch.randn(hw, C, generator=g)
    x = (0.5 * base.repeat(F, 1)[None] + torch.randn(B, N, C, generator=g)).to(dev)
    pos = torch.arange(N) % hw
    pool = torch.zeros(B, N, 4)
    pool[:, :, 0], pool[:, :, 1] = (pos // SIDE).float(), (pos % SIDE).float()
    pool = pool.to(dev)
    frame = torch.arange(N) // hw
    a_rows = torch.nonzero(frame != 1).flatten().to(torch.int32).expand(B, -1).contiguous().to(dev)
    b_rows = torch.nonzero(frame == 1).flatten().to(torch.int32).expand(B, -1).contiguous().to(dev)
    Ns, Nd = a_rows.shape[1], b_rows.shape[1]
    a_op, _ = _lib.normalize_gather(x, None, a_rows)
    b_op, _ = _lib.normalize_gather(x, None, b_rows)
    plain = lambda: _lib.match(a_op, b_op, Ns, Nd, False)
    out = {"skip": not os.environ.get("VTM_DEBUG_NOBOXSKIP"), "device": torch.cuda.get_device_name(0), "fields": {}}
    assert torch.equal(_lib.match_masked(a_op, b_op, Ns, Nd, False, pool, a_rows, b_rows, _lib.mask_threshold(1e9)), plain())
    sc, dc = pool[0, a_rows[0].long(), :2], pool[0, b_rows[0].long(), :2]
    for rec in REC_FIELDS:
        T = _lib.mask_threshold(rec)
        masked = lambda: _lib.match_masked(a_op, b_op, Ns, Nd, False, pool, a_rows, b_rows, T)
        keys = masked()
        share = float(((sc[:, None, :] - dc[None, :, :]).square().sum(-1) > T).float().mean())
        entry = _timed({"masked": masked, "plain": plain}, args.warmup, args.reps)
        entry.update(masked_pairs=round(share, 4), checksum=int(keys.sum().item()))
        out["fields"][str(rec)] = entry
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    result = {"tool": "rf_match", "unit": "us", "reps": args.reps,
              "shape": f"F={F} of {SIDE}x{SIDE}, C={C}, B={B}, Ns={(F - 1) * SIDE * SIDE}, Nd={SIDE * SIDE}"}
    for name, hook in (("skip_on", None), ("skip_off", "1")):
        env = {k: v for k, v in os.environ.items() if k != "VTM_DEBUG_NOBOXSKIP"}
        if hook:
            env["VTM_DEBUG_NOBOXSKIP"] = hook
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--warmup",
                            str(args.warmup)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.exit(f"{name}: the child failed ({p.returncode}):\n{p.stdout}")
        result[name] = json.loads(lines[-1][len("RESULT "):])
        assert result[name]["skip"] == (hook is None)
    for rec in result["skip_on"]["fields"]:
        assert result["skip_on"]["fields"][rec]["checksum"] == result["skip_off"]["fields"][rec]["checksum"], rec
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
