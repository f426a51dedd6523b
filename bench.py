#!/usr/bin/env python3
"""Benchmark of the VidToMe token-merging hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

Metric (BASELINE.json): denoising steps/sec for a 16-frame 512x512 SD-1.5 chunk, merge ratio 0.5.
A *step* is one pass of the hot path over one chunk: the patched self-attention segment
``norm1 -> compute_merge -> attn1 -> unmerge -> + residual`` (vidtome/patch.py:139-169) at all 16 SD-1.5
transformer-block sites (10 merged: 5x N=4096/C=320/d=40 and 5x N=1024/C=640/d=80; 6 un-merged at C=1280),
batch 2 (CFG [uncond | cond]) x 16 frames, local merge 0.5 + global merge 0.5 in steady state (the
block's anchor tokens were populated by a preceding chunk, as for every chunk but the first of a step).
Synthetic fp16 hidden states (frame-correlated), random-init weights; inputs are resident in HBM before
the timed region.  The passes rotate over `--chunks` (3) distinct chunks of ONE synthetic clip (shared per-sample base,
independent frame noise), so every pass merges against anchor tokens that came from a DIFFERENT chunk -- the regime of
generate.py:215-219 (`--same-chunk` = rounds 1-2's regime: one chunk fed to every pass, whose anchors are then copies of
its own rows; kept for the A/B under profiles/).  HIP events are recorded around the hot launches on every
`--event-every`-th timed pass only (the other passes run event-free); a background thread samples the GPU's shader
clock and package power during the timed region.
`python bench.py --gpus N` with N > 1 and no launcher starts its N ranks itself (one process per GPU, RCCL, rendezvous
on 127.0.0.1); under torchrun it uses the RANK / LOCAL_RANK / WORLD_SIZE it is given.
N > 1: one process per GPU, each rank runs its own chunk (weak scaling); local merging needs
no collective, the global level takes its anchor tokens from the previous rank's chunk (chunk_parallel.py:
`--exchange neighbour` = point-to-point shift of every rank's local merged tokens over one xGMI link, the default;
`allgather` = the same semantics through an RCCL all-gather per merging block; `ring` = the exact serial chain);
value = chunk-steps per second over all ranks.

A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the line: nothing else.  `--full` adds
what takes runs of its own after the headline region: the matcher's counter pass (matching.counters), the other token
regimes (`regimes`), two chunks in flight (`two_in_flight`), the other BASELINE configurations (`workloads`), the other
exchange modes at N > 1 (`exchange_modes`), the real-UNet probe and the CPU baseline (`cpu_baseline`).

The JSON line also carries
  roofline:     the dominant kernel (attention_kernel: flash attention over the merged tokens, fp16 MFMA), its
                executed FLOPs / HIP-event time over the timed region vs the 2.5 PFLOP/s dense fp16 peak;
  matching:     the fused similarity + top-1 step (fp16-MFMA filter + exact fp32 refine): executed fp16 FLOPs / HIP-event
                time vs the same fp16 peak (the exact fp32-MFMA fallback would be bounded by 157.3 TFLOP/s);
  gather_path:  the HBM-bound kernels (LayerNorm, merge gather, unmerge + residual): algorithmic bytes / HIP-event time
                vs 8 TB/s, next to the counter-derived (rocprofv3 FETCH_SIZE / WRITE_SIZE) rates from profiles/;
  cpu_baseline: (--full) a plain-PyTorch CPU restatement of the same segment (oracle/torch_baseline.py: bmm + max + argsort +
                gather + SDPA, fp32) TIMED on this host's cores on one full site of every kind and summed to a step.
"""
import argparse
import glob
import json
import os
import socket
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# multi-process GPU work on this pool needs dmabuf IPC (RCCL otherwise fails in hipIpcGetMemHandle)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

FP32_PEAK_TFLOPS = 157.3          # MI355X fp32 vector / fp32-MFMA peak (MI355X_MICROARCH.md)
FP16_PEAK_TFLOPS = 2500.0         # dense fp16/bf16 MFMA peak (not the 2:1-sparse marketing figure)
HBM_PEAK_GBPS = 8000.0            # HBM3E spec (~6300 achievable, MI355X_MICROARCH.md)
BATCH, FRAMES, LATENT = 2, 16, (64, 64)
LOCAL_RATIO, GLOBAL_RATIO = 0.5, 0.5
# BASELINE.json's single-GPU configurations.  cfg2 is the one the metric is quoted on (the headline);
# `--workload cfg3 | cfg5` are secondary lines with the same kernel split.  cfg-1 is the reference's CPU plumbing case and
# cfg-4 is the 8-GPU case (`--frames 8` gives one of its chunks): parity-test cases, not bench lines.
WORKLOADS = {
    "cfg2": dict(sites="sd15", batch=2, frames=16, latent=(64, 64), local=0.5, glob=0.5, align=False, pnp=False,
                 label="SD-1.5 16 frames 512x512 (cfg-2)"),
    "cfg3": dict(sites="sd15", batch=3, frames=16, latent=(64, 64), local=0.5, glob=0.5, align=True, pnp=True,
                 label="SD-1.5 + PnP injection, 16 frames 512x512, batch 3 [source | uncond | cond], align_batch, shared attention "
                       "probabilities at the 8 decoder sites of pnp_utils.py:98-105 (cfg-3; the 7 un-patched ControlNet blocks are "
                       "not on the path)"),
    "cfg5": dict(sites="sd21", batch=2, frames=16, latent=(96, 96), local=0.6, glob=0.6, align=False, pnp=False,
                 label="SD-2.1-768 16 frames 768x768, head dim 64, merge ratio 0.6 (cfg-5)"),
}
# SURVEY.md 8d names two synthetic inputs: N(0,1) (`n01`) and base + 0.1 N(0,1) (`corr01`, "realistic high cross-frame
# cosine").  `value` is quoted on corr01 -- the input that looks like video -- and it is the FASTER of the two since round 5
# (the scout / position-order plans prune it best): the line therefore also carries `value_worst_named` = the slower of the two
# at top level, and `regimes` holds corr05 (the headline regime of rounds 1-4) next to them.
HEADLINE_REGIME = "corr01"
# untimed passes in front of a secondary regime's region: the launch planners (merge.MatchPlanner, one per block and level)
# start every regime afresh, spend one exploring call each -- the global level's first one comes with the first anchors -- and
# read its counters a call later; in a real run that happens once per 256 calls of a level, in a ten-pass region it would be a
# tenth of the time
REGIME_WARMUP = 5
DUMP_BYTES = 48 << 20             # --dump-outputs: total size of the written arrays (float32)
REGIME_NOTES = {
    "n01": "h ~ N(0,1), frames uncorrelated (SURVEY 8d)",
    "corr01": "h[f] = base + 0.1 N(0,1) (SURVEY 8d: realistic cross-frame cosine)",
    "corr002": "h[f] = base + 0.02 N(0,1) (static shot: cross-frame cosine ~0.9996)",
    "corr05": "h[f] = base + 0.5 N(0,1) (the headline regime of rounds 1-4)",
    "smooth": "spatially low-passed field drifting sub-pixel per frame + 0.05 N(0,1)",
    "flat25": "corr05 + a flat region over a quarter of every frame (candidate-list overflow -> exact escape)",
    "dup": "corr05 + a fifth of the positions exact copies of others"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, run every secondary measurement too: the matcher's counter pass, the CPU "
                         "baseline, the other token regimes, two chunks in flight, the other workloads and exchange modes")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--cpu-seconds", type=float, default=90.0,
                    help="time budget of the CPU baseline: a top site whose full batch would not fit is timed on one "
                         "batch sample and doubled")
    ap.add_argument("--cpu-baseline", choices=["torch", "port"], default="torch",
                    help="torch = plain-PyTorch restatement, timed on full sites; port = the C/OpenMP oracle, row slices")
    ap.add_argument("--exchange", choices=["neighbour", "allgather", "ring"], default=None,
                    help="how the global level gets its anchor tokens (chunk_parallel.py); default: neighbour at N > 1, "
                         "none at N = 1 (the reference's chained anchors).  Given explicitly at N = 1 (neighbour / ring) the "
                         "single rank runs the same protocol in place -- the N = 1 point of that mode's scaling curve")
    ap.add_argument("--local-only", action="store_true", help="merge_global=False variant (not the headline)")
    ap.add_argument("--chunks", type=int, default=3,
                    help="distinct chunks of the synthetic clip the passes rotate over (anchors come from another chunk)")
    ap.add_argument("--chunks-per-step", type=int, default=8,
                    help="N = 1: chunks of a denoising step -- the anchor chain is re-seeded every chunks_per_step - 1 "
                         "passes with the first chunk's local tokens (the reference resets the anchors after every step)")
    ap.add_argument("--frames", type=int, default=FRAMES,
                    help="frames per chunk (16 = the headline cfg-2 chunk; 8 = one of cfg-4's eight chunks -- not the headline)")
    ap.add_argument("--full-block", action="store_true",
                    help="secondary measurement (NOT the headline): every pass runs the WHOLE patched block at the 16 sites -- "
                         "the hot-path segment plus the cross-attention over 77 text tokens and the GEGLU feed-forward "
                         "(patch.py:171-199)")
    ap.add_argument("--same-chunk", action="store_true",
                    help="rounds 1-2's regime: every pass processes the same chunk (anchors = copies of its own rows)")
    ap.add_argument("--data", default=HEADLINE_REGIME, choices=sorted(REGIME_NOTES),
                    help="synthetic token regime of the headline (vidtome_amd/sites.DATA_REGIMES): n01 = N(0,1) and corr01 = base + "
                         "0.1 N(0,1) are the two SURVEY.md 8d names (corr01, the harder one, is the default); corr05 = base + 0.5 "
                         "N(0,1) is what rounds 1-4 quoted; corr002 / smooth = static / smooth content; flat25 / dup load the "
                         "matcher's candidate logic")
    ap.add_argument("--regimes", default="all",
                    help="--full, N = 1: the other token regimes measured after the headline and reported under `regimes` "
                         "(comma-separated names, `all`, or `none`)")
    ap.add_argument("--regime-steps", type=int, default=10, help="timed passes per secondary regime")
    ap.add_argument("--workloads", default="all",
                    help="--full, N = 1 headline run: secondary workloads appended to the line as `workloads` (each in a child "
                         "process of this script): all | none | comma list of cfg3,cfg5,full_block")
    ap.add_argument("--workload-steps", type=int, default=10, help="timed passes per secondary workload")
    ap.add_argument("--no-inflight-line", dest="inflight_line", action="store_false",
                    help="--full, N = 1: skip the secondary `two_in_flight` region (two chunks on two HIP streams)")
    ap.add_argument("--inflight", type=int, default=1,
                    help="N = 1 A/B: run the HEADLINE region with this many chunks in flight (the line then says so in "
                         "config.parallelism; the default line keeps `value` on one stream)")
    ap.add_argument("--workload", default="cfg2", choices=sorted(WORKLOADS),
                    help="cfg2 = the headline configuration; cfg3 / cfg5 = secondary lines (BASELINE.json configs[2] / [4])")
    ap.add_argument("--exchange-modes", default="all",
                    help="--full, N > 1: after the headline's exchange mode, time the other modes too and report them under "
                         "`exchange_modes` (comma-separated, `all`, or `none`); a mode that makes no progress is reported as such "
                         "and the headline line is still printed")
    ap.add_argument("--watchdog-seconds", type=float, default=120.0,
                    help="N > 1: a rank that makes no progress for this long prints where it is stuck (pass, block, exchange "
                         "phase, peer) and exits with code 3 (0 = off)")
    ap.add_argument("--event-every", type=int, default=5,
                    help="record HIP events around the hot launches on every k-th timed pass (the others are event-free)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the headline region, write what its LAST timed pass returned (the output of every site) as "
                         "DIR/<name>.npy in float32 (whole when small, else a fixed seeded sample of token rows, all channels; "
                         f"{DUMP_BYTES >> 20} MB in all) plus DIR/moments.npy over every element.  Same arguments -> same "
                         "inputs, so two builds compare output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def dump_outputs(outs, site_list, out_dir: str, rank: int, world: int) -> None:
    """`outs`: the per-site (B*F, N, C) outputs of one pass.  Each site gets an equal share of DUMP_BYTES (split over the
    ranks too); a site whose output is larger keeps the token rows numpy.random.default_rng(site index) picks, in row
    order -- the same rows for the same shapes on every run.  `moments.npy` (float64, one row per site: sum, sum |x|,
    sum x^2, max |x|) covers every element of the outputs, sampled or not."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_BYTES // (len(outs) * world)
    prefix = f"rank{rank}_" if world > 1 else ""
    moments = []
    for i, (o, s_) in enumerate(zip(outs, site_list)):
        rows = o.reshape(-1, o.shape[-1])
        x = rows.double()
        moments.append([x.sum().item(), x.abs().sum().item(), (x * x).sum().item(), x.abs().max().item()])
        del x
        keep = max(1, share // (4 * rows.shape[1]))
        if keep < rows.shape[0]:
            pick = np.sort(np.random.default_rng(i).choice(rows.shape[0], keep, replace=False))
            rows = rows[torch.from_numpy(pick).to(rows.device)]
        np.save(os.path.join(out_dir, f"{prefix}site{i:02d}_{s_.name}.npy"), rows.float().cpu().numpy())
    np.save(os.path.join(out_dir, f"{prefix}moments.npy"), np.array(moments, dtype=np.float64))


def self_launch(args) -> int:
    """`python bench.py --gpus N` without a launcher: start the N ranks (one process per GPU) and wait for them.
    Rank 0 prints the JSON line on the inherited stdout.  Returns the first non-zero exit code (the other ranks are
    then terminated by PID), 0 otherwise."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus),
                   LOCAL_WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   VIDTOME_BENCH_LAUNCHER="self")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc, live = 0, list(procs)
    while live:
        time.sleep(0.05)
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0 and rc == 0:
                rc = code
                for other in live:                      # a rank died: do not leave the others in a collective
                    other.terminate()
    return rc


class BoxSampler(threading.Thread):
    """Shader clock and package power of the GPU this rank runs on, sampled from sysfs (amdgpu hwmon) during the
    timed region: the dominant kernels are power-limited (profiles/HISTORY.md section 10), so the number belongs next to the
    roofline fraction -- measured on THIS box, in THIS run."""

    def __init__(self, device_index: int, period_s: float = 0.05):
        super().__init__(daemon=True)
        self.period = period_s
        self.samples = []
        self._halt = threading.Event()
        self.files = self._find(device_index)

    @staticmethod
    def _find(device_index: int):
        want = None
        try:
            pr = torch.cuda.get_device_properties(device_index)
            want = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}"
        except Exception:
            pass
        cands = []
        for card in sorted(glob.glob("/sys/class/drm/card[0-9]*")):
            devp = os.path.realpath(os.path.join(card, "device"))
            for hw in glob.glob(os.path.join(devp, "hwmon", "hwmon*")):
                pw = next((f for f in (os.path.join(hw, n) for n in ("power1_average", "power1_input")) if os.path.exists(f)), None)
                fq = os.path.join(hw, "freq1_input")
                if pw or os.path.exists(fq):
                    cands.append((devp, pw, fq if os.path.exists(fq) else None))
        if not cands:
            return None
        for devp, pw, fq in cands:
            if want and want in devp:
                return pw, fq
        return cands[min(device_index, len(cands) - 1)][1:]

    def run(self):
        if not self.files:
            return
        pw, fq = self.files
        while not self._halt.is_set():
            try:
                w = int(open(pw).read()) / 1e6 if pw else None
                f = int(open(fq).read()) / 1e6 if fq else None
                self.samples.append((w, f))
            except Exception:
                pass
            self._halt.wait(self.period)

    def stop(self):
        self._halt.set()
        if self.is_alive():
            self.join(timeout=2.0)
        if not self.samples:
            return None
        out = {"samples": len(self.samples), "period_ms": self.period * 1e3, "source": "sysfs amdgpu hwmon (power1_average, freq1_input)"}
        for name, idx in (("power_w", 0), ("sclk_mhz", 1)):
            v = [s_[idx] for s_ in self.samples if s_[idx] is not None]
            if v:
                out[name] = {"mean": round(sum(v) / len(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
        return out


class Watchdog(threading.Thread):
    """N > 1: a rank stuck in a collective / point-to-point transfer would otherwise burn the driver's whole timeout
    without a word.  The main thread ticks after every pass; when nothing has ticked for `limit_s` the watchdog prints
    where the rank is (pass, and the exchange's last bookkeeping entry: block key, phase, peer rank) and ends the process
    with code 3 -- the launcher (self_launch / torchrun) then takes the other ranks down."""

    def __init__(self, rank: int, limit_s: float, where):
        super().__init__(daemon=True)
        self.rank, self.limit, self.where = rank, limit_s, where
        self.last = time.monotonic()
        self.label = "start-up"
        self.phase = None              # set while the SECONDARY exchange modes run
        self.fallback = None           # ... together with what to do instead of failing (rank 0: print the headline line)
        self._halt = threading.Event()

    def tick(self, label: str) -> None:
        self.last, self.label = time.monotonic(), label

    def run(self):
        while not self._halt.wait(1.0):
            idle = time.monotonic() - self.last
            if idle > self.limit:
                sys.stderr.write(f"bench.py watchdog: rank {self.rank} made no progress for {idle:.0f} s after '{self.label}'; "
                                 f"exchange state: {self.where()}\n")
                sys.stderr.flush()
                if self.fallback is not None:      # a secondary exchange mode hung: the headline was measured, keep it
                    sys.stderr.write(f"bench.py watchdog: exchange mode '{self.phase}' abandoned, headline line kept\n")
                    sys.stderr.flush()
                    self.fallback()
                    os._exit(0)
                os._exit(3)

    def stop(self):
        self._halt.set()


class KernelTimer:
    """HIP events around the hot kernels' launches, recorded on the launch stream (torch's current stream):
    `attention` = vtm_attention (one kernel), `matching` = vtm_match_filtered / vtm_match (the fused
    score + top-1 step; the filtered variant is filter + refine kernels)."""

    def __init__(self, lib_mod):
        self.lib_mod = lib_mod
        self.orig = {}
        self.records = {"attention": [], "matching": [], "layernorm": [], "gather_rows": [], "unmerge_add": [],
                        "projections": [], "ff_geglu": [], "linear_panels": [], "layernorm_panels": []}
        self.enabled = False
        self.ref_flops = 0.0           # attention flops of the same launches had every merged row been a query

    def _wrap(self, name, kind, flops_of):
        orig = getattr(self.lib_mod, name)
        self.orig[name] = orig

        def timed(*a, **k):
            if not self.enabled:
                return orig(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = orig(*a, **k)
            e1.record()
            self.records[kind].append((flops_of(*a, **k), e0, e1))
            return out
        setattr(self.lib_mod, name, timed)

    def __enter__(self):
        # attention(q, k, vt, heads, M, scale, share): 4 * B * M^2 * C flops (QK^T + PV, all heads)
        def sa_flops(q, k, vt, heads, M, scale, share=1):
            f = 4.0 * q.shape[0] * M * M * q.shape[2]
            self.ref_flops += f
            return f
        self._wrap("attention", "attention", sa_flops)
        # attention_kv(q, k, vt, heads, Mq, Mk, scale): 4 * B * Mq * Mk * C executed flops
        # (with a device-side query bound the executed rows are the per-sample counts, rounded up to whole query blocks
        # of 256 (d <= 48) / 512 (d <= 96) / 128 queries: read back AFTER the timed region)
        def kv_flops(q, k, vt, heads, Mq, Mk, scale, use_workspace=True, q_count=None, k_fold=None, share_groups=1):
            self.ref_flops += 4.0 * q.shape[0] * (Mk * Mk if Mq > 256 and Mk > Mq else Mq * Mk) * q.shape[2]
            if q_count is None and k_fold is None:
                return 4.0 * q.shape[0] * Mq * Mk * q.shape[2]
            d = q.shape[2] // heads
            qb = 256 if d <= 48 else 512 if d <= 96 else 128
            # (clones: the workspace-free tensors may be recycled by the allocator before the read-back)
            keep = q_count.clone() if q_count is not None else None
            kkeep = k_fold[0].clone() if k_fold is not None else None     # folded keys: a device-side KEY count too

            def executed():
                B = q.shape[0]
                qn = ((keep.cpu().long() + qb - 1) // qb * qb).clamp(max=Mq) if keep is not None else torch.full((B,), Mq)
                kn = ((kkeep.cpu().long() + 63) // 64 * 64).clamp(max=Mk) if kkeep is not None else torch.full((B,), Mk)
                if kkeep is not None:
                    self.folded_keys.append((int(kkeep.cpu().long().sum()), B * Mk))
                return 4.0 * float((qn * kn).sum()) * q.shape[2]
            return executed
        self.folded_keys = []
        self._wrap("attention_kv", "attention", kv_flops)
        # match_filtered(x0, x1, a_rows, b_rows, align): 2 * B * Ns * Nd * C algorithmic flops
        self._wrap("match_filtered", "matching",
                   lambda x0, x1, ar, br, align, want_flag=False, seed=None, **kw: 2.0 * x0.shape[0] * ar.shape[1] * br.shape[1] * x0.shape[2])
        # the matcher's device-side counters (refined pairs, escaped rows) come from ONE extra, untimed pass after the timed
        # region (`count`): the read-back is a small device copy per call that must not sit inside the event brackets
        timed_match = self.lib_mod.match_filtered
        self.match_flags = []

        self.count = False             # set for ONE untimed pass after the timed region
        self.plan_modes = []           # the launch plan merge.MatchPlanner chose for each call of that pass
        self.plan_scouts, self.plan_ordered = [], []    # ... the scout's depth (1 = one channel step), position-ordered rows?

        def match_with_counters(x0, x1, ar, br, align, want_flag=False, seed=None, **kw):
            if not self.count or want_flag:
                return timed_match(x0, x1, ar, br, align, want_flag, seed=seed, **kw)
            # the counter pass reads the ONE-LAUNCH plan's counters (blocks tested / alive at the 40 % test of every tile) as
            # a device tensor; which plan the timed passes took is reported separately (matching.plan)
            kw.pop("stats_host", None)
            self.plan_modes.append(kw.pop("mode", 0))
            self.plan_scouts.append(kw.pop("scout_steps", 0))
            self.plan_ordered.append(kw.get("order") is not None)
            best, flag = timed_match(x0, x1, ar, br, align, True, seed=seed, **kw)     # (kw: the position order's inverse maps)
            self.match_flags.append((flag, ar.shape[1] if align else x0.shape[0] * ar.shape[1], x0.shape[2]))
            return best
        self.lib_mod.match_filtered = match_with_counters
        self._wrap("match", "matching", lambda a, b, Ns, Nd, align: 2.0 * a.shape[0] * Ns * Nd * a.shape[1] * 8)
        # the position sort in front of levels 2 / global (vtm_position_order) is matcher time (its calls are not counted as
        # matcher calls: `order_calls`)
        self.records["position_order"] = []
        self._wrap("position_order", "position_order", lambda *a, **k: 0.0)
        # the HBM-bound kernels: algorithmic BYTES per call (rows read + rows written, indices ignored)
        esz = lambda t: t.element_size()
        self._wrap("layernorm", "layernorm", lambda x, w, b, eps: 2.0 * x.numel() * esz(x))
        self._wrap("gather_rows", "gather_rows",
                   lambda x0, x1, idx, pad_to=1: 2.0 * idx.numel() * x0.shape[2] * esz(x0))
        # linear_rows(x0, x1, rows, rows2, n, weight, bias, ...): 2 B n K N flops (the gather-fused projection GEMMs)
        self._wrap("linear_rows", "projections",
                   lambda x0, x1, rows, rows2, n, weight, bias=None, transposed=False, pad_to=8, out=None:
                   2.0 * x0.shape[0] * n * weight.shape[0] * weight.shape[1])
        # panel GEMMs of the full block (csrc/ff.hip): flops = 2 n K (rows of the weight operand)
        self._wrap("ff_geglu", "ff_geglu", lambda xp, n, w1, D, bias: 2.0 * n * xp.shape[0] * 8 * 2 * D)
        self._wrap("linear_panels", "linear_panels", lambda xp, n, w, N, bias, resid=None, out=None: 2.0 * n * xp.shape[0] * 8 * N)
        self._wrap("layernorm_panels", "layernorm_panels", lambda x, w, b, eps: 2.0 * x.numel() * esz(x))
        self._wrap("unmerge_add", "unmerge_add",
                   lambda y, inv, resid: (2.0 + (resid is not None)) * inv.numel() * y.shape[2] * esz(y))
        # everything else the path launches (index algebra, sort, panel writers, query compaction): time only, so that the
        # components of the line add up to the step
        for name in ("sort_desc", "partition_local", "partition_global", "plan_apply", "compose", "decode_best",
                     "compact_queries", "fold_keys", "anchor_pos", "anchor_maps", "transpose_cols", "to_panels", "gather_panels", "geglu", "normalize_gather"):
            if hasattr(self.lib_mod, name):
                self.records[name] = []
                self._wrap(name, name, lambda *a, **k: 0.0)
        return self

    def __exit__(self, *exc):
        for name, fn in self.orig.items():
            setattr(self.lib_mod, name, fn)

    def _resolve(self):
        for kind, rec in self.records.items():
            self.records[kind] = [((r[0]() if callable(r[0]) else r[0]), r[1], r[2]) for r in rec]

    def summary(self, kind):
        self._resolve()
        rec = self.records[kind]
        flops = sum(r[0] for r in rec)
        ms = sum(r[1].elapsed_time(r[2]) for r in rec)
        return flops, ms, len(rec)

    def match_counters(self):
        """(refined pairs per src row, escaped rows, whole-call escapes, src rows) of the counter pass."""
        if not getattr(self, "match_flags", None):
            return None
        f = torch.stack([fl for fl, _, _ in self.match_flags]).cpu().long()
        rows = sum(r for _, r, _ in self.match_flags)
        out = {"scout_range_calls": int(sum(1 for m_ in self.plan_modes if m_ == 1)),
               "shallow_scout_calls": int(sum(1 for m_, k_ in zip(self.plan_modes, self.plan_scouts) if m_ == 1 and k_ > 0)),
               "position_ordered_calls": int(sum(self.plan_ordered)),
               "refined_pairs_per_src_row": round(float(f[:, 3].sum()) / rows, 3),
               "escaped_rows": int(f[:, 2].sum()), "escaped_row_fraction": round(float(f[:, 2].sum()) / rows, 5),
               "whole_call_escapes": int(f[:, 0].sum()), "calls": len(self.match_flags)}
        # partial-sum pruning of filter_kernel: flags[4] = 32 x 32 score blocks tested after KP of the KT 64-channel steps of
        # their dst tile, flags[5] = blocks still alive after the test (the others skip their remaining MFMAs).  Calls whose
        # rows are too short to prune (KT < 4) test nothing and execute everything.
        tested, alive, mfma_all, mfma_done = 0, 0, 0.0, 0.0
        for (fl, _, C), fr in zip(self.match_flags, f):
            KT = (C + 63) // 64
            KP = (2 * KT + 2) // 5 if KT >= 4 else 0
            t, a = int(fr[4]), int(fr[5])
            tested, alive = tested + t, alive + a
            if t > 0 and 0 < KP < KT:
                mfma_all += t * KT
                mfma_done += t * KP + a * (KT - KP)
        if tested > 0:
            out["blocks_tested"] = tested
            out["pruned_block_fraction"] = round(1.0 - alive / tested, 4)
            out["executed_mfma_fraction"] = round(mfma_done / mfma_all, 4) if mfma_all else None
            out["pruning_note"] = ("32 x 32 score blocks of the calls that prune (C >= 256): fraction whose remaining MFMAs were "
                                   "skipped at the test depth, and the fraction of the nominal MFMA work executed")
        return out

    def ms_by_kind(self):
        """{kind: total HIP-event ms} of every wrapped launch kind that ran."""
        self._resolve()
        return {k: sum(r[1].elapsed_time(r[2]) for r in rec) for k, rec in self.records.items() if rec}

    def largest(self, kind):
        """(flops, average ms, count) of the launches with the most work -- the top-block launches, whose average
        duration is what the rocprofv3 summary under profiles/ lists for the same kernel instantiation."""
        self._resolve()
        rec = self.records[kind]
        if not rec:
            return 0.0, 0.0, 0
        # (launches of the largest shape: a device-side query bound lowers the executed flops of some of them)
        top = max(r[0] for r in rec)
        sel = [r for r in rec if r[0] >= 0.75 * top]
        return sum(r[0] for r in sel) / len(sel), sum(r[1].elapsed_time(r[2]) for r in sel) / len(sel), len(sel)


def _profile_json(name):
    try:
        with open(os.path.join(ROOT, "profiles", name)) as f:
            return json.load(f), name
    except Exception:
        return None, None


def pmc_traffic():
    """HBM bytes per launch of the dominant kernel's largest configuration (top-block attention: 34 816 live queries
    x 52 224 keys).  NOT measured in this run: read from the committed rocprofv3 PMC passes under profiles/
    (FETCH_SIZE doubled per the gfx950 note + WRITE_SIZE, separate --pmc runs of tools/kbench.py on the same shape).
    Returns (bytes or None, source string)."""
    for fname in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json",
                  "r01_pmc_traffic.json"):
        d, src = _profile_json(fname)
        if not d:
            continue
        for key in sorted(d, reverse=True):
            # (round 6: the bench's d = 40 launches are attention16s_kernel; older profiles hold attention_kernel's)
            if key.split("<")[0] in ("attention16s_kernel", "attention_kernel") and "<half,40> B=2 h=8 Mq=34816 Mk=52224" in key \
                    and "hbm_bytes_per_launch" in d[key]:
                return int(d[key]["hbm_bytes_per_launch"]), f"profiles/{src}: {key} (rocprofv3 --pmc, not this run)"
    return None, None


def pmc_gather_path():
    """Counter-derived HBM rates of the gather-path kernels at working sets beyond the 256 MB Infinity Cache
    (profiles/r02_pmc_traffic.json, section "gather_path"); None when the profile is absent."""
    d = src = None
    for fname in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json"):
        d, src = _profile_json(fname)
        if d and "gather_path" in d:
            break
    if not d or "gather_path" not in d:
        return None
    out = dict(d["gather_path"])
    out["source"] = f"profiles/{src} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes; not this run)"
    return out


def probe_real_unet():
    """Is a real SD-1.5 UNet available on this box?  Needs the `diffusers` package AND local weights (there is no network):
    a directory named by VIDTOME_SD15_UNET (a `UNet2DConditionModel.from_pretrained` folder), or a cached snapshot under
    HF_HOME.  Returns what was found; when both exist the patched UNet's forward is timed by tools/real_unet.py (not part
    of the headline: the site harness is the step the contract names)."""
    import importlib.util
    have_pkg = importlib.util.find_spec("diffusers") is not None
    path = os.environ.get("VIDTOME_SD15_UNET", "")
    if not path:
        hub = os.path.join(os.environ.get("HF_HOME", os.path.expanduser("~/.cache/huggingface")), "hub")
        cands = glob.glob(os.path.join(hub, "models--runwayml--stable-diffusion-v1-5", "snapshots", "*", "unet")) + \
            glob.glob(os.path.join(hub, "models--stable-diffusion-v1-5--stable-diffusion-v1-5", "snapshots", "*", "unet"))
        path = cands[0] if cands else ""
    have_weights = bool(path) and os.path.isdir(path)
    return {"diffusers_importable": have_pkg, "sd15_unet_weights": path if have_weights else None,
            "timed_in_real_unet": False,
            "note": "the site harness is the step (SURVEY.md 8d)" + ("" if have_pkg and have_weights else
                    ": diffusers and / or local SD-1.5 weights are not present on this box (no network)")}


def cpu_baseline_port(target_seconds: float):
    """`--cpu-baseline port`: time the C/OpenMP CPU oracle on a bounded sample of the cfg-2 step and extrapolate to the whole step.
    Sample: for one top site (N=4096, C=320) and one mid site (N=1024, C=640): the three matching levels on a
    slice of src rows, the attention on a slice of query rows, and the projections on a slice of rows; the
    un-merged sites are cheap and measured on one site each.  Everything is scaled by (full rows / sampled
    rows) x (sites of that kind)."""
    import numpy as np
    from oracle import oracle
    oracle.build()
    cores = oracle.num_threads()
    rng = np.random.default_rng(0)
    total = 0.0
    spent = 0.0
    detail = {}
    scale_rows = max(0.25, min(target_seconds, 20.0) / 20.0)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def two_point(fn, r, full):
        """t(rows) = fixed + slope * rows measured at r and 2r (the fixed part -- operand transposes, thread
        start-up -- must not be multiplied by the extrapolation factor)."""
        nonlocal spent
        t1, t2 = timed(lambda: fn(r)), timed(lambda: fn(2 * r))
        spent += t1 + t2
        slope = max(t2 - t1, 0.0) / r
        fixed = max(t1 - slope * r, 0.0)
        return fixed + slope * full

    for kind, N, C, heads, nsites in (("top", 4096, 320, 8, 5), ("mid", 1024, 640, 8, 5)):
        L = FRAMES * N
        levels = [(3 * L // 4, L // 4)]                                     # level 1: 12 src / 4 dst frames
        U1 = levels[0][0] - int(levels[0][0] * LOCAL_RATIO)
        levels.append((3 * N, N + U1))                                       # level 2
        Ml = (levels[1][0] - int(levels[1][0] * LOCAL_RATIO)) + levels[1][1]
        levels.append((Ml, Ml))                                              # global (square)
        M = (Ml - int(Ml * GLOBAL_RATIO)) + Ml
        t_kind = 0.0
        for (Ns, Nd) in levels:
            a = rng.standard_normal((BATCH, Ns, C)).astype(np.float32)
            b = rng.standard_normal((BATCH, Nd, C)).astype(np.float32)
            r = int(min(Ns // 2, max(256, 32 * cores * scale_rows)))
            t_kind += two_point(lambda rows: oracle.match(a, b, rows=(0, rows)), r, Ns)
        q = rng.standard_normal((BATCH, M, C)).astype(np.float32)
        r = int(min(M // 2, max(64, 16 * cores * scale_rows)))
        t_kind += two_point(lambda rows: oracle.attention(q, q, q, heads, rows=(0, rows)), r, M)
        w = rng.standard_normal((C, C)).astype(np.float32)
        r = min(M // 2, 4096)
        t_kind += two_point(lambda rows: [q[:, :rows] @ w for _ in range(4)], r, M)
        detail[kind] = round(t_kind, 2)
        total += t_kind * nsites
    # un-merged sites: per-frame attention, N=256 (5 sites) and N=64 (1 site), C=1280
    for N, nsites in ((256, 5), (64, 1)):
        C, heads = 1280, 8
        x = rng.standard_normal((4, N, C)).astype(np.float32)
        w = rng.standard_normal((C, C)).astype(np.float32)
        t = timed(lambda: (oracle.attention(x, x, x, heads), [x.reshape(-1, C) @ w for _ in range(4)]))
        spent += t
        total += t * (BATCH * FRAMES / 4) * nsites
    return {"value": 1.0 / total, "unit": "steps/s", "cores": cores, "kind": "port",
            "sample": f"oracle (C/OpenMP fp32) on {cores} host threads: matching on row slices of the 3 levels, "
                      f"attention on query-row slices, projections on row slices of one top and one mid site "
                      f"(+1 un-merged site each), {spent:.1f} s measured, extrapolated to the full 16-site step "
                      f"({total:.0f} s/step)",
            "seconds_per_step_estimate": round(total, 1)}


def cpu_baseline_torch(budget_s: float):
    """The reference's PyTorch CPU path, restated (oracle/torch_baseline.py), TIMED on this host: one full site of
    every kind of the cfg-2 step in steady state (anchors populated), fp32, torch's default intra-op threads (the physical cores); a step = sum over the 16
    sites.  Nothing is extrapolated from slices; if the top site's full batch would exceed the budget it is timed on
    one of the two batch samples and doubled (every operation of the path is independent per sample)."""
    from oracle import torch_baseline as tb
    from vidtome_amd import sites
    # torch's own default intra-op thread count (= the physical cores it detects): what the reference would run with
    args = {"max_downsample": 2, "target_stride": 4, "local_merge_ratio": LOCAL_RATIO, "merge_global": True,
            "global_merge_ratio": GLOBAL_RATIO, "global_rand": 0.5}
    r = tb.time_step(BATCH, FRAMES, LATENT, sites.sd15_sites(), args, budget_s)
    cpu = ""
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next((ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")), "")
    except Exception:
        pass
    how = "every site kind timed in full" if not r["sampled"] else \
        f"site kinds {r['sampled']} timed on 1 of {BATCH} batch samples and doubled, the others in full"
    return {"value": 1.0 / r["seconds_per_step"], "unit": "steps/s", "cores": torch.get_num_threads(),
            # "port" in the contract's sense (the oracle's restatement, not the reference's own files -- the reference is
            # Python and cannot travel to the GPU box); `port_of` says which restatement
            "kind": "port", "port_of": "plain-PyTorch restatement (oracle/torch_baseline.py), the reference's own tensor ops",
            "cpu": cpu,
            "sample": f"plain-PyTorch fp32 restatement of the segment (LayerNorm, normalise, bmm score matrix, max, "
                      f"argsort, gather / scatter merge + unmerge, global level, Linear projections, SDPA) on "
                      f"{torch.get_num_threads()} host threads, one site of each of the 4 kinds of the cfg-2 step in steady "
                      f"state, {how}; per kind one untimed warm-up pass + the median of two timed passes; "
                      f"{r['spent']:.1f} s of CPU work -> {r['seconds_per_step']:.1f} s per 16-site step",
            "seconds_per_step": round(r["seconds_per_step"], 2), "detail": r["detail"]}


PNP_SITES = ("up1.1", "up1.2", "up2.0", "up2.1", "up2.2", "up3.0", "up3.1", "up3.2")   # pnp_utils.py:98-105


def main():
    global FRAMES, BATCH, LATENT, LOCAL_RATIO, GLOBAL_RATIO
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args))
    wl = WORKLOADS[args.workload]
    BATCH, LATENT, LOCAL_RATIO, GLOBAL_RATIO = wl["batch"], wl["latent"], wl["local"], wl["glob"]
    FRAMES = args.frames
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the product path)")
    # VIDTOME_BENCH_BACKEND=gloo is a test hook: it lets the N > 1 code path run on a box with fewer GPUs than
    # ranks (the ranks then share devices); the driver's runs use RCCL with one GPU per rank
    backend = os.environ.get("VIDTOME_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank %= torch.cuda.device_count()
    elif local_rank >= torch.cuda.device_count():
        raise SystemExit(f"bench.py: rank {rank} needs cuda:{local_rank} but this node has {torch.cuda.device_count()} "
                         f"GPU(s) (one process per GPU over RCCL)")
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)    # backend "nccl" is RCCL on ROCm
        else:
            dist.init_process_group(backend)

    import vidtome_amd
    from vidtome_amd import _lib, sites

    site_list = sites.sd15_sites() if wl["sites"] == "sd15" else sites.sd21_sites()
    unet = sites.SiteUNet(site_list, seed=0, full=args.full_block).to(device=dev, dtype=torch.float16)
    vidtome_amd.apply_patch(unet, local_merge_ratio=LOCAL_RATIO, merge_global=not args.local_only,
                            global_merge_ratio=GLOBAL_RATIO, batch_size=BATCH, target_stride=4, global_rand=0.5,
                            align_batch=wl["align"])
    unet.set_size(LATENT)
    if wl["pnp"]:      # what pnp.register_attention_control + register_time leave on the decoder blocks at an injection timestep
        for blk, s_ in zip(unet.blocks, site_list):
            if s_.name in PNP_SITES:
                blk.attn1.injection_schedule, blk.attn1.t, blk.attn1.vtm_num_inputs = [981], 981, BATCH
    merged_sites = sum(1 for s_ in site_list if s_.downsample <= 2)
    torch.manual_seed(123)           # the block generators fork this state (default.yaml seed)
    mode = args.exchange or ("neighbour" if world > 1 else None)
    if args.local_only:
        mode = None
    K = 1 if args.same_chunk else max(2, args.chunks)
    cond = (torch.randn(BATCH * FRAMES, 77, 768, generator=torch.Generator().manual_seed(77))
            .to(device=dev, dtype=torch.float16) if args.full_block else None)
    every = max(1, args.event_every)
    transport = [None]               # the N > 1 transport (per-edge communicators) is created once and shared by the modes
    dog = None
    if world > 1 and args.watchdog_seconds > 0:
        dog = Watchdog(rank, args.watchdog_seconds, lambda: "no exchange")
        dog.start()

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def run_region(regime, steps, warmup, xmode, with_box, inflight=1, dump=False, counters=True):
        """One measured region: a fresh chunk stream of `regime`, anchors populated, `warmup` untimed and `steps` timed passes
        between two fences (barrier + synchronize), HIP events on every `every`-th pass, with `counters` one extra untimed
        pass for the matcher's device-side counters.  Returns everything the line is built from.  With `dump`, what the last
        timed pass returned goes to --dump-outputs."""
        total_passes = 1 + warmup + steps
        for b in unet.blocks:                       # a region starts like a denoising step: no anchors
            b.global_tokens = None
            # ... and like a new clip: the matcher's launch planners (merge.MatchPlanner) start over -- a planner that the
            # PREVIOUS regime sent to the one-launch plan would sit out its cool-down in this one (regimes do not alternate in
            # a real run; the populate / warm-up passes below absorb the planner's first, exploring call)
            b.__dict__.pop("_vtm_match_plans", None)      # (the previous region ended on a fence: no counter copy in flight)
        ex = None
        if xmode is not None:
            # every rank owns one chunk per pass; per merging block the global level takes its anchor tokens from the
            # previous rank's chunk over RCCL / xGMI (chunk_parallel.py).  The whole region is ONE stream of chunks
            # (chunk index = pass * world + rank), so the exchange knows which chunk is the last and leaves no send unmatched.
            from vidtome_amd import chunk_parallel as cp
            if transport[0] is None:
                transport[0] = cp.DistTransport() if world > 1 else cp.LocalTransport.fabric(1)[0]
            ex = cp.AnchorExchange(xmode, transport=transport[0])
            cp.enable(unet, ex)
            ex.begin_step([FRAMES] * (total_passes * world))
            if dog is not None:
                dog.where = lambda: ex.where
        # The region is one stream of chunks of ONE synthetic clip (sites.ClipStream): chunk c = pass * world + rank holds
        # frame set c % K, so the anchor tokens a chunk merges against always come from a different chunk, at every N.
        # N = 1 (no exchange): the reference's chained anchors, re-seeded every chunks_per_step - 1 passes with what the first
        # chunk of a denoising step would have stored (generate.py:233-236 resets the anchors after every step).
        # With an exchange the anchors are whatever the exchange mode defines (neighbour / all-gather: the previous chunk's
        # local tokens, i.e. always a chain of length 1; ring: the exact chain, unbounded over the run).
        stream = sites.ClipStream(unet, site_list, BATCH, FRAMES, LATENT, torch.float16, dev, n_sets=args.chunks,
                                  chunks_per_step=args.chunks_per_step, same_chunk=args.same_chunk, rank=rank,
                                  reseed=ex is None, regime=regime, gen_device=dev,
                                  sets=None if ex is None else {(p_ * world + rank) % K for p_ in range(total_passes)},
                                  cond=cond, inflight=inflight if ex is None else 1)
        passes = [0]

        def step():
            c = passes[0] * world + rank
            passes[0] += 1
            if dog is not None:
                dog.tick(f"{regime} / {xmode}: pass {passes[0] - 1} started (chunk {c})")
            if ex is None:
                return stream.step(c)
            ex.begin_chunk(c)
            with torch.no_grad():
                return stream._run(stream.sets[c % K])

        if ex is None:
            stream.populate()             # untimed: the first chunk(s) of a step fill the anchor tokens (steady state)
        else:
            step()                        # chunk 0 of the stream has no predecessor: it only publishes its tokens
        for _ in range(warmup):
            step()
        sampler = BoxSampler(local_rank) if (rank == 0 and with_box) else None
        with KernelTimer(_lib) as mt:
            fence()
            if sampler is not None:
                sampler.start()
            t0 = time.perf_counter()
            pass_events = []
            for i in range(steps):
                mt.enabled = i % every == 0           # HIP events on every k-th pass only
                if mt.enabled:                        # ... bracketed as a whole too: what the itemised kernels leave is gaps
                    pe0, pe1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    pe0.record()
                if dump and i == steps - 1:      # (earlier passes' outputs are dropped at once, as without the dump)
                    last = step()
                else:
                    step()
                if mt.enabled:
                    pe1.record()
                    pass_events.append((pe0, pe1))
            mt.enabled = False
            fence()
            dt = time.perf_counter() - t0
            if dump:                                  # sampled before the counter pass below can touch any shared buffer
                dump_outputs(last, site_list, args.dump_outputs, rank, world)
            event_pass_ms = sum(a.elapsed_time(b) for a, b in pass_events) / max(1, len(pass_events))
            if ex is None and counters:               # one untimed pass for the matcher's counters (N = 1: the chunk stream
                mt.count = True                       # of an exchange has no spare chunk)
                step()
                mt.count = False
                torch.cuda.synchronize()
        box = sampler.stop() if sampler is not None else None
        if dog is not None:
            dog.tick(f"{regime} / {xmode}: timed region done")
        if ex is not None:
            ex.end_step()
            from vidtome_amd import chunk_parallel as cp
            cp.disable(unet)
        # (gloo -- the test hook -- moves host tensors)
        mine = torch.tensor([dt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        per_rank = [mine.clone() for _ in range(world)]
        if world > 1:
            dist.all_gather(per_rank, mine)
        return {"dt": max(float(t.item()) for t in per_rank),        # MAX over ranks
                "per_rank_ms": [round(float(t.item()) / steps * 1e3, 3) for t in per_rank],
                "mt": mt, "event_pass_ms": event_pass_ms, "box": box, "steps": steps,
                "timed_passes": len(range(0, steps, every)), "total_passes": total_passes,
                "exchange": None if ex is None else
                {"sent": int(ex.bytes_sent / max(1, total_passes)), "received": int(ex.bytes_received / max(1, total_passes)),
                 "note": "this rank, averaged over all passes (N = 1: handed over in place, nothing crosses a link)"}}

    def compact(r):
        """The per-regime entry of `regimes`: step time, the two big components, what is left, and the matcher's counters."""
        mt, tp = r["mt"], r["timed_passes"]
        comp = mt.ms_by_kind()
        att, mat = comp.get("attention", 0.0) / tp, (comp.get("matching", 0.0) + comp.get("position_order", 0.0)) / tp
        cnt = mt.match_counters() or {}
        return {"ms_per_step": round(r["dt"] / r["steps"] * 1e3, 3), "steps_per_s": round(world * r["steps"] / r["dt"], 3),
                "steps": r["steps"], "attention_ms": round(att, 3), "matching_ms": round(mat, 3),
                "other_launches_ms": round(sum(comp.values()) / tp - att - mat, 3),
                "pairs_per_row": cnt.get("refined_pairs_per_src_row"), "escaped": cnt.get("escaped_rows"),
                "escaped_row_fraction": cnt.get("escaped_row_fraction"), "whole_call_escapes": cnt.get("whole_call_escapes"),
                "scout_range_calls": cnt.get("scout_range_calls"),
                "pruned_block_fraction": cnt.get("pruned_block_fraction"),
                "executed_mfma_fraction": cnt.get("executed_mfma_fraction")}

    head = run_region(args.data, args.steps, args.warmup, mode, True, inflight=max(1, args.inflight) if world == 1 else 1,
                      dump=args.dump_outputs is not None, counters=args.full)
    mt, dt, box = head["mt"], head["dt"], head["box"]
    timed_passes, total_passes, event_pass_ms = head["timed_passes"], head["total_passes"], head["event_pass_ms"]
    aflops, ams, an = mt.summary("attention")
    top_flops, top_ms, top_n = mt.largest("attention")
    mflops, mms, mn = mt.summary("matching")
    _, oms, on = mt.summary("position_order")
    mms += oms
    line = None

    if rank == 0:
        ms_per_step = dt / args.steps * 1e3
        value = world * args.steps / dt
        att_tf = aflops / (ams * 1e-3) / 1e12 if ams > 0 else 0.0
        mat_tf = mflops / (mms * 1e-3) / 1e12 if mms > 0 else 0.0
        from vidtome_amd import merge as _merge
        filtered = _merge.MATCH_MODE != "exact"
        traffic, traffic_src = pmc_traffic()

        def hbm(kind):
            """algorithmic bytes / HIP-event time of one HBM-bound kernel: all launches, and the largest ones alone"""
            by, ms, n = mt.summary(kind)
            tb_, tms, tn = mt.largest(kind)
            rate = lambda b_, m_: round(b_ / (m_ * 1e-3) / 1e9, 1) if m_ > 0 else 0.0
            return {"launches": n, "ms_per_step": round(ms / timed_passes, 3), "GBps": rate(by, ms),
                    "largest": {"launches": tn, "MB": round(tb_ / 1e6, 1), "avg_us": round(tms * 1e3, 1),
                                "GBps": rate(tb_, tms), "frac_of_hbm_peak": round(rate(tb_, tms) / HBM_PEAK_GBPS, 3)}}

        # the clock the chip actually sustained in THIS run (sysfs samples during the timed region): the MFMA roof scales
        # with it -- 2.5 PFLOP/s is the dense fp16 peak at the nominal 2.4 GHz
        sclk = (box or {}).get("sclk_mhz", {}).get("mean")
        watts = (box or {}).get("power_w", {}).get("mean")
        roof_at_clock = FP16_PEAK_TFLOPS * sclk / 2400.0 if sclk else None
        if sclk and watts:
            box_note = (f"this run: package power {watts:.0f} W mean, shader clock {sclk / 1e3:.2f} GHz mean over the timed region "
                        f"(bench.box) -- the fp16 MFMA roof at that clock is {roof_at_clock:.0f} TFLOP/s; with non-toggling "
                        f"operands the same launch reaches 1 130-1 166 TFLOP/s at 2.4 GHz = the floor of its instruction mix "
                        f"(profiles/r02_ubench.txt, DESIGN.md section 8)")
        else:
            box_note = "no clock / power sample available on this box (sysfs hwmon not readable)"
        # every launch kind of the path, HIP-event time per step on the event passes; what is left of the step is dispatch
        # gaps and host time
        comp = {k: round(v / timed_passes, 3) for k, v in sorted(mt.ms_by_kind().items(), key=lambda kv: -kv[1])}
        comp_sum = sum(comp.values())
        side = comp_sum - comp.get("attention", 0.0) - comp.get("matching", 0.0) - comp.get("position_order", 0.0)

        par = f"chunk-parallel x{world}" + (f", {args.inflight} chunks in flight on {args.inflight} HIP streams (NOT the default line)"
                                            if world == 1 and args.inflight > 1 else "")
        if mode is not None:
            par += {"neighbour": ", anchor tokens = the previous rank's local merged tokens, point-to-point over RCCL/xGMI "
                                 "per merging block",
                    "allgather": ", RCCL all-gather of the composed merge maps per merging block, tokens point-to-point",
                    "ring": ", exact serial anchor chain (ring hand-off over RCCL/xGMI)"}[mode]
        headline = args.workload == "cfg2" and FRAMES == 16 and not args.full_block and not args.local_only and \
            not (world == 1 and args.inflight > 1)
        line = {
            "metric": "denoising steps/sec, 16-frame 512x512 SD-1.5 chunk, ratio=0.5" +
                      (" -- FULL transformer blocks (secondary measurement, not the headline)" if args.full_block else "") +
                      ("" if args.workload == "cfg2" else f" -- SECONDARY workload {args.workload} (not the headline configuration)"),
            "value": round(value, 4), "unit": "steps/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None,
            # what the communicator reports, and every rank's own time per step (value uses the slowest)
            "ranks": dist.get_world_size() if world > 1 else 1,
            "backend": ("rccl (torch.distributed 'nccl')" if backend == "nccl" else backend) if world > 1 else None,
            "launcher": os.environ.get("VIDTOME_BENCH_LAUNCHER", "torchrun/env" if "WORLD_SIZE" in os.environ else "single process"),
            "per_rank_ms_per_step": head["per_rank_ms"],
            "box": box,
            # the arithmetic types of the path: tokens fp16; matching = fp16-MFMA candidate filter + fp32 exact
            # refinement (result bit-identical to an all-fp32 matcher); attention = fp16 MFMA, fp32 accumulate / softmax
            "dtype": "f16 tokens; matching f16-MFMA filter + f32 exact refine (f32-identical indices); attention f16 MFMA "
                     "with f32 accumulate" if filtered else
                     "f16 tokens; matching f32 MFMA (exact); attention f16 MFMA with f32 accumulate",
            "data": "synthetic",
            "config": {"workload": (wl["label"] if FRAMES == 16 else
                                    f"SD-1.5 {FRAMES}-frame chunk 512x512 (NOT the headline chunk size)") +
                                   f": hot-path pass over the {len(site_list)} transformer-block "
                                   f"sites, batch {BATCH}, local merge {LOCAL_RATIO}" +
                                   ("" if args.local_only else f" + global merge {GLOBAL_RATIO} (steady state)"),
                       "headline_configuration": headline,
                       "regime": ("same chunk fed to every pass (anchors = copies of its own rows; rounds 1-2)"
                                  if args.same_chunk else
                                  f"{K} distinct chunks of one synthetic clip rotate: every pass's anchor tokens come "
                                  f"from a different chunk (generate.py:215-219); " +
                                  (f"anchor chain of 1..{max(1, args.chunks_per_step - 1)} updates, re-seeded with the first "
                                   f"chunk's local tokens like a denoising step of {args.chunks_per_step} chunks "
                                   f"(generate.py:233-236)" if mode is None else
                                   "anchors as the exchange mode defines them")),
                       "data_regime": args.data + ": " + REGIME_NOTES[args.data] +
                                      "; tokens drawn on the device (torch CUDA generator, fixed seeds)",
                       "full_block": bool(args.full_block),
                       "sites": len(site_list), "merged_sites": merged_sites, "chunk_frames": FRAMES, "batch": BATCH,
                       "matcher": _merge.MATCH_MODE + (" (fp16-MFMA filter, fp32 refine; global-level index order inside "
                                                       "groups of EXACTLY equal similarity is the stable one, the "
                                                       "reference's is implementation-defined)" if filtered else ""),
                       "parallelism": par, "exchange": mode,
                       "exchange_bytes_per_step": head["exchange"]},
            # dominant single kernel of the step: the merged-token self-attention (MFMA-bound)
            # `achieved` counts EXECUTED flops (4 B Mq Mk C per launch): with a global level the block only computes the
            # attention rows unmerge() reads, so the reference-algorithmic 4 B M^2 C would overstate the kernel
            "roofline": {"kernel": "attention16s_kernel<half,40> / attention16g_kernel (d = 40: 64-query wave tile, skewed in-wave "
                                   "pipeline; shared probabilities computed once) + attention_kernel<half,d> (d = 80, 64, 160): flash "
                                   "attention over merged tokens, v_mfma_f32_32x32x16_f16 / 16x16x32; executed flops",
                         "bound": "mfma", "achieved": round(att_tf, 1), "peak": FP16_PEAK_TFLOPS,
                         "unit": "TFLOP/s", "frac": round(att_tf / FP16_PEAK_TFLOPS, 4), "traffic": traffic,
                         "traffic_source": traffic_src,
                         "launches": an, "avg_launch_ms": round(ams / max(an, 1), 4),
                         # the top-block launches alone (compare with attention_kernel<half,40> in profiles/*_kernel_stats.txt)
                         "top_block": {"launches": top_n, "avg_ms": round(top_ms, 4),
                                       "tflops": round(top_flops / (top_ms * 1e-3) / 1e12, 1) if top_ms > 0 else 0.0},
                         "attention_ms_per_step": round(ams / timed_passes, 3),
                         # for context only: the reference computes attention outputs for EVERY merged row (M^2 instead of the
                         # live / distinct Mq x M): the same time expressed in those flops
                         "reference_equivalent_tflops": round(mt.ref_flops / (ams * 1e-3) / 1e12, 1) if ams > 0 else 0.0,
                         "event_passes": timed_passes,
                         # duplicate keys folded away (vtm_fold_keys): keys the event-timed launches really scanned / keys of
                         # the merged sequences (launches whose anchors carried content ids only)
                         "folded_launches": len(mt.folded_keys),
                         "folded_key_fraction": round(1.0 - sum(a for a, _ in mt.folded_keys) / sum(t for _, t in mt.folded_keys), 4)
                         if mt.folded_keys else 0.0,
                         "sustained_sclk_mhz": sclk,
                         "frac_at_sustained_clock": round(att_tf / roof_at_clock, 4) if roof_at_clock else None,
                         "note": box_note},
            # the fused similarity + top-1 step (second largest).  `nominal_tflops` = the reference's 2 B Ns Nd C flops per call /
            # HIP-event time of the whole vtm_match_filtered call: the fp16-MFMA filter would execute exactly those once, but
            # its partial-sum pruning skips the MFMAs of 32 x 32 blocks that can no longer matter -- `counters` carries the
            # fraction of blocks pruned and of MFMA work really executed (--full: device-side counters of one extra untimed pass).
            # The exact fallback kernel runs on the fp32 MFMA (157.3 TFLOP/s).
            "matching": {"kernels": "prep_operand + filter_kernel + refine_kernel + exact_rows_kernel (vtm_match_filtered{,_ordered}) + vtm_position_order" if filtered
                                    else "match_kernel (vtm_match)",
                         "nominal_tflops": round(mat_tf, 1),
                         "peak": FP16_PEAK_TFLOPS if filtered else FP32_PEAK_TFLOPS,
                         "nominal_frac": round(mat_tf / (FP16_PEAK_TFLOPS if filtered else FP32_PEAK_TFLOPS), 4),
                         "calls": mn, "matching_ms_per_step": round(mms / timed_passes, 3),
                         "position_order_calls": on, "position_order_ms_per_step": round(oms / timed_passes, 3),
                         # --full: device-side counters of one extra untimed pass: pairs the exact refine pass evaluated per src row,
                         # rows whose candidate list overflowed (exact_rows_kernel), calls recomputed as a whole, blocks pruned
                         "counters": mt.match_counters() if filtered else None},
            # q / k / v^T / out projections: GEMMs whose A rows are gathered through the composed merge map
            "projections": (lambda f, ms, n: {"kernel": "linear_rows_ws_kernel / linear_rows_kernel (vtm_linear_rows, fp16 MFMA)", "launches": n,
                                              "ms_per_step": round(ms / timed_passes, 3),
                                              "tflops": round(f / (ms * 1e-3) / 1e12, 1) if ms > 0 else 0.0})(
                *mt.summary("projections")),
            # EVERY launch kind of the pass (vidtome_amd._lib entry points), HIP-event ms per step on the event passes; the
            # panel-GEMM projections of the C >= 640 / un-merged sites are `linear_panels` + their panel writers
            "components_ms_per_step": comp,
            "components_sum_ms": round(comp_sum, 3),
            # everything that is neither attention nor the matcher (VERDICT r04 item 3's "side kernels")
            "side_launches_ms_per_step": round(side, 3),
            # the event passes are bracketed as a whole as well: their own duration (they carry ~2 events per launch, so they
            # run a little longer than the mean pass) minus the itemised launches = dispatch gaps + host-side stalls
            "event_pass_ms": round(event_pass_ms, 3),
            "unaccounted_ms_per_step": round(event_pass_ms - comp_sum, 3),
            "timing": f"value = {args.steps} passes / wall time between two fences (barrier + synchronize; perf_counter), "
                      f"i.e. the MEAN pass; kernel figures = HIP events on every {every}-th pass "
                      f"({timed_passes} event passes)",
            # the HBM-bound kernels of the path: algorithmic bytes (rows read + rows written) / HIP-event time.  The
            # cfg-2 working sets (<= 212 MB) fit the 256 MB Infinity Cache, so `pmc` carries the counter-derived rates
            # measured beyond it
            "gather_path": {"hbm_peak_GBps": HBM_PEAK_GBPS, "layernorm": hbm("layernorm"),
                            "gather_rows": hbm("gather_rows"), "unmerge_add": hbm("unmerge_add"),
                            "pmc": pmc_gather_path()},
        }
        # "if Diffusers + weights happen to be importable on the GPU box (probe, never assume) the same step is
        # also timed inside a real UNet; otherwise the site harness *is* the step" -- probed, reported, never assumed
        if args.full:
            line["real_unet_probe"] = probe_real_unet()
        if args.full_block:
            def gemm(kind):
                f, ms, n = mt.summary(kind)
                lf, lms, ln = mt.largest(kind)
                return {"launches": n, "ms_per_step": round(ms / timed_passes, 3),
                        "tflops": round(f / (ms * 1e-3) / 1e12, 1) if ms > 0 else 0.0,
                        "frac_of_fp16_mfma_peak": round(f / (ms * 1e-3) / 1e12 / FP16_PEAK_TFLOPS, 4) if ms > 0 else 0.0,
                        "largest": {"launches": ln, "avg_us": round(lms * 1e3, 1),
                                    "tflops": round(lf / (lms * 1e-3) / 1e12, 1) if lms > 0 else 0.0}}
            line["full_block"] = {
                "what": "the whole patched block per site: hot-path segment + norm2 / attn2 (77 text tokens) + norm3 / GEGLU "
                        "feed-forward (patch.py:171-199); panel GEMMs of csrc/ff.hip unless VIDTOME_FF=blas",
                "ff_mode": __import__("vidtome_amd.patch", fromlist=["FF_MODE"]).FF_MODE,
                "ff_geglu": gemm("ff_geglu"), "linear_panels": gemm("linear_panels"),
                "layernorm_panels": hbm("layernorm_panels")}

    # ---- N = 1: the other token regimes, same harness, fewer passes (SURVEY 8d names n01 and corr01) ----
    if args.full and world == 1 and mode is None and args.regimes != "none":
        names = [n for n in ("n01", "corr01", "corr05", "corr002", "smooth", "dup", "flat25")] if args.regimes == "all" else \
            [n.strip() for n in args.regimes.split(",") if n.strip()]
        regs = {args.data: compact(head)}
        for name in names:
            if name in regs:
                continue
            if name not in REGIME_NOTES:
                raise SystemExit(f"bench.py: unknown regime {name!r}")
            # (SURVEY 8d's other named input and rounds 1-4's headline get the full count, the rest half)
            rsteps = max(1, args.regime_steps if name in ("n01", "corr01", "corr05") else (args.regime_steps + 1) // 2)
            regs[name] = compact(run_region(name, rsteps, REGIME_WARMUP, None, False))
        base = regs.get("corr05", {}).get("ms_per_step")
        for name, r in regs.items():
            r["vs_corr05"] = round(r["ms_per_step"] / base, 3) if base else None
            r["what"] = REGIME_NOTES[name]
        line["regimes"] = regs
        line["regimes_note"] = (f"`value` is the {args.data} entry ({args.steps} passes); n01 / corr01 / corr05 ran "
                                f"{max(1, args.regime_steps)} timed passes, the others {max(1, (args.regime_steps + 1) // 2)}, in the "
                                f"same process, same harness; vs_corr05 = ms_per_step / corr05's (the regime rounds 1-4 quoted as "
                                f"the headline)")
        named = {n: regs[n]["steps_per_s"] for n in ("corr01", "n01") if n in regs}
        if len(named) == 2:       # both inputs SURVEY.md 8d names, at top level
            worst = min(named, key=named.get)
            line["value_worst_named"] = {"value": named[worst], "unit": "steps/s", "regime": worst, "both": named}

    # ---- N = 1: two chunks in flight on two HIP streams (round 6) ----
    # Same chunk stream, same anchor chain, same results (tests/test_gpu_parity.py::test_two_chunks_in_flight_equal_one_stream):
    # chunk c runs on stream c % 2, on the device chunk c + 1 waits block by block for chunk c's anchors (patch.mark_anchors_ready /
    # await_anchors).  The dispatch gaps and the ~400 small launches of one chunk then run beside the other chunk's big kernels.
    # `value` stays the ONE-stream number (like for like with rounds 1-5); this is what a video of several chunks per denoising
    # step gets on one GPU.
    if args.full and world == 1 and mode is None and rank == 0 and args.inflight_line and args.workload == "cfg2" \
            and not args.local_only:
        try:
            r2 = run_region(args.data, args.steps, args.warmup + 2, None, False, inflight=2)
            c2 = compact(r2)
            line["two_in_flight"] = {"steps_per_s": c2["steps_per_s"], "ms_per_chunk_step": c2["ms_per_step"], "steps": c2["steps"],
                                     "streams": 2, "vs_value": round(c2["steps_per_s"] / line["value"], 4),
                                     "note": "chunk c on HIP stream c % 2; anchors handed over by device-side events; results "
                                             "bit-identical to the one-stream run; `value` is NOT this number"}
        except Exception as e:                       # a secondary line must never take the headline with it
            line["two_in_flight"] = {"error": f"{type(e).__name__}: {e}"[:300]}

    # ---- N = 1 headline run: the other single-GPU BASELINE configurations, driver-timed ----
    if args.full and world == 1 and mode is None and rank == 0 and args.workloads != "none" and args.workload == "cfg2" \
            and not args.full_block and not args.local_only and FRAMES == 16:
        import subprocess
        want = ["cfg3", "cfg5", "full_block"] if args.workloads == "all" else \
            [w.strip() for w in args.workloads.split(",") if w.strip()]
        torch.cuda.synchronize()
        torch.cuda.empty_cache()          # the children run on this GPU while this process waits
        wls = {}
        for w in want:
            if w not in ("cfg3", "cfg5", "full_block"):
                raise SystemExit(f"bench.py: unknown secondary workload {w!r}")
            cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(args.workload_steps), "--warmup", "3",
                   "--data", args.data] + (["--full-block"] if w == "full_block" else ["--workload", w])
            t0 = time.perf_counter()
            try:
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
                wls[w] = {"what": d["config"]["workload"], "ms_per_step": d["ms_per_step"], "steps_per_s": d["value"],
                          "steps": d["steps"], "attention_ms": d["roofline"]["attention_ms_per_step"],
                          "matching_ms": d["matching"]["matching_ms_per_step"],
                          "side_launches_ms": d["side_launches_ms_per_step"],
                          "roofline_frac": d["roofline"]["frac"], "attention_tflops": d["roofline"]["achieved"],
                          "top_block": d["roofline"]["top_block"], "wall_s": round(time.perf_counter() - t0, 1)}
                if w == "full_block":
                    wls[w]["ff_geglu"] = d["full_block"]["ff_geglu"]
                    wls[w]["linear_panels"] = d["full_block"]["linear_panels"]
            except Exception as e:       # a secondary line must never take the headline with it
                wls[w] = {"error": f"{type(e).__name__}: {e}"[:300]}
        line["workloads"] = wls
        line["workloads_note"] = (f"secondary single-GPU configurations of BASELINE.json, {args.workload_steps} timed passes each, "
                                  f"same harness (`python bench.py --workload cfg3|cfg5` / `--full-block`), each in a child "
                                  f"process after the headline region; `value` is NOT computed from them")

    # ---- N > 1: the other exchange modes (ring = the exact chain, neighbour / allgather = parallel anchors) ----
    if args.full and world > 1 and mode is not None and args.exchange_modes != "none":
        want = ["neighbour", "ring", "allgather"] if args.exchange_modes == "all" else \
            [m.strip() for m in args.exchange_modes.split(",") if m.strip()]
        modes = {mode: {"ms_per_step": round(dt / args.steps * 1e3, 3), "steps_per_s": round(world * args.steps / dt, 3),
                        "per_rank_ms_per_step": head["per_rank_ms"], "exchange_bytes_per_step": head["exchange"]}}
        if rank == 0:
            line["exchange_modes"] = modes
        if dog is not None:       # from here on a stuck rank must not take the headline with it
            dog.fallback = (lambda: print(json.dumps(line), flush=True)) if rank == 0 else (lambda: None)
        xsteps = max(2, min(args.steps, 10))
        for m in want:
            if m in modes:
                continue
            if dog is not None:
                dog.phase = m
            if rank == 0:
                modes[m] = {"error": "did not finish (watchdog)"}        # overwritten when the region completes
            r = run_region(args.data, xsteps, 1, m, False)
            modes[m] = {"ms_per_step": round(r["dt"] / xsteps * 1e3, 3), "steps_per_s": round(world * xsteps / r["dt"], 3),
                        "steps": xsteps, "per_rank_ms_per_step": r["per_rank_ms"], "exchange_bytes_per_step": r["exchange"]}
        if dog is not None:
            dog.fallback = None

    if rank == 0:
        if args.full and not args.no_cpu_baseline and world == 1 and not args.full_block and args.workload == "cfg2":
            # rank 0 at N = 1 only; the CPU leg times the segment at the headline configuration
            line["cpu_baseline"] = (cpu_baseline_torch if args.cpu_baseline == "torch" else cpu_baseline_port)(
                args.cpu_seconds)
        print(json.dumps(line), flush=True)
    if dog is not None:
        dog.stop()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
