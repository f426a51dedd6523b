"""Every launch plan of the 16-bit attention core against the oracle (double accumulation), in fp16 and bf16.

`attention_any` (csrc/attention.hip) picks a kernel family -- attention_kernel<T, D, FOLD>, attention16s_kernel (d = 40,
self-attention and folded keys) or attention16g_kernel (d = 40, probabilities shared over 2 or 3 groups) -- and a plan: a
single launch, the host key-split tail (plan_tail + a combine kernel), the host split-all plan of query-bounded launches,
the device-planned tail (attention16_plan_kernel) or a plain launch for want of a workspace.  Each plan has its own grid
arithmetic, partial-record layout and combine, so each is pinned here on its own:

* the selection is restated in plain Python below (line references are to the sources it mirrors) and checked against
  the library: the workspace sizes of both *_ws_bytes exports over a grid of shapes, and after every launch the plan it
  left behind -- the DevPlan header of a device-planned launch field for field, and for every plan exactly which
  partial records of the workspace were written (records of live split items all written, every other byte untouched);
* outputs are compared with oracle.attention_qkv on rows of every query block below each sample's count, with dominant
  keys planted where the plans cut the key axis (key 0, the last key of a ragged tile, the first and last key of every
  split piece), large finite garbage in every operand element the kernels must not read, operands with ld = 2C / 3C and
  an output window with ldo > C inside a larger buffer whose gap columns and guard rows must keep their canaries.

The fp32 family (attention_f32_kernel, csrc/attention_f32.hip: 32-key tiles, 4 waves, its own partial record and combine
kernel, sharing done in-kernel) goes through the same planner and is pinned by the same harness as a fourth kind, "f32":
fp32 operands in the same windows, 1e30 in the V^T columns no kernel may use, a 32-bit NaN canary around the output
window (rows Mq .. Mqp included), the workspace checked record by record.  Also here: split pieces that hold no key tile
(129 tiles cut 16 ways, every family), and the workspace the Python binding hands to an fp32 launch.

Bars (unchanged from the rest of the suite): 1e-3 (fp16) / 8e-3 (bf16) of max(1, |ref|max); fp32: 2e-5 of |ref|max per
launch (BAR of test_gpu_fp32_attention.py, derived there from the fp32 rounding of the longest sums)."""
import zlib

import numpy as np
import pytest
import torch

from test_gpu_fp32_attention import BAR               # 2e-5 of the output scale (derivation: that module's docstring)

pytestmark = pytest.mark.gpu
DEV = "cuda"
KV = 64                                               # keys per tile (attention_common.h:21)
QW = 32                                               # queries per wave (attention_common.h:20)
DEVPLAN_HEADER = 256                                  # attention_plan.h:326
PLAN_TIERS, PLAN_MAX_SPLIT = 8, 16                    # attention_plan.h:169-170
KT32 = 32                                             # keys per tile of the fp32 kernel (attention_f32.hip:30)
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}
DT_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
KERNEL_DIMS = (8, 16, 32, 64, 80, 96, 128, 160)
F32_DIMS = (8, 16, 32, 40, 64, 80, 96, 128, 160)
CANARY = 0x7E5A                                       # a NaN in fp16 and in bf16: no kernel result has these bits
CANARY32 = 0x7FC5A5A5                                 # a quiet NaN with a payload no fp32 arithmetic produces
GUARD_ROWS = 16
# score of a planted key for its query, natural-log units: 14, capped at 1.5 sqrt(d).  The same key gives every other query
# a score k_j . q_m = PLANT_LOGIT cos(q_i, q_m) |q_m| / |q_i|, spread ~ PLANT_LOGIT / sqrt(d): the cap keeps those scores
# in the range the bars are stated for.  Uncapped at d = 8 they reach tens of log2 units, where the one fp16 rounding of
# the pre-scaled query of a d % 16 != 0 head costs |logit| 2^-12 (see test_attention_rescale_paths in test_gpu_parity.py).
# 1.5 sqrt(d) = 4.2 at d = 8 still gives the planted key a weight of a few per cent among 2 000 random keys: losing it
# moves its query's output by ten times the bar and more
PLANT_LOGIT, PLANT_SPREAD = 14.0, 1.5
GARBAGE_K, GARBAGE_V, GARBAGE_Q = 200.0, 30000.0, 200.0
# fp32: a probability of 2e-5 / 1e30 leaking onto a key behind Mk still moves the output by the whole bar
GARBAGE_V32 = 1e30


@pytest.fixture(scope="module")
def L():
    from vidtome_amd import _lib
    _lib.lib()
    return _lib


def cdiv(a, b):
    return -(-a // b)


def pad8(n):
    return (n + 7) // 8 * 8


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------------------------------------------------------------
# the selection, restated
# ---------------------------------------------------------------------------------------------------------------------
def waves_for(D):                                     # attention_common.h:19
    return 8 if D <= 48 else 16 if D <= 96 else 4


def pv16_for(D):                                      # attention_common.h:29
    return D % 32 != 0 and (D + 16) // 16 * 16 < (D + 31) // 32 * 32


def acc_floats(D):                                    # attention_common.h:33-35
    return (D + 16) // 16 * 8 if pv16_for(D) else (D + 31) // 32 * 16


def rec_floats(D):
    return acc_floats(D) + (2 if pv16_for(D) else 1) + 1


def rec16(D):                                         # attention16_parts.h:12
    return (D + 16) // 16 * 8 + 2 + 1


class Family:
    """Launch constants of one kernel family: query rows per workgroup, resident workgroups per CU, bytes of one
    key-split workgroup's partial record, the query blocks from which (sample, head) pairs are pinned to XCDs, keys per
    tile (what a device plan counts and what the pieces of a split item are cut from)."""

    def __init__(self, kind, d, ng=1):
        self.kind, self.d, self.ng = kind, d, ng
        self.key_tile = KV
        if kind == "f32":                             # the Family of attention_f32.hip:405-419
            nqh = 1 if d >= 128 else 2                # query halves per wave (attention_f32.hip:34)
            self.QB = 4 * 16 * nqh                    # 4 waves (attention_f32.hip:29, 35)
            self.wg = 2 if d <= 128 else 1            # attention_f32.hip:37
            self.rec = (cdiv(d, 16) * 4 * nqh + 1) * 256 * 4     # attention_f32.hip:42-44
            self.xcd_min = 64                         # attention_f32.hip:36
            self.key_tile = KT32                      # attention_f32.hip:30, 413
        elif kind == "k":                               # the Family of attention.hip:612-624
            self.QB, self.wg = waves_for(d) * QW, 2 if d <= 48 else 1
            self.rec = rec_floats(d) * waves_for(d) * 64 * 4
            self.xcd_min = 64
        elif kind == "16s":                           # the Family of attention16.hip:487-496
            self.QB, self.wg, self.rec, self.xcd_min = 8 * QW * 2, 1, 2 * rec16(40) * 512 * 4, 32
        else:                                         # the Family of attention16g.hip:424-439
            self.QB, self.wg, self.rec, self.xcd_min = 8 * QW, 1, ng * rec16(40) * 512 * 4, 32

    def slots(self, n_cus):
        return n_cus * self.wg


def plan_tail(B_items, h, Mq, Mk, QB, wg, rec, bounded, n_cus):
    """attention_plan.h:36-68."""
    nqb = cdiv(Mq, QB)
    total = nqb * h * B_items
    slots = n_cus * wg
    full = total // slots * slots
    rem, ntiles = total - full, cdiv(Mk, KV)
    p = dict(nqb=nqb, total=total, full=full, nsplit=1, ws_bytes=0, split_all=False)
    if bounded and total >= 2 * slots and ntiles >= 64 and total % 8 == 0:
        p.update(full=0, nsplit=2, split_all=True, ws_bytes=total * 2 * rec)
        return p
    if full > 0 and rem > 0 and rem * 4 <= slots and ntiles >= 32:
        ns = min(slots // rem, 16, ntiles // 8)
        if ns >= 2:
            p.update(nsplit=ns, ws_bytes=rem * ns * rec)
    if p["nsplit"] == 1:
        p["full"] = total
    return p


def devplan_ws_bytes(slots, rec):                     # attention_plan.h:283, 328
    return DEVPLAN_HEADER + (PLAN_TIERS - 1) * slots * rec


def ws_bytes_k(D, B, h, Mq, Mk, bounded, n_cus):     # attention_plan.h:415-420
    F = Family("k", D)
    n = plan_tail(B, h, Mq, Mk, F.QB, F.wg, F.rec, bounded, n_cus)["ws_bytes"]
    if bounded and cdiv(Mk, KV) >= 16:
        n = max(n, devplan_ws_bytes(F.slots(n_cus), F.rec))
    return n


def ws_bytes16(B, h, Mq, Mk, bounded, n_cus):        # attention_plan.h:415-420
    F = Family("16s", 40)
    n = plan_tail(B, h, Mq, Mk, F.QB, 1, F.rec, bounded, n_cus)["ws_bytes"]
    return max(n, devplan_ws_bytes(n_cus, F.rec)) if bounded else n


def ws_bytes16g(ng, src, h, Mq, Mk, bounded, n_cus):  # attention_plan.h:415-420
    F = Family("16g", 40, ng)
    n = plan_tail(src, h, Mq, Mk, F.QB, 1, F.rec, False, n_cus)["ws_bytes"]
    return max(n, devplan_ws_bytes(n_cus, F.rec)) if bounded else n


def ws_bytes_f32(B, h, Mq, Mk, d, bounded, n_cus):    # attention_f32.hip: ws_bytes_f32 (ws_devplan_min_tiles = 0)
    if B <= 0 or h <= 0 or Mq <= 0 or Mk <= 0 or d not in F32_DIMS:
        return 0
    F = Family("f32", d)
    n = plan_tail(B, h, Mq, Mk, F.QB, F.wg, F.rec, bounded, n_cus)["ws_bytes"]
    return max(n, devplan_ws_bytes(F.slots(n_cus), F.rec)) if bounded else n


def ws_bytes_any(B, h, Mq, Mk, d, bounded, n_cus):    # attention.hip:636-648
    if B <= 0 or h <= 0 or Mq <= 0 or Mk <= 0:
        return 0
    if d == 40:
        n = max(ws_bytes_k(40, B, h, Mq, Mk, bounded, n_cus), ws_bytes16(B, h, Mq, Mk, bounded, n_cus))
        for ng in (2, 3):
            if B % ng == 0:
                n = max(n, ws_bytes16g(ng, B // ng, h, Mq, Mk, bounded, n_cus))
        return n
    return ws_bytes_k(d, B, h, Mq, Mk, bounded, n_cus) if d in KERNEL_DIMS else 0


def shape16_for(d, share_groups):                     # attention.hip:629-632 (16-bit dtypes)
    return (share_groups if share_groups <= 3 else 0) if d == 40 else 0


def device_plan(counts, H, QB, slots, ntiles):
    """attention16_plan_kernel (attention_plan.h:286-323): the 44 int32 of the DevPlan it writes."""
    nqb = max([1] + [cdiv(c, QB) for c in counts])
    Lit, S = nqb * H * len(counts), slots
    max_ns = max(1, min(PLAN_MAX_SPLIT, ntiles // 8))
    tiers = []
    whole = Lit - Lit % S
    if max_ns < 2 or (Lit % S) * 5 >= S * 4 or (Lit < S and Lit * 2 > S):
        whole = Lit
    tiers.append([0, 0, whole, 1, 0])
    wg = item = whole
    rec = 0
    while item < Lit and len(tiers) < PLAN_TIERS:
        rem = Lit - item
        n = 2
        while n < max_ns and S // n > rem:
            n *= 2
        n = min(n, max_ns)
        take = min(S // n, rem)
        if len(tiers) == PLAN_TIERS - 1:
            take = rem
        tiers.append([wg, item, take, n, rec])
        wg += take * n
        rec += take * n
        item += take
    ntiers = len(tiers)
    while len(tiers) < PLAN_TIERS:
        tiers.append([wg, item, 0, 1, rec])
    return [nqb, ntiers, Lit - whole, 0] + [x for t in tiers for x in t]


def item_of(pos, nqb, xcd_groups):                    # attention_common.h:88-92
    if xcd_groups == 0:
        return pos
    xcd, slot = pos & 7, pos >> 3
    return (xcd + 8 * (slot // nqb)) * nqb + slot % nqb


class Selection:
    """What attention_any / vtm_attention_kv_folded launch for a call: family, plan, combine kernel, and the work items
    that run key-split as (position in the grid order, pieces, first partial record)."""

    def __init__(self, call, d, B, h, Mq, Mk, share, ldvt, ws_bytes, counts, n_cus, f32=False):
        bounded = counts is not None                  # (a query count is what makes a launch bounded)
        if f32:                                       # attention.hip: attention_any, dtype VTM_F32 -- whatever share_groups
            kind = "f32"                              # is: the grid runs over all B samples, host_split_all, its own combine
        elif call == "folded":                          # attention.hip:738-739
            kind = "16s" if d == 40 else "k"
        else:                                         # attention.hip:686-696
            ng = shape16_for(d, share)
            if ng == 1:
                kind = "16s"
            elif ng > 1 and ng * (B // share) * h * d * ldvt * 2 < 2 ** 31:
                kind = "16g"
            else:
                kind = "k"
        F = self.F = Family(kind, d, share if kind == "16g" else 1)
        self.kind, self.h = kind, h
        self.items_B = B // share if kind == "16g" else B    # the samples the grid runs over (16g: the sources)
        self.counts = None if counts is None else list(counts[:self.items_B])
        slots = F.slots(n_cus)
        xcd_pairs = (self.items_B * h) // 8 if (self.items_B * h) % 8 == 0 else 0
        nqb_max = cdiv(Mq, F.QB)
        self.header = None
        # the device plan: attention_plan.h:368-369
        if bounded and ws_bytes is not None and ws_bytes >= devplan_ws_bytes(slots, F.rec) and \
                nqb_max * h * self.items_B >= 2 * slots:
            self.plan, self.combine = "device", "f32" if f32 else "16" if kind != "k" else "plain"
            self.header = device_plan(self.counts, h, F.QB, slots, cdiv(Mk, F.key_tile))
            self.nqb = self.header[0]
            xg = xcd_pairs if self.nqb >= F.xcd_min else 0
            self.rec_base = DEVPLAN_HEADER
            self.split = []
            for t in range(1, self.header[1]):
                wg0, item0, items, ns, rec0 = self.header[4 + 5 * t: 9 + 5 * t]
                self.split += [(item_of(item0 + i, self.nqb, xg), ns, rec0 + i * ns) for i in range(items)]
            self.ws_used = DEVPLAN_HEADER + sum(ns for _, ns, _ in self.split) * F.rec
            return
        # the host plans: attention_plan.h:388-395
        p = plan_tail(self.items_B, h, Mq, Mk, F.QB, F.wg, F.rec, bounded and kind != "16g", n_cus)
        if p["split_all"] and (ws_bytes is None or ws_bytes < p["ws_bytes"]):
            p = plan_tail(self.items_B, h, Mq, Mk, F.QB, F.wg, F.rec, False, n_cus)
        if p["nsplit"] > 1 and (ws_bytes is None or ws_bytes < p["ws_bytes"]):
            p.update(nsplit=1, full=p["total"], split_all=False, ws_bytes=0)
        self.p, self.nqb = p, p["nqb"]
        rem = p["total"] - p["full"]
        self.plan = "split_all" if p["split_all"] else "tail" if p["nsplit"] > 1 else "single"
        if self.plan == "single":
            self.combine = None
        elif f32:                                     # attention_f32.hip: launch_combine
            self.combine = "f32"
        elif kind != "k":
            self.combine = "16"
        else:                                         # attention.hip:600-602
            self.combine = "parts" if (not pv16_for(d) and rem * 4 <= n_cus) else "plain"
        xg = xcd_pairs if p["nqb"] >= F.xcd_min else 0   # attention_plan.h:406
        self.rec_base = 0
        self.split = [(item_of(p["full"] + i, p["nqb"], xg), p["nsplit"], i * p["nsplit"]) for i in range(rem)] \
            if p["nsplit"] > 1 else []
        self.ws_used = p["ws_bytes"]

    def where(self, lin):
        """(sample, head, query block) of work item `lin`."""
        nqb = self.nqb
        return lin // (nqb * self.h), (lin // nqb) % self.h, lin % nqb

    def live(self, lin):
        b, _, qb = self.where(lin)
        return self.counts is None or qb * self.F.QB < self.counts[b]


def pieces(Mk, ns, tile=KV):
    """Key ranges of the pieces of an item split `ns` ways over Mk keys that hold a tile (attention.hip:534-536,
    attention16.hip:320-322; tile = 32: attention_f32.hip:327-329).  Fewer than `ns` ranges: the last pieces are empty."""
    ntiles = cdiv(Mk, tile)
    tps = cdiv(ntiles, ns)
    out = []
    for s in range(ns):
        tb, te = s * tps, min(s * tps + tps, ntiles)
        if tb < te:
            out.append((tb * tile, min(te * tile, Mk)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# one launch against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _fold_bias_word(lg, dtype):
    hi = lg.to(dtype)
    lo = (lg - hi.float()).to(dtype)
    return (hi.view(torch.int16).int() & 0xffff) | (lo.view(torch.int16).int() << 16)


def run_case(L, oracle, call, dtype, d, B, h, Mq, Mk, expect, share=1, counts=None, ws="lib", mult=None, seed=0,
             min_live_per_tier=1, hook=None):
    """One raw library call.  `call`: kv / bounded / shared_bounded / folded; `counts`: per-sample query counts (None =
    unbounded); `ws`: "lib" (the size the library asks for), None (no workspace) or a byte count; `mult` (folded keys):
    (B, Mk) multiplicities, 0 = no such key -- the oracle attends over the sequence with the copies.  `expect` =
    (family, plan, combine).  Returns the Selection.

    `hook` (tests/test_gpu_core_softmax_corners.py) brings operands and a comparison of its own and leaves everything
    else -- windows, garbage, canaries, the selection and the workspace check -- to this function:
    hook.operands(sel, q, k, v, rows, cnt, kc) writes the live windows of q / k / v in place of the planted keys below and
    adds the rows it wants compared; hook.compare(sel, launch, out, vt, rows, cnt, kc) stands in for the oracle comparison
    (`launch()` runs the call again on what vt holds by then, checks 1 and 2 included, and returns its output)."""
    n_cus = cus()
    f32 = dtype == torch.float32
    C = h * d
    scale = d ** -0.5
    src = B // share
    Mqp, Mkp, ldvt = pad8(Mq) + 8, pad8(Mk) + 8, pad8(Mk) + 16
    g = torch.Generator(device=DEV).manual_seed(1000 * d + Mq + seed)
    # operand windows: q in a (B, Mqp, 2C) buffer, k in a (B, Mkp, 3C) one (patch.py passes fused projections)
    qbuf = torch.randn(B, Mqp, 2 * C, generator=g, device=DEV).to(dtype)
    kbuf = torch.randn(B, Mkp, 3 * C, generator=g, device=DEV).to(dtype)
    v = torch.randn(B, Mk, C, generator=g, device=DEV).to(dtype)
    q, k = qbuf[:, :, :C], kbuf[:, :, C:2 * C]
    q[:, Mq:] = GARBAGE_Q
    if f32 and share > 1:                             # probabilities come from the source samples' q / k alone
        q[src:] = GARBAGE_Q
        k[src:] = GARBAGE_K
    # the device-side key count of every sample (folded keys: the distinct ones)
    if mult is not None:
        mult = torch.as_tensor(mult)
        kc = [int((mult[b] > 0).sum()) for b in range(B)]
    else:
        kc = [Mk] * B
    sel = Selection(call, d, B, h, Mq, Mk, share, ldvt,
                    None if ws is None else _ws_size(L, call, d, B, h, Mq, Mk, counts, ws, f32), counts, n_cus, f32)
    assert (sel.kind, sel.plan, sel.combine) == expect, ("the shape does not select the plan it names",
                                                         (sel.kind, sel.plan, sel.combine), expect)
    # rows compared: first, last and two random rows of every query block below the count, and count - 1
    rs = np.random.default_rng(seed + d)
    cnt = [Mq] * B if counts is None else list(counts)
    QB = sel.F.QB
    rows = []
    for b in range(B):
        r = {cnt[b] - 1}
        for qb in range(cdiv(cnt[b], QB)):
            lo, hi = qb * QB, min((qb + 1) * QB, cnt[b])
            r |= {lo, hi - 1} | set(rs.integers(lo, hi, 2).tolist())
        rows.append(r)
    # plant a dominant key (k_j = alpha q_i, per head) where the plans cut the key axis, each for one query row inside a
    # split item of its sample (any compared row when the plan splits nothing)
    live_split = [(lin, ns) for lin, ns, _ in sel.split if sel.live(lin)]
    tiers = sorted({ns for _, ns, _ in sel.split})
    for ns in tiers:
        assert sum(1 for _, n in live_split if n == ns) >= min_live_per_tier, ("no live item splits", ns)
    if hook is not None:
        hook.operands(sel, q, k, v, rows, cnt, kc)
    for bs in range(src if hook is None else 0):
        mk = kc[bs]
        targets = {}
        for ns in tiers or [1]:
            cand = [lin for lin, n in live_split if n == ns and sel.where(lin)[0] % src == bs] if tiers else []
            for lo, hi in pieces(mk, ns, sel.F.key_tile):
                for j in (lo, hi - 1):
                    targets.setdefault(j, cand)
        targets.setdefault(mk - 1, [])
        used = set()
        for n, (j, cand) in enumerate(sorted(targets.items())):
            if cand:
                _, _, qb = sel.where(cand[n % len(cand)])
                lo, hi = qb * QB, min((qb + 1) * QB, cnt[bs])
            else:
                lo, hi = 0, cnt[bs]
            i = int(rs.integers(lo, hi))
            if i in used:
                continue
            used.add(i)
            qi = q[bs, i].float().view(h, d)
            # (|q_i|^2 floored at d: a short q_i would otherwise need a long key, whose scores with the other queries spread
            # by PLANT_LOGIT |q_m| / |q_i|)
            alpha = min(PLANT_LOGIT, PLANT_SPREAD * d ** 0.5) / (scale * (qi * qi).sum(1).clamp_min(d))
            k[bs, j] = (alpha[:, None] * qi).reshape(C).to(dtype)
            for b in range(bs, B, src):
                rows[b].add(i)
    # what the kernels must not read: K rows past the key count, V^T columns past it, bias words past it
    for b in range(B):
        k[b, kc[b]:] = GARBAGE_K
    vt = torch.empty(B, C, ldvt, dtype=dtype, device=DEV)
    vt[:, :, :Mk] = v.transpose(1, 2)
    vt[:, :, Mk:] = GARBAGE_V32 if f32 else GARBAGE_V
    for b in range(B):
        vt[b, :, kc[b]:] = GARBAGE_V32 if f32 else GARBAGE_V
    kbias = None
    if mult is not None:
        kbias = torch.empty(B, Mk, dtype=torch.int32)
        kbias[:] = _fold_bias_word(torch.tensor([12.0]), dtype)
        for b in range(B):
            live = torch.nonzero(mult[b]).flatten()
            assert torch.equal(live, torch.arange(kc[b])), "folded keys are the first k_count entries"
            kbias[b, :kc[b]] = _fold_bias_word(torch.log2(mult[b, :kc[b]].float()), dtype)
        kbias = kbias.to(DEV)
    # output window (B, Mqp, C) with ldo > C inside a buffer with a guard block behind the last row
    ldo = C + 24
    canary = CANARY32 if f32 else CANARY
    nb = 0 if ws is None else _ws_size(L, call, d, B, h, Mq, Mk, counts, ws, f32)
    qc = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=DEV)
    kcd = torch.tensor(kc, dtype=torch.int32, device=DEV) if mult is not None else None
    lib, s = L.lib(), L._stream()
    P = lambda t: None if t is None else t.data_ptr()

    def launch():
        obuf = torch.full(((B * Mqp + GUARD_ROWS) * ldo,), canary, dtype=torch.int32 if f32 else torch.int16, device=DEV)
        wsb = None if ws is None else torch.full((nb + 65536,), -1, dtype=torch.int8, device=DEV)
        head = (P(q), 2 * C, P(k), 3 * C, P(vt), ldvt, P(obuf), ldo, DT_CODE[dtype], B, h, Mq, Mqp, Mk, Mkp, d, float(scale))
        if call == "kv":
            rc = lib.vtm_attention_kv(*head, share, P(wsb), nb, s)
        elif call == "bounded":
            rc = lib.vtm_attention_kv_bounded(*head, P(qc), P(wsb), nb, s)
        elif call == "shared_bounded":
            rc = lib.vtm_attention_kv_shared_bounded(*head, share, P(qc), P(wsb), nb, s)
        else:
            rc = lib.vtm_attention_kv_folded(*head, P(qc), P(kcd), P(kbias), Mk, P(wsb), nb, s)
        L._check(rc, call)
        torch.cuda.synchronize()
        # 1. nothing written outside the (B, Mqp, C) window
        ob = obuf.view(B * Mqp + GUARD_ROWS, ldo)
        assert bool((ob[:B * Mqp, C:] == canary).all()), "a write into the gap columns past C"
        assert bool((ob[B * Mqp:] == canary).all()), "a write behind the last output row"
        if f32:
            assert bool((ob[:B * Mqp].view(B, Mqp, ldo)[:, Mq:] == canary).all()), "a write into the rows Mq .. Mqp"
        # 2. the plan the launch took
        if wsb is not None:
            _check_workspace(sel, wsb, nb)
        return ob[:B * Mqp, :C].contiguous().view(dtype).view(B, Mqp, C)

    out = launch()
    if hook is not None:
        hook.compare(sel, launch, out, vt, rows, cnt, kc)
        return sel
    # 3. the oracle, over each sample's own keys (folded: with the copies)
    worst, scale_max = 0.0, 0.0 if f32 else 1.0       # (fp32: of max|ref| over the launch, not of max(1, .))
    for b in range(B):
        bs = b % src
        ridx = torch.tensor(sorted(rows[b]), device=DEV)
        if mult is not None:
            idx = torch.repeat_interleave(torch.arange(kc[b]), mult[b, :kc[b]].long()).to(DEV)
            kk, vv = k[bs, idx], v[b, idx]
        else:
            kk, vv = k[bs, :Mk], v[b]
        ref = oracle.attention_qkv(q[bs, ridx][None].float().cpu().numpy(), kk[None].float().cpu().numpy(),
                                   vv[None].float().cpu().numpy(), h, scale)[0]
        got = out[b, ridx].float().cpu().numpy()
        assert np.isfinite(got).all(), (b, "non-finite output")
        worst = max(worst, float(np.abs(got - ref).max()))
        scale_max = max(scale_max, float(np.abs(ref).max()))
    print(f"{sel.kind} {sel.plan} d={d} {dtype}: worst {worst:.3g} of scale {scale_max:.3g} = {worst / scale_max:.3g}")
    if f32:
        assert scale_max > 0.05, "the comparison should not be about zeros"
        assert worst <= BAR * scale_max, (sel.kind, sel.plan, d, worst, scale_max, worst / scale_max)
    else:
        assert worst < TOL[dtype] * scale_max, (sel.kind, sel.plan, d, str(dtype), worst, scale_max)
    return sel


def _binding_ws(L, dtype, B, h, Mq, Mk, d, bounded):
    """The workspace size _lib.attention / _lib.attention_kv hand to a launch of `dtype` operands (_lib._attention_ws, and
    for a launch with a q_count the larger of the two exports); 0 where they pass None."""
    code = DT_CODE[dtype]
    nb = int(L.lib().vtm_attention_ws_bytes_dtype(code, B, h, Mq, Mk, d))
    if bounded:
        nb = max(nb, int(L.lib().vtm_attention_kv_bounded_ws_bytes_dtype(code, B, h, Mq, Mk, d)))
    return nb


def _ws_size(L, call, d, B, h, Mq, Mk, counts, ws, f32=False):
    if ws != "lib":
        return int(ws)
    if f32:
        return max(_binding_ws(L, torch.float32, B, h, Mq, Mk, d, counts is not None), 65536)
    nb = int(L.lib().vtm_attention_ws_bytes(B, h, Mq, Mk, d))
    if counts is not None:                            # _lib.attention_kv: the larger of the two
        nb = max(nb, int(L.lib().vtm_attention_kv_bounded_ws_bytes(B, h, Mq, Mk, d)))
    return max(nb, 65536)                             # (a plan without records must leave a workspace untouched)


def _check_workspace(sel, wsb, nb):
    """The records a plan writes: every record of a live split item, nothing else (header: the DevPlan, exactly)."""
    w = wsb.view(torch.int32)
    if sel.header is not None:
        got = w[:44].cpu().tolist()
        assert got == sel.header, ("DevPlan", got, sel.header)
        assert bool((w[44:DEVPLAN_HEADER // 4] == -1).all())
    rw = sel.F.rec // 4
    base = sel.rec_base // 4
    assert sel.ws_used <= nb
    nrec = (sel.ws_used - sel.rec_base) // sel.F.rec if sel.split else 0
    region = w[base: base + nrec * rw].view(nrec, rw)
    written = (region != -1).all(1).cpu().tolist()
    untouched = (region == -1).all(1).cpu().tolist()
    for lin, ns, rec0 in sel.split:
        if sel.live(lin):
            assert all(written[rec0:rec0 + ns]), ("a record of a live split item was not written", sel.plan, lin, rec0)
        else:
            assert all(untouched[rec0:rec0 + ns]), ("a record of a dead item was written", sel.plan, lin, rec0)
    assert bool((w[sel.ws_used // 4:] == -1).all()), ("a write past the plan's records", sel.plan, sel.ws_used)


# ---------------------------------------------------------------------------------------------------------------------
# shapes that land on each plan (from the slot count of this device)
# ---------------------------------------------------------------------------------------------------------------------
def _shape(plan, F, items_per_block, n_cus):
    """(Mq, Mk, counts-or-None) for `plan` with `items_per_block` = (sources) x heads work items per query block."""
    S, QB, P = F.slots(n_cus), F.QB, items_per_block
    if plan == "single":
        return 3 * QB - 5, 1000, None
    if plan == "tail":                               # one whole round + a last round of P items, 33 key tiles
        nqb = S // P + 1
        return (nqb - 1) * QB + QB // 2 + 3, 2100, None
    if plan in ("device", "nows"):                   # 2.6 rounds of live items: tiers split 2 and 4 ways
        nqb = cdiv(2 * S + 5 * S // 8, P)
        return nqb * QB - QB // 2, 2100, "device"
    if plan == "split_all":                           # >= 2 rounds, 65 key tiles, a workspace window below the device plan
        nqb = 2 * S // P + 2
        return (nqb - 1) * QB + QB // 2, 4100, "split_all"
    raise AssertionError(plan)


def _counts(kind, B, Mq, QB, share=1):
    nqb = cdiv(Mq, QB)
    if kind == "device":      # one sample inside its first block, the others long and different
        c = [77, (nqb - 3) * QB + QB // 2 + 1, (nqb - 1) * QB + QB // 3][-B:] if B <= 3 else None
        return c
    return [(nqb - 1) * QB + 7, QB + 3][:B]           # split_all


def _mult(B, Mu, seed):
    rng = np.random.default_rng(seed)
    m = rng.choice([1, 1, 2, 4], size=(B, Mu))
    for b in range(B):
        m[b, Mu - 3 - 250 * b:] = 0                   # per-sample device-side key counts below the host bound
    return m


PLANS = ("single", "tail", "device", "nows", "split_all")
EXPECT = {"single": "single", "tail": "tail", "device": "device", "nows": "single", "split_all": "split_all"}


def plan_args(kind, d, plan, n_cus, fold=False, ng=1, src=1, h=8):
    """The run_case arguments of one (family, plan) case on a device of `n_cus` CUs (host arithmetic only)."""
    F = Family(kind, d, ng)
    share = ng
    if plan in ("device", "nows") and ng == 1:
        B = 3
    else:
        B = 2 * ng if (ng > 1 and src == 2) else (ng if ng > 1 else 2)
    items_B = B // share if kind == "16g" else B
    Mq, Mk, ck = _shape(plan, F, items_B * h, n_cus)
    counts = None
    if ck is not None:
        if ng > 1:                                   # every sample of a group: its source's count
            cs = _counts(ck, src, Mq, F.QB) if src > 1 else [(cdiv(Mq, F.QB) - 1) * F.QB + F.QB // 3]
            counts = [cs[b % src] for b in range(B)]
        else:
            counts = _counts(ck, B, Mq, F.QB)
    if ng > 1:
        call = "shared_bounded" if counts is not None else "kv"
    elif fold:
        call = "folded"
    else:
        call = "bounded" if counts is not None else "kv"
    ws = "lib"
    if plan == "nows":
        ws = None
    elif plan == "split_all":
        p = plan_tail(B, h, Mq, Mk, F.QB, F.wg, F.rec, True, n_cus)
        dev = devplan_ws_bytes(F.slots(n_cus), F.rec)
        assert p["split_all"] and p["ws_bytes"] < dev, ("empty workspace window for split_all", p, dev)
        ws = p["ws_bytes"]
    combine = None
    if EXPECT[plan] != "single":
        combine = "f32" if kind == "f32" else "16" if kind != "k" else ("plain" if (pv16_for(d) or EXPECT[plan] != "tail") else "parts")
    mult = _mult(B, Mk, d + B) if fold else None
    return dict(call=call, d=d, B=B, h=h, Mq=Mq, Mk=Mk, expect=(kind, EXPECT[plan], combine), share=share, counts=counts,
                ws=ws, mult=mult, seed=zlib.crc32(f"{kind}/{plan}/{ng}/{src}".encode()) % 1000)


def ws_size_restated(call, d, B, h, Mq, Mk, counts, ws, f32, n_cus):
    """_ws_size from the restated planners (test_workspace_sizes_equal_the_restated_plans and
    test_binding_workspace_holds_the_fp32_plans hold them to the library's exports)."""
    if ws != "lib":
        return int(ws)
    size = ws_bytes_f32 if f32 else (lambda B, h, Mq, Mk, d, bounded, n: ws_bytes_any(B, h, Mq, Mk, d, bounded, n))
    nb = size(B, h, Mq, Mk, d, False, n_cus)
    if counts is not None:
        nb = max(nb, size(B, h, Mq, Mk, d, True, n_cus))
    return max(nb, 65536)


def _plan_case(L, oracle, kind, dtype, d, plan, fold=False, ng=1, src=1, h=8):
    return run_case(L, oracle, dtype=dtype, **plan_args(kind, d, plan, cus(), fold=fold, ng=ng, src=src, h=h))


DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("d", KERNEL_DIMS)
def test_attention_kernel_plans(L, oracle, d, plan, dtype):
    """attention_kernel<T, D>: every head dim under every plan (host tail: the parts combine at d != 8, the plain one at
    d = 8 -- 16-row O^T records)."""
    _plan_case(L, oracle, "k", dtype, d, plan)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("plan", PLANS)
def test_attention_kernel_folded_d8_plans(L, oracle, plan, dtype):
    """attention_kernel<T, 8, FOLD = true> (vtm_attention_kv_folded at d = 8): device-side key counts in every plan."""
    _plan_case(L, oracle, "k", dtype, 8, plan, fold=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("fold", [False, True], ids=["unfolded", "folded"])
def test_attention16s_plans(L, oracle, fold, plan, dtype):
    """attention16s_kernel<T, 40, FOLD>: self-attention and folded keys under every plan, attention16_combine_kernel."""
    _plan_case(L, oracle, "16s", dtype, 40, plan, fold=fold)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("plan", ["single", "tail", "device", "nows"])
@pytest.mark.parametrize("ng,src", [(2, 1), (3, 1), (2, 2), (3, 2)])
def test_attention16g_plans(L, oracle, ng, src, plan, dtype):
    """attention16g_kernel<T, 40, NG>: probabilities of source sample b for samples b + g * src_batch, one and two source
    samples (the device plan through vtm_attention_kv_shared_bounded)."""
    _plan_case(L, oracle, "16g", dtype, 40, plan, ng=ng, src=src)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("plan", ["single", "tail", "device"])
@pytest.mark.parametrize("d,ng", [(64, 3), (40, 4)])
def test_attention_kernel_shared_plans(L, oracle, d, ng, plan, dtype):
    """attention_kernel's shared-probability path: d = 64 over 3 groups, and d = 40 over 4 (beyond attention16g)."""
    _plan_case(L, oracle, "k", dtype, d, plan, ng=ng)


# ---------------------------------------------------------------------------------------------------------------------
# device plans on both sides of a family's XCD threshold
# ---------------------------------------------------------------------------------------------------------------------
XCD_SIDES = ("below_split", "below", "at", "above")


def _xcd_threshold_case(L, oracle, kind, dtype, d, B, side):
    """A device-planned launch whose (sample, head) pairs divide over the 8 XCDs, with the live query blocks per pair
    (the longest sample's, DevPlan.nqb) just below and at the family's xcd_min_nqb: the main kernel and the combine kernel
    each decide from that device value whether the items are pinned to XCDs (item_of), and a combine kernel that decided
    otherwise would merge other items' records.  The smallest shape that takes the device plan: B h = 8 pairs per round of
    slots, Mq = threshold x QB rows, 16 key tiles (a tier may split in two, 8 tiles per piece).
    "below" / "at": threshold - 1 / threshold live blocks, as close as the threshold can be straddled.  With B h a multiple
    of 8 these two plans have no split tier on a 256-CU device (threshold x B h is a whole number of rounds, one block less
    a last round more than 0.8 full), so the combine kernel has no item there; "above" (threshold + 1 blocks, Mq one block
    longer) and "below_split" (the largest count below the threshold whose plan has a split tier) are the nearest counts
    on either side at which main and combine kernel have to agree on the placement."""
    n_cus, h, Mk = cus(), 8, 1000
    F = Family(kind, d)
    S, thr = F.slots(n_cus), F.xcd_min
    assert (B * h) % 8 == 0
    plan_of = lambda n: device_plan([77] * (B - 1) + [n * F.QB], h, F.QB, S, cdiv(Mk, F.key_tile))
    if side == "below_split":
        live = next((n for n in range(thr - 1, 0, -1) if plan_of(n)[1] >= 2), None)
        assert live is not None, "no count below the threshold gives this device a split tier"
    else:
        live = thr + {"below": -1, "at": 0, "above": 1}[side]
    Mq = max(thr, live) * F.QB
    counts = [77] * (B - 1) + [(live - 1) * F.QB + F.QB // 3]
    assert cdiv(Mq, F.QB) * h * B >= 2 * S, "the shape does not take the device plan"
    sel = run_case(L, oracle, "bounded", dtype, d, B, h, Mq, Mk,
                   (kind, "device", "f32" if kind == "f32" else "16" if kind != "k" else "plain"),
                   counts=counts, seed=zlib.crc32(f"xcd/{kind}/{side}".encode()) % 1000)
    assert sel.nqb == live and (live >= thr) == (side in ("at", "above")), (sel.nqb, live, thr)
    if side in ("below_split", "above"):
        assert sel.header[1] >= 2 and sel.split, sel.header


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("side", XCD_SIDES)
def test_attention_kernel_plans_around_the_xcd_threshold(L, oracle, side, dtype):
    """attention_kernel<T, 64>: one sample of 8 heads, 63 / 64 (and 57 / 65) live blocks of 512 rows."""
    _xcd_threshold_case(L, oracle, "k", dtype, 64, 1, side)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("side", XCD_SIDES)
def test_attention16s_plans_around_the_xcd_threshold(L, oracle, side, dtype):
    """attention16s_kernel<T, 40>: 31 / 32 (and 28 / 33) live blocks of 512 rows.  Two samples of 8 heads: at 32 blocks
    one sample's 256 items are a single round of the 256 slots, which takes no device plan."""
    _xcd_threshold_case(L, oracle, "16s", dtype, 40, 2, side)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against the library
# ---------------------------------------------------------------------------------------------------------------------
def test_workspace_sizes_equal_the_restated_plans(L):
    """vtm_attention_ws_bytes / vtm_attention_kv_bounded_ws_bytes = the restated plans' sizes (d = 40: the largest over the
    three families, ws_bytes_any) over a grid of shapes that crosses every threshold of the planners."""
    n_cus = cus()
    lib = L.lib()
    n = 0
    for d in (8, 16, 32, 40, 64, 80, 96, 128, 160, 24):
        for B in (1, 2, 3, 4, 6):
            for h in (1, 5, 8):
                for Mq in (1, 100, 4100, 8448, 8704, 17408, 34816, 64513):
                    for Mk in (1, 77, 1000, 1024, 2048, 2100, 4032, 4100, 52224):
                        for bounded, fn in ((False, lib.vtm_attention_ws_bytes), (True, lib.vtm_attention_kv_bounded_ws_bytes)):
                            want = ws_bytes_any(B, h, Mq, Mk, d, bounded, n_cus)
                            got = int(fn(B, h, Mq, Mk, d))
                            assert got == want, (d, B, h, Mq, Mk, bounded, got, want)
                            n += 1
    assert n > 10000


# ---------------------------------------------------------------------------------------------------------------------
# the headline launches at full size
# ---------------------------------------------------------------------------------------------------------------------
def _mult_to(B, Mdup, seed):
    """Per sample: multiplicities 1 / 1 / 2 / 4 whose copies add up to exactly Mdup keys."""
    rng = np.random.default_rng(seed)
    rows = []
    for b in range(B):
        m = rng.choice([1, 1, 2, 4], size=Mdup)
        c = np.cumsum(m)
        n = int(np.searchsorted(c, Mdup)) + 1
        m = m[:n].copy()
        m[-1] -= int(c[n - 1] - Mdup)
        rows.append(m)
    Mu = max(len(r) for r in rows) + 41
    out = np.zeros((B, Mu), np.int64)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def _live_counts(F, B, h, Mq, Mk, min_tiers=2):
    """Per-sample counts of about 0.78 and 0.9 of Mq (the live fractions of the cfg-2 top block) for which the device
    plan has split tiers on this device: the second fraction is lowered from 0.9 until the last round is short enough."""
    for f1 in np.arange(0.90, 0.80, -0.005):
        counts = [int(0.78 * Mq), int(f1 * Mq)]
        if device_plan(counts, h, F.QB, F.slots(cus()), cdiv(Mk, KV))[1] >= min_tiers:
            return counts
    raise AssertionError("no live fraction near 0.9 gives this launch a split tail")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_headline_folded_bounded_launch_at_full_size(L, oracle, dtype):
    """The cfg-2 top block in steady state: attention16s_kernel<T, 40, FOLD = true> on 34 816 query rows with per-sample
    counts of 0.78 / 0.9 of them, keys folded from 52 224 copies (multiplicities 1 / 1 / 2 / 4), device-planned -- against the
    oracle over the DUPLICATED key sequence, at the plain bar (no per-element allowance)."""
    B, h, d, Mq, Mdup = 2, 8, 40, 34816, 52224
    mult = _mult_to(B, Mdup, 7)
    Mu = mult.shape[1]
    counts = _live_counts(Family("16s", d), B, h, Mq, Mu, min_tiers=3)
    sel = run_case(L, oracle, "folded", dtype, d, B, h, Mq, Mu, ("16s", "device", "16"), counts=counts, mult=mult, seed=3)
    assert sel.header[1] >= 3, sel.header            # whole items and at least two split tiers


@pytest.mark.parametrize("name,B,h,d,Mq,Mk,expect", [
    ("cfg-4 top block", 2, 8, 40, 18432, 27648, ("16s", "device", "16")),
    ("cfg-5 top block", 2, 5, 64, 64513, 90319, ("k", "device", "plain")),
])
def test_top_blocks_bounded_at_full_size(L, oracle, name, B, h, d, Mq, Mk, expect):
    """cfg-4 / cfg-5's largest self-attention launches, query-bounded (0.78 / 0.9 live), against the oracle."""
    counts = _live_counts(Family(expect[0], d), B, h, Mq, Mk)
    run_case(L, oracle, "bounded", torch.float16, d, B, h, Mq, Mk, expect, counts=counts, seed=5)


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 family: attention_f32_kernel under every plan
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("d", F32_DIMS)
def test_attention_f32_plans(L, oracle, d, plan):
    """attention_f32_kernel<D>: every head dim under every plan -- 128-row blocks on 2 workgroups per CU below d = 128,
    64-row blocks from there on, one workgroup per CU and the LDS opt-in at d = 160, the half chunk of d = 8 / 40;
    attention_f32_combine_kernel behind every split plan.  A device plan counts 33 x 2 key tiles where the host tail
    counts 33."""
    _plan_case(L, oracle, "f32", torch.float32, d, plan)


@pytest.mark.parametrize("plan", ["single", "tail", "device"])
@pytest.mark.parametrize("ng", [2, 3])
@pytest.mark.parametrize("d", [40, 160])
def test_attention_f32_shared_plans(L, oracle, d, ng, plan):
    """Shared probabilities in attention_f32_kernel (b % src_batch): vtm_attention_kv over 2 and 3 groups under the single
    and the host tail plan, vtm_attention_kv_shared_bounded under the device plan.  The grid runs over all samples; the
    sharing samples' q / k hold garbage and their expected rows come from the source's."""
    _plan_case(L, oracle, "f32", torch.float32, d, plan, ng=ng)


@pytest.mark.parametrize("side", XCD_SIDES)
@pytest.mark.parametrize("d,B", [(64, 2), (160, 1)])
def test_attention_f32_plans_around_the_xcd_threshold(L, oracle, d, B, side):
    """attention_f32_kernel / attention_f32_combine_kernel on both sides of F_XCD_MIN_NQB = 64 live blocks: d = 64 (two
    samples of 8 heads on 2 workgroups per CU: 64 blocks of 128 rows are the two rounds a device plan asks for) and
    d = 160 (one sample, 64-row blocks, one workgroup per CU)."""
    _xcd_threshold_case(L, oracle, "f32", torch.float32, d, B, side)


# ---------------------------------------------------------------------------------------------------------------------
# split pieces that hold no tile
# ---------------------------------------------------------------------------------------------------------------------
EMPTY_PIECE_CASES = [("f32", torch.float32, 40, "device"), ("f32", torch.float32, 160, "device")] + \
    [(kind, dt, d, plan) for kind, d in (("k", 64), ("16s", 40)) for dt in DTYPES for plan in ("tail", "device")]


@pytest.mark.parametrize("kind,dtype,d,plan", EMPTY_PIECE_CASES,
                         ids=[f"{k}-{str(t).split('.')[-1]}-d{d}-{p}" for k, t, d, p in EMPTY_PIECE_CASES])
def test_split_pieces_without_a_tile(L, oracle, kind, dtype, d, plan):
    """129 key tiles cut 16 ways: tps = ceil(129 / 16) = 9, piece 14 holds tiles 126 .. 128 and piece 15 starts at tile 135,
    behind the last key.  Its workgroup must read nothing, still leave a record (max = -inf, denominator 0), and the
    combine kernel must pass over it.  fp32: 129 tiles of 32 keys under a device plan (the host tail counts 64-key
    tiles and splits 65 of them at most 8 ways); 16-bit: 129 tiles of 64 keys under the host tail (B h = 16 items in
    the last round) and under a device plan.  Shapes from this device's slots: 2 samples of 8 heads; tail: one whole
    round and 16 items; device: two rounds and a sixteenth, which the plan gives one 16-way tier."""
    n_cus, h, B = cus(), 8, 2
    F = Family(kind, d)
    S, P = F.slots(n_cus), B * h
    Mk = 4100 if kind == "f32" else 8200              # 128 whole tiles and 4 / 8 keys of another
    assert cdiv(Mk, F.key_tile) == 129 and len(pieces(Mk, 16, F.key_tile)) < 16, "no piece of this split is empty"
    if plan == "tail":
        nqb = S // P + 1
        Mq, counts, call = (nqb - 1) * F.QB + F.QB // 2 + 3, None, "kv"
        combine = "16" if kind != "k" else "parts" if P * 4 <= n_cus else "plain"
    else:
        nqb = cdiv(2 * S + S // 16, P)
        Mq, counts, call = nqb * F.QB, [77, (nqb - 1) * F.QB + F.QB // 3], "bounded"
        combine = "f32" if kind == "f32" else "16" if kind != "k" else "plain"
    sel = run_case(L, oracle, call, dtype, d, B, h, Mq, Mk, (kind, plan, combine), counts=counts,
                   seed=zlib.crc32(f"empty/{kind}/{plan}".encode()) % 1000)
    live16 = [lin for lin, ns, _ in sel.split if ns == 16 and sel.live(lin)]
    assert live16, ("the shape does not give a live item a 16-way split", sel.plan, sel.header)


# ---------------------------------------------------------------------------------------------------------------------
# the workspace the Python binding hands to an fp32 launch
# ---------------------------------------------------------------------------------------------------------------------
def _mid_block_shape(n_cus):
    """One sample of 8 heads at d = 80 whose fp32 plan has a short last round: one round of 128-row blocks and 4 blocks per
    head more over 13 056 keys.  256 CUs: Mq = 8704, the cfg-2 mid block's launch."""
    F = Family("f32", 80)
    return 1, 8, 80, (F.slots(n_cus) // 8 + 4) * F.QB, 13056


def test_fp32_and_16bit_plans_want_different_workspaces():
    """The shape that showed it, on 256 CUs, by the restated planners alone: the 16-bit planner sees 136 items of 512 rows
    on 256 slots (no whole round, no workspace), the fp32 planner 544 items of 128 rows on 512 slots -- a last round of 32
    items split 16 ways.  Neither family's size bounds the other's: the size has to be asked with the dtype."""
    B, h, d, Mq, Mk = _mid_block_shape(256)
    assert (Mq, Mk) == (8704, 13056)
    assert ws_bytes_any(B, h, Mq, Mk, d, False, 256) == 0
    assert ws_bytes_f32(B, h, Mq, Mk, d, False, 256) == 32 * 16 * 41984
    assert ws_bytes_f32(2, 8, 34816, 52224, 40, False, 256) < ws_bytes_any(2, 8, 34816, 52224, 40, False, 256)


def test_binding_workspace_holds_the_fp32_plans(L):
    """What _lib.attention / _lib.attention_kv hand to an fp32 launch (_binding_ws) is what the restated fp32 plans take --
    unbounded and bounded, all nine head dims, over a grid that crosses the planner's thresholds and holds the mid-block
    shape above -- and the 16-bit sizes asked with a dtype are the ones asked without."""
    n_cus = cus()
    lib = L.lib()
    mid = _mid_block_shape(n_cus)
    n = 0
    for d in F32_DIMS:
        shapes = [(B, h, Mq, Mk) for B in (1, 2, 3) for h in (5, 8) for Mq in (100, 4100, 8448, 8704, 17408, 34816)
                  for Mk in (77, 1000, 2100, 4100, 13056, 52224)] + [(mid[0], mid[1], mid[3], mid[4])]
        for B, h, Mq, Mk in shapes:
            for bounded in (False, True):
                want = ws_bytes_f32(B, h, Mq, Mk, d, bounded, n_cus)
                if bounded:                           # _lib.attention_kv: the larger of the two exports
                    want = max(want, ws_bytes_f32(B, h, Mq, Mk, d, False, n_cus))
                got = _binding_ws(L, torch.float32, B, h, Mq, Mk, d, bounded)
                assert got >= want, ("the binding hands an fp32 launch less than its plan takes", d, B, h, Mq, Mk, bounded,
                                     got, want)
                assert got == want, (d, B, h, Mq, Mk, bounded, got, want)
                for dt in DTYPES:
                    assert int(lib.vtm_attention_ws_bytes_dtype(DT_CODE[dt], B, h, Mq, Mk, d)) == \
                        int(lib.vtm_attention_ws_bytes(B, h, Mq, Mk, d))
                    assert int(lib.vtm_attention_kv_bounded_ws_bytes_dtype(DT_CODE[dt], B, h, Mq, Mk, d)) == \
                        int(lib.vtm_attention_kv_bounded_ws_bytes(B, h, Mq, Mk, d))
                n += 1
    assert n > 3000
    assert ws_bytes_f32(*mid[:2], mid[3], mid[4], 80, False, n_cus) > 0, "the mid-block shape has no tail on this device"


def test_binding_gives_fp32_its_host_tail(L, oracle):
    """_lib.attention_kv on the mid-block shape in fp32: the launch leaves every record of its 16-way tail in the binding's
    workspace (prefilled with 0xFF), and rows of whole and of split items agree with the oracle."""
    n_cus = cus()
    B, h, d, Mq, Mk = _mid_block_shape(n_cus)
    F = Family("f32", d)
    p = plan_tail(B, h, Mq, Mk, F.QB, F.wg, F.rec, False, n_cus)
    assert p["nsplit"] > 1 and p["ws_bytes"] > 0, ("the shape does not select the plan it names", p)
    C = h * d
    g = torch.Generator(device=DEV).manual_seed(5)
    q = torch.randn(B, Mq, C, generator=g, device=DEV)
    k = torch.randn(B, Mk, C, generator=g, device=DEV)
    vt = torch.randn(B, C, Mk, generator=g, device=DEV)
    ws, nb = L._attention_ws(B, h, Mq, Mk, d, q.device, q.dtype)
    assert ws is not None and nb >= p["ws_bytes"], (nb, p)
    ws.fill_(255)
    o = L.attention_kv(q, k, vt, h, Mq, Mk, d ** -0.5)
    torch.cuda.synchronize()
    w = ws[:ws.numel() // 4 * 4].view(torch.int32)
    assert bool((w[:p["ws_bytes"] // 4] != -1).all()), "a record of the tail was not written: the launch took no tail"
    assert bool((w[p["ws_bytes"] // 4:] == -1).all()), "a write past the tail's records"
    rs = np.random.default_rng(11)
    rows = np.unique(np.concatenate([np.arange(4), rs.integers(0, Mq, 40), np.arange(Mq - 4, Mq)]))
    ridx = torch.from_numpy(rows).to(DEV)
    ref = oracle.attention_qkv(q[:, ridx].cpu().numpy(), k.cpu().numpy(),
                               np.ascontiguousarray(vt.transpose(1, 2).cpu().numpy()), h, d ** -0.5)
    err = float(np.abs(o[:, ridx].cpu().numpy() - ref).max()) / float(np.abs(ref).max())
    print(f"fp32 mid block through the binding: {err:.3g} of max|ref|")
    assert err <= BAR, err
