"""Online-softmax corner scenarios for the self-attention core -- attention_kernel, attention16s_kernel, attention16g_kernel,
attention_f32_kernel and the combine kernels behind their key-split plans -- placed relative to the launch plan, with the
float64 models that prove on the host what each scenario reaches.  The side kernels' counterpart is softmax_corners.py,
whose census, state machine and planting scheme (query g u, key c u, the other keys orthogonal to u) are reused here; the
plans are the restated planner of test_gpu_attention_plans.py.  Host only (numpy / torch CPU).

One launch carries every scenario.  Each (source sample, head) pair of a call is a softmax of its own -- a SLOT -- and gets
one scenario (SCENARIOS; folded-key calls add fold_bias_driven) or stays the unplanted CONTROL.  Score heights are
softmax_corners': spikes of 12 log2 units, staircases of 10 and of 6.8 .. 7.7 per tile, +-200 / -230 for the dominant and
very negative rows, x3 operands for wide_range.

Placement follows the Selection of the call:
  * planted query rows lie in a whole item, in a live split item of every tier the slot has, in the partial last wave of the
    last block and at row count - 1 (Slot.blocks / Slot.rows);
  * in a block the rows go to single ROW GROUPS -- the rows that share one `__all(...)` test, machine() -- so that a planted
    group rescales next to groups that do not.  attention16s_kernel: groups 2 w and 2 w + 1 are sub-tiles A and B of wave w
    (attention16.hip:98); group 2 is wave 1's A alone, group 7 wave 3's B alone, groups 10 and 11 both sub-tiles of wave 5;
  * planted keys sit (key_tiles) in the last tile of a piece, the first tile of the next piece, the tile after that (the
    first one a piece can rescale a finite state in), the last full tile and the ragged last tile -- of the finest split
    the plan has, of a two-way cut for a single launch.  late_spike's spikes climb by 12 over the first four positions, so
    that each is a rescale of a finite state and every piece's record carries another maximum; its key in the ragged tile
    stays 3 below the last spike: a weight of 1/8 in the tile right after a raise, which a shift that is stale for one tile
    turns into 2^9.  The rescale IN the ragged tile is the staircases' (a step in every tile) and last_key_dominant's.

Where the split items are.  Work items run query blocks fastest, so the short last round of a host tail belongs to the
LAST (sample, head) pair alone and a device plan's tiers to the last few pairs; only split_all splits every item.  The
scenarios that matter to a combine kernel (COMBINE_FIRST) are dealt to the slots with split items first, in an order that
rotates with the configuration and dtype: across the tail cases each of them meets each combine kernel, and the host test
asserts per case which ones did.

Folded keys: multiplicities are per (sample, key), shared by the heads.  The key of multiplicity 4096 sits in sample 0 one
tile behind the third spike position (every planted row is at 36 or more by then, so the other heads of sample 0 do not
notice it); every planted key has multiplicity 1."""
import collections
import functools
import math
import zlib

import numpy as np
import torch

import softmax_corners as SC
import test_gpu_attention_plans as P
from test_gpu_fp32_attention import BAR

LOG2E = SC.LOG2E
H = 8
THR = 8.0                                                     # DEFER_THR, attention_common.h:23
SCENARIOS = ("late_spike", "staircase_over", "staircase_under", "first_key_dominant", "last_key_dominant",
             "all_very_negative", "wide_range")
FOLD_SCENARIO, CONTROL = "fold_bias_driven", "control"
COMBINE_FIRST = ("staircase_over", "last_key_dominant", "late_spike", "first_key_dominant")
DROP_ALPHA = ("late_spike", "staircase_over", "staircase_under", FOLD_SCENARIO)
EQUAL_MAXIMA = COMBINE_FIRST
STALE_SHIFT = ("late_spike",)
ONE_KEY = {"first_key_dominant": "first", "last_key_dominant": "last"}
PRESCALED = ("wide_range",)                                   # the slots whose bar carries prescaled_term on d % 16 != 0 heads
COMPANION = 3.0                                               # late_spike's last key: so far below the last spike
SPIKE, RISE_OVER, RISE_UNDER, UNDER_SPREAD, DOMINANT, NEGATIVE = 12.0, 10.0, 6.8, 0.13, 200.0, 230.0
FOLD_MULT = 4096
TOL = P.TOL

Config = collections.namedtuple("Config", "name kind d fold ng plans dtypes")
_P4, _P3 = ("single", "tail", "device", "split_all"), ("single", "tail", "device")
_D16 = (torch.float16, torch.bfloat16)
CONFIGS = (
    Config("k-d64", "k", 64, False, 1, _P4, _D16), Config("k-d80", "k", 80, False, 1, _P4, _D16),
    Config("k-d160", "k", 160, False, 1, _P4, _D16), Config("k-d8", "k", 8, False, 1, _P4, _D16),
    Config("k-d8-folded", "k", 8, True, 1, _P4, _D16),
    Config("k-d40-x4", "k", 40, False, 4, _P3, _D16),       # the only way to attention_kernel's PV16 path at d = 40
    Config("k-d64-x3", "k", 64, False, 3, _P3, _D16),
    Config("16s", "16s", 40, False, 1, _P4, _D16), Config("16s-folded", "16s", 40, True, 1, _P4, _D16),
    Config("16g-x2", "16g", 40, False, 2, _P3, _D16), Config("16g-x3", "16g", 40, False, 3, _P3, _D16),
    Config("f32-d40", "f32", 40, False, 1, _P4, (torch.float32,)), Config("f32-d64", "f32", 64, False, 1, _P4, (torch.float32,)),
    Config("f32-d160", "f32", 160, False, 1, _P4, (torch.float32,)),
)
CONFIG = {c.name: c for c in CONFIGS}
SENSITIVITY_PLAN = "device"                                   # the split plan every family has


def gpu_cases():
    """Every (configuration, plan, dtype) the GPU module runs; the host module proves the preconditions of exactly these."""
    return [(c.name, plan, t) for c in CONFIGS for plan in c.plans for t in c.dtypes]


def case_id(c):
    return f"{c[0]}-{c[1]}-{str(c[2]).split('.')[-1]}"


def machine(kind, d):
    """(rows per group, keys per tile) of the family's branch `if (!__all(... <= m_run + DEFER_THR))`:
    attention_kernel: the 32 queries of a wave, q0 + (lane & 31), 64-key tiles (attention.hip:199, 365 / 381, 422);
    attention16s_kernel: per sub-tile of 32 rows, qblock0 + (wave * 2 + sub) * 32 + (lane & 31) (attention16.hip:98, 260, 390,
    416); attention16g_kernel: the 32 queries of a wave (attention16g.hip:321, 330); attention_f32_kernel: the 16 * NQH
    queries of a wave, q0 + 16 qh + (lane & 15), NQH = 1 from d = 128 on, 32-key tiles (attention_f32.hip:30, 34, 286-288)."""
    if kind == "f32":
        return 16 * (1 if d >= 128 else 2), P.KT32
    return P.QW, P.KV


def scenarios_of(cfg):
    return SCENARIOS + ((FOLD_SCENARIO,) if cfg.fold else ())


# ---------------------------------------------------------------------------------------------------------------------
# the float64 models
# ---------------------------------------------------------------------------------------------------------------------
def combine64(records, equal_maxima=False):
    """The combine kernels in float64: records [(o unnormalised, m, l)] of the pieces of an item -> o / l with every record
    weighted by exp2(m_piece - m_all) (attention.hip:61-77, 115-128).  equal_maxima: the records are added as they are."""
    m_all = np.max([m for _, m, _ in records], axis=0)
    o = np.zeros_like(records[0][0])
    l = np.zeros_like(records[0][2])
    for oi, mi, li in records:
        w = np.ones_like(mi) if equal_maxima else np.exp2(mi - m_all)
        o += w[:, None] * oi
        l += w * li
    return o / l[:, None]


def split_softmax64(S, V, pcs, width, tile, dead, drop_alpha=False, stale_shift=False, combine_equal_maxima=False):
    """An item's rows (whole row groups; S: rows x keys in log2 units, V: keys x d) the way a plan computes them:
    online_softmax64 per piece [lo, hi) of `pcs` with the family's group width and tile, the pieces folded by combine64.
    -> (o / l, [the piece maxima])."""
    recs = []
    for lo, hi in pcs:
        (o, m, l), = SC.online_softmax64([S[:, lo:hi]], [V[lo:hi]], tile=tile, wave=width, thr=THR, dead=[dead[lo:hi]],
                                         drop_alpha=drop_alpha, stale_shift=stale_shift)
        recs.append((o * l[:, None], m, l))
    if len(recs) == 1 and not combine_equal_maxima:
        return recs[0][0] / recs[0][2][:, None], [recs[0][1]]
    return combine64(recs, combine_equal_maxima), [m for _, m, _ in recs]


# ---------------------------------------------------------------------------------------------------------------------
# a launch: plan, slots, placement, operands
# ---------------------------------------------------------------------------------------------------------------------
Block = collections.namedtuple("Block", "qb lo groups items special")   # items: [(grid sample, pieces of its item)]


class Slot:
    """One (source sample, head): its scenario, where its planted rows and keys are, and its direction u."""


def key_tiles(mk, ns, tile):
    """The five tile positions of the planted keys for `mk` keys cut `ns` ways (see the module docstring)."""
    pcs = P.pieces(mk, ns, tile)
    te0, tb1 = pcs[0][1] // tile, pcs[1][0] // tile
    assert mk % tile, "the shapes of the plan cases all end on a ragged tile"
    out = [te0 - 1, tb1, tb1 + 1, mk // tile - 1, mk // tile]
    assert out == sorted(set(out)) and out[0] >= 1, out
    return out


def _key_in(t, off, mk, tile):
    return t * tile + off % min(tile, mk - t * tile)


def _slot_blocks(sel, slot_b, head, src, Mq, cnt, width, mk, tile):
    """The query blocks a slot's rows are planted in: the first whole item, the first live item of every split tier, the
    block of row count - 1 and the block that ends in a partial wave."""
    QB, nqb = sel.F.QB, sel.nqb
    ns_of = {lin: ns for lin, ns, _ in sel.split if sel.live(lin)}
    per_qb = {}
    for gb in range(slot_b, sel.items_B, src):
        for qb in range(nqb):
            lin = (gb * sel.h + head) * nqb + qb
            if sel.live(lin) and qb * QB < cnt:
                per_qb.setdefault(qb, []).append((gb, ns_of.get(lin, 1)))
    want = {}
    for qb in sorted(per_qb):
        for _, ns in per_qb[qb]:
            want.setdefault(ns, qb)
    special_rows = {cnt - 1}
    if Mq % width and (Mq // width) * width < cnt:
        special_rows.add(min(cnt - 1, (Mq // width) * width + (Mq % width) // 2))
    picked = sorted(set(want.values()) | {r // QB for r in special_rows})
    blocks = []
    for qb in picked:
        lo, hi = qb * QB, min((qb + 1) * QB, cnt)
        ng = P.cdiv(hi - lo, width)
        groups = [g for g in (2, 7, 10, 11) if g < ng] or [ng - 1]
        rows = {}
        for g in groups:
            live = min(width, hi - lo - g * width)
            rows[g] = [lo + g * width + (5 + 3 * g) % live]
        special = sorted(r for r in special_rows if r // QB == qb)
        for r in special:
            rows.setdefault((r - lo) // width, []).append(r)
        items = [(gb, P.pieces(mk, ns, tile)) for gb, ns in per_qb[qb]]
        blocks.append(Block(qb, lo, {g: sorted(set(r)) for g, r in rows.items()}, items, bool(special)))
    return blocks


class Launch:
    """Everything of one (configuration, plan, dtype) on a device of n_cus CUs: the run_case arguments, the Selection, the
    slots, and the operands -- q (src, Mq, C) and k (src, Mk, C) of the source samples, v (B, Mk, C) -- in the call's dtype."""

    def slot_of(self, b, head):
        return self.slots[(b % self.src, head)]

    # -- float64 views -------------------------------------------------------------------------------------------------
    def scores(self, s, rows, k=None, bias=None, prescaled=False):
        """(rows, mk) scores of slot s in log2 units from the rounded operands (prescaled: from the query pre-scaled in
        fp32 and rounded to the operand type once more, as the headers of the d % 16 != 0 kernels state --
        attention.hip:170-175, 232)."""
        d, sl = self.d, slice(s.head * self.d, (s.head + 1) * self.d)
        if k is None:
            kk = self._f64.get(("k", s.b, s.head))
            if kk is None:
                kk = self._f64[("k", s.b, s.head)] = self.k[s.b, :s.mk, sl].double().numpy()
        else:
            kk = k[:s.mk].double().numpy()
        qq = self.q[s.b, rows, sl]
        if prescaled:
            c = np.float32(np.float32(d ** -0.5) * np.float32(LOG2E))
            S = (qq.float() * float(c)).to(self.dtype).double().numpy() @ kk.T
        else:
            S = qq.double().numpy() @ kk.T * (d ** -0.5 * LOG2E)
        bias = self.bias[s.b] if bias is None else bias
        return S + bias[None, :s.mk]

    def values(self, b, s, v=None):
        if v is not None:
            return v[b, :s.mk, s.head * self.d:(s.head + 1) * self.d].double().numpy()
        key = ("v", b, s.head)
        if key not in self._f64:
            self._f64[key] = self.v[b, :s.mk, s.head * self.d:(s.head + 1) * self.d].double().numpy()
        return self._f64[key]

    def reference(self, b, s, rows, v=None, unplanted=False, prescaled=False):
        """The plain float64 softmax of output sample b's rows in slot s (unplanted: without what the scenario planted)."""
        S = self.scores(s, rows, k=s.k0 if unplanted else None, bias=s.bias0 if unplanted else None, prescaled=prescaled)
        return SC.plain_softmax64([S], [self.values(b, s, v)])[0][0]

    def bar(self, ref_absmax):
        return BAR * ref_absmax if self.dtype == torch.float32 else TOL[self.dtype] * max(1.0, ref_absmax)

    def bar_upper(self):
        """The largest bar a run of this launch can have: every output is a convex combination of v rows."""
        return self.bar(float(self.v.abs().max()))

    def carries_prescaled_term(self, s):
        return self.dtype != torch.float32 and self.d % 16 != 0 and s.name in PRESCALED

    def prescaled_term(self, b, s, rows, ref):
        """|reference with the query pre-scaled and rounded as the kernel header states - plain reference| x 2, per
        element; from the operands alone."""
        return 2.0 * np.abs(self.reference(b, s, rows, prescaled=True) - ref)


def _assign(cfg, dtype, slots, split_slots):
    """slot -> scenario name.  fold_bias_driven goes to sample 0; the combine scenarios go to the slots with split items
    first (rotated by configuration and dtype), then every name at least once, then the control, then the names again."""
    names = list(scenarios_of(cfg))
    rot = zlib.crc32(f"{cfg.name}/{dtype}".encode()) % len(COMBINE_FIRST)
    first = list(COMBINE_FIRST[rot:] + COMBINE_FIRST[:rot])
    order = first + [n for n in names if n not in first and n != FOLD_SCENARIO]
    out = {}
    if cfg.fold:
        home = [s for s in slots if s[0] == 0 and s not in split_slots] or [s for s in slots if s[0] == 0]
        out[home[0]] = FOLD_SCENARIO
    free_split = [s for s in split_slots if s not in out]
    free_other = [s for s in slots if s not in out and s not in free_split]
    todo = list(order)
    for s in free_split:
        if not todo:
            break
        out[s] = todo.pop(0)
    free_split = [s for s in free_split if s not in out]
    rest = free_other + free_split
    for s in rest:
        if s in out:
            continue
        if todo:
            out[s] = todo.pop(0)
        elif CONTROL not in out.values():
            out[s] = CONTROL
        else:
            out[s] = order[len(out) % len(order)]
    assert not todo and CONTROL in out.values(), (cfg.name, todo)
    return out


def _round(t, dtype):
    return t.to(dtype, copy=True)


def _direction(g, d):
    """A direction u with |u|^2 = d: d - 1 elements of one size with random signs and one of an eighth of it, which gives
    _along an element whose rounding step is 64 times finer than the others' to end on."""
    u = torch.where(torch.rand(d, generator=g) < 0.5, -1.0, 1.0)
    u[-1] *= 0.125
    return u * (math.sqrt(d) / float(u.norm()))


def _along(c, u, dtype):
    """c u in `dtype` with the rounding error fed forward from element to element, the small element last, so that (the
    rounded vector) . u is c |u|^2 to within that element's rounding: a staircase of 65 steps in bf16 is otherwise off by a
    log2 unit at its top, more than the margin between its rises and the threshold."""
    out = torch.empty_like(u)
    rem, left = c * float(u @ u), float(u @ u)
    for e in torch.argsort(u.abs(), descending=True).tolist():
        ue = float(u[e])
        x = torch.tensor(rem * ue / left).to(dtype).float()
        out[e] = x
        rem -= float(x) * ue
        left -= ue * ue
    return out


@functools.lru_cache(maxsize=2)
def build(name, plan, dtype, n_cus):
    """The Launch of one case.  Cached: the tests share one build and must not write into it."""
    cfg = CONFIG[name]
    f32 = dtype == torch.float32
    L = Launch()
    L._f64 = {}                                      # float64 views of k and v per (sample, head), made once
    L.cfg, L.plan, L.dtype, L.d = cfg, plan, dtype, cfg.d
    args = L.args = P.plan_args(cfg.kind, cfg.d, plan, n_cus, fold=cfg.fold, ng=cfg.ng)
    d, B, Mq, Mk, share, counts = cfg.d, args["B"], args["Mq"], args["Mk"], args["share"], args["counts"]
    C = H * d
    src = L.src = B // share
    L.B, L.Mq, L.Mk = B, Mq, Mk
    L.cnt = cnt = [Mq] * B if counts is None else list(counts)
    width, tile = L.width, L.tile = machine(cfg.kind, d)
    mult = None if args["mult"] is None else np.array(args["mult"])
    L.kc = kc = [Mk] * B if mult is None else [int((mult[b] > 0).sum()) for b in range(B)]
    ws_bytes = P.ws_size_restated(args["call"], d, B, H, Mq, Mk, counts, args["ws"], f32, n_cus)
    sel = L.sel = P.Selection(args["call"], d, B, H, Mq, Mk, share, P.pad8(Mk) + 16, ws_bytes, counts, n_cus, f32)
    assert (sel.kind, sel.plan, sel.combine) == args["expect"], ((sel.kind, sel.plan, sel.combine), args["expect"])
    tiers = sorted({ns for lin, ns, _ in sel.split if sel.live(lin)})
    L.ns_keys = max(tiers) if tiers else 2

    # the slots, their blocks and their scenario
    keys = [(b, head) for b in range(src) for head in range(H)]
    blocks = {s: _slot_blocks(sel, s[0], s[1], src, Mq, cnt[s[0]], width, kc[s[0]], tile) for s in keys}
    is_split = lambda s: any(len(pcs) > 1 for blk in blocks[s] for _, pcs in blk.items)
    split_slots = sorted((s for s in keys if is_split(s)), reverse=True)
    names = _assign(cfg, dtype, keys, split_slots)
    L.slots = {}
    for (b, head) in keys:
        s = Slot()
        s.b, s.head, s.name, s.mk, s.blocks = b, head, names[(b, head)], kc[b], blocks[(b, head)]
        s.rows = sorted(r for blk in s.blocks for rr in blk.groups.values() for r in rr)
        s.tiles = key_tiles(s.mk, L.ns_keys, tile)
        s.keys, s.k0, s.bias0, s.one_key = [], None, None, None
        L.slots[(b, head)] = s

    # folded keys: log2 of the multiplicities; every planted position 1, the fold key of sample 0 FOLD_MULT
    L.fold_key = None
    if mult is not None:
        for b in range(src):
            pos = {0, kc[b] - 1} | {_key_in(t, 3, kc[b], tile) for t in key_tiles(kc[b], L.ns_keys, tile)} \
                | {_key_in(t, 1, kc[b], tile) for t in range(P.cdiv(kc[b], tile))}
            mult[b, sorted(pos)] = 1
        L.fold_key = _key_in(key_tiles(kc[0], L.ns_keys, tile)[2] + 1, 5, kc[0], tile)
        mult[0, L.fold_key] = FOLD_MULT
        L.bias = np.where(mult > 0, np.log2(np.maximum(mult, 1)), 0.0).astype(np.float64)
    else:
        L.bias = np.zeros((src, Mk))
    L.mult = mult

    # the operands
    g = torch.Generator().manual_seed(zlib.crc32(f"{name}/{plan}".encode()))
    L.v = _round(torch.randn(B, Mk, C, generator=g), dtype)
    L.q = torch.empty(src, Mq, C, dtype=dtype)
    L.k = torch.empty(src, Mk, C, dtype=dtype)
    unit = math.sqrt(d) * LOG2E
    g0 = 128.0 / math.sqrt(d)                       # planted rows' length: a planted key of height h is, for every other
    for (b, head), s in L.slots.items():            # row, one more random key of spread h / 128 log2 units
        sl = slice(head * d, (head + 1) * d)
        Q, K = torch.randn(Mq, d, generator=g), torch.randn(Mk, d, generator=g)
        u = s.u = _direction(g, d)
        mk, nm = s.mk, s.name
        planted = nm in ("late_spike", "staircase_over", "staircase_under", FOLD_SCENARIO)
        if planted or nm in ONE_KEY:
            K[:mk] = SC._project(K[:mk], u)
        if planted:
            spread = UNDER_SPREAD if nm == "staircase_under" else 0.07
            # (fold_bias_driven plants no tall key, and its rows weigh ordinary keys against each other: short rows, whose
            # pre-scaled rounding on the d % 16 != 0 heads is the one N(0, 1) rows have)
            gain = SC._gain_base(d) if nm == FOLD_SCENARIO else g0
            for i, r in enumerate(s.rows):
                Q[r] = _along(gain * (1.0 + spread * (i % 8) / 7.0), u, dtype)
        if nm == "late_spike":
            s.keys = [_key_in(t, 3, mk, tile) for t in s.tiles]
            s.k0 = _round(K, dtype)
            for n, j in enumerate(s.keys):
                height = SPIKE * (n + 1) if n < len(s.keys) - 1 else SPIKE * n - COMPANION
                K[j] = _along(height / (g0 * unit), u, dtype)
        elif nm.startswith("staircase"):
            rise = RISE_OVER if nm == "staircase_over" else RISE_UNDER
            s.keys = [_key_in(t, 1, mk, tile) for t in range(P.cdiv(mk, tile))]
            s.k0 = _round(K, dtype)
            for t, j in enumerate(s.keys):
                K[j] = _along(rise * (t + 1) / (g0 * unit), u, dtype)    # (tile 0 too: above its rounding residue and fold bias)
        elif nm in ONE_KEY:
            Q += max(1.5, 7.0 / math.sqrt(d)) * u
            along = float((_round(Q, dtype).double() @ u.double()).min()) * d ** -0.5 * LOG2E
            assert along > 0
            s.one_key = 0 if nm == "first_key_dominant" else mk - 1
            s.keys = [s.one_key]
            s.k0 = _round(K, dtype)
            K[s.one_key] = DOMINANT / along * u
        elif nm == "all_very_negative":
            rows = sorted(r for blk in s.blocks for g_ in blk.groups
                          for r in range(blk.lo + g_ * width, min(blk.lo + (g_ + 1) * width, cnt[b])))
            s.rows = rows
            Q[rows] = SC._project(Q[rows], u) - 2.0 * u
            K[:mk] += NEGATIVE / (2.0 * unit) * u
        elif nm == "wide_range":
            Q *= 3.0
            K *= 3.0
        elif nm == FOLD_SCENARIO:
            s.keys = [L.fold_key]
            s.bias0 = L.bias[b].copy()
            s.bias0[L.fold_key] = 0.0
        L.q[b, :, sl], L.k[b, :, sl] = _round(Q, dtype), _round(K, dtype)
    return L


def group_rows(L, blk, groups):
    """All rows below Mq of `groups` of a block (whole row groups: what the models are run on)."""
    return [r for g in groups for r in range(blk.lo + g * L.width, min(blk.lo + (g + 1) * L.width, L.Mq))]
