"""Online-softmax corner scenarios for the cross-attention side kernels, with a float64 census of the branches they reach.

The six kernels (vtm_attention_kv_sets / _sets_masked / _sets_src, vtm_attention_kv_bias, vtm_attention_probs,
vtm_attention_word_map) each carry an online softmax of their own.  On N(0, 1) operands none of them ever rescales a finite
state; this module builds the operands on which they do and proves, on the host and in float64, that each scenario reaches the
branch it is named after:

  * ``census``            replays the branch structure of one (sample, head[, set]) score matrix and counts what was reached;
  * ``online_softmax64``  is the tile-wise state machine itself in float64, with three switches that each reproduce one
                          plausible kernel mistake -- a scenario is only worth running if its switch moves the result;
  * ``scenario``          builds the 16-bit operands (seeded randn, keys planted as multiples of a query direction);
  * ``reference`` / ``replay`` / ``bar``  the plain float64 result, the replayed one, and the bound a kernel is held to.

Host only (numpy / torch CPU).  Scores are in log2 units throughout: q . k * scale * log2(e) + bias * log2(e).

How keys are planted.  A planted query row is g * u for a direction u with |u|^2 = d (one per sample, head and query
operand), a planted key is c * u, and the other keys of the set are made orthogonal to u: the planted row scores 0 against
them (up to the 16-bit rounding) and g * c * sqrt(d) * log2(e) against the planted key, so a rise is what the builder says
it is, at every head dim.  Every other row sees c * u as one more random key of norm c * sqrt(d).
"""
import collections
import copy
import functools
import math

import numpy as np
import torch

LOG2E = 1.4426950408889634
TILE, WAVE, DEFER_THR = 64, 32, 8.0
U = 2.0 ** -24
B, H = 2, 2
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}            # the attention core's figures
DTYPES = (torch.float16, torch.bfloat16)
PAD = 3.0e4                                                  # pad keys between and behind the sets: never read as keys

SET_KINDS = ("sets", "sets_masked", "sets_src")
KEY_KINDS = ("bias", "probs", "words")
KINDS = SET_KINDS + KEY_KINDS
DIMS = (40, 64, 160)
SET_LAYOUTS = ((257, 77), (130, 5, 257))
SET_WEIGHTS = {2: (1.0, 0.6), 3: (1.0, -0.5, 1.5)}
SET_SRC = {2: (1, 0), 3: (1, 0, 1)}                          # "sets_src"; "sets_src_b" reads the operands the other way round
MK = {"bias": (130, 200), "probs": (130, 256), "words": (130, 256)}
MQ = {"sets": 300, "sets_masked": 300, "sets_src": 300, "sets_src_b": 300, "bias": 300, "probs": 150, "words": 150}

MASKED_VARIANTS = ("lead1", "lead2", "lead70", "interior_inf", "interior_1e4", "last", "single")
SCENARIOS = ("late_spike", "staircase_over", "staircase_under", "first_key_dominant", "all_very_negative", "wide_range",
             "bias_driven", "set_isolation") + tuple("masked_tiles:" + v for v in MASKED_VARIANTS)
DROP_ALPHA = ("late_spike", "staircase_over", "staircase_under", "bias_driven")   # the scenarios drop_alpha must move


def kinds_of(name):
    if name == "bias_driven" or name.startswith("masked_tiles"):
        return KEY_KINDS
    if name == "set_isolation":
        return SET_KINDS
    if name == "late_spike":
        return SET_KINDS + ("sets_src_b",) + KEY_KINDS
    return KINDS


def dims_of(name):
    return (8,) + DIMS if name == "late_spike" else DIMS


def gpu_cases():
    """Every (scenario, kind, d, dtype) the GPU tests run; the host tests prove the preconditions of exactly these."""
    return [(n, k, d, t) for n in SCENARIOS for k in kinds_of(n) for d in dims_of(n) for t in DTYPES]


def case_id(c):
    return f"{c[0]}-{c[1]}-d{c[2]}-{str(c[3]).split('.')[-1]}"


def layouts_of(kind):
    return SET_LAYOUTS if kind.startswith("sets") else MK[kind]


def is_pv(kind):
    return kind.startswith("sets") or kind == "bias"


def machine(kind):
    """(wave, thr) of the kernel's branch: the PV kernels test a wave of 32 rows against m_run + 8 (deferred rescale); the
    probs and word-map kernels rescale per row whenever the maximum rises."""
    return (WAVE, DEFER_THR) if is_pv(kind) else (1, 0.0)


# ---------------------------------------------------------------------------------------------------
# 1. the census and the float64 state machine
# ---------------------------------------------------------------------------------------------------
Census = collections.namedtuple("Census", "rescales rescale_tiles max_deferred masked score_absmax min_row_max rescale_waves "
                                          "waves")


def _pad_rows(S, wave, dead):
    """The rows a partial last wave adds: a dead lane's query reads as zero, its scores are the bias alone."""
    Mq, n = S.shape
    pad = -Mq % wave
    if not pad:
        return S
    row = np.zeros(n) if dead is None else np.asarray(dead, dtype=np.float64)
    return np.concatenate([S, np.broadcast_to(row, (pad, n))])


def census(S, tile=TILE, wave=WAVE, thr=DEFER_THR, dead=None, masked_below=-np.inf):
    """Replay the branch structure of one (sample, head[, set]) score matrix S (queries x keys, log2 units, -inf allowed):
    per wave of ``wave`` query rows and per tile of ``tile`` keys the test ``all(mt <= m_run + thr)``.  Returns

      rescales        how often the branch was taken by a wave in which a live row held a finite m_run (alpha != 0), and
      rescale_tiles   the tile indices at which that happened (rescale_waves: the waves, waves: how many there are);
      max_deferred    the largest rise of a row's tile maximum over its (possibly stale) m_run that was NOT followed;
      masked          (leading, interior, trailing) counts of tiles whose every score is <= masked_below (-inf);
      score_absmax    the largest finite |score|;
      min_row_max     the smallest row maximum."""
    S = np.asarray(S, dtype=np.float64)
    Mq, n = S.shape
    P = _pad_rows(S, wave, dead)
    rows = P.shape[0]
    nw = rows // wave
    live = np.arange(rows) < Mq
    m = np.full(rows, -np.inf)
    rescales, tiles, waves, max_def, dead_tiles = 0, set(), set(), 0.0, []
    for t, t0 in enumerate(range(0, n, tile)):
        s = P[:, t0:t0 + tile]
        dead_tiles.append(bool((S[:, t0:t0 + tile] <= masked_below).all()))
        mt = s.max(1)
        take = ~(mt <= m + thr).reshape(nw, wave).all(1)
        hit = take & (np.isfinite(m) & live).reshape(nw, wave).any(1)
        rescales += int(hit.sum())
        if hit.any():
            tiles.add(t)
            waves |= set(int(w) for w in np.nonzero(hit)[0])
        take_row = np.repeat(take, wave)
        left = ~take_row & live & np.isfinite(m) & np.isfinite(mt)
        if left.any():
            max_def = max(max_def, float((mt[left] - m[left]).max()))
        m = np.where(take_row, np.maximum(m, mt), m)
    nt = len(dead_tiles)
    lead = next((i for i, x in enumerate(dead_tiles) if not x), nt)
    trail = 0 if lead == nt else next(i for i, x in enumerate(reversed(dead_tiles)) if not x)
    finite = S[np.isfinite(S)]
    return Census(rescales, sorted(tiles), max_def, (lead, sum(dead_tiles) - lead - trail, trail),
                  float(np.abs(finite).max()) if finite.size else 0.0, float(S.max(1).min()), sorted(waves), nw)


def online_softmax64(S_sets, V_sets=None, *, tile=TILE, wave=WAVE, thr=DEFER_THR, dead=None, drop_alpha=False,
                     no_set_reset=False, exp_against_zero=False, stale_shift=False):
    """The kernels' state machine in float64: for every set s (S_sets[s]: queries x keys of the set, log2 units; V_sets[s]:
    keys x columns, or None) walk the tiles, keep (m_run, l_run, o) per row, follow the maximum only where the wave's branch
    is taken, take the exponent against m_run (against 0 while it is -inf) and fold the set as o / l.  Returns a list of
    (o / l or None, the m the exponents were last taken against, l) per set.  With no switch on this equals the plain
    softmax.  The switches, one kernel mistake each:

      drop_alpha        a taken rescale of a finite state does not multiply o and l_run (the word map's numerator is o);
      no_set_reset      m_run and l_run are carried across the end of a set (o is cleared by the fold itself);
      exp_against_zero  every exponent is taken against 0 instead of the running maximum.  Softmax is shift-invariant, so
                        this shows only through the range of the format p is computed in: p passes through fp32 here;
      stale_shift       the tile after a taken rescale of a finite state still takes its exponents against the maximum
                        from before that rescale (the kernels that carry the shift in the query's spare k-slot and do
                        not write it back after a raise)."""
    Mq = S_sets[0].shape[0]
    rows = Mq + (-Mq % wave)
    nw = rows // wave
    m, l = np.full(rows, -np.inf), np.zeros(rows)
    out = []
    for si, S in enumerate(S_sets):
        P = _pad_rows(np.asarray(S, dtype=np.float64), wave, None if dead is None else dead[si])
        V = None if V_sets is None or V_sets[si] is None else np.asarray(V_sets[si], dtype=np.float64)
        o = None if V is None else np.zeros((rows, V.shape[1]))
        if not no_set_reset:
            m, l = np.full(rows, -np.inf), np.zeros(rows)
        stale, m_stale = np.zeros(rows, dtype=bool), np.zeros(rows)
        for t0 in range(0, P.shape[1], tile):
            s = P[:, t0:t0 + tile]
            mt = s.max(1)
            take_row = np.repeat(~(mt <= m + thr).reshape(nw, wave).all(1), wave)
            m_new = np.where(take_row, np.maximum(m, mt), m)
            fin = np.isfinite(m)
            alpha = np.zeros(rows)                       # nothing finite seen before: exp2(-inf) = 0, and o = l = 0
            alpha[fin] = np.exp2(m[fin] - m_new[fin])
            if drop_alpha:
                alpha[fin & take_row] = 1.0
            raised = fin & take_row
            m_before = m
            m = m_new
            l = l * alpha
            m_use = np.where(np.isneginf(m), 0.0, m)
            if exp_against_zero:
                m_use = np.zeros(rows)
            if stale_shift:
                m_use = np.where(stale, m_stale, m_use)
                stale, m_stale = raised, m_before
            with np.errstate(over="ignore"):
                p = np.exp2(s - m_use[:, None])
                if exp_against_zero:
                    p = p.astype(np.float32).astype(np.float64)
            l = l + p.sum(1)
            if o is not None:
                vv = V[t0:t0 + tile]
                with np.errstate(invalid="ignore"):
                    o = o * alpha[:, None] + np.where(p == 0.0, 0.0, p) @ vv
        with np.errstate(invalid="ignore", divide="ignore"):
            out.append((None if o is None else (o / l[:, None])[:Mq], m_use[:Mq].copy(), l[:Mq].copy()))
    return out


def plain_softmax64(S_sets, V_sets=None):
    """The same return value from the textbook softmax."""
    out = []
    for si, S in enumerate(S_sets):
        S = np.asarray(S, dtype=np.float64)
        mx = S.max(1)
        p = np.exp2(S - mx[:, None])
        l = p.sum(1)
        V = None if V_sets is None or V_sets[si] is None else np.asarray(V_sets[si], dtype=np.float64)
        out.append((None if V is None else (p @ V) / l[:, None], mx, l))
    return out


# ---------------------------------------------------------------------------------------------------
# 2. the scenarios
# ---------------------------------------------------------------------------------------------------
class Case:
    """The operands of one call: q (B, Mqp, C), k / v (B, Mkp, C) in the 16-bit dtype (v is handed over transposed), ``sets``
    [(start, len, weight)] (one set for the per-key-bias kinds), and where they apply q_src / set_src, set_mask / mask, bias
    (B, Mk) fp32, w (B, Mk) fp32.  ``rows[b]``: the planted query rows of sample b; ``unplanted``: the same call without what
    the scenario planted (None: nothing was planted); ``masked[b]``: the keys of sample b whose probability is exactly 0."""

    def replace(self, **kw):
        c = copy.copy(self)
        c._cache = {}
        for n, v in kw.items():
            setattr(c, n, v)
        return c


def _r8(n):
    return (n + 7) // 8 * 8


def _slice(head, d):
    return slice(head * d, (head + 1) * d)


def _unit(d):
    return math.sqrt(d) * LOG2E      # the score of (g u) . (c u) is g * c * _unit(d)


def _direction(g, d):
    u = torch.randn(d, generator=g)
    return u * (math.sqrt(d) / float(u.norm()))


def _project(rows, u):
    """rows (n, d) made orthogonal to u."""
    return rows - (rows @ u)[:, None] * u[None, :] / float(u @ u)


def _planted_rows(Mq, b, every_wave):
    """One row in some waves, but not all (or in every wave); other rows per sample; the partial last wave is one of them."""
    nw = (Mq + WAVE - 1) // WAVE
    waves = range(nw) if every_wave else sorted({1, nw // 2 - b, nw - 1})
    rows = []
    for w in waves:
        width = min(WAVE, Mq - w * WAVE)
        rows.append(w * WAVE + (5 + 11 * b + 3 * w) % width)
    return rows


def _block_rows(Mq, b):
    """A block of queries: two whole waves and half of a third, another place per sample."""
    r0 = 32 + 32 * b
    return list(range(r0, min(Mq, r0 + 80)))


class _Builder:
    """fp32 masters of one call; ``finish`` rounds them to the dtype and lays them out."""

    def __init__(self, kind, d, dtype, seed, layout):
        self.kind, self.d, self.dtype = kind, d, dtype
        self.g = g = torch.Generator().manual_seed(seed)
        self.Mq = MQ[kind]
        self.Mqp = _r8(self.Mq)
        C = H * d
        self.setk = kind.startswith("sets")
        if self.setk:
            lens = layout
            src = SET_SRC[len(lens)] if kind.startswith("sets_src") else (0,) * len(lens)
            self.set_src = tuple(1 - s for s in src) if kind == "sets_src_b" else src
            self.sets, end = [], 0
            for n, w in zip(lens, SET_WEIGHTS[len(lens)]):
                self.sets.append((end, n, w))
                end = _r8(end + n)
            self.Mk, self.Mkp = None, end
        else:
            self.Mk = layout
            self.Mkp = _r8(layout) if kind == "bias" else layout
            self.sets, self.set_src = [(0, layout, 1.0)], (0,)
        self.q = torch.randn(B, self.Mqp, C, generator=g)
        self.q_src = torch.randn(B, self.Mqp, C, generator=g) if kind.startswith("sets_src") else None
        self.k = torch.randn(B, self.Mkp, C, generator=g)
        self.v = torch.randn(B, self.Mkp, C, generator=g)
        self.bias = (torch.rand(B, self.Mk, generator=g) * 2 - 1) if not self.setk else None
        self.w = torch.randn(B, self.Mk, generator=g) if kind == "words" else None
        self.mask = (torch.rand(B, len(self.sets), self.Mqp, generator=g) * 0.75 + 0.25) if kind == "sets_masked" else None
        self.dirs = {(b, head, op): _direction(g, d) for b in range(B) for head in range(H) for op in (0, 1)}
        self.rows = {b: [] for b in range(B)}
        self.masked = {b: [] for b in range(B)}
        self.k0 = self.bias0 = None
        self.meta = {}

    def operand(self, s):
        return self.q_src if self.set_src[s] else self.q

    def u(self, b, head, s):
        return self.dirs[(b, head, self.set_src[s])]

    def operands(self):
        return [(0, self.q)] + ([(1, self.q_src)] if self.q_src is not None else [])

    def plant_rows(self, rows_of, gain):
        """Row rows_of(b)[i] of every query operand becomes gain(i) * u."""
        for b in range(B):
            self.rows[b] = rows_of(b)
            for op, t in self.operands():
                for head in range(H):
                    for i, r in enumerate(self.rows[b]):
                        t[b, r, _slice(head, self.d)] = gain(i) * self.dirs[(b, head, op)]

    def orthogonal_keys(self, s):
        """The keys of set s lose their component along the direction of the operand the set reads."""
        start, n, _ = self.sets[s]
        for b in range(B):
            for head in range(H):
                sl = _slice(head, self.d)
                self.k[b, start:start + n, sl] = _project(self.k[b, start:start + n, sl], self.u(b, head, s))

    def snapshot(self):
        self.k0 = self.k.clone()
        self.bias0 = None if self.bias is None else self.bias.clone()

    def plant_key(self, s, j, c, zero_bias=False):
        """Key j of set s becomes c * u (c: a number, or a function of (b, head)); zero_bias: and its bias 0."""
        start = self.sets[s][0]
        for b in range(B):
            for head in range(H):
                cc = c(b, head) if callable(c) else c
                self.k[b, start + j, _slice(head, self.d)] = cc * self.u(b, head, s)
            if self.w is not None:
                self.w[b, j] = 1.5
            if zero_bias and self.bias is not None:
                self.bias[b, j] = 0.0

    def finish(self, name):
        c = Case()
        c.name, c.kind, c.d, c.dtype, c.Mq, c.Mk = name, self.kind, self.d, self.dtype, self.Mq, self.Mk
        rnd = lambda t: None if t is None else t.to(self.dtype)
        live = torch.zeros(self.Mkp, dtype=torch.bool)
        for start, n, _ in self.sets:
            live[start:start + n] = True

        def keys(t):
            t = t.clone()
            t[:, ~live] = PAD
            return t.to(self.dtype)

        c.q, c.q_src, c.k, c.v = rnd(self.q), rnd(self.q_src), keys(self.k), keys(self.v)
        c.sets, c.set_src = list(self.sets), self.set_src
        c.set_mask = list(range(len(self.sets))) if self.mask is not None else None
        c.mask, c.bias, c.w = self.mask, self.bias, self.w
        c.rows, c.masked, c.meta = dict(self.rows), dict(self.masked), dict(self.meta)
        c.unplanted = None
        if self.k0 is not None:
            c.unplanted = c.replace(k=keys(self.k0), bias=self.bias0, unplanted=None)
        return c


def _gain_base(d):
    """The planted rows' length factor: keeps the planted keys short, so that they stay ordinary keys for every other
    row at every head dim (c * log2(e) <= 1.5 log2 units of spread per 12 units of planted score)."""
    return max(1.0, 8.0 / math.sqrt(d))


def _tiles(n):
    return (n + TILE - 1) // TILE


def _late_spike(bd):
    d, G = bd.d, _gain_base(bd.d)
    bd.plant_rows(lambda b: _planted_rows(bd.Mq, b, False), lambda i: G * (1.0 + 0.1 * i))
    ns = len(bd.sets)
    targets = [(0, _tiles(bd.sets[0][1]) - 1)] if bd.setk else []
    targets.append((ns - 1, 1))
    for s in sorted({s for s, _ in targets}):
        bd.orthogonal_keys(s)
    bd.snapshot()
    for s, t in targets:                                   # 12 log2 units over the planted rows' maximum of 0
        width = min(TILE, bd.sets[s][1] - t * TILE)
        bd.plant_key(s, t * TILE + 3 % width, 12.0 / (G * _unit(d)))
    bd.meta["targets"] = targets


def _staircase(bd, rise, spread):
    d, G = bd.d, _gain_base(bd.d)
    nrows = (bd.Mq + WAVE - 1) // WAVE
    bd.plant_rows(lambda b: _planted_rows(bd.Mq, b, True), lambda i: G * (1.0 + spread * i / (nrows - 1)))
    for s in range(len(bd.sets)):
        bd.orthogonal_keys(s)
    if bd.bias is not None:                                # the steps are the planted keys' alone: every other bias <= 0
        bd.bias = -bd.bias.abs()
    bd.snapshot()
    for s, (_, n, _) in enumerate(bd.sets):                # tile t holds a key at `rise` * t: `rise` above tile t - 1's
        for t in range(0, _tiles(n)):
            width = min(TILE, n - t * TILE)
            bd.plant_key(s, t * TILE + 1 % width, rise * t / (G * _unit(d)), zero_bias=True)


def _first_key_dominant(bd):
    """Every query gets 1.5 u added, key 0 of every set is c * u and the set's other keys are orthogonal to u: key 0 leads
    every row by at least 175 log2 units, so that exp2 of every other score is 0 in fp32 and in both 16-bit types."""
    d = bd.d
    for op, t in bd.operands():
        for b in range(B):
            for head in range(H):
                t[b, :, _slice(head, d)] += 1.5 * bd.dirs[(b, head, op)]
    for s in range(len(bd.sets)):
        bd.orthogonal_keys(s)
    bd.snapshot()
    sl = d ** -0.5 * LOG2E

    def c_of(s):
        def c(b, head):
            qq = bd.operand(s)[b, :bd.Mq, _slice(head, d)].to(bd.dtype).double()
            along = float((qq @ bd.u(b, head, s).double()).min()) * sl      # > 0: 1.5 d against a N(0, d) part
            assert along > 0
            return 200.0 / along
        return c

    for s in range(len(bd.sets)):
        bd.plant_key(s, 0, c_of(s))
    for b in range(B):
        bd.rows[b] = list(range(bd.Mq))


def _all_very_negative(bd):
    """A block of queries becomes (its part orthogonal to u) - 2 u and every key gains c * u: -230 log2 units on every
    score of the block; for the other rows the term is a shift that is the same for every key.  (The same shift for
    every key of a row: the softmax is what it was, only harder to compute -- nothing is planted that could be removed.)"""
    d = bd.d
    for b in range(B):
        bd.rows[b] = _block_rows(bd.Mq, b)
        for op, t in bd.operands():
            for head in range(H):
                sl, u = _slice(head, d), bd.dirs[(b, head, op)]
                t[b, bd.rows[b], sl] = _project(t[b, bd.rows[b], sl], u) - 2.0 * u
    for s, (start, n, _) in enumerate(bd.sets):
        for b in range(B):
            for head in range(H):
                bd.k[b, start:start + n, _slice(head, d)] += 230.0 / (2.0 * _unit(d)) * bd.u(b, head, s)


def _wide_range(bd):
    bd.q *= 3.0
    bd.k *= 3.0
    if bd.q_src is not None:
        bd.q_src *= 3.0


def _bias_driven(bd):
    bd.snapshot()
    for b in range(B):
        j = TILE + 7 + 5 * b
        bd.bias[b, j] += 12.0
        if bd.w is not None:
            bd.w[b, j] = 1.5
        bd.rows[b] = list(range(bd.Mq))


def _masked_tiles(bd, variant):
    Mk, nt = bd.Mk, _tiles(bd.Mk)
    last0 = (nt - 1) * TILE
    per_sample = {"lead1": ("lead1", "lead2"), "lead2": ("lead2", "lead70"), "lead70": ("lead70", "lead1"),
                  "interior_inf": ("tile1", "tile1+" if nt == 3 else "tile2"),
                  "interior_1e4": ("tile1", "tile1+" if nt == 3 else "tile2"),
                  "last": ("last", "last+"), "single": ("single_end", "single_start")}[variant]
    keys = {"lead1": range(0, 64), "lead2": range(0, 128), "lead70": range(0, 70), "tile1": range(64, 128),
            "tile1+": list(range(64, 128)) + [3, Mk - 1], "tile2": range(128, 192), "last": range(last0, Mk),
            "last+": list(range(last0, Mk)) + [5], "single_end": [j for j in range(Mk) if j != Mk - 1],
            "single_start": [j for j in range(Mk) if j != last0]}
    lead = {"lead1": 1, "lead2": 2, "lead70": 1, "single_end": nt - 1, "single_start": nt - 1}
    bd.snapshot()
    value = -10000.0 if variant == "interior_1e4" else float("-inf")
    expect = []
    for b in range(B):
        what = per_sample[b]
        bd.masked[b] = sorted(keys[what])
        bd.k[b, bd.masked[b]] *= 4.0                    # unmasked they would dominate the rows they are aligned with
        bd.bias[b, bd.masked[b]] = value
        bd.rows[b] = list(range(bd.Mq))
        expect.append((lead.get(what, 0), 1 if what.startswith("tile") else 0, 1 if what.startswith("last") else 0))
    bd.meta["masked_expect"] = expect
    bd.meta["masked_below"] = -10000.0 if variant == "interior_1e4" else -np.inf
    if variant == "single":
        bd.meta["single"] = [Mk - 1, last0]


def _set_isolation(bd, height):
    """A block of queries is (its part orthogonal to u) + 2 u; set 0's keys are orthogonal to u but for one in its tile 1 at
    `height` log2 units; every key of set 1 loses c * u, -230 log2 units on every score of the block."""
    d = bd.d
    for b in range(B):
        bd.rows[b] = _block_rows(bd.Mq, b)
        for op, t in bd.operands():
            for head in range(H):
                sl, u = _slice(head, d), bd.dirs[(b, head, op)]
                t[b, bd.rows[b], sl] = _project(t[b, bd.rows[b], sl], u) + 2.0 * u
    bd.orthogonal_keys(0)
    bd.snapshot()
    bd.plant_key(0, TILE + 9, height / (2.0 * _unit(d)))
    start, n, _ = bd.sets[1]
    for b in range(B):
        for head in range(H):
            bd.k[b, start:start + n, _slice(head, d)] -= 230.0 / (2.0 * _unit(d)) * bd.u(b, head, 1)


@functools.lru_cache(maxsize=None)
def scenario(name, kind, d, dtype, layout, seed=0, height=40.0):
    """The operands of scenario ``name`` for one kernel kind, head dim, dtype and key layout (a tuple of set lengths for the
    set kinds, Mk for the others).  Cached: the tests share one build and must not write into it."""
    assert kind in kinds_of(name) and layout in layouts_of(kind), (name, kind, layout)
    seed = seed + 7919 * SCENARIOS.index(name) + 101 * d + 13 * (KINDS + ("sets_src_b",)).index(kind) \
        + (sum(layout) if isinstance(layout, tuple) else layout)
    bd = _Builder(kind, d, dtype, seed, layout)
    if name == "late_spike":
        _late_spike(bd)
    elif name == "staircase_over":
        _staircase(bd, 10.0, 0.3)
    elif name == "staircase_under":
        _staircase(bd, 6.8, 0.13)        # rises of 6.8 .. 7.7 per tile and row
    elif name == "first_key_dominant":
        _first_key_dominant(bd)
    elif name == "all_very_negative":
        _all_very_negative(bd)
    elif name == "wide_range":
        _wide_range(bd)
    elif name == "bias_driven":
        _bias_driven(bd)
    elif name == "set_isolation":
        _set_isolation(bd, height)
    else:
        _masked_tiles(bd, name.split(":")[1])
    return bd.finish(name)


# ---------------------------------------------------------------------------------------------------
# 3. float64 results of a case
# ---------------------------------------------------------------------------------------------------
def _cached(case, key, make):
    """Float64 views of a case are made once (Case.replace starts a fresh cache); nobody writes into them."""
    cache = case.__dict__.setdefault("_cache", {})
    if key not in cache:
        cache[key] = make()
    return cache[key]


def _head(case, name, b, head):
    """Operand ``name`` of (sample b, head) as float64 (rows, d)."""
    t = _cached(case, name, lambda: getattr(case, name).double().numpy())
    return t[b][:, _slice(head, case.d)]


def set_scores(case, b, head, s):
    """The (Mq, len_s) score matrix of set s of (sample b, head) in log2 units, from the 16-bit operands."""
    def make():
        start, n, _ = case.sets[s]
        S = _head(case, "q_src" if case.set_src[s] else "q", b, head)[:case.Mq] @ _head(case, "k", b, head)[start:start + n].T \
            * (case.d ** -0.5 * LOG2E)
        if case.bias is not None:
            S = S + case.bias[b, :n].double().numpy()[None, :] * LOG2E
        return S
    return _cached(case, ("S", b, head, s), make)


def dead_scores(case, b, s):
    """The scores of a dead lane's zero query: the bias alone."""
    n = case.sets[s][1]
    return np.zeros(n) if case.bias is None else case.bias[b, :n].double().numpy() * LOG2E


def case_census(case, b, head, s, **kw):
    wave, thr = machine(case.kind)
    return census(set_scores(case, b, head, s), wave=wave, thr=thr, dead=dead_scores(case, b, s), **kw)


def _result(case, engine):
    """The call's float64 result through ``engine(S_sets, V_sets, dead)``: (B, Mq, C) for the PV kinds, the head-averaged
    (B, Mq, Mk) map for probs, (B, Mq) for words."""
    d, Mq, ns = case.d, case.Mq, len(case.sets)
    if case.kind == "probs":
        out = np.zeros((B, Mq, case.Mk))
    elif case.kind == "words":
        out = np.zeros((B, Mq))
    else:
        out = np.zeros((B, Mq, H * d))
    for b in range(B):
        for head in range(H):
            S = [set_scores(case, b, head, s) for s in range(ns)]
            dead = [dead_scores(case, b, s) for s in range(ns)]
            if case.kind == "probs":
                (_, m, l), = engine(S, None, dead)
                with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                    out[b] += np.exp2(S[0] - m[:, None]) / l[:, None] / H
            elif case.kind == "words":
                (o, _, _), = engine(S, [case.w[b].double().numpy()[:, None]], dead)
                out[b] += o[:, 0] / H
            else:
                V = [_head(case, "v", b, head)[st:st + n] for st, n, _ in case.sets]
                for s, (o, _, _) in enumerate(engine(S, V, dead)):
                    f = case.sets[s][2]
                    if case.mask is not None and case.set_mask[s] >= 0:
                        f = f * case.mask[b, case.set_mask[s], :Mq].double().numpy()[:, None]
                    out[b][:, _slice(head, d)] += f * o
    return out


def reference(case):
    """The plain float64 expression on the same 16-bit operands."""
    return _result(case, lambda S, V, dead: plain_softmax64(S, V))


def replay(case, **switches):
    """The same through the kernel's state machine (online_softmax64 with the kernel's wave and threshold)."""
    wave, thr = machine(case.kind)
    return _result(case, lambda S, V, dead: online_softmax64(S, V, wave=wave, thr=thr, dead=dead, **switches))


def score_term(case):
    """What the fp32 rounding of large scores may add to a probability (absolute; the only widening the probs and word-map
    bounds get, and only where the census reports |score|max > 16 log2 units).  A score is fma(acc, c, bias') with acc the
    fp32 sum of d exact products: |acc - exact| <= (d - 1) u A', c = fl(scale * log2(e)) carries at most 3 u, the fma one
    more: |score error| <= (d + 3) u A, A = max sum_i |q_i k_i| scale log2(e) + |bias| log2(e) >= |score|max (equal for
    a planted key, whose products share one sign), over the keys whose bias is above -1000: a masked key's p is exactly 0.  The exponent's argument s - m carries the error of both and its own
    rounding, (2 (d + 3) + 2) u A; p = e_j / sum e takes that relative error times ln 2 in the numerator and again in the
    denominator, and p <= 1:  term = 4 ln 2 (d + 4) 2^-24 A."""
    d, A = case.d, 0.0
    for b in range(B):
        bias, open_ = 0.0, slice(None)
        if case.bias is not None:
            bb = case.bias[b].double().numpy()
            open_ = bb > -1000.0
            bias = float(np.abs(bb[open_]).max()) * LOG2E
        for head in range(H):
            for s, (start, n, _) in enumerate(case.sets):
                a = np.abs(_head(case, "q_src" if case.set_src[s] else "q", b, head)[:case.Mq]) \
                    @ np.abs(_head(case, "k", b, head)[start:start + n][open_]).T
                A = max(A, float(a.max()) * d ** -0.5 * LOG2E + bias)
    return 4.0 * math.log(2.0) * (d + 4) * U * A


def score_absmax(case):
    """|score|max over the keys that can hold probability (scores above -1000 log2 units)."""
    big = 0.0
    for b in range(B):
        for head in range(H):
            for s in range(len(case.sets)):
                S = set_scores(case, b, head, s)
                big = max(big, float(np.abs(S[S > -1000.0]).max()))
    return big


def bar(case, ref):
    """The absolute bound a kernel's result is held to: the existing bars -- TOL of max(1, |ref|max) for the sets and bias
    kernels, (Mk + 8) 2^-24 for the map, 2 (Mk + 8) 2^-24 max|w| for the word map -- and for the last two score_term where
    |score|max > 16."""
    if is_pv(case.kind):
        return TOL[case.dtype] * max(1.0, float(np.abs(ref).max()))
    term = score_term(case) if score_absmax(case) > 16.0 else 0.0
    if case.kind == "probs":
        return (case.Mk + 8) * U + term
    return (2 * (case.Mk + 8) * U + term) * float(case.w.abs().max())


def row_error(a, b_):
    """max |a - b| per (sample, query row); a non-finite difference counts as infinite."""
    diff = np.abs(a - b_).reshape(a.shape[0], a.shape[1], -1).max(-1)
    return np.where(np.isfinite(diff), diff, np.inf)
