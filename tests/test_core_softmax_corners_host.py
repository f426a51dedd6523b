"""Host tests of tests/core_softmax_corners.py (no GPU), for a nominal 256-CU device: the float64 models against the plain
softmax, and for every (family configuration, plan, dtype) of test_gpu_core_softmax_corners.py the three conditions that make
its launch worth a GPU run -- every scenario reaches the branch it is named after in the row groups it was planted in (and
not in the control group next to them), what it planted matters, and the kernel mistake it is aimed at -- alpha dropped in a
rescale, records combined as if their maxima were equal, a shift that stays stale for a tile after a raise -- moves its
planted rows by more than ten times the bar.  These are conditions on the inputs, not measurements: a scenario that misses
one is rebuilt.  The census and the models run on the planted row groups and one control group per block, not on whole
score matrices."""
import numpy as np
import pytest
import torch

import core_softmax_corners as CSC
import softmax_corners as SC

N_CUS = 256
INF = float("inf")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the models
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,tile", [(32, 64), (16, 32)])
def test_split_softmax64_is_the_plain_softmax(width, tile):
    """Scores spread over +-60 log2 units, 70 rows (a partial last group), 1000 keys whole and cut 2, 4 and 5 ways: per
    piece online_softmax64, folded by combine64, equals the plain float64 softmax to 1e-12; each switch does not."""
    g = np.random.default_rng(7)
    S, V = g.normal(size=(70, 1000)) * 20, g.normal(size=(1000, 5))
    S[:, 640:] += np.arange(360) * 0.5                       # the maximum climbs over the later pieces
    want = SC.plain_softmax64([S], [V])[0][0]
    dead = np.zeros(1000)
    for ns in (1, 2, 4, 5):
        pcs = CSC.P.pieces(1000, ns, tile)
        got, maxima = CSC.split_softmax64(S, V, pcs, width, tile, dead)
        assert len(maxima) == len(pcs) and np.abs(got - want).max() <= 1e-12, ns
        for sw in ("drop_alpha", "stale_shift") + (("combine_equal_maxima",) if ns > 1 else ()):
            moved, _ = CSC.split_softmax64(S, V, pcs, width, tile, dead, **{sw: True})
            assert np.nan_to_num(np.abs(moved - want), nan=INF).max() > 1e-3, (ns, sw)


def test_combine64_weights_the_records():
    """Two records of one row, maxima 0 and 12: the first one's weight is 2^-12; added as they are it is 1."""
    recs = [(np.array([[1.0]]), np.array([0.0]), np.array([1.0])), (np.array([[3.0]]), np.array([12.0]), np.array([1.0]))]
    w = 2.0 ** -12
    assert abs(CSC.combine64(recs)[0, 0] - (w + 3.0) / (w + 1.0)) < 1e-15
    assert CSC.combine64(recs, equal_maxima=True)[0, 0] == 2.0


def test_the_cases_cover_every_family_plan_and_dtype():
    cases = CSC.gpu_cases()
    assert len(cases) == len(set(cases)) == 92
    assert {CSC.CONFIG[c[0]].kind for c in cases} == {"k", "16s", "16g", "f32"}
    assert {c[1] for c in cases} == {"single", "tail", "device", "split_all"}
    assert all(CSC.SENSITIVITY_PLAN in c.plans for c in CSC.CONFIGS)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the launches of the GPU module
# ---------------------------------------------------------------------------------------------------------------------
def _local(t, pcs, tile):
    """Global key tile t -> (piece index, tile index inside the piece)."""
    for i, (lo, hi) in enumerate(pcs):
        if lo <= t * tile < hi:
            return i, t - lo // tile
    raise AssertionError(t)


def _census(L, S, pcs, piece, dead, wave=None):
    lo, hi = pcs[piece]
    return SC.census(S[:, lo:hi], tile=L.tile, wave=L.width if wave is None else wave, thr=CSC.THR, dead=dead[lo:hi])


def _check_slot_block(L, s, blk, bar, seen):
    """The three conditions for slot s in one of its blocks, for every item (output sample) the block has there."""
    name, width, tile = s.name, L.width, L.tile
    control = [g for g in (0,) if g not in blk.groups]
    groups = control + sorted(blk.groups)
    rows = CSC.group_rows(L, blk, groups)
    at = {r: i for i, r in enumerate(rows)}
    planted = [at[r] for g in blk.groups for r in blk.groups[g] if r in at]
    gidx = {g: i for i, g in enumerate(groups)}              # group -> wave index in the census of `rows`
    S = L.scores(s, rows)
    dead = L.bias[s.b][:s.mk]
    tag = (name, "slot", (s.b, s.head), "block", blk.qb)
    for gb, pcs in blk.items:
        split = len(pcs) > 1
        V = L.values(gb, s)
        ref = SC.plain_softmax64([S], [V])[0][0]
        got, maxima = CSC.split_softmax64(S, V, pcs, width, tile, dead)
        assert np.abs(got - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), tag
        pm = np.stack(maxima)[:, planted]                    # piece maxima of the planted rows
        # -- 1. the branch is reached
        if name in ("late_spike", CSC.FOLD_SCENARIO):
            targets = s.tiles[:-1] if name == "late_spike" else [L.fold_key // tile]   # (the last tile: the companion key)
            hit = 0
            for t in targets:
                piece, lt = _local(t, pcs, tile)
                if lt == 0:                                  # a piece's first tile installs from -inf: no finite state
                    continue
                c = _census(L, S, pcs, piece, dead)
                assert lt in c.rescale_tiles, ("no finite-state rescale at the target tile", tag, t, c)
                hit += 1
            assert hit >= (3 if name == "late_spike" else 1) or (split and hit >= 1), tag
            # which groups rescale a finite state anywhere: the planted ones, not the control
            waves = set()
            for piece in range(len(pcs)):
                waves |= set(_census(L, S, pcs, piece, dead).rescale_waves)
            assert {gidx[g] for g in blk.groups} <= waves, tag
            # (a multiplicity is its key's for every row of the sample: the control group sees the same + 12)
            folded_sample = L.fold_key is not None and s.b == 0
            assert not control or folded_sample or gidx[0] not in waves, ("the control group rescales too", tag)
            if L.cfg.kind == "16s" and name == "late_spike" and not blk.special and {2, 7, 10, 11} <= set(blk.groups):
                # wave 1: sub-tile A (group 2) alone; wave 3: B (group 7) alone; wave 5: both -- groups 3 and 6 are not
                # among the planted ones, so the census above never saw them: count them here
                pair = CSC.group_rows(L, blk, [3, 6])
                Sp = L.scores(s, pair)
                if L.fold_key is not None and s.b == 0:          # (the folded key's + 12 is every row's of sample 0)
                    Sp[:, L.fold_key] -= L.bias[0][L.fold_key]
                quiet = set()
                for piece in range(len(pcs)):
                    quiet |= set(_census(L, Sp, pcs, piece, dead).rescale_waves)
                assert not quiet, ("the other sub-tile of an A-only / B-only wave rescales", tag, quiet)
                seen.add("16s_sub_tiles")
            if name == CSC.FOLD_SCENARIO:
                raw = L.scores(s, [rows[i] for i in planted], bias=np.zeros_like(L.bias[s.b]))
                assert np.abs(raw).max() < 3.0, ("the raw scores are not ordinary", tag)
            if split and name == "late_spike":
                top = np.sort(pm, axis=0)
                assert float((top[-1] - top[-2]).min()) > 8.0, ("piece maxima", tag)
        elif name.startswith("staircase"):
            Sp = S[planted]
            nt = CSC.P.cdiv(s.mk, tile)
            tmax = np.stack([Sp[:, t * tile:(t + 1) * tile].max(1) for t in range(nt)])
            rises = np.diff(tmax, axis=0)
            if name == "staircase_over":
                assert float(rises.min()) > 8.0, (tag, float(rises.min()))
                for piece, (lo, hi) in enumerate(pcs):
                    c = _census(L, Sp, pcs, piece, dead, wave=1)
                    assert c.rescale_tiles == list(range(1, CSC.P.cdiv(hi - lo, tile))), (tag, piece, c.rescale_tiles)
                    assert len(c.rescale_waves) == c.waves or hi - lo <= tile
                if split:
                    assert float(np.diff(pm, axis=0).min()) >= 10.0, ("piece maxima", tag)
            else:
                assert 6.0 <= float(rises.min()) and float(rises.max()) <= 7.9, (tag, float(rises.min()), float(rises.max()))
                c = _census(L, Sp, pcs, 0, dead, wave=1)
                assert 6.0 <= c.max_deferred <= 8.0 and c.rescales >= 1, (tag, c)
        elif name in CSC.ONE_KEY:
            lead = S[:, s.one_key] - np.delete(S, s.one_key, axis=1).max(1)
            assert float(lead.min()) >= 150.0, (tag, float(lead.min()))
            if split:
                home = next(i for i, (lo, hi) in enumerate(pcs) if lo <= s.one_key < hi)
                others = np.delete(np.stack(maxima), home, axis=0)
                gap = np.stack(maxima)[home][None, :] - others
                assert float(gap.min()) >= 150.0, ("piece maxima", tag)
                assert not np.exp2(-gap.astype(np.float32)).any(), "the other pieces' weights are not 0 in fp32"
        elif name == "all_very_negative":
            assert float(S[planted].max()) <= -100.0, tag
        elif name == "wide_range":
            c = [_census(L, S, pcs, piece, dead) for piece in range(len(pcs))]
            assert max(x.score_absmax for x in c) > 16.0 and sum(x.rescales for x in c) >= 1, tag
        # -- 2. what was planted matters
        if s.k0 is not None or s.bias0 is not None:
            prows = [rows[i] for i in planted]
            leak = np.abs(L.reference(gb, s, prows, unplanted=True) - ref[planted]).max(1)
            assert float(leak.min()) > 10 * bar, ("what was planted would not be noticed", tag, float(leak.min()), bar)
        else:
            assert name in ("wide_range", "all_very_negative", CSC.CONTROL)
        # -- 3. the mistakes the scenario is aimed at move its planted rows
        switches = []
        if name in CSC.DROP_ALPHA:
            switches.append("drop_alpha")
        if split and name in CSC.EQUAL_MAXIMA:
            switches.append("combine_equal_maxima")
        if L.d % 16 != 0 and L.dtype != torch.float32 and name in CSC.STALE_SHIFT:
            switches.append("stale_shift")
        for sw in switches:
            moved, _ = CSC.split_softmax64(S, V, pcs, width, tile, dead, **{sw: True})
            diff = np.nan_to_num(np.abs(moved - ref)[planted], nan=INF).max()
            assert diff > 10 * bar, (sw, "would not be noticed", tag, diff, bar)
            seen.add((name, sw))
        if split:
            seen.add((name, "split"))


@pytest.mark.parametrize("case", CSC.gpu_cases(), ids=CSC.case_id)
def test_launch_preconditions(case):
    L = CSC.build(*case, N_CUS)
    cfg, sel = L.cfg, L.sel
    bar = L.bar_upper()
    names = [s.name for s in L.slots.values()]
    assert set(names) == set(CSC.scenarios_of(cfg)) | {CSC.CONTROL}, "a scenario has no slot"
    seen = set()
    tiers_planted = set()
    for s in L.slots.values():
        assert s.rows and all(r < L.cnt[s.b] for r in s.rows)
        for blk in s.blocks:
            if s.name != CSC.CONTROL:
                _check_slot_block(L, s, blk, bar, seen)
            tiers_planted |= {len(pcs) for _, pcs in blk.items}
    # placement: a whole item, every split tier of the plan, row count - 1, the partial last wave
    tiers = {ns for lin, ns, _ in sel.split if sel.live(lin)}
    pieces_of = lambda ns: len(CSC.P.pieces(min(L.kc), ns, L.tile))
    assert {pieces_of(ns) for ns in tiers} <= tiers_planted, (tiers, tiers_planted)
    assert 1 in tiers_planted or sel.plan == "split_all"
    for s in L.slots.values():
        assert L.cnt[s.b] - 1 in s.rows
        if L.Mq % L.width and L.cnt[s.b] > L.Mq // L.width * L.width:
            assert any(r >= L.Mq // L.width * L.width for r in s.rows), "no row in the partial last wave"
    # what the case proves about the three mistakes
    for name in CSC.DROP_ALPHA:
        if name in names:
            assert (name, "drop_alpha") in seen, name
    if tiers:
        met = [n for n in CSC.EQUAL_MAXIMA if (n, "combine_equal_maxima") in seen]
        assert met, "no scenario of this launch meets the combine kernel on unequal records"
        split_slots = {(s.b, s.head) for s in L.slots.values() if any(len(p) > 1 for blk in s.blocks for _, p in blk.items)}
        if len(split_slots) >= len(CSC.EQUAL_MAXIMA):
            assert met == list(CSC.EQUAL_MAXIMA), met
    if L.d % 16 != 0 and L.dtype != torch.float32:
        assert all((n, "stale_shift") in seen for n in CSC.STALE_SHIFT)
    if cfg.kind == "16s":
        assert "16s_sub_tiles" in seen, "no block shows the A-only / B-only / both waves"


def test_every_combine_scenario_meets_every_combine_kernel_under_the_host_tail():
    """The host tail's split items all belong to the last (sample, head) pair, which carries one scenario per case: over
    the tail cases, the rotation gives each combine kernel (parts, plain, 16, f32) several of the four scenarios."""
    met = {}
    for case in CSC.gpu_cases():
        if case[1] != "tail":
            continue
        L = CSC.build(*case, N_CUS)
        for s in L.slots.values():
            if any(len(p) > 1 for blk in s.blocks for _, p in blk.items):
                met.setdefault(L.sel.combine, set()).add(s.name)
    assert set(met) == {"parts", "plain", "16", "f32"}
    for combine, names in met.items():
        assert len(names & set(CSC.EQUAL_MAXIMA)) >= 2, (combine, names)
