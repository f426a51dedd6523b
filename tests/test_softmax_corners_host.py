"""Host tests of tests/softmax_corners.py (no GPU): the census on hand-written score matrices, the float64 state machine
against the plain softmax, and for every (scenario, kernel kind, d, dtype) of test_gpu_cross_softmax_corners.py the three
conditions that make the scenario worth a GPU run -- it reaches the branch it is named after, what it planted matters, and
the kernel mistake it is aimed at would move the result by more than ten times the bar.  These are conditions on the inputs,
not measurements: a scenario that misses one is rebuilt."""
import numpy as np
import pytest
import torch

import softmax_corners as SC

INF = float("inf")


# ---------------------------------------------------------------------------------------------------
# 1. the census
# ---------------------------------------------------------------------------------------------------
def test_census_deferred_rise_then_a_taken_rescale():
    """Tiles of 2 keys, one wave of 2 rows, threshold 8.  Tile 0 installs (1, 0) from nothing (not counted: no finite
    state); tile 1 rises by 4 in row 0, deferred; tile 2 rises 19 over the stale 1: taken with a finite state."""
    S = [[0, 1, 5, 2, 20, 0],
         [0, 0, 0, 0, 0, 0]]
    c = SC.census(S, tile=2, wave=2, thr=8.0)
    assert (c.rescales, c.rescale_tiles, c.rescale_waves, c.waves) == (1, [2], [0], 1)
    assert c.max_deferred == 4.0 and c.masked == (0, 0, 0) and c.score_absmax == 20.0 and c.min_row_max == 0.0


def test_census_the_threshold_is_inclusive_and_stale():
    """A rise of exactly 8 is deferred (mt <= m_run + 8); the next tile is measured against the stale maximum: 0 -> 8
    deferred, then 8 -> 9 is a rise of 9 over m_run = 0 and is taken."""
    c = SC.census([[0, 0, 8, 0, 9, 0, 9.5, 0]], tile=2, wave=1, thr=8.0)
    assert (c.rescales, c.rescale_tiles, c.max_deferred) == (1, [2], 8.0)


def test_census_masked_tiles_leading_interior_trailing():
    """One row, tiles of 2: two leading -inf tiles, a key, an interior -inf tile, two keys, a trailing -inf tile.  The first
    finite tile installs from -inf (not counted), the interior tile leaves the state alone, 3 -> 4 is deferred."""
    S = [[-INF, -INF, -INF, -INF, 3, -INF, -INF, -INF, 4, 1, -INF, -INF]]
    c = SC.census(S, tile=2, wave=1, thr=8.0)
    assert c.masked == (2, 1, 1) and c.rescales == 0 and c.max_deferred == 1.0
    assert c.score_absmax == 4.0 and c.min_row_max == 4.0
    c = SC.census([[-20000, -20000, 0, 1]], tile=2, wave=1, masked_below=-10000.0)
    assert c.masked == (1, 0, 0) and c.rescales == 1          # a finite -20000 IS a state: the next tile rescales it away


def test_census_a_wave_follows_any_of_its_rows_and_its_dead_lanes():
    """Two waves of 2 rows: only row 3 jumps, wave 1 takes the branch, wave 0 does not.  A partial last wave is filled with
    dead lanes whose scores are `dead`: they vote in the wave's test but hold no state."""
    S = [[0, 0, 1, 0], [0, 0, 2, 0], [0, 0, 3, 0], [0, 0, 30, 0]]
    c = SC.census(S, tile=2, wave=2, thr=8.0)
    assert (c.rescales, c.rescale_tiles, c.rescale_waves, c.waves, c.max_deferred) == (1, [1], [1], 2, 2.0)
    c = SC.census([[0, 0, 1, 1]], tile=2, wave=2, thr=8.0, dead=[0, 0, 100, 100])
    assert (c.rescales, c.rescale_waves, c.max_deferred) == (1, [0], 0.0)
    c = SC.census([[0, 0, 1, 1]], tile=2, wave=2, thr=8.0)
    assert (c.rescales, c.max_deferred) == (0, 1.0)


def test_census_per_row_machine_of_the_map_kernels():
    """wave = 1, thr = 0: every rise of a row's maximum is a rescale."""
    c = SC.census([[1, 2, 3, 0, 2, 2], [5, 0, 1, 1, 1, 1]], tile=2, wave=1, thr=0.0)
    assert (c.rescales, c.rescale_tiles, c.rescale_waves, c.waves, c.max_deferred) == (1, [1], [0], 2, 0.0)


# ---------------------------------------------------------------------------------------------------
# 2. the float64 state machine
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wave,thr", [(32, 8.0), (1, 0.0)])
def test_online_softmax64_is_the_plain_softmax(wave, thr):
    """Two sets (five tiles and a ragged second one), scores spread over +-60 log2 units with -inf tiles in one of them: the
    tile-wise machine with no switch on equals the plain float64 softmax to 1e-12, stats and all."""
    g = np.random.default_rng(5)
    S = [g.normal(size=(70, 257)) * 20, g.normal(size=(70, 77)) * 3]
    S[0][:, :128] = -INF
    S[0][:, 192:256] = -INF
    V = [g.normal(size=(257, 7)), g.normal(size=(77, 7))]
    got = SC.online_softmax64(S, V, wave=wave, thr=thr)
    want = SC.plain_softmax64(S, V)
    for (o, m, l), (o0, m0, l0) in zip(got, want):
        assert np.abs(o - o0).max() <= 1e-12
        assert np.abs(np.log2(l) + m - (np.log2(l0) + m0)).max() <= 1e-12     # the stats agree up to the common shift
    # and each switch is a different function on these scores
    for sw in ("drop_alpha", "no_set_reset", "exp_against_zero"):
        moved = SC.online_softmax64(S, V, wave=wave, thr=thr, **{sw: True})
        with np.errstate(invalid="ignore"):
            diff = max(np.nan_to_num(np.abs(a[0] - b[0]), nan=INF).max() for a, b in zip(moved, want))
        assert diff > 1e-3, sw


# ---------------------------------------------------------------------------------------------------
# 3. the scenarios of the GPU tests
# ---------------------------------------------------------------------------------------------------
def _censuses(case, **kw):
    return {(b, head, s): SC.case_census(case, b, head, s, **kw)
            for b in range(SC.B) for head in range(SC.H) for s in range(len(case.sets))}


def _rises(case, b, head, s, row):
    """The rise of `row`'s tile maximum over its true running maximum, per tile >= 1 of set s."""
    S = SC.set_scores(case, b, head, s)[row]
    return [float(S[t0:t0 + SC.TILE].max() - S[:t0].max()) for t0 in range(SC.TILE, len(S), SC.TILE)]


def _precondition(case):
    name, pv, cen = case.name, SC.is_pv(case.kind), _censuses(case)
    ns = len(case.sets)
    if name == "late_spike":
        targets = dict(case.meta["targets"])                 # set -> tile
        assert len(targets) == (2 if case.kind.startswith("sets") else 1)
        for (b, head, s), c in cen.items():
            if s not in targets:
                continue
            t = targets[s]
            assert t >= 1 and t in c.rescale_tiles, ("no finite-state rescale at the target tile", b, head, s, c)
            assert len(c.rescale_waves) < c.waves, ("every wave rescales", b, head, s)
            for row in case.rows[b]:
                assert _rises(case, b, head, s, row)[t - 1] > 8.0, (b, head, s, row)
            if pv:                                           # the planted waves, and only a few others
                assert {r // SC.WAVE for r in case.rows[b]} <= set(c.rescale_waves)
    elif name in ("staircase_over", "staircase_under"):
        for (b, head, s), c in cen.items():
            nt = SC._tiles(case.sets[s][1])
            if nt < 2:
                continue
            rises = [r for row in case.rows[b] for r in _rises(case, b, head, s, row)]
            if name == "staircase_over":
                assert min(rises) > 8.0, (b, head, s, min(rises))
                assert c.rescale_tiles == list(range(1, nt)), (b, head, s, c.rescale_tiles)
                assert not pv or len(c.rescale_waves) == c.waves
            else:
                assert 6.0 <= min(rises) and max(rises) <= 7.9, (b, head, s, min(rises), max(rises))
                if pv:
                    assert 7.0 <= c.max_deferred <= 8.0, (b, head, s, c.max_deferred)
                    assert nt < 3 or c.rescales >= 1, (b, head, s)
    elif name == "first_key_dominant":
        for b in range(SC.B):
            for head in range(SC.H):
                for s in range(ns):
                    S = SC.set_scores(case, b, head, s)
                    assert float((S[:, 0] - S[:, 1:].max(1)).min()) >= 160.0, (b, head, s)
    elif name == "all_very_negative":
        for (b, head, s), c in cen.items():
            assert float(SC.set_scores(case, b, head, s)[case.rows[b]].max()) <= -100.0, (b, head, s)
            assert c.min_row_max <= -100.0
    elif name == "wide_range":
        assert all(c.score_absmax > 16.0 for c in cen.values())
        for b in range(SC.B):                                # (a set of one or two tiles may have none)
            for head in range(SC.H):
                assert sum(cen[(b, head, s)].rescales for s in range(ns)) >= 1, (b, head)
    elif name == "bias_driven":
        for (b, head, s), c in cen.items():
            assert 1 in c.rescale_tiles and (not pv or len(c.rescale_waves) == c.waves), (b, head, c)
            qk = case.replace(bias=None)
            assert SC.case_census(qk, b, head, s).score_absmax < 12.0, "the q . k scores are not random"
    elif name == "set_isolation":
        for b in range(SC.B):
            for head in range(SC.H):
                S0, S1 = (SC.set_scores(case, b, head, s)[case.rows[b]] for s in (0, 1))
                assert float(S0.max(1).min()) >= float(S1.max()) + 40.0 and float(S1.max()) <= -100.0, (b, head)
                assert 1 in cen[(b, head, 0)].rescale_tiles
    else:
        cen = _censuses(case, masked_below=case.meta["masked_below"])
        for (b, head, s), c in cen.items():
            assert c.masked == case.meta["masked_expect"][b], (b, head, c.masked, case.meta["masked_expect"][b])
        assert case.masked[0] != case.masked[1]


def _switch_of(name):
    if name in SC.DROP_ALPHA:
        return "drop_alpha"
    return {"set_isolation": "no_set_reset", "all_very_negative": "exp_against_zero"}.get(name)


@pytest.mark.parametrize("case", SC.gpu_cases(), ids=SC.case_id)
def test_scenario_preconditions(case):
    name, kind, d, dtype = case
    for layout in SC.layouts_of(kind):
        c = SC.scenario(name, kind, d, dtype, layout)
        ref = SC.reference(c)
        assert np.isfinite(ref).all()
        bar = SC.bar(c, ref)
        # the replayed state machine is the reference (the scenario does not break the restatement itself)
        assert float(SC.row_error(SC.replay(c), ref).max()) <= 1e-9 * max(1.0, float(np.abs(ref).max()))
        # 1. the branch is reached
        _precondition(c)
        # 2. what was planted matters: on every planted row where rows were planted, and in every sample where keys were
        # masked (the leak > 10 * TOL pattern of test_gpu_masked_cross.py).  wide_range and all_very_negative scale or shift
        # every key of a row alike: nothing is planted.
        if c.unplanted is not None:
            leak = SC.row_error(SC.reference(c.unplanted), ref)
            if name.startswith("masked_tiles"):
                worst = min(float(leak[b].max()) for b in range(SC.B))
            else:
                worst = min(float(leak[b, r]) for b in range(SC.B) for r in c.rows[b])
            assert worst > 10 * bar, (layout, "what was planted would not be noticed", worst, bar)
        else:
            assert name in ("wide_range", "all_very_negative")
        # 3. the mistake the scenario is aimed at moves the result
        sw = _switch_of(name)
        if sw is not None:
            moved = float(SC.row_error(SC.replay(c, **{sw: True}), ref).max())
            assert moved > 10 * bar, (layout, sw, moved, bar)
