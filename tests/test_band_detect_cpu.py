"""CPU: the column-band plan of a window-parallel day that keeps `Out_2` distributed (`apply.window_band_plan`, merge="columns") and
the C ABI of the band candidate kernel (genie_band_peaks_count / _fill: declared in the header, bound in `_lib.SYMBOLS`).

The plan is host arithmetic on the `window_cols_table` of all windows: 1 to 7 ranks, ranks without windows (n < world), the three step
sizes and a caller-supplied `times`.
"""
import os
import re

import numpy as np
import pytest

from genie_amd import _lib, apply

HEADER = os.path.join(_lib.REPO, "include", "genie_hip.h")
BAND_SYMBOLS = ("genie_band_peaks_count", "genie_band_peaks_fill")


def _table(step_size, n_windows=None, times=None, seed=3):
    """(cols table of all windows, n_cols) of a default-schedule day (or of the caller's `times` on that day's axis)."""
    rng = np.random.default_rng(seed)
    picks = np.sort(rng.uniform(1000.0, 1400.0, 400))
    tsteps, offsets, step, n_overlap, dt_win = apply.window_schedule(picks, 20.0, t_win=6.0, step_size=step_size)
    tsteps_abs = np.arange(tsteps.min() - 3.0, tsteps.max() + 3.0 + dt_win, dt_win)
    if times is None:
        times = tsteps if n_windows is None else tsteps[:n_windows]
    return apply.window_cols_table(tsteps_abs, times, offsets, step_size == "half"), len(tsteps_abs), tsteps_abs, np.asarray(times)


CASES = [("full", None, None), ("half", None, None), ("partial", None, None), ("half", 3, None), ("full", 1, None), ("partial", 0, None),
         ("half", None, 1003.7 + 1.0 * np.arange(60)),                 # a caller's 1 s stride: several ranks' first windows share a column
         ("half", None, np.array([1010.0, 1010.2, 1010.4, 1200.0]))]   # near-coincident windows and a long gap


@pytest.mark.parametrize("world", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("step_size,n_windows,times", CASES)
def test_band_plan_partitions_and_lists_every_strip(step_size, n_windows, times, world):
    cols, n_cols, tsteps_abs, times = _table(step_size, n_windows, times)
    margin = 1 + world % 2
    plan = apply.window_band_plan(cols, n_cols, world, margin=margin, n_rows=10, tsteps_abs=tsteps_abs, times=times)
    info = apply.window_parallel_info(cols, n_cols, world)
    assert plan["windows"] == info["windows"] and plan["world"] == world and plan["n_cols"] == n_cols
    own, band = plan["own"], plan["band"]
    # the own ranges partition [0, n_cols), in rank order
    assert own[0][0] == 0 and own[-1][1] == n_cols
    assert all(lo <= hi for lo, hi in own) and all(own[r][1] == own[r + 1][0] for r in range(world - 1))
    nonempty = [r for r, (lo, hi) in enumerate(plan["windows"]) if hi > lo]
    for r in range(world):
        lo, hi = plan["windows"][r]
        if hi > lo:
            first = cols[lo][cols[lo] >= 0].min()
            if r > 0:
                assert own[r][0] == first                          # the cut: the first column of the rank's first window
            assert plan["fed"][r] == info["columns"][r]
        elif nonempty or r > 0:
            assert own[r][0] == own[r][1]                          # a rank without windows owns nothing
    if nonempty:
        assert own[nonempty[-1]][1] == n_cols
    for r in range(world):
        # the band holds own +- margin, clipped, and every column the rank feeds
        assert band[r][0] <= max(own[r][0] - margin, 0) and band[r][1] >= min(own[r][1] + margin, n_cols)
        assert 0 <= band[r][0] <= band[r][1] <= n_cols
        lo, hi = plan["windows"][r]
        fed = np.unique(cols[lo:hi])
        fed = fed[fed >= 0]
        assert all(band[r][0] <= c < band[r][1] for c in fed)
        # every column the rank feeds outside its own range: exactly one strip of its `send` list goes to the column's OWNER and
        # holds it, and that strip is in the owner's `recv` list (bands overlap by the margin, so a third rank may get the column too)
        for c in fed:
            if own[r][0] <= c < own[r][1]:
                continue
            owner = [q for q in range(world) if own[q][0] <= c < own[q][1]]
            assert len(owner) == 1 and owner[0] != r
            hits = [(q, a, b) for q, a, b in plan["send"][r] if q == owner[0] and a <= c < b]
            assert len(hits) == 1
            assert (r, hits[0][1], hits[0][2]) in plan["recv"][owner[0]]
        # and the other way round: the two lists describe the same strips, inside both bands, and `recv` covers every foreign
        # column of the band
        for p, a, b in plan["recv"][r]:
            assert (r, a, b) in plan["send"][p] and band[r][0] <= a < b <= band[r][1] and band[p][0] <= a and b <= band[p][1]
        covered = np.zeros(n_cols, dtype=bool)
        for p, a, b in plan["recv"][r]:
            covered[a:b] = True
        for p in range(world):
            lo, hi = plan["windows"][p]
            if p != r:
                f = np.unique(cols[lo:hi])
                f = f[(f >= band[r][0]) & (f < band[r][1])]
                assert covered[f].all()
        assert [p for p, _, _ in plan["recv"][r]] == sorted({p for p, _, _ in plan["recv"][r]})
        assert plan["band_bytes"][r] == 40 * (band[r][1] - band[r][0]) and plan["dense_bytes"][r] == 40 * n_cols
        assert plan["strip_bytes"][r] == 40 * sum(b - a for _, a, b in plan["recv"][r])
    assert sum(len(s) for s in plan["send"]) == sum(len(s) for s in plan["recv"])


def test_band_plan_is_smaller_than_the_dense_merge_on_a_long_day():
    cols, n_cols, _, _ = _table("half")
    plan = apply.window_band_plan(cols, n_cols, 4)
    assert sum(plan["band_bytes"]) < 1.2 * plan["dense_bytes"][0]           # the bands tile the axis with a small overlap
    assert max(plan["strip_bytes"]) < 0.2 * plan["dense_bytes"][0]


def test_band_plan_needs_an_ascending_axis():
    cols, n_cols, tsteps_abs, times = _table("half")
    with pytest.raises(ValueError, match='merge="dense"'):                  # a descending output axis: the columns descend
        apply.window_band_plan(apply.window_cols_table(tsteps_abs[::-1], times, apply.window_schedule([0.0, 100.0], 10.0)[1], True), n_cols, 3)
    with pytest.raises(ValueError, match='merge="dense"'):
        apply.window_band_plan(cols, n_cols, 3, tsteps_abs=tsteps_abs[::-1])
    with pytest.raises(ValueError, match='merge="dense"'):                  # window times that do not ascend
        apply.window_band_plan(cols[::-1], n_cols, 3)
    with pytest.raises(ValueError, match='merge="dense"'):
        apply.window_band_plan(cols, n_cols, 3, times=times[::-1])
    with pytest.raises(ValueError, match="margin"):
        apply.window_band_plan(cols, n_cols, 3, margin=0)


def test_day_plan_refuses_columns_without_ranks_or_order():
    t = np.sort(np.random.default_rng(5).uniform(1000.0, 1100.0, 200))
    args = (t, 20.0, 86400.0, 6.0, "half", 1)
    split = apply._RankSplit(1, 3, None, False)
    with pytest.raises(ValueError, match="window_parallel"):
        apply._day_plan(*args, None, None, 1.0, 1.0, None, False, "columns")
    with pytest.raises(ValueError, match="merge must be"):
        apply._day_plan(*args, None, None, 1.0, 1.0, split, False, "rows")
    plan = apply._day_plan(*args, None, None, 1.0, 1.0, split, False, "columns")
    b_lo, b_hi = plan.bands["band"][1]
    assert plan.width == b_hi - b_lo and 0 < plan.width < len(plan.tsteps_abs)
    valid = plan.h_cols[plan.h_cols >= 0]
    assert valid.min() >= 0 and valid.max() < plan.width                    # the table counts from the band's first column
    dense = apply._day_plan(*args, None, None, 1.0, 1.0, split, False)
    assert dense.bands is None and dense.width == len(dense.tsteps_abs)
    assert np.array_equal(np.where(plan.h_cols >= 0, plan.h_cols + b_lo, -1), dense.h_cols)
    with pytest.raises(ValueError, match='merge="dense"'):
        apply._day_plan(*args, plan.tsteps_abs[::-1].copy(), None, 1.0, 1.0, split, False, "columns")


def test_band_peaks_abi_is_declared_and_bound():
    text = open(HEADER).read()
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    for name in BAND_SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name + " is not declared in include/genie_hip.h"
        assert name in bound, name + " is not in _lib.SYMBOLS"
        assert len(bound[name]) == len(m.group(1).split(",")), name + ": the binding and the declaration differ in their argument count"
    declared = set(re.findall(r"\b(genie_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(bound)                                           # the header and the binding name the same entry points
