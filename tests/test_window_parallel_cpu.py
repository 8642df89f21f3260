"""CPU: the host side of the window-parallel apply loop and of the fused stacking (genie_amd/apply.py): the split of a day's windows
into contiguous blocks, the `exact_merge` flag against a dense count of ranks per column, the `cols` table of `genie_stack_windows`
against the reference's stacking statement, and the C ABI of the new entry point."""
import os
import re

import numpy as np
import pytest

from genie_amd import _lib, apply


@pytest.mark.parametrize("world", [1, 2, 3, 8, 16])
def test_window_blocks_are_contiguous_balanced_and_cover(world):
    for n in range(41):
        blocks = apply.window_blocks(n, world)
        assert len(blocks) == world
        assert blocks[0][0] == 0 and blocks[-1][1] == n
        assert all(b[1] == nb[0] for b, nb in zip(blocks, blocks[1:]))          # contiguous and disjoint: each starts where the last ended
        lens = [hi - lo for lo, hi in blocks]
        assert min(lens) >= 0 and max(lens) - min(lens) <= 1
        assert np.array_equal(np.concatenate([np.arange(lo, hi) for lo, hi in blocks]), np.arange(n))
        assert (0 in lens) == (n < world)


def _dense_ranks_per_column(table, n_cols, world):
    """[world, n_cols] booleans, the slow way: rank r touches column c when any window of its block lists c."""
    touched = np.zeros((world, n_cols), dtype=bool)
    for r, (lo, hi) in enumerate(apply.window_blocks(table.shape[0], world)):
        for w in range(lo, hi):
            for c in table[w]:
                if c >= 0:
                    touched[r, c] = True
    return touched


def _schedules():
    rng = np.random.default_rng(5)
    picks = np.sort(rng.uniform(5000.0, 5400.0, 500))
    tsteps, offsets, step, n_overlap, dt_win = apply.window_schedule(picks, 40.0, step_size="half")
    tsteps_abs = np.arange(tsteps.min() - 3.0, tsteps.max() + 3.0 + dt_win, dt_win)
    stride = tsteps.min() + 0.3 + 1.0 * np.arange(120)
    shuffled = tsteps_abs[np.random.default_rng(6).permutation(len(tsteps_abs))]
    return {"half": (tsteps_abs, tsteps, offsets), "stride_1s": (tsteps_abs, stride, offsets), "shuffled": (shuffled, stride, offsets)}


WORLDS = (1, 2, 3, 8, 16, 40, 120)


@pytest.mark.parametrize("name", ["half", "stride_1s", "shuffled"])
def test_exact_merge_equals_dense_count_of_ranks_per_column(name):
    """`exact_merge` == (no column is fed by more than two ranks), the count taken densely here. Default 'half' schedule: a column has
    two contributions, so the flag is true for every world. 1 s stride: 6-7 windows feed a column, so the flag turns false once a rank
    holds fewer windows than that. Shuffled (non-ascending) `tsteps_abs` under the 1 s stride: false there as well -- and because a
    permutation of the axis only relabels the columns (`nearest_index` finds the same nearest VALUE by a dense scan), for exactly the
    worlds for which the ascending axis gives false; the permuted column labels are what the dense count pins."""
    tsteps_abs, times, offsets = _schedules()[name]
    assert apply.is_ascending(tsteps_abs) == (name != "shuffled")
    table = apply.window_cols_table(tsteps_abs, times, offsets, True)
    assert table.shape == (len(times), len(offsets)) and table.dtype == np.int32 and len(times) >= 60
    flags = {}
    for world in WORLDS:
        info = apply.window_parallel_info(table, len(tsteps_abs), world)
        dense = _dense_ranks_per_column(table, len(tsteps_abs), world)
        assert np.array_equal(info["ranks_per_column"], dense.sum(0))
        assert info["exact_merge"] == bool(dense.sum(0).max() <= 2)
        assert info["windows"] == apply.window_blocks(len(times), world) and info["world"] == world
        for r, rng_ in enumerate(info["columns"]):
            cols = np.flatnonzero(dense[r])
            assert rng_ == ((int(cols.min()), int(cols.max())) if cols.size else None)
        flags[world] = info["exact_merge"]
    if name == "half":
        assert all(flags.values())
    else:
        assert flags[1] and flags[2] and flags[3] and not flags[40] and not flags[120]
    if name == "shuffled":
        asc_axis, _, _ = _schedules()["stride_1s"]
        asc_table = apply.window_cols_table(asc_axis, times, offsets, True)
        assert not np.array_equal(asc_table, table)            # other columns ...
        assert flags == {w: apply.window_parallel_info(asc_table, len(asc_axis), w)["exact_merge"] for w in WORLDS}   # ... same sharing
        wide = [hi - lo for lo, hi in apply.window_parallel_info(table, len(tsteps_abs), 3)["columns"]]
        assert min(wide) > len(tsteps_abs) // 2                # a rank's columns lie scattered over the whole axis


def _stack_numpy(out, x, cols, scale):
    """The semantics of genie_stack_windows, restated: for k, for j in order, c = cols[k][j]; skip c < 0; out[:, c] += x[k, :, j] * scale."""
    for k in range(cols.shape[0]):
        for j in range(cols.shape[1]):
            c = cols[k, j]
            if c >= 0:
                out[:, c] = out[:, c] + x[k, :, j] * scale
    return out


@pytest.mark.parametrize("drop_last", [False, True])
def test_cols_table_reproduces_the_reference_stacking_statement(drop_last):
    rng = np.random.default_rng(11)
    offsets = np.arange(-3.0, 3.0 + 0.75, 0.75)[:9]
    fine = np.arange(100.0, 160.0, 0.75)
    coarse = np.arange(100.0, 160.0, 1.5)          # two offsets share a column: `Out_2[:, cols] += vals` keeps the LAST occurrence
    for tsteps_abs, dup in ((fine, False), (coarse, True)):
        times = np.array([110.2, 113.9, 114.0, 131.7])
        table = apply.window_cols_table(tsteps_abs, times, offsets, drop_last)
        x = rng.standard_normal((len(times), 7, len(offsets))).astype(np.float32)
        want = np.zeros((7, len(tsteps_abs)), dtype=np.float32)
        has_dup = False
        for w, t0 in enumerate(times):
            i0 = int(np.abs(tsteps_abs - t0).argmin())                                                     # process_continuous_days.py:766
            ip = np.abs(tsteps_abs.reshape(-1, 1) - (tsteps_abs[i0] + offsets).reshape(1, -1)).argmin(0)   # :797
            vals = x[w] * np.float32(0.5)
            if drop_last:
                ip, vals = ip[:-1], vals[:, :-1]                                                           # :802-803
            has_dup = has_dup or len(np.unique(ip)) < len(ip)
            want[:, ip] += vals                                                                            # numpy fancy +=
            cols, keep = apply.window_columns(tsteps_abs, t0, offsets, drop_last)
            assert np.array_equal(table[w][table[w] >= 0], cols) and np.array_equal(np.flatnonzero(table[w] >= 0), keep)
            if drop_last:
                assert table[w, -1] == -1
        assert has_dup == dup
        got = _stack_numpy(np.zeros_like(want), x, table, np.float32(0.5))
        assert np.array_equal(got, want) and float(np.abs(want).max()) > 0


def test_stack_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(_lib.INCLUDE, "genie_hip.h")).read()
    assert re.search(r"\bint\s+genie_stack_windows\s*\(", header), "genie_stack_windows is not declared in genie_hip.h"
    assert "genie_stack_windows" in {name for name, _, _ in _lib.SYMBOLS}, "genie_stack_windows is not in _lib.SYMBOLS"
    assert getattr(_lib.load(), "genie_stack_windows").restype is not None
