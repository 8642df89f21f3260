"""CPU: the host side of the online day over several source grids. The number of legs L enters the day's plan through the stacking scale
alone -- the ready rule, the frontiers, the batches and the ring minimum take no leg argument -- and a saved day's fingerprint names
`n_legs`, after `scale`."""
import inspect

import numpy as np
import pytest
import torch

from genie_amd import apply, checkpoint


def _axis(step_size="half", stride=None):
    max_t = 20.0
    tsteps, offsets, _, n_overlap, dt_win = apply.window_schedule([5000.0, 5140.0], max_t, t_win=6.0, step_size=step_size)
    tsteps_abs = np.arange(tsteps.min() - 3.0, tsteps.max() + 3.0 + dt_win, dt_win)
    times = tsteps if stride is None else tsteps.min() + 0.3 + stride * np.arange(110)
    return tsteps_abs, times, max_t, n_overlap


def test_the_schedule_functions_take_no_leg_argument():
    for fn in (apply.online_read_bounds, apply.online_ready, apply.online_frontiers, apply.online_batch_spans, apply.online_batches,
               apply.online_ring_min, apply.online_source_ready, apply.online_t_low, apply.online_retain_from, apply.online_marching_final,
               apply.online_marching_verdicts):
        names = list(inspect.signature(fn).parameters)
        assert not [n for n in names if "leg" in n or "grid" in n or "lane" in n], (fn.__name__, names)
    assert "n_grids" in inspect.signature(apply.online_day_plan).parameters


@pytest.mark.parametrize("tail_batch", [1, 3, 16])
@pytest.mark.parametrize("step_size,stride", [("half", None), ("full", None), ("partial", None), ("half", 1.0)])
def test_the_plan_of_l_legs_is_the_plan_of_one_but_for_the_scale(step_size, stride, tail_batch):
    """`OnlineDay` takes its plan from `online_day_plan`, to which L legs are `n_grids = L`: every array is the one the host functions
    give for the schedule alone, for every L; the scale is the fp32 reciprocal of `n_overlap * L`, the one of `apply_windows_legs`."""
    tsteps_abs, times, max_t, n_overlap = _axis(step_size, stride)
    offsets = apply.window_schedule([5000.0, 5140.0], max_t, t_win=6.0, step_size=step_size)[1]
    h_cols = apply.window_cols_table(tsteps_abs, times, offsets, step_size == "half", True)
    frontiers = apply.online_frontiers(h_cols, len(tsteps_abs))
    ring_min = apply.online_ring_min(h_cols, len(tsteps_abs), tail_batch)
    plans = {L: apply.online_day_plan(tsteps_abs, times, max_t, 6.0, step_size, tail_batch, 1.0 if L == 1 else L) for L in (1, 2, 3, 32)}
    for L, plan in plans.items():
        assert np.array_equal(plan.tsteps_abs, tsteps_abs) and np.array_equal(plan.times, times) and np.array_equal(plan.offsets, offsets)
        assert plan.h_cols.dtype == h_cols.dtype and np.array_equal(plan.h_cols, h_cols)
        assert np.array_equal(plan.frontiers, frontiers)
        assert (plan.ring_min, plan.ring_cols, plan.tail_batch) == (ring_min, ring_min, tail_batch)
        assert plan.scale == float(np.float32(1.0) / np.float32(n_overlap * L)) == apply._stack_scale(n_overlap, L)[1]
    assert len({plan.scale for plan in plans.values()}) == 4
    for t_now in (5010.0, 5060.5, 5200.0):                       # which windows a feed runs: the schedule and the clock, no L
        ready = apply.online_ready(times, t_now, max_t, 4.0, 6.0)
        assert (ready[:-1] >= ready[1:]).all()
    with pytest.raises(ValueError, match="ring_cols = %d" % (ring_min - 1)):
        apply.online_day_plan(tsteps_abs, times, max_t, 6.0, step_size, tail_batch, 2, ring_cols=ring_min - 1)
    assert apply.online_day_plan(tsteps_abs, times, max_t, 6.0, step_size, tail_batch, 2, ring_cols=ring_min + 3).ring_cols == ring_min + 3


def _fingerprint(n_legs, n_grids=None):
    """`OnlineDay._fingerprint` of a day of `n_legs` legs, on an object given the attributes it reads (the constructor needs a GPU)."""
    tsteps_abs, times, max_t, _ = _axis()
    plan = apply.online_day_plan(tsteps_abs, times, max_t, 6.0, "half", 16, n_grids if n_grids is not None else (1.0 if n_legs == 1 else n_legs))
    day = object.__new__(apply.OnlineDay)
    day.tsteps_abs, day.times, day.offsets, day.step_size, day.scale, day.tail_batch = tsteps_abs, plan.times, plan.offsets, "half", plan.scale, 16
    day.max_t, day.kernel_sig_t, day.t_win, day.min_required_picks, day.dt_embed = max_t, 4.0, 6.0, 1, 0.4
    day.ring, day.lanes = torch.zeros((5, plan.ring_cols)), [None] * n_legs
    return day._fingerprint()


def test_the_fingerprint_names_n_legs_last_and_scale_before_it():
    one, two = _fingerprint(1), _fingerprint(2)
    assert list(one)[-1] == "n_legs" and one["n_legs"] == 1 and two["n_legs"] == 2
    assert list(one)[:-1] == ["tsteps_abs", "times", "offsets", "step_size", "scale", "tail_batch", "max_t", "kernel_sig_t", "t_win",
                              "min_required_picks", "dt_embed", "n_query"]           # the comparison order of before stands
    checkpoint.check_fingerprint("OnlineDay", {"fingerprint": two}, _fingerprint(2))
    with pytest.raises(ValueError, match=r"^OnlineDay\.load_state_dict: the state belongs to another scale "):
        checkpoint.check_fingerprint("OnlineDay", {"fingerprint": two}, one)           # both differ: `scale` comes first
    same_scale = _fingerprint(1, n_grids=2.0)                                          # one leg given the two-leg divisor
    assert same_scale["scale"] == two["scale"] and checkpoint.fingerprint_diff(two, same_scale) == "n_legs"
    with pytest.raises(ValueError, match=r"another n_legs \(saved: 2, this object: 1\)"):
        checkpoint.check_fingerprint("OnlineDay", {"fingerprint": two}, same_scale)
    older = {k: v for k, v in one.items() if k != "n_legs"}                            # a state saved before the field existed
    assert checkpoint.fingerprint_diff(older, one) == "n_legs"
