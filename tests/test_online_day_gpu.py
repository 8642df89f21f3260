"""GPU: the online day loop (`apply.OnlineDay`) against the offline one (`apply_windows_device(stack_on_device=True)`) on the same
schedule: the blocks of closed columns, concatenated, are the offline `Out_2` bit for bit -- for irregular chunks, at the smallest
ring, with tails per window and batched, with chunks that arrive out of order, after a refused pick, under `min_required_picks`."""
import functools
import types

import numpy as np
import pytest
import torch

from genie_amd import apply, engine, module, synthetic
from tests.util import Case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _setup():
    """17 stations x 64 source nodes, 100 queries, 300 picks over ~100 s."""
    geom = synthetic.Geometry(17, 64, L=60e3, n_query=100, seed=71)
    P = synthetic.make_picks(geom, 300, seed=72)
    P[:, 0] = P[:, 0] * 2.5 + 5000.0
    P = P[np.argsort(P[:, 0], kind="stable")]
    trv = geom.travel_times().astype(np.float32)
    c = Case("tiny_6x40")
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV)
    net.load_state_dict({k: v.clone() for k, v in c.weights.items()})
    net.eval()
    net.set_adjacencies_base(torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src), torch.from_numpy(geom.edge_attr()).to(DEV),
                             torch.from_numpy(geom.locs).float().to(DEV), torch.from_numpy(geom.x_grid).float().to(DEV))
    max_t = float(np.ceil(trv.max() + 1.0))
    tsteps, _, _, _, dt_win = apply.window_schedule(P[:, 0], max_t, t_win=6.0, step_size="half")
    tsteps_abs = np.arange(tsteps.min() - 3.0, tsteps.max() + 3.0 + dt_win, dt_win)       # the offline default axis of these picks
    return net, geom, P, trv, max_t, tsteps, tsteps_abs


def _times(stride):
    tsteps = _setup()[5]
    return tsteps if stride == "half" else tsteps.min() + 0.3 + 1.0 * np.arange(int(tsteps.max() - tsteps.min()))


@functools.lru_cache(maxsize=None)
def _offline(stride, tail_batch):
    net, geom, P, trv, max_t, _, tsteps_abs = _setup()
    out, used = apply.apply_windows_device(net, geom, P, trv, tsteps_abs=tsteps_abs, times=_times(stride), max_t=max_t, tail_batch=tail_batch,
                                           stack_on_device=True)
    torch.cuda.synchronize()
    assert float(out.abs().max()) > 0 and len(used) >= 20
    return out, used


def _cuts():
    """Irregular `t_now` values over the picks' span: a repeated one (an empty chunk), two neighbouring pick times (a chunk of one pick)
    and a jump of 30 s (many windows ready in one call)."""
    t = _setup()[2][:, 0]
    rng = np.random.default_rng(9)
    head = t[0] + np.cumsum(rng.uniform(0.2, 7.0, 8))
    k = int(np.searchsorted(t, head[-1])) + 2
    assert head[-1] < t[k - 1] < t[k] < t[k + 1]
    cuts = np.concatenate([head, [t[k], t[k + 1], t[k + 1]], t[k + 1] + 30.0 + np.cumsum(rng.uniform(0.5, 9.0, 6))])
    assert (np.diff(cuts) >= 0).all()
    return cuts


def _online(stride, tail_batch, **kw):
    net, geom, P, trv, max_t, _, tsteps_abs = _setup()
    kw.setdefault("times", _times(stride))
    return apply.OnlineDay(net, geom, trv, tsteps_abs, max_t=max_t, tail_batch=tail_batch, **kw)


def _feed_all(day, cuts, ahead=0.0, seed=0):
    """Feed the picks cut at `cuts`: at every call everything before `t_now` that has not been fed, plus (`ahead` > 0) a random third of
    the picks of the next `ahead` seconds -- so that later chunks reach back below the resident tail. Returns (Out_2, chunk sizes,
    windows run per call)."""
    P = _setup()[2]
    rng = np.random.default_rng(seed)
    fed = np.zeros(len(P), dtype=bool)
    blocks, sizes, ran, at = [], [], [], day.closed
    for t_now in cuts:
        take = ~fed & ((P[:, 0] < t_now) | ((P[:, 0] < t_now + ahead) & (rng.random(len(P)) < 0.33)))
        fed |= take
        n_run = day.n_run
        first, block = day.feed(P[take], t_now)
        assert first == at and block.shape[0] == day.ring.shape[0] and day.closed == first + block.shape[1]
        at = day.closed
        blocks.append(block)
        sizes.append(int(take.sum()))
        ran.append(day.n_run - n_run)
    first, block = day.finish() if fed.all() else day.feed(P[~fed], np.inf)
    assert first == at and day.closed == len(day.tsteps_abs) == at + block.shape[1]
    return torch.cat(blocks + [block], dim=1), sizes, ran


@pytest.mark.parametrize("stride", ["half", "1s"])
def test_online_equals_offline_at_the_smallest_ring(stride):
    """(a) tails per window, `ring_cols` at its minimum (the default): the ring wraps many times over the axis."""
    want, used = _offline(stride, 1)
    day = _online(stride, 1)
    assert day.ring_cols == day.ring_min == apply.online_ring_min(day.h_cols, len(day.tsteps_abs), 1) < len(day.tsteps_abs) // 4
    got, sizes, ran = _feed_all(day, _cuts())
    assert 0 in sizes and 1 in sizes and max(ran) >= 3 and 0 in ran
    assert np.array_equal(day.times_used, used)
    assert torch.equal(got, want)
    assert len(day.picks) == 0 and day.picks.capacity <= 4096            # trimmed behind the windows


@pytest.mark.parametrize("stride", ["half", "1s"])
def test_online_with_batched_tails_equals_offline(stride):
    """(b) `tail_batch=16` in both loops: the batches differ (the online ones end with each call), the bits do not."""
    want, used = _offline(stride, 16)
    assert torch.equal(want, _offline(stride, 1)[0])                     # (what the docstring's contract rests on)
    day = _online(stride, 16)
    got, _, ran = _feed_all(day, _cuts())
    assert max(ran) > (16 if stride == "1s" else 3) and np.array_equal(day.times_used, used)
    assert torch.equal(got, want)


def test_late_chunks_go_through_the_merge_kernel(monkeypatch):
    """(c) chunks that reach back below the resident tail (never below `frozen_t`) are merged on the device; same `Out_2`."""
    calls = []
    merge = engine.picks_merge
    monkeypatch.setattr(engine, "picks_merge", lambda *a: calls.append(1) or merge(*a))
    want, used = _offline("half", 16)
    day = _online("half", 16, ring_cols=200)
    got, sizes, _ = _feed_all(day, _cuts(), ahead=12.0, seed=4)
    assert len(calls) >= 5 and np.array_equal(day.times_used, used)
    assert torch.equal(got, want)


def test_a_pick_older_than_frozen_t_is_refused_and_the_feed_goes_on():
    """(d)"""
    want, _ = _offline("half", 1)
    day = _online("half", 1)
    P, cuts = _setup()[2], _cuts()
    blocks = [day.feed(P[P[:, 0] < cuts[10]], cuts[10])[1]]
    frozen = day.picks.frozen_t
    assert np.isfinite(frozen) and day.n_run > 0
    bad = P[(P[:, 0] >= cuts[10]) & (P[:, 0] < cuts[12])].copy()
    bad[0, 0] = frozen - 1.0
    state = (day.n_run, day.closed, day.t_now, len(day.picks))
    with pytest.raises(ValueError) as err:
        day.feed(bad, cuts[12])
    assert repr(float(frozen)) in str(err.value) and state == (day.n_run, day.closed, day.t_now, len(day.picks))
    with pytest.raises(ValueError):
        day.feed(None, cuts[10] - 1.0)                                   # t_now never decreases
    blocks.append(day.feed(P[(P[:, 0] >= cuts[10]) & (P[:, 0] < cuts[12])], cuts[12])[1])
    blocks.append(day.feed(P[P[:, 0] >= cuts[12]], np.inf)[1])
    assert torch.equal(torch.cat(blocks, dim=1), want)


def test_min_required_picks_drops_the_same_windows_as_offline():
    """(e) the offline loop on its default schedule (its count filter applies) against the online loop given every window start of that
    schedule as a candidate."""
    net, geom, P, trv, max_t, tsteps, tsteps_abs = _setup()
    want, used = apply.apply_windows_device(net, geom, P, trv, max_t=max_t, min_required_picks=40, tail_batch=16, stack_on_device=True)
    torch.cuda.synchronize()
    assert 5 <= len(used) < len(tsteps) - 5 and want.shape[1] == len(tsteps_abs)
    day = _online("half", 16, times=tsteps, min_required_picks=40)
    got, _, _ = _feed_all(day, _cuts())
    assert np.array_equal(day.times_used, used) and day.n_run == len(tsteps)
    assert torch.equal(got, want)


def test_finish_returns_the_rest_of_the_axis():
    """(f)"""
    want, _ = _offline("half", 16)
    day = _online("half", 16)
    P = _setup()[2]
    first, block = day.feed(P, P[60, 0])                                 # everything fed at once, most of it ahead of t_now
    assert first == 0 and day.closed == block.shape[1] < len(day.tsteps_abs) and 0 < day.n_run < len(day.times)
    first2, rest = day.finish()
    assert first2 == block.shape[1] and day.closed == len(day.tsteps_abs) == first2 + rest.shape[1] and day.n_run == len(day.times)
    assert torch.equal(torch.cat([block, rest], dim=1), want)
    first3, none = day.finish()
    assert first3 == len(day.tsteps_abs) and none.shape == (want.shape[0], 0)


def test_refusals():
    """(g)"""
    net, geom, P, trv, max_t, _, tsteps_abs = _setup()
    leg = apply.GridLeg(net, geom.x_grid, trv)
    for bad, kw in ((types.SimpleNamespace(is_sharded=True), {}), ([leg, leg], {}), (net, {"window_parallel": (0, 2)}), (net, {"merge": "columns"})):
        with pytest.raises(NotImplementedError) as err:
            apply.OnlineDay(bad, geom, trv, tsteps_abs, max_t=max_t, **kw)
        assert "OnlineDay" in str(err.value)
    ring_min = _online("half", 16).ring_min
    with pytest.raises(ValueError) as err:
        _online("half", 16, ring_cols=ring_min - 1)
    assert str(ring_min) in str(err.value)
    for bad in (None, tsteps_abs[::-1].copy()):
        with pytest.raises(ValueError):
            apply.OnlineDay(net, geom, trv, bad, max_t=max_t)
    with pytest.raises(ValueError):
        _online("half", 16, times=_times("half")[::-1].copy())
