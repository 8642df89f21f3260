"""CPU: the host side of the online day loop (`apply.OnlineDay`) -- the ready rule against a brute-force restatement, the closed frontier,
the ring minimum (sufficient and tight under a replay of the loop's batching), the growable pick store on CPU tensors against
`ResidentPicks` on the concatenation -- and the three C-ABI symbols the loop adds."""
import os
import re

import numpy as np
import pytest
import torch

from genie_amd import _lib, apply

OFFSETS = apply.window_schedule([0.0, 100.0], 10.0)[1]          # the nine origin-time offsets of a window


# ---- ready windows -------------------------------------------------------------------------------------------------------------------------

def _reads(t, t0, max_t, sig, t_win):
    """Does the window starting at t0 read a pick at time t? The embedding's range (strict, process_utils.py:476) or the count's ball
    (inclusive, process_continuous_days.py:725-741), written out."""
    c, r = t0 + max_t / 2.0, t_win + max_t / 2.0
    return (t0 - 2.0 * sig < t < t0 + max_t + 2.0 * sig) or (c - r <= t <= c + r)


@pytest.mark.parametrize("seed", range(6))
def test_ready_set_is_every_window_whose_reads_end_before_t_now(seed):
    """A window is ready iff no pick at or after `t_now` (the picks that may still be missing) is one it reads. The reads of a window are
    an interval from below, so the pick AT `t_now` decides."""
    rng = np.random.default_rng(seed)
    max_t, sig, t_win = float(rng.uniform(5.0, 60.0)), float(rng.uniform(0.5, 4.0)), float(rng.uniform(1.0, 10.0))
    times = np.sort(rng.uniform(1000.0, 1300.0, 80))
    _, embed_end, count_end = apply.online_read_bounds(times, max_t, sig, t_win)
    nows = np.sort(np.concatenate([rng.uniform(1000.0, 1400.0, 40), embed_end[::7], count_end[::5], np.nextafter(count_end[::5], np.inf)]))
    seen = np.zeros(len(times), dtype=bool)
    for t_now in nows:
        got = apply.online_ready(times, t_now, max_t, sig, t_win)
        want = np.array([not _reads(t_now, t0, max_t, sig, t_win) and t_now > t0 for t0 in times])
        assert np.array_equal(got, want)
        assert (got | ~seen).all() and (got[:-1] >= got[1:]).all()       # never un-ready again; a prefix of the ascending schedule
        seen = got


def test_ready_is_strict_where_the_reads_are():
    """The embedding reads t < t0 + max_t + 2 sigma: a window whose bound EQUALS t_now is ready (2 sigma > t_win: the embedding decides).
    The count reads t <= t0 + max_t + t_win: a pick exactly at t_now may be missing, so that window is not ready until t_now is past it."""
    t0 = np.array([100.0])
    assert apply.online_ready(t0, 100.0 + 20.0 + 8.0, 20.0, 4.0, 6.0)[0]
    assert not apply.online_ready(t0, np.nextafter(128.0, 0.0), 20.0, 4.0, 6.0)[0]
    assert not apply.online_ready(t0, 100.0 + 20.0 + 6.0, 20.0, 1.0, 6.0)[0]
    assert apply.online_ready(t0, np.nextafter(126.0, np.inf), 20.0, 1.0, 6.0)[0]
    first, _, _ = apply.online_read_bounds(t0, 20.0, 4.0, 6.0)
    assert first[0] == 92.0 and apply.online_read_bounds(t0, 20.0, 1.0, 6.0)[0][0] == 94.0


# ---- closed frontier and ring minimum -------------------------------------------------------------------------------------------------------

def _schedules():
    rng = np.random.default_rng(11)
    out = []
    for step_size, stride in (("half", None), ("full", None), ("half", 1.0)):
        tsteps, offsets, step, _, dt_win = apply.window_schedule([5000.0, 5140.0], 20.0, t_win=6.0, step_size=step_size)
        tsteps_abs = np.arange(tsteps.min() - 3.0, tsteps.max() + 3.0 + dt_win, dt_win)
        times = tsteps if stride is None else tsteps.min() + 0.3 + stride * np.arange(110)
        times = times[rng.random(len(times)) < 0.9]                      # gaps in the schedule
        out.append((step_size, tsteps_abs, apply.window_cols_table(tsteps_abs, times, offsets, step_size == "half")))
    coarse = np.arange(4970.0, 5150.0, 1.5)                              # 1.5 s columns under 0.75 s offsets: duplicates become -1
    out.append(("full", coarse, apply.window_cols_table(coarse, np.arange(4980.0, 5120.0, 6.75), OFFSETS, False)))
    return out


@pytest.mark.parametrize("step_size,tsteps_abs,cols", _schedules())
def test_frontier_is_the_first_column_of_any_unrun_window(step_size, tsteps_abs, cols):
    n_cols = len(tsteps_abs)
    assert (cols == -1).any() or step_size == "full"
    fr = apply.online_frontiers(cols, n_cols)
    assert fr.shape == (len(cols) + 1,) and fr[-1] == n_cols
    for k in range(len(cols) + 1):
        listed = cols[k:][cols[k:] >= 0]
        assert fr[k] == (listed.min() if listed.size else n_cols)
    assert (np.diff(fr) >= 0).all()


def _replay(cols, n_cols, tail_batch, ends, W):
    """The loop of `OnlineDay.feed` on the host: `ends` = the number of windows ready at each call. Returns the widest set of columns
    open at once, and whether two open columns ever shared a slot of a ring of W."""
    fr = apply.online_frontiers(cols, n_cols)
    closed, last, widest, clash, n_run = int(fr[0]), -1, 0, False, 0
    for end in ends:
        for a, b in apply.online_batches(n_run, end, tail_batch):
            used = cols[a:b][cols[a:b] >= 0]
            if used.size:
                assert used.min() >= closed                              # a closed column is never fed again
                last = max(last, int(used.max()))
            open_cols = np.arange(closed, last + 1)
            widest = max(widest, len(open_cols))
            clash |= len(np.unique(open_cols % W)) < len(open_cols)
            closed = max(closed, int(fr[b]))
        n_run = end
    return widest, clash


@pytest.mark.parametrize("tail_batch", [1, 3, 16])
@pytest.mark.parametrize("step_size,tsteps_abs,cols", _schedules())
def test_ring_minimum_suffices_and_is_tight(step_size, tsteps_abs, cols, tail_batch):
    n, n_cols = len(cols), len(tsteps_abs)
    W = apply.online_ring_min(cols, n_cols, tail_batch)
    spans = apply.online_batch_spans(cols, n_cols, tail_batch)
    assert W == spans.max() and 1 <= W < n_cols
    rng = np.random.default_rng(5)
    feeds = [[n], list(range(1, n + 1)), sorted(set(rng.integers(0, n + 1, 12).tolist() + [n]))]
    worst = int(np.argmax(spans))                                        # a batch that starts at the widest point of the schedule
    feeds.append([worst, n] if worst else [n])
    for ends in feeds:
        widest, clash = _replay(cols, n_cols, tail_batch, ends, W)
        assert widest <= W and not clash
    widest, clash = _replay(cols, n_cols, tail_batch, feeds[-1], W - 1)
    assert widest == W and clash                                         # one column fewer and two open columns share a slot


def test_batches_cover_the_ready_windows_in_order():
    assert apply.online_batches(3, 3, 4) == []
    assert apply.online_batches(3, 12, 4) == [(3, 7), (7, 11), (11, 12)]
    assert apply.online_batches(0, 2, 1) == [(0, 1), (1, 2)]


# ---- PickStore on CPU tensors ---------------------------------------------------------------------------------------------------------------

S_ALL = 30
IND_USE = np.random.default_rng(3).permutation(S_ALL)[:20]               # 10 stations are not the model's


def _chunk(rng, m, t_lo, t_hi, decimals):
    t = np.round(rng.uniform(t_lo, t_hi, m), decimals)                   # whole seconds: ties inside and across chunks
    return np.stack([t, rng.integers(0, S_ALL, m).astype(np.float64), rng.random(m), rng.random(m), rng.integers(0, 2, m).astype(np.float64)], axis=1)


def _same(store, ref):
    for f in ("t", "sta", "phase", "phase_f", "index"):
        a, b = getattr(store, f), getattr(ref, f)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), f
    assert np.array_equal(store.t_host, ref.t_host) and len(store) == len(ref)


@pytest.mark.parametrize("use_phase_types", [True, False])
@pytest.mark.parametrize("seed", range(8))
def test_pick_store_equals_resident_picks_of_the_concatenation(seed, use_phase_types):
    rng = np.random.default_rng(seed)
    store = apply.PickStore(IND_USE, S_ALL, "cpu", use_phase_types=use_phase_types, capacity=4)
    chunks = []
    for c in range(int(rng.integers(2, 9))):
        lo = 5.0 * c if seed % 2 else 0.0                                # advancing chunks (mostly appended) / overlapping ones (merged)
        chunks.append(_chunk(rng, int(rng.integers(0, 40)), lo, lo + 30.0, 0 if seed % 3 else 3))
        assert store.append(chunks[-1]) == 0
        _same(store, apply.ResidentPicks(np.concatenate(chunks), IND_USE, S_ALL, "cpu", use_phase_types=use_phase_types))
    ref = apply.ResidentPicks(np.concatenate(chunks), IND_USE, S_ALL, "cpu", use_phase_types=use_phase_types)
    assert store.n_fed == len(ref.P) and store.capacity >= len(store)
    assert np.array_equal(store.meta(store.index[::3]), ref.meta(ref.index[::3]))
    for t0 in (3.0, 12.5, 40.0):
        assert store.embed_range(t0, 10.0, 1.0) == ref.embed_range(t0, 10.0, 1.0)
        for a, b in zip(store.pick_inputs(t0, 10.0, 1.0), ref.pick_inputs(t0, 10.0, 1.0)):
            assert torch.equal(a, b)


def test_merge_ranks_pins_the_order_of_ties():
    """Equal times: the resident pick first, then the chunk's, each run in its own order."""
    a, b = np.array([1.0, 2.0, 2.0, 5.0]), np.array([0.0, 2.0, 2.0, 5.0, 6.0])
    pos_a, pos_b = apply.merge_ranks(a, b)
    assert pos_a.tolist() == [1, 2, 3, 6] and pos_b.tolist() == [0, 4, 5, 7, 8]
    t_a, t_b = apply.merge_ranks(torch.from_numpy(a), torch.from_numpy(b))
    assert t_a.tolist() == pos_a.tolist() and t_b.tolist() == pos_b.tolist()
    for x, y in ((a, b[:0]), (a[:0], b)):
        pa, pb = apply.merge_ranks(x, y)
        assert pa.tolist() == list(range(len(x))) and pb.tolist() == list(range(len(y)))


def test_trim_and_compaction_keep_the_views_of_the_untrimmed_store():
    rng = np.random.default_rng(21)
    trimmed = apply.PickStore(IND_USE, S_ALL, "cpu", capacity=8)
    whole = apply.PickStore(IND_USE, S_ALL, "cpu", capacity=8)
    caps = set()
    for c in range(40):
        P = _chunk(rng, 12, 4.0 * c - 3.0, 4.0 * c + 6.0, 1)             # every chunk reaches back below the resident tail
        trimmed.append(P)
        whole.append(P)
        t_before = 4.0 * c - 8.0
        live = trimmed.trim(t_before)
        assert live == int((whole.t_host > t_before).sum()) and (trimmed.t_host > t_before).all()
        caps.add(trimmed.capacity)
        for t0 in (4.0 * c - 6.0, 4.0 * c - 1.0):                        # windows that read nothing at or below t_before
            lo, hi = trimmed.embed_range(t0, 5.0, 1.0)
            lo_w, hi_w = whole.embed_range(t0, 5.0, 1.0)
            assert hi - lo == hi_w - lo_w
            for f in ("t", "sta", "phase", "index"):
                assert torch.equal(getattr(trimmed, f)[lo:hi], getattr(whole, f)[lo:hi_w][-(hi - lo):] if hi > lo else getattr(whole, f)[:0])
            assert np.array_equal(trimmed.meta(trimmed.index[lo:hi]), whole.meta(whole.index[lo_w:hi_w]))
    assert max(caps) <= 64 < whole.capacity                              # compaction, not growth, kept the trimmed store small
    with pytest.raises(KeyError):
        trimmed.meta(whole.index[:1])


def test_late_pick_raises_and_leaves_the_store_unchanged_or_is_dropped():
    rng = np.random.default_rng(8)
    store = apply.PickStore(IND_USE, S_ALL, "cpu", capacity=16)
    first = _chunk(rng, 30, 100.0, 130.0, 2)
    store.append(first)
    store.frozen_t = 110.0
    store.trim(110.0)
    before = [getattr(store, f).clone() for f in ("t", "sta", "phase", "index")] + [store.t_host.copy(), store.n_fed, store.capacity]
    late = _chunk(rng, 6, 112.0, 140.0, 2)
    late[2, 0], late[2, 1] = 109.5, float(IND_USE[0])
    late[4, 0], late[4, 1] = 50.0, float(np.setdiff1d(np.arange(S_ALL), IND_USE)[0])      # old, but not a station of the model: not late
    with pytest.raises(ValueError) as err:
        store.append(late)
    assert "109.5" in str(err.value) and "110.0" in str(err.value)
    after = [getattr(store, f) for f in ("t", "sta", "phase", "index")] + [store.t_host, store.n_fed, store.capacity]
    for x, y in zip(before[:4], after[:4]):
        assert torch.equal(x, y)
    assert np.array_equal(before[4], after[4]) and before[5:] == after[5:]
    assert store.append(late, late="drop") == 1
    kept = np.concatenate([first, late])
    ref = apply.ResidentPicks(kept, IND_USE, S_ALL, "cpu")
    live = (ref.t_host > 110.0) & (ref.t_host != 109.5)
    assert np.array_equal(store.t_host, ref.t_host[live]) and np.array_equal(store.index.numpy(), ref.index.numpy()[live])
    with pytest.raises(ValueError):
        store.append(first, late="ignore")


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["genie_picks_merge", "genie_stack_windows_ring", "genie_ring_close"])
def test_online_symbols_are_declared_bound_and_exported(name):
    header = open(os.path.join(_lib.INCLUDE, "genie_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % name, header), "%s is not declared in genie_hip.h" % name
    assert name in {n for n, _, _ in _lib.SYMBOLS}, "%s is not in _lib.SYMBOLS" % name
    assert getattr(_lib.load(), name).restype is not None
