"""CPU: the host rules of the online catalogue (`apply.OnlineCatalogue`), each replayed without a GPU.

* read replay: a CPU `PickStore` trimmed as `OnlineDay.feed` trims it, stub windows from `window_schedule`, candidate columns from a
  seeded generator released by `postproc.online_release` behind a bound that trails the closed columns as `StreamPeaks`' does. With
  `online_source_ready` (rule 2) and `online_retain_from` (rule 3) every refine range and every association range, for every `tq[j]`,
  is live in the store when its source runs, and every source runs; with `retain_from` left at +inf some range is not;
* marching cuts: `online_marching_verdicts` (rule 4) over random arrival orders gives `retained_after_marching` of the whole list;
* keyed offset: a sub-list's host draw under `source_offset` is `PhiloxCloud.host(offset + i, n)`."""
import numpy as np
import pytest

from genie_amd import apply, postproc

SIG, MAX_T, T_WIN = 3.0, 24.0, 6.0
D, BREAK_WIN = 4, 2.5
TQS = (np.arange(-3.0, 3.75, 0.75), np.arange(-1.5, 4.5, 0.75), np.arange(-4.5, 0.75, 0.75))     # symmetric, late, early


class _StubDay(object):
    """What `OnlineDay.feed` does to its pick store and its column counter, without the windows' work."""

    def __init__(self, tsteps_abs, times, offsets, step_size):
        self.tsteps_abs, self.times = tsteps_abs, times
        cols = apply.window_cols_table(tsteps_abs, times, offsets, step_size == "half", True)
        self.frontiers = apply.online_frontiers(cols, len(tsteps_abs))
        self.picks = apply.PickStore(np.arange(5), 5, "cpu", capacity=32)
        self.n_run, self.closed, self.retain_from = 0, 0, np.inf

    def feed(self, P_chunk, t_now):
        if P_chunk is not None and (self.n_run < len(self.times) or self.retain_from < np.inf):
            self.picks.append(P_chunk)
        ready = apply.online_ready(self.times[self.n_run:], t_now, MAX_T, SIG, T_WIN)
        self.n_run += int(np.argmin(ready)) if not ready.all() else len(ready)
        self.closed = int(self.frontiers[self.n_run])
        first_read = apply.online_read_bounds(self.times[self.n_run:self.n_run + 1], MAX_T, SIG, T_WIN)[0]
        first_read = float(first_read[0]) if self.n_run < len(self.times) else np.inf
        self.picks.frozen_t = min(first_read, t_now)
        self.picks.trim(np.nextafter(min(first_read, self.retain_from), -np.inf))       # the line under test (rule 3)


def _replay(seed, retain):
    """One day. Returns (sources run, ranges that were not live when their source ran)."""
    rng = np.random.default_rng(seed)
    tq = TQS[seed % 3]
    step_size = ("half", "full")[(seed // 3) % 2]
    n_picks = int(rng.integers(150, 400))
    t_all = np.sort(rng.uniform(1000.0, 1000.0 + rng.uniform(60.0, 160.0), n_picks))
    P = np.zeros((n_picks, 5))
    P[:, 0], P[:, 1] = t_all, rng.integers(0, 5, n_picks)
    tsteps, offsets, _, _, dt_win = apply.window_schedule(t_all, MAX_T, t_win=T_WIN, step_size=step_size)
    ts = np.arange(tsteps.min() - 3.0, tsteps.max() + 3.0 + dt_win, dt_win)
    n_cols = len(ts)
    day = _StubDay(ts, np.asarray(tsteps, dtype=np.float64), offsets, step_size)
    cand = np.sort(rng.choice(n_cols, int(rng.integers(3, 14)), replace=False).repeat(rng.integers(1, 3)))      # candidate columns, repeats
    seen_c, held, bound, pending, n_ran, bad, fed, t_now = 0, np.zeros(0, dtype=np.int64), 0, np.zeros(0), 0, 0, 0, t_all[0] - 1.0

    def live(t0):
        lo_t, hi_t = t0 - 2.0 * SIG, t0 + MAX_T + 2.0 * SIG
        assert hi_t <= t_now                                                       # rule 2: nothing the range reads can still arrive
        want = np.flatnonzero((t_all > lo_t) & (t_all < hi_t))                     # (every such pick has been fed: the promise)
        lo, hi = day.picks.embed_range(t0, MAX_T, SIG)
        return np.array_equal(np.sort(day.picks.index_host[lo:hi]), np.sort(order_fed[want])) if want.size else hi == lo

    order_fed = np.full(n_picks, -1, dtype=np.int64)                               # pick -> its `index` (row of the concatenated feed)
    while True:
        last = fed == n_picks and day.n_run == len(day.times) and rng.random() < 0.5
        t_now = np.inf if last else t_now + rng.uniform(0.0, 12.0)
        take = np.flatnonzero((t_all < t_now) & (order_fed < 0))
        early = np.flatnonzero((t_all >= t_now) & (t_all < t_now + 2.0) & (order_fed < 0))
        take = rng.permutation(np.concatenate((take, early[rng.random(early.size) < 0.3])))      # out of order, some ahead of t_now
        if retain:
            day.retain_from = apply.online_retain_from(pending, held, bound, day.closed, ts, tq, SIG)
        if day.n_run < len(day.times) or day.retain_from < np.inf:                 # (otherwise `feed` stores nothing any more)
            order_fed[take] = day.picks.n_fed + np.arange(take.size)
        else:
            order_fed[take] = -2
        fed += take.size
        day.feed(P[take], t_now)
        # the detector: the bound trails the closed columns by the extent of an open run, never falls, and ends at n_cols
        bound = n_cols if day.closed == n_cols else max(bound, day.closed - int(rng.integers(0, 6)))
        held = np.sort(np.concatenate((held, cand[(cand >= seen_c) & (cand < day.closed)])))
        seen_c = day.closed
        k = postproc.online_release(held, bound, ts, D, BREAK_WIN)
        pending, held = np.concatenate((pending, ts[held[:k]])), held[k:]
        assert np.array_equal(pending, np.sort(pending))                           # units come out in ascending time
        ready = apply.online_source_ready(pending, t_now, tq, MAX_T, SIG)
        n_ready = int(np.argmin(ready)) if not ready.all() else len(ready)
        for t_d in pending[:n_ready]:
            bad += not live(t_d)                                                   # the refine pass's window
            bad += sum(not live(t_d + dq) for dq in tq)                            # the association pass's, wherever the refine pass lands
        n_ran += n_ready
        pending = pending[n_ready:]
        if last:
            break
    assert len(pending) == 0 and len(held) == 0 and n_ran == len(cand)             # every source ran
    return n_ran, bad


@pytest.mark.parametrize("seed", range(50))
def test_every_read_of_a_source_is_live_when_it_runs(seed):
    n_ran, bad = _replay(seed, retain=True)
    assert n_ran >= 3 and bad == 0


def test_without_retain_from_the_store_forgets_what_a_source_reads():
    """The reason for rule 3: `feed`'s own trim follows the windows, which are ahead of the sources."""
    bad = [_replay(seed, retain=False)[1] for seed in range(50)]
    assert max(bad) > 0, "no seed shows a forgotten read: the replay does not exercise the retention"


def test_source_ready_and_retain_from_on_hand_made_values():
    tq = np.array([-1.5, 0.0, 2.25])
    assert apply.online_source_ready([100.0], 100.0 + 2.25 + MAX_T + 2 * SIG, tq, MAX_T, SIG).all()          # equality is ready
    assert not apply.online_source_ready([100.0], np.nextafter(100.0 + 2.25 + MAX_T + 2 * SIG, 0.0), tq, MAX_T, SIG).any()
    assert apply.online_source_ready([100.0], 130.0, np.array([-3.0, -1.0]), MAX_T, SIG).all()                # tq_hi = max(tq, 0) = 0
    ts = np.arange(10) * 0.75 + 50.0
    assert apply.online_t_low([], [], 10, 10, ts) == np.inf
    assert apply.online_t_low([70.0], [4, 6], 5, 7, ts) == ts[4]
    assert apply.online_t_low([51.0], [4, 6], 5, 7, ts) == 51.0
    assert apply.online_t_low([], [], 3, 7, ts) == ts[3]
    assert apply.online_retain_from([], [4], 5, 7, ts, tq, SIG) == (ts[4] - 1.5) - 2 * SIG
    assert apply.online_retain_from([], [4], 5, 7, ts, np.array([0.5, 1.0]), SIG) == ts[4] - 2 * SIG         # tq_lo = min(tq, 0) = 0
    assert apply.online_marching_final([1.0, 2.0, 30.0], 20.0, tq, 5.0) == 2                                   # 2 + 10 < 18.5 <= 30 + 10
    assert apply.online_marching_final([1.0, 8.5], 20.0, tq, 5.0) == 1                                         # 8.5 + 10 < 18.5 is false
    assert apply.online_marching_final([1.0, 8.5], np.inf, tq, 5.0) == 2


# ---- rule 4 -----------------------------------------------------------------------------------------------------------------------------

TC_WIN, SP_WIN, SCALE_DEPTH = 6.0, 20e3, 0.2
IDENT = lambda x: x                                                                                            # noqa: E731
MARCH = dict(tc_win=TC_WIN, sp_win=SP_WIN, scale_depth=SCALE_DEPTH, n_steps_max=2, use_directed=False)


def _refined(seed):
    """40 to 200 refined sources, sorted by time: clusters in time and space (chains longer than two hops among them), distinct values."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(40, 201))
    centres = rng.uniform(0.0, 40.0 * n ** 0.5, max(3, n // 6))
    t = centres[rng.integers(0, len(centres), n)] + rng.normal(0.0, 4.0, n)
    x = np.c_[rng.uniform(0, 50e3, (n, 2)), rng.uniform(-30e3, 0, n)]
    tight = rng.random(n) < 0.5
    x[tight] = x[0] + rng.normal(0.0, 4e3, (int(tight.sum()), 3))          # half of them close in space: pairs within both windows
    srcs = np.c_[x, t, rng.permutation(n) / float(n) + 0.1]
    assert len(np.unique(srcs[:, 3])) == n and len(np.unique(srcs[:, 4])) == n
    return srcs[np.argsort(srcs[:, 3])]


def _host_flags(srcs):
    kept = postproc.local_marching(srcs, IDENT, **MARCH)
    return (srcs[:, None, :] == kept[None, :, :]).all(axis=2).any(axis=1)


@pytest.mark.parametrize("seed", range(4))
def test_marching_in_arrival_order_equals_the_marching_of_the_whole_list(seed):
    srcs = _refined(seed)
    n = len(srcs)
    want = apply.retained_after_marching(srcs, IDENT, TC_WIN, SP_WIN, SCALE_DEPTH)
    whole = _host_flags(srcs)
    assert np.array_equal(np.flatnonzero(whole), want)                     # the match back by row index is the cKDTree match
    assert len(want) < n                                                   # the marching removes something ...
    dt, dx = np.abs(srcs[:, None, 3] - srcs[None, :, 3]), np.linalg.norm((srcs[:, None, :3] - srcs[None, :, :3]) * [1, 1, SCALE_DEPTH], axis=2)
    linked = ((dt <= TC_WIN) & (dx <= SP_WIN)).sum(axis=1) > 1
    assert linked[want].any()                                              # ... and keeps a source that has a neighbour
    rng = np.random.default_rng(100 + seed)
    tq = TQS[seed % 3]
    tq_lo = min(tq.min(), 0.0)
    for cut in range(25):                                                  # 4 seeds x 25 = 100 arrival orders
        n_stage = int(rng.integers(1, 12))
        bounds = np.sort(rng.uniform(srcs[0, 3] - 5.0, srcs[-1, 3] + 5.0, n_stage))
        arrived, decided, rows, got = np.zeros(n, dtype=bool), np.zeros((0, 5)), np.zeros((0, 5)), []
        for b in list(bounds) + [np.inf]:
            # every source still to come has t_r >= b = t_low + tq_lo; of those at or above b a random part has arrived already
            new = ~arrived & ((srcs[:, 3] < b) | (rng.random(n) < 0.3))
            arrived |= new
            rows = np.concatenate((rows, srcs[new]))
            rows = rows[np.argsort(rows[:, 3], kind="stable")]
            keep, decided = apply.online_marching_verdicts(decided, rows, b - tq_lo, tq, TC_WIN, _host_flags)
            assert len(keep) == apply.online_marching_final(rows[:, 3], b - tq_lo, tq, TC_WIN)
            got.append(rows[:len(keep)][keep])
            rows = rows[len(keep):]
        assert arrived.all() and len(rows) == 0
        got = np.concatenate(got)
        assert np.array_equal(got, srcs[want]), (seed, cut)                # the same rows, in refined-time order: indices included


# ---- rule 1's keyed draw ------------------------------------------------------------------------------------------------------------------

def test_a_sub_list_draws_the_clouds_of_its_place_in_the_day(monkeypatch):
    """The host-cloud branch of `refine_sources` under `source_offset`: local source i is refined from `PhiloxCloud.host(offset + i, n)`."""
    seen = []

    class Leg(object):
        device = "cpu"
        net = None

        def embed(self, *a):
            return None                                                    # no window: the read-out stays zero, nothing touches a GPU

        def check(self):
            pass

    rand = apply.PhiloxCloud(77)
    host = rand.host
    monkeypatch.setattr(rand, "host", lambda source, n: seen.append((source, n)) or host(source, n))
    srcs = np.array([[1e3, 2e3, -3e3, 10.0, 0.5], [4e3, 5e3, -6e3, 20.0, 0.5], [7e3, 8e3, -9e3, 30.0, 0.5]])
    ranges = ((-1e5, 1e5), (-1e5, 1e5), (-1e5, 1e5))
    args = ([Leg()], None, srcs, np.zeros((4, 3)), np.arange(-1.0, 2.0), MAX_T, np.array([[-5e3, -5e3, -3e3]]), np.array([[10e3, 10e3, 6e3]]),
            16, IDENT, IDENT) + ranges
    got, _ = apply.refine_sources(*args, rand=rand, source_offset=5)
    assert seen == [(5, 16), (6, 16), (7, 16)]
    for i in range(3):                                                     # an all-zero read-out refines to the cloud's first query
        first = srcs[i, 0:3] + (host(5 + i, 16)[0] * np.array([10e3, 10e3, 6e3]) + np.array([-5e3, -5e3, -3e3]))
        assert np.array_equal(got[i, 0:3], first)
    seen.clear()
    apply.refine_sources(*args, rand=rand)
    assert seen == [(0, 16), (1, 16), (2, 16)]                             # the default is the whole list
    with pytest.raises(ValueError, match="source_offset"):
        apply.refine_sources(*args, rand=rand, source_offset=-1)
