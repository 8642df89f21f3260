"""Sliding-window apply loop around `forward_fixed_source` — the caller of the hot path
(`/root/reference/Code/process_continuous_days.py:761-810`, setup `:357-381, :571, :725-754`).

Semantics kept from the reference:
* prediction window of `n_resolution = 9` origin-time offsets `arange(-t_win/2, t_win/2 + dt_win, dt_win)` (`:357-362`);
* window starts `tsteps = arange(max(0, min(pick_t) - max_t), min(day_len, max(pick_t)), step)`, `step` and `n_overlap`
  from `step_size` in {'full', 'partial', 'half'} (`:367-381, :571`);
* windows with fewer than `min_required_picks` picks in `[t0 - t_win, t0 + max_t + t_win]` are skipped (`:725-741`);
* `Out_2[:, idx(tsteps_abs[idx(t0)] + offsets)] += x[:, :, 0] / n_overlap / n_grids`, dropping the last offset when
  `step_size == 'half'` (`:766, :797-805`): the window start is snapped to `tsteps_abs` first, and a column listed twice is
  written once (numpy fancy `+=`), see `window_columns`;
* windows with no pick in the embedding range are skipped (`:792-793`).
Differences by design: `Out_2` stays on the GPU and is accumulated with `index_add_` (the reference copies every window's
output to the host, `:803-805`); nothing in the loop synchronises with the host.

`apply_windows` takes any host embedding callable (default: `genie_amd.synthetic.make_slice_mask`, the exact
nearest-pick semantics of `process_utils.py:262-275`). `apply_windows_device` is the GPU-only loop: picks and the static
travel-time table stay resident on the device and every window's `Slice/Mask` is produced by `genie_embed_window`
(`extract_input_from_data`, `process_utils.py:460-642`), so a window costs no host->device copy at all. `apply_windows_legs` runs
the same loop over several source grids into one `Out_2`. Both are adapters: their arguments become a `_day_plan` (schedule, pick
ranges, this rank's windows, column table: host arithmetic, once) and a list of lanes, and `_run_day` is the one loop over them.
`OnlineDay` runs the same per-window body (`_WindowBody`) for a live feed: picks arrive in chunks (`PickStore`), windows run as they
become ready, and the columns of `Out_2` are returned as they close.
"""
import collections
import threading
import types

import numpy as np
import torch

from . import checkpoint, engine, synthetic


def window_schedule(pick_times, max_t, day_len=86400.0, t_win=6.0, n_resolution=9, step_size="half"):
    """(tsteps, offsets, step, n_overlap, dt_win) exactly as process_continuous_days.py:357-381,571 builds them."""
    dt_win = float(np.diff(np.linspace(-t_win / 2.0, t_win / 2.0, n_resolution))[0])
    if step_size == "full":
        step, n_overlap = n_resolution * dt_win, 1.0
    elif step_size == "partial":
        step, n_overlap = (n_resolution / 3) * dt_win, 3.0
    elif step_size == "half":
        step, n_overlap = int(np.floor(n_resolution / 2)) * dt_win, 2.0
    else:
        raise ValueError("step_size must be 'full', 'partial' or 'half'")
    t = np.asarray(pick_times, dtype=np.float64)
    tsteps = np.arange(max(0.0, t.min() - max_t), min(day_len, t.max()), step)
    offsets = np.arange(-t_win / 2.0, t_win / 2.0 + dt_win, dt_win)[:n_resolution]
    return tsteps, offsets, step, n_overlap, dt_win


def windows_with_enough_picks(pick_times, tsteps, max_t, t_win, min_required_picks):
    """Keep window starts whose neighbourhood holds >= min_required_picks picks (process_continuous_days.py:725-741:
    ball of radius t_win + max_t/2 around t0 + max_t/2)."""
    t = np.sort(np.asarray(pick_times, dtype=np.float64))
    c = tsteps + max_t / 2.0
    r = t_win + max_t / 2.0
    n = np.searchsorted(t, c + r, side="right") - np.searchsorted(t, c - r, side="left")
    return tsteps[n >= max(1, int(min_required_picks))]


def is_ascending(grid):
    grid = np.asarray(grid)
    return bool(grid.shape[0] < 2 or np.all(grid[1:] >= grid[:-1]))


def nearest_index(grid, values, ascending=None):
    """Index of the `grid` entry nearest to every value (ties -> the lower index, as `np.abs(grid - v).argmin()` gives): a
    binary search + a choice between the two bracketing entries when `grid` is ascending (the reference's `tsteps_abs`,
    process_continuous_days.py:374-381, queried through a cKDTree at :766 / :797) -- O(log n) per value instead of a dense scan
    of a day-long grid per window; any other grid takes the dense scan."""
    grid = np.asarray(grid, dtype=np.float64)
    values = np.asarray(values, dtype=np.float64)
    n = grid.shape[0]
    if ascending is None:
        ascending = is_ascending(grid)
    if n < 2 or not ascending:
        return np.abs(grid.reshape(-1, 1) - values.reshape(1, -1)).argmin(0)
    hi = np.clip(np.searchsorted(grid, values, side="left"), 0, n - 1)
    lo = np.clip(hi - 1, 0, n - 1)
    take_lo = np.abs(grid[lo] - values) <= np.abs(grid[hi] - values)
    idx = np.where(take_lo, lo, hi)
    # equal grid entries: argmin returns the first of them
    first = np.searchsorted(grid, grid[idx], side="left")
    return first.astype(np.int64)


def window_columns(tsteps_abs, t0, offsets, drop_last, ascending=None):
    """Columns of `Out_2` one window adds to, as process_continuous_days.py:766,797-805 finds them: the window start is first
    SNAPPED to its nearest `tsteps_abs` entry (`tree_tsteps.query`, :766), the nine offsets are added to that entry and
    looked up again (:797), the last one is dropped for step_size 'half' (:802-803). numpy's `Out_2[:, cols] += vals` writes
    a column that appears twice only once (the LAST occurrence wins), so duplicates are reduced to their last occurrence.
    Returns (cols int64 [m], keep int64 [m]: offset index feeding each column)."""
    tsteps_abs = np.asarray(tsteps_abs, dtype=np.float64)
    if ascending is None:
        ascending = is_ascending(tsteps_abs)          # (loops over many windows pass it: one O(n) check per grid, not per window)
    i0 = int(nearest_index(tsteps_abs, np.asarray([t0], dtype=np.float64), ascending)[0])
    ip = nearest_index(tsteps_abs, tsteps_abs[i0] + np.asarray(offsets, dtype=np.float64), ascending)
    if drop_last:
        ip = ip[:-1]
    keep = np.array([k for k in range(len(ip)) if ip[k] not in ip[k + 1:]], dtype=np.int64)
    return ip[keep].astype(np.int64), keep


def window_cols_table(tsteps_abs, times, offsets, drop_last, ascending=None):
    """The `cols` table of `genie_stack_windows` for a list of window starts: int32 [len(times), len(offsets)], entry [w, j] = the
    column of `Out_2` offset j of window w adds to (`window_columns`), or -1 where the offset adds nothing: the last offset of
    step_size 'half' (`drop_last`) and every occurrence but the last of a column one window lists twice."""
    tsteps_abs = np.asarray(tsteps_abs, dtype=np.float64)
    if ascending is None:
        ascending = is_ascending(tsteps_abs)
    table = np.full((len(times), len(offsets)), -1, dtype=np.int32)
    for w, t0 in enumerate(times):
        cols, keep = window_columns(tsteps_abs, t0, offsets, drop_last, ascending)
        table[w, keep] = cols
    return table


def window_blocks(n, world):
    """[(lo, hi)] * world: `range(n)` cut into `world` contiguous blocks whose lengths differ by at most one (the longer ones
    first; blocks are empty only when n < world). Rank r of a window-parallel apply loop takes windows [lo_r, hi_r)."""
    n, world = int(n), int(world)
    if n < 0 or world < 1:
        raise ValueError("window_blocks needs n >= 0 and world >= 1")
    base, extra = divmod(n, world)
    blocks, lo = [], 0
    for r in range(world):
        hi = lo + base + (1 if r < extra else 0)
        blocks.append((lo, hi))
        lo = hi
    return blocks


def window_parallel_info(cols, n_cols, world):
    """What a window-parallel run over `world` ranks does with the windows of a `cols` table (`window_cols_table`, [n, T], -1 = no
    column), on the host: a dict with `world`; `windows` [(lo, hi)] per rank (`window_blocks`); `columns` [(c_min, c_max) or None for a rank
    without windows] per rank; `ranks_per_column` int32 [n_cols] = how many ranks add to each column of `Out_2`; and `exact_merge` = no
    column is fed by more than two ranks. Then every element's sum over the ranks has at most two non-zero terms; adding zeros is exact and
    fp32 addition commutes, so the merged `Out_2` does not depend on the order in which the collective adds the ranks' partials.
    False for tiny days (fewer windows per rank than windows per column) or a `times` list that does not ascend: the merge is then still
    the right sum, up to rounding that depends on the collective. (A `tsteps_abs` that does not ascend only relabels the columns: the
    flag is the one of the sorted axis, while a rank's column RANGE can then span the whole axis.)"""
    cols = np.asarray(cols)
    blocks = window_blocks(cols.shape[0], world)
    per_col = np.zeros(int(n_cols), dtype=np.int32)
    ranges = []
    for lo, hi in blocks:
        c = np.unique(cols[lo:hi])
        c = c[c >= 0]
        per_col[c] += 1
        ranges.append((int(c[0]), int(c[-1])) if c.size else None)
    return {"world": int(world), "windows": blocks, "columns": ranges, "ranks_per_column": per_col,
            "exact_merge": bool(per_col.max(initial=0) <= 2)}


def window_band_plan(cols, n_cols, world, margin=1, n_rows=1, tsteps_abs=None, times=None):
    """The column bands of a window-parallel run that keeps `Out_2` distributed (`merge="columns"`), on the host, from the `cols` table
    of ALL windows (`window_cols_table`, [n, T], -1 = no column) -- next to `window_parallel_info`, which describes the dense merge. A
    dict of per-rank lists:
    * `own` [(o_lo, o_hi)]: half-open ranges that partition [0, n_cols). The cut between two ranks is the first column of the later
      rank's first window; rank 0 starts at 0, the last rank with windows ends at n_cols, a rank without windows owns the empty range
      (n_cols, n_cols) (rank 0 owns the whole axis of a day without windows). A rank reports the peaks whose column it owns.
    * `band` [(b_lo, b_hi)]: what the rank allocates, the hull of the columns its own windows feed and of [o_lo - margin, o_hi +
      margin), clipped to the axis: a peak needs its two neighbours, a flat top its whole extent (`postproc.detect_sources_banded`).
    * `recv`, `send` [[(peer, c_lo, c_hi)]]: the strips of columns inside a rank's band that another rank's windows feed (the peer's
      fed range cut to the band), each listed in the receiver's `recv` and in the feeder's `send`, ascending by peer.
    * `band_bytes`, `strip_bytes` (received), `dense_bytes`: fp32 bytes per rank for `n_rows` rows of `Out_2` -- the band and its
      strips against the full-size matrix every rank allocates and all-reduces under `merge="dense"`.
    Plus `world`, `margin`, `n_cols`, `windows` (`window_blocks`) and `fed` [(c_min, c_max) or None].
    The cuts need windows whose columns ascend: `tsteps_abs` and `times` (checked with `is_ascending` when given, as the window starts'
    first columns always are) must ascend; otherwise a ValueError points to `merge="dense"`, which needs no order."""
    cols = np.asarray(cols).astype(np.int64)
    n_cols, world, margin = int(n_cols), int(world), int(margin)
    if margin < 1:
        raise ValueError("window_band_plan: margin must be >= 1 (a peak needs both neighbours)")
    n = cols.shape[0]
    big = np.iinfo(np.int64).max
    first = np.where(cols >= 0, cols, big).min(axis=1) if n else np.zeros(0, dtype=np.int64)
    last = cols.max(axis=1) if n else np.zeros(0, dtype=np.int64)
    if not (all(is_ascending(a) for a in (first, last) + tuple(x for x in (tsteps_abs, times) if x is not None))
            and (first < big).all() and (n == 0 or last.max() < n_cols)):
        raise ValueError('window_band_plan: the column bands need an ascending tsteps_abs and ascending window times (every window '
                         'inside the axis); use merge="dense" for a day whose windows are not ordered along the axis')
    blocks = window_blocks(n, world)
    fed = [(int(first[lo]), int(last[hi - 1])) if hi > lo else None for lo, hi in blocks]
    cuts = [0 if r == 0 else (fed[r][0] if fed[r] is not None else n_cols) for r in range(world)] + [n_cols]
    own = [(cuts[r], cuts[r + 1]) for r in range(world)]
    band = []
    for r in range(world):
        lo, hi = own[r][0] - margin, own[r][1] + margin
        if fed[r] is not None:
            lo, hi = min(lo, fed[r][0]), max(hi, fed[r][1] + 1)
        band.append((max(lo, 0), min(hi, n_cols)))
    recv, send = [[] for _ in range(world)], [[] for _ in range(world)]
    for r in range(world):
        for p in range(world):
            if p != r and fed[p] is not None:
                c_lo, c_hi = max(band[r][0], fed[p][0]), min(band[r][1], fed[p][1] + 1)
                if c_hi > c_lo:
                    recv[r].append((p, c_lo, c_hi))
                    send[p].append((r, c_lo, c_hi))
    row = 4 * int(n_rows)
    return {"world": world, "margin": margin, "n_cols": n_cols, "windows": blocks, "fed": fed, "own": own, "band": band, "recv": recv,
            "send": send, "band_bytes": [row * (hi - lo) for lo, hi in band],
            "strip_bytes": [row * sum(c_hi - c_lo for _, c_lo, c_hi in strips) for strips in recv], "dense_bytes": [row * n_cols] * world}


class BandedOut2(object):
    """This rank's column band of a window-parallel day's `Out_2` (`apply_windows_device` / `apply_windows_legs` with
    `merge="columns"`): `band` = the fp32 device tensor [Q, b_hi - b_lo] of the global columns [b_lo, b_hi), of which this rank OWNS
    [o_lo, o_hi) of the `n_cols` of the axis (`window_band_plan`, kept whole in `plan`, this rank being `rank`). `complete`: the other
    ranks' strips have been added, so every column of the band holds the day's full sum; until then it holds this rank's windows only
    (tuple form: the caller exchanges the strips of `plan["recv"][rank]` itself and calls `add_strips`). `group`, `timeout`: the process
    group the strips came over (True: the default group), or None. `postproc.detect_sources_banded` takes it in place of the dense `Out_2`."""

    def __init__(self, band, rank, plan, complete=False, group=None, timeout=60.0):
        self.band, self.rank, self.plan, self.complete, self.group, self.timeout = band, int(rank), plan, bool(complete), group, float(timeout)
        (self.b_lo, self.b_hi), (self.o_lo, self.o_hi) = plan["band"][self.rank], plan["own"][self.rank]
        self.n_cols = plan["n_cols"]

    def strip(self, c_lo, c_hi):
        """The band's global columns [c_lo, c_hi) (a view): what this rank sends for an entry (peer, c_lo, c_hi) of its `send` list."""
        if not self.b_lo <= c_lo <= c_hi <= self.b_hi:
            raise ValueError("BandedOut2.strip: [%d, %d) is not inside the band [%d, %d)" % (c_lo, c_hi, self.b_lo, self.b_hi))
        return self.band[:, c_lo - self.b_lo:c_hi - self.b_lo]

    def add_strips(self, strips):
        """Complete the band: `strips` = {peer: tensor [Q, c_hi - c_lo]} for every entry of `plan["recv"][rank]`, each that peer's own
        (not yet completed) columns. A column's contributions are added in ascending rank order, this rank's own among them, `((p_a +
        p_b) + p_c)`, from zero as a rank-ordered sum of dense partials runs; a rank that does not feed a column adds nothing. The
        result is therefore a fixed function of the ranks' partials for any world size, and the dense all-reduce's wherever its own
        order does not matter (`exact_merge`)."""
        if self.complete:
            raise ValueError("BandedOut2.add_strips: the band is complete already")
        recv = self.plan["recv"][self.rank]
        if sorted(strips) != [p for p, _, _ in recv]:
            raise ValueError("BandedOut2.add_strips: strips of the peers %s expected" % [p for p, _, _ in recv])
        lower = [e for e in recv if e[0] < self.rank]
        if len(lower) > 1:       # (p_a + p_b) first, then this rank's part: fp32 addition commutes but does not associate
            lo, hi = min(e[1] for e in lower), max(e[2] for e in lower)
            acc = torch.zeros((self.band.shape[0], hi - lo), dtype=self.band.dtype, device=self.band.device)
            for p, c_lo, c_hi in lower:
                acc[:, c_lo - lo:c_hi - lo] += strips[p]
            mine = self.strip(lo, hi)
            torch.add(acc, mine, out=mine)
        for p, c_lo, c_hi in (lower if len(lower) == 1 else []) + [e for e in recv if e[0] > self.rank]:
            self.strip(c_lo, c_hi).add_(strips[p])
        self.complete = True
        return self

    def dense(self):
        """The full-size matrix [Q, n_cols] with this band in place and zeros elsewhere (for tests and callers that want it: it is what
        `merge="columns"` avoids)."""
        out = torch.zeros((self.band.shape[0], self.n_cols), dtype=self.band.dtype, device=self.band.device)
        out[:, self.b_lo:self.b_hi] = self.band
        return out

    def own_dense(self):
        """The full-size matrix with this rank's OWN columns only: the ranks' `own_dense()` of completed bands add up to the day's
        `Out_2` with one non-zero term per element (the dense fallback of `postproc.detect_sources_banded`)."""
        out = torch.zeros((self.band.shape[0], self.n_cols), dtype=self.band.dtype, device=self.band.device)
        if self.o_hi > self.o_lo:
            out[:, self.o_lo:self.o_hi] = self.strip(self.o_lo, self.o_hi)
        return out


def picks_in_embed_range(pick_times_sorted, t0, max_t, kernel_sig_t):
    """[lo, hi) of the picks with t0 - 2 sigma < t < t0 + max_t + 2 sigma (process_utils.py:476); the reference skips a window
    whose range is empty (process_continuous_days.py:792-793)."""
    lo = int(np.searchsorted(pick_times_sorted, t0 - 2.0 * kernel_sig_t, side="right"))
    hi = int(np.searchsorted(pick_times_sorted, t0 + max_t + 2.0 * kernel_sig_t, side="left"))
    return lo, hi


_RankSplit = collections.namedtuple("_RankSplit", "rank world group collective")


def _rank_split(parallel, name, sharded):
    """`_RankSplit(rank, world, group, collective)` of a `window_parallel` / `source_parallel` argument (`name` in messages) -- `(rank,
    world)`: no collective; a `torch.distributed` process group or True for the default group: collective -- or None. `sharded`: a model
    involved is source-node-sharded, which is refused. Checked before anything touches a device."""
    if parallel is None or parallel is False:
        return None
    if sharded:
        raise NotImplementedError("%s on a source-node-sharded model: the hybrid of %s replicas and source-node shards is not built; "
                                  "use an unsharded model per GPU" % (name, name.replace("_", "-")))
    from . import dist as _dist
    if isinstance(parallel, (tuple, list)):
        return _RankSplit(*_dist.resolve_shard(shard=parallel), collective=False)
    return _RankSplit(*_dist.resolve_shard(process_group=parallel), collective=True)


def _day_schedule(P, max_t, day_len, t_win, step_size, min_required_picks, tsteps_abs, times=None):
    """(tsteps_abs, times, offsets, n_overlap) of a day's apply loop: the reference's axis and kept window starts, or the caller's own."""
    tsteps, offsets, step, n_overlap, dt_win = window_schedule(P[:, 0], max_t, day_len, t_win, 9, step_size)
    if tsteps_abs is None:
        tsteps_abs = np.arange(tsteps.min() - t_win / 2.0, tsteps.max() + t_win / 2.0 + dt_win, dt_win)
    if times is None:
        times = windows_with_enough_picks(P[:, 0], tsteps, max_t, t_win, min_required_picks)
    return tsteps_abs, np.asarray(times, dtype=np.float64), offsets, n_overlap


def _check_verdicts(net):
    """Raise what the device-side checks of the completed calls found, on every context of the model (a shard's local one included)."""
    for hp in net._contexts():
        hp.check_input_range()


def apply_windows(net, geom, P, tsteps_abs=None, t_win=6.0, step_size="half", min_required_picks=1, n_grids=1.0,
                  day_len=86400.0, device=None, embed=None):
    """Run `net.forward_fixed_source` over every kept window and stack the query read-out into `Out_2[Q, len(tsteps_abs)]`.

    net: genie_amd.module.GCN_Detection_Network_extended with adjacencies set; geom: genie_amd.synthetic.Geometry (locs,
    x_grid, x_query, travel times); P: picks [n, 5] (t, station, amp, prob, phase). Returns (Out_2 on device, times used).
    """
    dev = device or next(net.parameters()).device
    max_t = geom.max_t
    tsteps_abs, times, offsets, n_overlap = _day_schedule(P, max_t, day_len, t_win, step_size, min_required_picks, tsteps_abs)
    Out_2 = torch.zeros((geom.x_query.shape[0], len(tsteps_abs)), dtype=torch.float32, device=dev)
    locs = torch.from_numpy(geom.locs).float().to(dev)
    xg = torch.from_numpy(geom.x_grid).float().to(dev)
    xq = torch.from_numpy(geom.x_query).float().to(dev)
    tq = torch.from_numpy(offsets.reshape(-1, 1)).float().to(dev)
    embed = embed or (lambda picks, t0: synthetic.make_slice_mask(geom, picks, t0))
    drop_last = step_size == "half"
    asc = is_ascending(tsteps_abs)
    used = []
    with torch.no_grad():
        for t0 in times:
            sel = (P[:, 0] > t0 - 2.0 * synthetic.KERNEL_SIG_T) & (P[:, 0] < t0 + max_t + 2.0 * synthetic.KERNEL_SIG_T)  # process_utils.py:476
            if not sel.any():
                continue                                                      # process_continuous_days.py:792-793
            used.append(t0)
            Slice, Mask = embed(P[sel], t0)
            if not getattr(net, "use_phase_types", True):        # process_continuous_days.py:783-786
                Slice, Mask = np.array(Slice, copy=True), np.array(Mask, copy=True)
                Slice[:, 2:] = 0.0
                Mask[:, 2:] = 0.0
            y, x = net.forward_fixed_source(torch.from_numpy(Slice).to(dev), torch.from_numpy(Mask).to(dev), None, None, None,
                                            locs, xg, xq, tq)
            cols, keep = window_columns(tsteps_abs, t0, offsets, drop_last, asc)
            Out_2.index_add_(1, torch.from_numpy(cols).to(dev), x[:, torch.from_numpy(keep).to(dev), 0] / (n_overlap * n_grids))
    return Out_2, np.asarray(used)


def apply_windows_device(net, geom, P, trv_times, tsteps_abs=None, t_win=6.0, step_size="half", min_required_picks=1,
                         n_grids=1.0, day_len=86400.0, kernel_sig_t=synthetic.KERNEL_SIG_T, dt_embed=None, max_t=None,
                         times=None, tail_batch=16, pairs=None, stack_on_device=False, window_parallel=None, return_info=False,
                         merge_timeout=60.0, merge="dense"):
    """GPU-only apply loop: `P` [n,5] (t, station index in the model's station order, amp, prob, phase) sorted by time,
    `trv_times` [G, S, 2] theoretical travel times; `pairs` [2, N] (station, source) = the product nodes of a `use_subgraph` model
    (`A_src_in_sta`), whose Slice / Mask rows follow that list. Returns (Out_2 on device, window start times used). `tail_batch`: windows
    per G-sized tail (1..16; 16 is the default of the bench and measured best with the device embedding in the loop, bench.py --mode
    stream: the tail kernels are latency-bound, their fixed costs are paid once per batch).

    `stack_on_device`: accumulate into `Out_2` with ONE `genie_stack_windows_legs` launch per flush (per window when `window_batch == 1`)
    instead of a slice, a scaling and an `index_add_` per window; same stacker stream, same summation order, bit-equal `Out_2`. The loop
    is the one of `apply_windows_legs` (`_run_day`), of which this is the one-grid case: the torch statements stay as the reference the
    kernel is held against.

    `window_parallel`: split the day's windows over GPUs. `(rank, world)`, or a `torch.distributed`
    process group (True: the default group). After all filters, rank r takes the contiguous block `window_blocks(len(times), world)[r]`
    of the final `times` and stacks it (on the device: `stack_on_device` is implied) into a zero-initialised full-size `Out_2`.
    * tuple form: no collective; returns (this rank's partial `Out_2`, this rank's `times`) -- for a caller with its own transport.
    * group form: one `all_reduce(SUM)` of the partials (in place on the device over "nccl"; staged through the host over gloo, where
      the wait ends after `merge_timeout` seconds; an RCCL group carries the finite timeout it was initialised with); every rank returns
      the full `Out_2` and the full `times`.
    Against one GPU the merged `Out_2` is bit-equal in every column fed by one rank's windows only; in a column at a block boundary it is
    `fl(prefix) + fl(suffix)` of that column's window contributions instead of one running sum, a difference of rounding only. With
    step_size 'half' or 'full' on the default schedule a column has at most two contributions, so the whole `Out_2` is bit-equal.
    `return_info`: a third return value, `window_parallel_info` of this run plus `rank` (its `exact_merge` tells whether the merged
    bits are independent of the collective's reduction order). A source-sharded model cannot be combined with `window_parallel`.
    No multi-GPU speed-up has been measured: ranks sharing one GPU say nothing about it, and the first run on N > 1 GPUs is still ahead
    (DESIGN.md section 9.1).

    `merge`: "dense" (the default) is everything above. "columns" (needs `window_parallel`, an ascending `tsteps_abs` and ascending
    `times`) keeps `Out_2` distributed: the rank allocates and stacks into its column band [Q, b_hi - b_lo] of `window_band_plan` only
    (the column table shifted by b_lo on the host, the stacking kernel unchanged), and the first return value is a `BandedOut2`.
    * tuple form: nothing is exchanged; the band holds this rank's windows (`complete` False), the plan lists the strips to exchange.
    * group form: after the day's one synchronisation the strips of the plan travel once, device to device over "nccl", staged
      through the host over gloo (`merge_timeout`), and are added in ascending rank order (`BandedOut2.add_strips`): every rank's band
      then holds the full sums of its columns, a fixed function of the ranks' partials that equals the dense all-reduce wherever
      `exact_merge` holds. `postproc.detect_sources_banded` (or `detect_refine_associate`) takes the `BandedOut2` from there.
    Not yet run on hardware: the device-to-device strip exchange between two or more GPUs (`batch_isend_irecv` over RCCL). What has run
    is the exchange over gloo between processes sharing one GPU and a one-rank RCCL group, which exchanges nothing."""
    sharded = getattr(net, "is_sharded", False)       # source-node-sharded model: this rank embeds and runs its owned + halo rows only;
    wp = _rank_split(window_parallel, "window_parallel", sharded)
    net.window_batch = 1 if sharded else tail_batch   # the tail follows the shard's all-gather, one per window (module.py docstring)
    max_t = float(max_t if max_t is not None else np.ceil(trv_times.max() + 1.0))
    dt_embed = _dt_embed(kernel_sig_t, dt_embed)
    Ps = P[np.argsort(P[:, 0], kind="stable")]
    plan = _day_plan(Ps[:, 0], max_t, day_len, t_win, step_size, min_required_picks, tsteps_abs, times, kernel_sig_t, n_grids, wp,
                     return_info, merge)              # (host only: a bad schedule argument raises before anything is uploaded)
    lane = GridLeg(net, geom.x_grid, trv_times, pairs=pairs)
    dev = lane.device
    ph = Ps[:, 4].astype(np.int32)
    if not getattr(net, "use_phase_types", True):        # process_continuous_days.py:562-563 (the embedding zeroes columns 2, 3: :783-786)
        ph = np.zeros_like(ph)
    picks = types.SimpleNamespace(t_host=Ps[:, 0], t=torch.from_numpy(Ps[:, 0].copy()).to(dev),
                                  sta=torch.from_numpy(Ps[:, 1].astype(np.int32)).to(dev), phase=torch.from_numpy(ph).to(dev))
    Out_2 = torch.zeros((geom.x_query.shape[0], plan.width), dtype=torch.float32, device=dev)
    xq = torch.from_numpy(geom.x_query).float().to(dev)
    add = _fused_add(plan, Out_2) if stack_on_device or wp is not None else _torch_add(plan, Out_2)
    return _run_day(plan, [lane], picks, xq, Out_2, add, dt_embed, merge_timeout)


_DayPlan = collections.namedtuple(
    "_DayPlan", "tsteps_abs offsets times lo hi all_times drop_last h_cols divisor scale info max_t kernel_sig_t split bands width")


def _day_plan(t_sorted, max_t, day_len, t_win, step_size, min_required_picks, tsteps_abs, times, kernel_sig_t, n_grids, split, return_info,
              merge="dense"):
    """What a day's apply loop knows before its first launch, host arithmetic on small arrays: the schedule (`_day_schedule` of the
    time-sorted pick times `t_sorted`, or the caller's `tsteps_abs` / `times`); per kept window the range [lo, hi) of the picks its
    embedding reads (a window whose range is empty is dropped); this rank's block of them under `split` (a `_RankSplit` or None;
    `all_times`: every rank's); `h_cols` = the block's `window_cols_table` (-1: an offset that adds nothing), of which a flush takes its
    rows; `divisor` = n_overlap * `n_grids` and `scale`, its fp32 reciprocal; `info` (`return_info`) = `window_parallel_info` plus
    `rank`. `merge` "columns": `bands` = `window_band_plan` of all windows, `width` = this rank's band (otherwise None and the
    whole axis) and `h_cols` counts from the band's first column, so that the loop stacks into the band as it would into `Out_2`."""
    if merge not in ("dense", "columns"):
        raise ValueError('merge must be "dense" or "columns"')
    if merge == "columns" and split is None:
        raise ValueError('merge="columns" splits Out_2 over the ranks of window_parallel: pass window_parallel=')
    tsteps_abs, times, offsets, n_overlap = _day_schedule(t_sorted.reshape(-1, 1), max_t, day_len, t_win, step_size, min_required_picks,
                                                          tsteps_abs, times)
    drop_last = step_size == "half"
    lo, hi = _embed_ranges(t_sorted, times, max_t, kernel_sig_t)
    nonempty = hi > lo                                                                             # process_continuous_days.py:792-793
    times, lo, hi = times[nonempty], lo[nonempty], hi[nonempty]
    asc = is_ascending(tsteps_abs)
    all_times, info, bands, width = times, None, None, len(tsteps_abs)
    if return_info or merge == "columns":               # (the table of ALL windows: a rank's loop needs its own block's rows only)
        rank, world = (split.rank, split.world) if split is not None else (0, 1)
        table = window_cols_table(tsteps_abs, times, offsets, drop_last, asc)
        if return_info:
            info = dict(window_parallel_info(table, len(tsteps_abs), world), rank=rank)
        if merge == "columns":
            bands = window_band_plan(table, len(tsteps_abs), world, tsteps_abs=tsteps_abs, times=times)
            width = bands["band"][rank][1] - bands["band"][rank][0]
    if split is not None:                               # this rank's contiguous block of the final window list
        b_lo, b_hi = window_blocks(len(times), split.world)[split.rank]
        times, lo, hi = times[b_lo:b_hi], lo[b_lo:b_hi], hi[b_lo:b_hi]
    h_cols = window_cols_table(tsteps_abs, times, offsets, drop_last, asc)
    if bands is not None:
        h_cols = np.where(h_cols >= 0, h_cols - bands["band"][split.rank][0], -1).astype(np.int32)
    divisor, scale = _stack_scale(n_overlap, n_grids)
    return _DayPlan(tsteps_abs, offsets, times, lo, hi, all_times, drop_last, h_cols, divisor, scale, info, max_t, kernel_sig_t, split, bands,
                    width)


def _embed_ranges(t_sorted, times, max_t, kernel_sig_t):
    """(lo, hi): per window start of `times` the range [lo, hi) of the time-sorted picks `t_sorted` its embedding reads."""
    lo = np.searchsorted(t_sorted, times - 2.0 * kernel_sig_t, side="right")                      # strict >, process_utils.py:476
    hi = np.searchsorted(t_sorted, times + max_t + 2.0 * kernel_sig_t, side="left")               # strict <
    return lo, hi


def _stack_scale(n_overlap, n_grids):
    """(divisor, scale) of a day's stacking: `n_overlap * n_grids` and its fp32 reciprocal."""
    divisor = n_overlap * n_grids
    return divisor, float(np.float32(1.0) / np.float32(divisor))       # `tensor / host scalar` in torch: times the fp32 reciprocal


def _fused_add(plan, Out_2):
    """`add(xs, first, n)` of `_run_day`: ONE `genie_stack_windows_legs` launch for the read-outs `xs` (one per lane) of windows first ..
    first + n - 1, over their rows of the column table."""
    d_cols = torch.from_numpy(plan.h_cols).to(Out_2.device)

    def add(xs, first, n):
        used = plan.h_cols[first:first + n]
        used = used[used >= 0]
        if used.size:
            engine.stack_windows_legs(Out_2, xs, d_cols[first:first + n], plan.scale, int(used.min()), int(used.max()))
    return add


def _torch_add(plan, Out_2):
    """`add(xs, first, n)` of `_run_day` in torch statements, the reference of the fused one (one lane): per window a slice, a scaling
    and an `index_add_`; a gather instead of the slice only for a window that lists a column twice."""
    n_off = plan.h_cols.shape[1] - (1 if plan.drop_last else 0)
    keeps = None
    if (plan.h_cols[:, :n_off] >= 0).all():                # the usual case: no duplicate column inside a window
        cols = torch.from_numpy(plan.h_cols[:, :n_off].astype(np.int64)).to(Out_2.device)
    else:
        cols = [torch.from_numpy(row[row >= 0].astype(np.int64)).to(Out_2.device) for row in plan.h_cols]
        keeps = [torch.from_numpy(np.flatnonzero(row >= 0)).to(Out_2.device) for row in plan.h_cols]

    def add(xs, first, n):
        (x,) = xs                                          # [n, Q, T, 1]
        for k in range(n):
            w = first + k
            vals = x[k][:, keeps[w], 0] if keeps is not None else (x[k][:, :-1, 0] if plan.drop_last else x[k][:, :, 0])
            Out_2.index_add_(1, cols[w], vals / plan.divisor)
    return add


class _WindowBody(object):
    """The per-window body of the day loops, shared by `_run_day` (a whole day, planned up front) and `OnlineDay.feed` (the windows that
    became ready): `lanes`: one per source grid, each with `net`, `x_grid_cart` and `trv` (a `GridLeg`), all with the same `window_batch`.
    `window` makes every lane, in lane order, embed one window and run its P-sized part (`push_window`), or the whole window with a tail
    of its own when `window_batch` is 1 (`forward_fixed_source_pipelined`: a source-node-sharded model among them), and returns the number
    of windows pending; `flush` runs every lane's tail on a side stream of its own (`flush_windows`) and hands `add(xs)` the lanes'
    read-outs `xs` of the pending windows on the one stacker stream: behind each tail's `done` event, and every flush behind the one
    before it (overlapping columns: a fixed summation order). `join` puts the main stream behind all of it; nothing here waits for the
    host. Construct and use it under `torch.no_grad()` with `xq`'s device current."""

    def __init__(self, lanes, xq, offsets, max_t, kernel_sig_t, dt_embed):
        dev = xq.device
        self.lanes, self.xq, self.max_t, self.kernel_sig_t, self.dt_embed = lanes, xq, max_t, kernel_sig_t, dt_embed
        self.tq = torch.from_numpy(offsets.reshape(-1, 1)).float().to(dev)
        self.batch = lanes[0].net.window_batch
        self.main = torch.cuda.current_stream(dev)
        self.stacker = torch.cuda.Stream(device=dev)      # every flush's stack runs here, so each one is behind the one before it
        self.stacker.wait_stream(self.main)               # Out_2's zeros and the tables
        self.xs = None

    def _on_stacker(self, x, done):                       # a lane's read-out, produced on its side stream, made known to the stacker
        self.stacker.wait_event(done)
        x.record_stream(self.stacker)
        return x

    def window(self, picks, t0, a, b):
        if self.batch == 1:
            self.xs = []
        for lane in self.lanes:
            Slice, Mask = lane.net.embed_window(picks.t[a:b], picks.sta[a:b], picks.phase[a:b], float(t0), self.max_t, self.kernel_sig_t,
                                                self.dt_embed, lane.trv, presplit=True)    # the call below is the only consumer of (Slice, Mask)
            if self.batch == 1:                       # one tail per window: the batch of one (a view, no launch)
                _, x, done = lane.net.forward_fixed_source_pipelined(Slice, Mask, None, None, None, None, lane.x_grid_cart, self.xq, self.tq)
                self.xs.append(self._on_stacker(x.unsqueeze(0), done))
                pending = 1
            else:
                pending = lane.net.push_window(Slice, Mask)
        return pending

    def flush(self, add):
        xs = self.xs
        if self.batch > 1:
            # every lane's tail + read-outs of the pushed windows in one set of launches, each on a side stream of its own
            xs = [self._on_stacker(*lane.net.flush_windows(lane.x_grid_cart, self.xq, self.tq)[1:]) for lane in self.lanes]
        self.xs = None
        with torch.cuda.stream(self.stacker):
            add(xs)

    def join(self):
        for lane in self.lanes:
            lane.net._hip.wait_tails()
        self.main.wait_stream(self.stacker)


def _run_day(plan, lanes, picks, xq, Out_2, add, dt_embed, merge_timeout):
    """The day's loop over the windows of `plan`: per window, in window order, the body of `_WindowBody` on `picks` (the time-sorted picks
    on the device: `t_host`, `t`, `sta`, `phase`: a `ResidentPicks`); when `window_batch` windows are pending, or at the last one, the
    flush, whose `add(xs, first, n)` puts the lanes' read-outs `xs` of windows first .. first + n - 1 into `Out_2`. Nothing waits for
    the host until the end: one synchronisation per day, then the verdicts of every lane and, in the group form of the plan's rank
    split, the merge. Returns (Out_2, times used[, info])."""
    dev = Out_2.device
    times = plan.times
    with torch.no_grad(), torch.cuda.device(dev):
        body = _WindowBody(lanes, xq, plan.offsets, plan.max_t, plan.kernel_sig_t, dt_embed)
        first = 0
        for w, t0 in enumerate(times):
            pending = body.window(picks, t0, int(plan.lo[w]), int(plan.hi[w]))
            if pending != body.batch and w != len(times) - 1:
                continue
            body.flush(lambda xs: add(xs, first, w + 1 - first))
            first = w + 1
        body.join()
    body.main.synchronize()                           # the verdicts of the day's last windows: one wait per day
    for lane in lanes:
        _check_verdicts(lane.net)
    split = plan.split
    if plan.bands is not None:                        # merge="columns": the band stays where it is; only the strips travel
        group = (True if split.group is None else split.group) if split.collective else None      # (True: the default group)
        Out_2 = BandedOut2(Out_2, split.rank, plan.bands, group=group, timeout=merge_timeout)
        if split.collective:
            Out_2.add_strips(_exchange_strips(Out_2, split.group, merge_timeout))
            times = plan.all_times
    elif split is not None and split.collective:      # group form: one all-reduce of the ranks' partials; every rank gets the day
        _merge_partials(Out_2, split.group, merge_timeout)
        times = plan.all_times
    return (Out_2, times) if plan.info is None else (Out_2, times, plan.info)


def _exchange_strips(banded, group, timeout):
    """{peer: strip} for `BandedOut2.add_strips`: this rank's `send` strips of the band plan go out and its `recv` strips come in, one
    message per (sender, receiver) pair -- device to device over RCCL ("nccl", one batch of point-to-point operations), staged through
    host memory over gloo, where every wait ends after `timeout` seconds, as `_merge_partials` stages its all-reduce."""
    import datetime
    import torch.distributed as dist
    recv, send = banded.plan["recv"][banded.rank], banded.plan["send"][banded.rank]
    on_device = dist.get_backend(group) == "nccl"
    where = banded.band.device if on_device else torch.device("cpu")
    rows = banded.band.shape[0]
    peer_rank = lambda p: dist.get_global_rank(group, p) if group is not None else p
    inbox = {p: torch.empty((rows, c_hi - c_lo), dtype=banded.band.dtype, device=where) for p, c_lo, c_hi in recv}
    outbox = [(p, banded.strip(c_lo, c_hi).contiguous().to(where)) for p, c_lo, c_hi in send]
    if on_device:
        ops = [dist.P2POp(dist.irecv, inbox[p], peer_rank(p), group) for p, _, _ in recv]
        ops += [dist.P2POp(dist.isend, t, peer_rank(p), group) for p, t in outbox]
        for work in (dist.batch_isend_irecv(ops) if ops else []):
            work.wait()
        return inbox
    works = [dist.irecv(inbox[p], src=peer_rank(p), group=group) for p, _, _ in recv]
    works += [dist.isend(t, dst=peer_rank(p), group=group) for p, t in outbox]
    for work in works:
        work.wait(datetime.timedelta(seconds=float(timeout)))
    return {p: t.to(banded.band.device) for p, t in inbox.items()}


def _merge_partials(Out_2, group, timeout):
    """`Out_2` <- sum over the ranks of `group` of their `Out_2`: in place on the device over RCCL ("nccl"), through host memory for a
    group without device collectives (gloo), as `dist.Transport` stages its collectives; that wait ends after `timeout` seconds."""
    import datetime
    import torch.distributed as dist
    if dist.get_backend(group) == "nccl":
        dist.all_reduce(Out_2, op=dist.ReduceOp.SUM, group=group)
        return
    h = Out_2.cpu()
    work = dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group, async_op=True)
    work.wait(datetime.timedelta(seconds=float(timeout)))
    Out_2.copy_(h)


# ---- per-window pick lists (process_utils.py:644-699) and the two other per-day loops of the caller ------------------------------------

class ResidentPicks(object):
    """The picks of a day resident on one device, in the form every per-window step of the caller needs.

    `P` [n, 5] float64 (t, ABSOLUTE station index, amp, prob, phase) in the caller's order (`load_picks`, utils.py:983: the pick file's
    order, not a time order); `ind_use` = the stations of the model, positions into the absolute station set of `n_sta_all` entries
    (`perm_vec`, process_utils.py:486-487 / :678-679). Kept here: the picks of those stations (the reference drops the others per
    window, :480-483 and :684 -- the filter does not depend on the window), stable-sorted by time, so that
      * the picks a window's embedding reads, `t0 - 2 sigma < t < t0 + max_t + 2 sigma` (:476), are ONE contiguous range `embed_range`
        found by two binary searches on a host copy of the times -- the tensors handed to `genie_embed_window` are views, and
      * the lists `forward_fixed` consumes (`extract_pick_inputs_from_data`, :644-699) are that range cut by the ball query (:665) and
        stable-sorted by station on the device: `np.lexsort((times, indices))` (:690) orders by station, then time, ties in the
        caller's order, which a stable sort by station of a stable time order reproduces exactly.
    Works on CPU tensors too (the CPU tests pin it to the reference's fixtures); nothing here touches the HIP library."""

    def __init__(self, P, ind_use, n_sta_all, device, use_phase_types=True):
        P = np.asarray(P, dtype=np.float64)
        ind_use = np.asarray(ind_use).astype(np.int64)
        perm_vec = -np.ones(int(n_sta_all), dtype=np.int64)
        perm_vec[ind_use] = np.arange(len(ind_use))
        sta = perm_vec[P[:, 1].astype(np.int64)]
        keep = np.nonzero(sta > -1)[0]
        keep = keep[np.argsort(P[keep, 0], kind="stable")]
        self.P = P
        self.index_host = keep                                   # rows of the caller's P, in this object's (time) order
        self.t_host = np.ascontiguousarray(P[keep, 0])
        self.device = torch.device(device)
        self.n_sta = int(len(ind_use))
        ph = P[keep, 4].copy()
        if not use_phase_types:                                  # process_continuous_days.py:562-563
            ph[:] = 0.0
        self.t = torch.from_numpy(self.t_host).to(self.device)
        self.sta = torch.from_numpy(sta[keep].astype(np.int32)).to(self.device)
        self.phase = torch.from_numpy(ph.astype(np.int32)).to(self.device)
        self.phase_f = torch.from_numpy(ph).to(self.device)
        self.index = torch.from_numpy(keep).to(self.device)

    def __len__(self):
        return int(self.t_host.shape[0])

    def embed_range(self, t0, max_t, kernel_sig_t):
        """[lo, hi) of the picks with `t0 - 2 sigma < t < t0 + max_t + 2 sigma` (strict, process_utils.py:476)."""
        return picks_in_embed_range(self.t_host, float(t0), float(max_t), float(kernel_sig_t))

    def embed_args(self, t0, max_t, kernel_sig_t):
        """(pick_t float64, pick_sta int32, pick_phase int32) views for `HipPath.embed_window`, or None for an empty range."""
        lo, hi = self.embed_range(t0, max_t, kernel_sig_t)
        if hi <= lo:
            return None
        return self.t[lo:hi], self.sta[lo:hi], self.phase[lo:hi]

    def pick_inputs(self, t0, max_t, kernel_sig_t, t_win=10.0):
        """`lp_times, lp_stations, lp_phases` of `extract_input_from_data(...)[1]` for the window starting at `t0`
        (process_utils.py:637 -> :644-699) as device tensors (float64 [m], int64 [m], float64 [m]) plus `index` int64 [m]: the rows of
        the caller's `P` they come from (`lp_meta = P[index]`). The ball query of :665 keeps `|t - (t0 + max_t / 2)| <= t_win + max_t / 2`
        of the window's slice; with `2 sigma <= t_win` that is all of it."""
        lo, hi = self.embed_range(t0, max_t, kernel_sig_t)
        t, sta, ph, idx = self.t[lo:hi], self.sta[lo:hi], self.phase_f[lo:hi], self.index[lo:hi]
        if 2.0 * float(kernel_sig_t) > float(t_win) and hi > lo:
            inside = (t - (float(t0) + float(max_t) / 2.0)).abs() <= (float(t_win) + float(max_t) / 2.0)
            t, sta, ph, idx = t[inside], sta[inside], ph[inside], idx[inside]
        order = torch.sort(sta, stable=True)[1]
        return t[order] - float(t0), sta[order].long(), ph[order], idx[order]

    def pick_inputs_device(self, t0, max_t, kernel_sig_t, t_win=10.0):
        """`pick_inputs` in one launch (genie_pick_lists through `engine.pick_lists`: ball query, counting sort by station and the four
        lists in one workgroup) instead of a slice, a mask, a `torch.sort`, four gathers and a subtraction: the same four tensors, bit
        for bit -- `pick_inputs` is its oracle. The number of kept picks is counted on the host from `t_host` with the ball query's own
        float64 arithmetic, so nothing here waits for the device. A GPU store only; a station set too large for the kernel's LDS
        table (`engine.pick_lists_max_sta()`) goes through `pick_inputs`."""
        if self.device.type != "cuda":
            raise ValueError("pick_inputs_device: the picks live on %s (pick_inputs runs anywhere)" % (self.device,))
        lo, hi = self.embed_range(t0, max_t, kernel_sig_t)
        if hi <= lo:
            f, i = (torch.empty(0, dtype=dt, device=self.device) for dt in (torch.float64, torch.int64))
            return f, i, f.clone(), i.clone()
        ball, m = None, hi - lo
        if 2.0 * float(kernel_sig_t) > float(t_win):
            ball = (float(t0) + float(max_t) / 2.0, float(t_win) + float(max_t) / 2.0)
            m = int(np.count_nonzero(np.abs(self.t_host[lo:hi] - ball[0]) <= ball[1]))
        out = engine.pick_lists((self.t[lo:hi], self.sta[lo:hi], self.phase[lo:hi], self.index[lo:hi]), self.n_sta, float(t0), ball)
        if out is None:
            return self.pick_inputs(t0, max_t, kernel_sig_t, t_win)
        return out[0][:m], out[1][:m], out[2][:m], out[3][:m]

    def meta(self, index):
        """`lp_meta` rows (host float64 [m, 5]) of a `pick_inputs` index."""
        return self.P[index.cpu().numpy()]


def merge_ranks(t_a, t_b):
    """(pos_a, pos_b): where the elements of two ascending runs land in their stable merge with `t_a` first among equal times -- element
    i of `t_a` moves up by the number of `t_b` entries strictly earlier, element j of `t_b` lands after every `t_a` entry <= it. The rule
    of genie_picks_merge, on numpy arrays or CPU tensors."""
    if torch.is_tensor(t_a):
        return (torch.arange(t_a.shape[0]) + torch.searchsorted(t_b, t_a, right=False),
                torch.arange(t_b.shape[0]) + torch.searchsorted(t_a, t_b, right=True))
    return np.arange(len(t_a)) + np.searchsorted(t_b, t_a, side="left"), np.arange(len(t_b)) + np.searchsorted(t_a, t_b, side="right")


class PickStore(ResidentPicks):
    """A `ResidentPicks` that grows: the picks of a live feed, time-sorted on one device, with the same views (`t`, `sta`, `phase`,
    `phase_f`, `index`, `t_host`) and methods (`embed_range`, `embed_args`, `pick_inputs`, `meta`), plus `append(P_chunk)`, `trim` and
    `frozen_t`. After any sequence of appends the stored order is the one of `ResidentPicks(np.concatenate(chunks), ...)`: a stable sort by
    time, ties in feed order; `index` counts rows of that concatenation (every row fed, kept or not).

    `append` stable-sorts the chunk on the host (chunks are small) and uploads it. A chunk that starts no earlier than the resident tail
    is copied onto the end; any other is merged by rank into a second buffer (genie_picks_merge on a GPU, one launch for the four
    arrays; `merge_ranks` in torch on a CPU store, where the tests pin the order). Capacity doubles on demand (allocate, copy, swap),
    so THE VIEWS ARE VALID UNTIL THE NEXT `append` ONLY: take them again after it. `trim(t_before)` forgets every pick with
    `t <= t_before` by moving an offset; `embed_range` and all views count from it, and once it passes half the capacity the next append
    compacts. The host keeps `t_host` (the binary searches run on it) and the fed rows of the live picks (`meta`) in step.
    `frozen_t`: `append` refuses a pick of the model's stations with `t < frozen_t` -- a window that has already run would have read
    it -- with a ValueError that names both and leaves the store as it was; with `late="drop"` such picks are left out (they still count
    in `index`) and `append` returns how many. `phase_f` is `phase` as float64: phase labels are whole numbers (0 = P, 1 = S).
    `state_dict()` / `load_state_dict(state)`: the live picks, `n_fed` and `frozen_t` as host arrays, into a new store of the same stations."""

    def __init__(self, ind_use, n_sta_all, device, use_phase_types=True, capacity=4096):
        ind_use = np.asarray(ind_use).astype(np.int64)
        self._perm = -np.ones(int(n_sta_all), dtype=np.int64)
        self._perm[ind_use] = np.arange(len(ind_use))
        self.device = torch.device(device)
        self.n_sta = int(len(ind_use))
        self.use_phase_types = bool(use_phase_types)
        self.frozen_t = -np.inf
        self.n_fed = 0                          # rows fed so far: the next chunk's first `index`
        self._base = self._n = 0                # the live picks are [base, n) of the buffers
        self._dev = self._device_buffers(max(1, int(capacity)))
        self._host = self._host_buffers(max(1, int(capacity)))

    def _device_buffers(self, cap):
        return tuple(torch.empty(cap, dtype=dtype, device=self.device) for _, dtype in engine.PICK_FIELDS)

    @staticmethod
    def _host_buffers(cap):
        return np.empty(cap, dtype=np.float64), np.empty((cap, 5), dtype=np.float64), np.empty(cap, dtype=np.int64)

    capacity = property(lambda self: int(self._host[0].shape[0]))
    t = property(lambda self: self._dev[0][self._base:self._n])
    sta = property(lambda self: self._dev[1][self._base:self._n])
    phase = property(lambda self: self._dev[2][self._base:self._n])
    index = property(lambda self: self._dev[3][self._base:self._n])
    phase_f = property(lambda self: self.phase.double())
    t_host = property(lambda self: self._host[0][self._base:self._n])
    index_host = property(lambda self: self._host[2][self._base:self._n])

    def meta(self, index):
        """`lp_meta` rows (host float64 [m, 5]) of a `pick_inputs` index, among the live picks (a trimmed pick raises KeyError)."""
        index = np.asarray(index.cpu() if torch.is_tensor(index) else index, dtype=np.int64)
        live = self.index_host
        order = np.argsort(live, kind="stable")
        at = np.clip(np.searchsorted(live[order], index), 0, max(len(live) - 1, 0))
        if index.size and (len(live) == 0 or not np.array_equal(live[order[at]], index)):
            raise KeyError("PickStore.meta: a pick of the index has been trimmed")
        return self._host[1][self._base:self._n][order[at]] if index.size else np.zeros((0, 5))

    def trim(self, t_before):
        """Forget every pick with `t <= t_before` (an offset moves; the memory is reclaimed by a later append). Returns the live count."""
        self._base += int(np.searchsorted(self.t_host, float(t_before), side="right"))
        return len(self)

    def append(self, P_chunk, late="raise"):
        """Add the rows `P_chunk` [m, 5] float64 (t, ABSOLUTE station index, amp, prob, phase), in the caller's order. Returns the
        number of picks dropped as late (always 0 with `late="raise"`, which raises ValueError instead and changes nothing)."""
        if late not in ("raise", "drop"):
            raise ValueError('PickStore.append: late must be "raise" or "drop"')
        P = np.asarray(P_chunk, dtype=np.float64).reshape(-1, 5)
        sta = self._perm[P[:, 1].astype(np.int64)]
        keep = np.nonzero(sta > -1)[0]
        too_late = P[keep, 0] < self.frozen_t
        dropped = int(too_late.sum())
        if dropped and late == "raise":
            raise ValueError("PickStore.append: a pick at t = %r is earlier than frozen_t = %r (a window that has run would have read it)"
                             % (float(P[keep[too_late], 0].min()), float(self.frozen_t)))
        keep = keep[~too_late]
        keep = keep[np.argsort(P[keep, 0], kind="stable")]
        m, live = len(keep), len(self)
        ph = P[keep, 4] if self.use_phase_types else np.zeros(m)                  # process_continuous_days.py:562-563
        h_chunk = (np.ascontiguousarray(P[keep, 0]), P[keep], self.n_fed + keep)
        self.n_fed += P.shape[0]
        if m == 0:
            return dropped
        d_chunk = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(self.device) for x in
                        (h_chunk[0], sta[keep].astype(np.int32), ph.astype(np.int32), h_chunk[2]))
        in_order = live == 0 or h_chunk[0][0] >= self._host[0][self._n - 1]
        if in_order and self._n + m <= self.capacity and 2 * self._base <= self.capacity:
            lo, hi = self._n, self._n + m                                          # onto the end, in place
            for buf, x in zip(self._dev + self._host, d_chunk + h_chunk):
                buf[lo:hi] = x
            self._n = hi
            return dropped
        cap = self.capacity                                                        # a second buffer: grown, compacted, or the merge's target
        while cap < live + m:
            cap *= 2
        dev, host = self._device_buffers(cap), self._host_buffers(cap)
        pos_a, pos_b = merge_ranks(self.t_host, h_chunk[0])
        for new, old, x in zip(host, self._host, h_chunk):
            new[pos_a], new[pos_b] = old[self._base:self._n], x
        if in_order:
            for new, old, x in zip(dev, self._dev, d_chunk):
                new[:live], new[live:live + m] = old[self._base:self._n], x
        elif self.device.type == "cuda":
            engine.picks_merge((self.t, self.sta, self.phase, self.index), d_chunk, tuple(x[:live + m] for x in dev))
        else:
            t_pos_a, t_pos_b = merge_ranks(self.t, d_chunk[0])
            for new, old, x in zip(dev, self._dev, d_chunk):
                new[t_pos_a], new[t_pos_b] = old[self._base:self._n], x
        self._dev, self._host, self._base, self._n = dev, host, 0, live + m
        return dropped

    def _fingerprint(self):
        return {"station_map": self._perm, "use_phase_types": self.use_phase_types}

    def state_dict(self):
        """What `append` and `trim` have made of the store, on the host: the live picks (their times, fed rows and `index`), `n_fed` and
        `frozen_t`, with the station map as fingerprint. A trimmed pick is not saved: the trim offset is how this object forgets, not
        something a reader can see. The device arrays are functions of the saved rows and are made again on load, as `append` makes them."""
        return {"fingerprint": checkpoint.to_host(self._fingerprint()), "frozen_t": float(self.frozen_t), "n_fed": int(self.n_fed),
                "t": self.t_host.copy(), "rows": self._host[1][self._base:self._n].copy(), "index": self.index_host.copy()}

    def _check_state(self, state):
        if self.n_fed or self._n:
            raise RuntimeError("PickStore.load_state_dict: this store has been fed; a state is loaded into a new one")
        checkpoint.check_fingerprint("PickStore", state, self._fingerprint())
        t, rows, index = (np.asarray(state[k]) for k in ("t", "rows", "index"))
        if not (t.dtype == np.float64 and index.dtype == np.int64 and t.ndim == 1 and rows.shape == (len(t), 5) and index.shape == t.shape
                and is_ascending(t)):
            raise ValueError("PickStore.load_state_dict: the saved picks are not a time-sorted run (t [n], rows [n, 5], index [n])")

    def load_state_dict(self, state):
        """Into a store nothing has been fed to (RuntimeError otherwise), built with the same stations (ValueError naming the field
        otherwise, nothing changed): the views `t`, `sta`, `phase`, `index`, `t_host`, and `meta`, `frozen_t` and the next `index` are
        those of the saved store, bit for bit; the picks sit at the start of the buffers, as after a compacting `append`."""
        self._check_state(state)
        t, rows, index = (np.ascontiguousarray(state[k]) for k in ("t", "rows", "index"))
        live, cap = len(t), self.capacity
        while cap < live:
            cap *= 2
        sta = self._perm[rows[:, 1].astype(np.int64)]
        ph = rows[:, 4] if self.use_phase_types else np.zeros(live)
        dev, host = self._device_buffers(cap), self._host_buffers(cap)
        for buf, x in zip(dev + host, (t, sta.astype(np.int32), ph.astype(np.int32), index, t, rows, index)):
            buf[:live] = torch.from_numpy(np.ascontiguousarray(x)).to(self.device) if torch.is_tensor(buf) else x
        self._dev, self._host, self._base, self._n = dev, host, 0, live
        self.n_fed, self.frozen_t = int(state["n_fed"]), float(state["frozen_t"])


class GridLeg(object):
    """One source grid of the per-day loops (`x_grid_ind` of process_continuous_days.py:770, :950, :1020): the model whose adjacencies were
    set on that grid, the grid's Cartesian node positions and its travel-time table `x_grids_trv[x_grid_ind]` [G, S, 2] resident on the
    device ([N, 2] rows per listed product node for a `use_subgraph` model: `pairs` [2, N] = `A_src_in_sta`)."""

    def __init__(self, net, x_grid_cart, trv_times, pairs=None, ind_use=None, knn_index=False):
        """`knn_index`: SETS the model's attribute of that name, to False too -- with True the per-source passes' query clouds are
        searched through a cell index of this grid (`engine.KnnIndex`, built at the first cloud) instead of brute force, with bit-equal
        results. The switch lives on the model, not on the leg: a leg built with the default turns off a `net.knn_index = True` set
        before it, and of several legs that share one model the one built last decides.
        `trv_times` [G, S', 2]: with `ind_use` the reference's table over ALL stations (`compute_travel_times(trv, locs, ...)`), cut to
        the model's stations here as process_utils.py:599 does (`trv_times[:, ind_use]`); without it the table must already be restricted
        to the model's stations, in the model's station order (its station axis is checked against the model's station count)."""
        self.net = net
        hp = net._hip
        if hp is None:
            raise RuntimeError("GridLeg: call net.set_adjacencies*(...) first")
        net.knn_index = bool(knn_index)
        self.device = hp.device
        self.x_grid_cart = torch.as_tensor(x_grid_cart).float().to(self.device)
        trv_times = np.asarray(trv_times, dtype=np.float32)
        if ind_use is not None:
            trv_times = trv_times[:, np.asarray(ind_use).astype(np.int64)]
        n_sta = net._shard.n_sta if getattr(net, "_shard", None) is not None else hp.n_sta
        if trv_times.ndim != 3 or trv_times.shape[1] != n_sta or trv_times.shape[2] != 2:
            raise ValueError("GridLeg: trv_times must be [G, %d, 2] over the model's stations (pass ind_use= to cut the table of all "
                             "stations down, process_utils.py:599), got %s" % (n_sta, tuple(trv_times.shape)))
        self.n_sta = int(n_sta)
        if pairs is not None:
            pairs = np.asarray(pairs)
            # (a source-node shard of the irregular graph keeps its owned + halo rows only: cut once, not per window)
            self.trv = net.node_rows(torch.from_numpy(np.ascontiguousarray(trv_times[pairs[1], pairs[0]]).reshape(-1, 2)), 2)
        else:
            self.trv = net.node_rows(trv_times, 2)

    def check(self):
        """Raise what the device-side checks of the calls COMPLETED so far found (`HipPath.check_input_range` / `check_index_flags`);
        the per-day loops call it after their final copy to the host, which has waited for every window."""
        _check_verdicts(self.net)

    def embed(self, picks, t0, max_t, kernel_sig_t, dt):
        """(Slice, Mask) of the window starting at t0 (genie_embed_window = extract_input_from_data, process_utils.py:460-642), or None
        when no pick falls in the embedding range."""
        args = picks.embed_args(t0, max_t, kernel_sig_t)
        if args is None:
            return None
        return self.net.embed_window(args[0], args[1], args[2], float(t0), float(max_t), float(kernel_sig_t), float(dt), self.trv)


def _dt_embed(kernel_sig_t, dt_embed):
    return float(dt_embed if dt_embed is not None else np.round(kernel_sig_t / 10.0, 2))          # process_continuous_days.py:608


_pinned = threading.local()


def _pinned_pair(n, device):
    """Two page-locked float64 [n, 3] staging buffers per (size, device) of the calling thread, kept for the life of that thread (pinning
    2.7 MB costs ~20 ms: not per call). Thread-local, so that concurrent refine passes -- one per GPU, or one per thread -- never share a
    pair and a finished thread's buffers are released with it."""
    pairs = _pinned.__dict__.setdefault("pairs", {})
    key = (int(n), str(device))
    if key not in pairs:
        pairs[key] = [torch.empty((n, 3), dtype=torch.float64).pin_memory() for _ in range(2)]
    return pairs[key]


def _gather_blocks(rows, blocks, group, timeout):
    """The ranks' row blocks `rows` (device tensor [hi_r - lo_r, C] on rank r, `blocks` = every rank's (lo, hi)) put together on every
    rank: host float64 [n, C]. One all-gather of blocks padded to the longest (they differ by at most one row): on the device over RCCL
    ("nccl"), staged through the host over gloo, where the wait ends after `timeout` seconds -- as `_merge_partials` chooses."""
    import datetime
    import torch.distributed as dist
    b_max = max(hi - lo for lo, hi in blocks)
    on_device = dist.get_backend(group) == "nccl"
    mine = rows if on_device else rows.cpu()
    send = torch.zeros((b_max, rows.shape[1]), dtype=rows.dtype, device=mine.device)
    send[: mine.shape[0]] = mine
    parts = [torch.empty_like(send) for _ in blocks]
    if on_device:
        dist.all_gather(parts, send, group=group)
    else:
        dist.all_gather(parts, send, group=group, async_op=True).wait(datetime.timedelta(seconds=float(timeout)))
    return torch.cat([p[: hi - lo] for p, (lo, hi) in zip(parts, blocks)]).cpu().numpy()


class PhiloxCloud(object):
    """The draws of a refine pass as a pure function of (key, source index, element): `rand=PhiloxCloud(key)` of `refine_sources` /
    `detect_refine_associate`. Source i's draw is `np.random.Generator(np.random.Philox(key=key, counter=[0, i, 0, 0])).random((n, 3))`
    (Philox4x64-10, counter-based): `host(i, n)` makes exactly that with numpy, and with `ftrns2_device` the refine pass makes the same
    bits on the device where they are consumed (`postproc.refine_cloud_device`), identical on any rank and never drawn for a source the
    rank does not own. `key`: an int below 2**128 or a pair of 64-bit words, as numpy takes it. Nothing here is stateful: the same
    (key, source, n) gives the same draw whenever and wherever it is asked for."""

    def __init__(self, key):
        from . import postproc
        self.key = postproc.philox_key_words(key)

    def host(self, source, n):
        """Source number `source`'s draw, float64 [n, 3], on the host: the reference of the device draw and the host-cloud branch's draw."""
        bits = np.random.Philox(key=np.array(self.key, dtype=np.uint64), counter=np.array([0, int(source), 0, 0], dtype=np.uint64))
        return np.random.Generator(bits).random((int(n), 3))


def refined_from_found(found, srcs, tq, ftrns2):
    """The end of the refine pass on the host: `found` float64 [n, 7] = per source (query row, offset index, value, any query inside the
    region, the refined query's position, of which `ftrns2` makes the geographic one) as either branch of `refine_sources` leaves them
    (the rows of all ranks of a source-parallel pass laid side by side in source order) -> (srcs_refined [n, 5] sorted by origin time,
    `order`)."""
    srcs = np.asarray(srcs, dtype=np.float64)
    found = np.asarray(found, dtype=np.float64).reshape(-1, 7)
    tq_host = np.asarray(tq.detach().cpu() if torch.is_tensor(tq) else tq, dtype=np.float64).reshape(-1)
    out = np.zeros((srcs.shape[0], 5))
    for i in range(srcs.shape[0]):
        if found[i, 3] == 0.0:
            raise ValueError("refine_sources: no query of source %d lies inside the region (the reference's argmax raises here too)" % i)
        out[i, 0:3] = ftrns2(found[i, 4:7].reshape(1, 3))[0]
        out[i, 3] = srcs[i, 3] + tq_host[int(found[i, 1])]
        out[i, 4] = found[i, 2]
    order = np.argsort(out[:, 3])
    return out[order], order


def refine_sources(legs, picks, srcs, locs_cart, tq, max_t, X_offset_min, X_offset_range, n_rand_query, ftrns1, ftrns2,
                   lat_range, lon_range, depth_range, kernel_sig_t=synthetic.KERNEL_SIG_T, dt_embed=None, rand=None, ftrns2_device=None,
                   source_parallel=None, merge_timeout=60.0, source_offset=0, source_batch=1):
    """The refine pass of the caller (process_continuous_days.py:926-980) on the device: for every candidate source `srcs[i]` = (lat, lon,
    depth, origin time, value) a cloud of `n_rand_query` random queries around it (`ftrns1(src) + rand(n, 3) * X_offset_range +
    X_offset_min`, kept where `ftrns2` of it lies strictly inside the three ranges, :929-936), one `forward_fixed_source` per grid
    leg on the window that STARTS at the source's origin time, read out at those queries (:971-972; the kNN of the cloud into the grid
    by `genie_knn`), the clouds' outputs averaged over the legs, and the refined source = the query and time offset of the maximum
    (`argmax` of the row maxima, then of that row, :976-978: first maximum in both). Sources whose window holds no pick keep an all-zero
    read-out (:966-967), i.e. their first query and `tq[0]`. Returns (srcs_refined float64 [n, 5] sorted by origin time (:981-982),
    `order` = that sort's permutation of the input rows). `rand(n, 3)` defaults to `np.random.rand` (the reference's draw); the
    per-source results stay on the device until one copy at the end; `rand=PhiloxCloud(key)` is the keyed, source-indexed draw described
    under `source_parallel` below. `ftrns2_device`: the inverse transform as a function of a float64
    GPU tensor [n, 3] (the reference also carries torch forms of its transforms, `ftrns2_diff`): the cloud's arithmetic, the region
    filter and the float32 rounding then run on the device in float64 -- the same values as the numpy path, whose 112 000 x 3 float64
    temporaries per source otherwise make the pass host-bound (37 ms per source at config 2 against ~6 ms of GPU work) -- and only the
    refined source's own query is transformed back on the host. In that branch the refined source is picked by ONE kernel per source
    (`postproc.refine_select_device`: the sum over the legs, the region mask and the nested argmax in one read of the read-outs)
    instead of ten torch passes over [n_rand_query, n_t]; the host-cloud branch keeps the torch statements, which are its reference.

    `source_parallel`: split the sources over GPUs (needs `ftrns2_device`). `(rank, world)`, or a
    `torch.distributed` process group (True: the default group) -- the forms of `window_parallel`. Rank r refines the contiguous block
    `window_blocks(len(srcs), world)[r]` of `srcs`. Every source has its own window, cloud and picks, so the split is exact: a source's
    row carries the same bits whichever rank computes it. With a plain callable `rand` the draws stay those of one GPU because every
    rank calls `rand` once per source, in source order, and discards the draws of the sources it does not own -- host time only, but
    `n_sources` draws on every rank whatever the split. `rand=PhiloxCloud(key)` removes that: source i's draw is a function of (key, i)
    alone, so no `rand` is called, the sources outside the rank's block are skipped entirely, and with `ftrns2_device` the cloud is
    made on the device by one launch per source (`postproc.refine_cloud_device`: no host draw, no staging copy); without
    `ftrns2_device` the host-cloud branch draws the same numbers with `PhiloxCloud.host`, so both branches keep meaning the same thing.
    * tuple form: no collective; returns (this rank's rows float64 [hi - lo, 7], (lo, hi)): `refined_from_found` turns the rows of
      all ranks, concatenated in rank order, into (srcs_refined, order).
    * group form: one all-gather of the fixed-size rows (`_gather_blocks`; the gloo wait ends after `merge_timeout` seconds), after which
      every rank finishes identically and returns the same (srcs_refined, order) as one GPU.
    A rank whose block is empty runs no window and still takes part in the collective; every rank checks the verdicts of its own
    contexts. A source-sharded model is refused.

    `source_offset`: the place of `srcs[0]` in a longer list of which `srcs` is a contiguous part (`OnlineCatalogue` refines a day's
    sources a few at a time): a keyed draw for local source i uses counter `source_offset + i`, so the part draws the clouds the whole
    list would have drawn for these sources. A plain callable `rand` has no counter and ignores it; 0 is the whole list.

    `source_batch`: 1 (default) refines one source after the other as described above. B in 2..16 (needs `ftrns2_device`; ValueError
    otherwise) takes the rank's sources B at a time, the last batch short: one cloud launch per batch (`postproc.refine_cloud_batch_device`;
    with a plain `rand` the staged draws stacked, `rand` still called once per source in source order), per leg one `push_window` per
    source whose window holds a pick and ONE G-sized tail with both read-outs for the batch (`flush_windows_clouds`: every window read
    out at its own cloud, one kNN search for all clouds), and one select launch pair (`postproc.refine_select_batch_device`). The
    region mask stays one `ftrns2_device` call per source. The rows, and so the results, are those of `source_batch=1` bit for bit.
    Each leg model's `window_batch` is set to B for the pass and put back afterwards (on an exception too, unless windows are still
    pending); unsharded models only. Measured at config 2 (112 000 queries, one leg, keyed draw; tools/refine_batch_time.py,
    profiles/EXPERIMENTS.md): 1.76 ms per source one by one, 1.33 / 1.29 / 1.23 ms in batches of 4 / 8 / 16, run-to-run spread 0.01 to
    0.1 ms -- 16 is the recommended value where the sources of a call are many; the default stays 1."""
    source_batch = _check_source_batch(source_batch, ftrns2_device)
    if source_batch > 1:
        for leg in legs:       # batched tails exist on unsharded models only: refused before anything touches a device
            leg.net._not_sharded("refine_sources(source_batch > 1): push_window / flush_windows_clouds")
    sp = _rank_split(source_parallel, "source_parallel", any(getattr(leg.net, "is_sharded", False) for leg in legs))
    keyed = rand if isinstance(rand, PhiloxCloud) else None
    source_offset = int(source_offset)
    if source_offset < 0:
        raise ValueError("refine_sources: source_offset must be >= 0")
    rand = rand or np.random.rand
    srcs = np.asarray(srcs, dtype=np.float64)
    b_lo, b_hi = 0, srcs.shape[0]
    if sp is not None:
        if ftrns2_device is None:
            raise ValueError("refine_sources: source_parallel needs ftrns2_device (the ranks exchange the device branch's fixed-size rows)")
        blocks = window_blocks(srcs.shape[0], sp.world)
        b_lo, b_hi = blocks[sp.rank]
    tq_host = np.asarray(tq.detach().cpu() if torch.is_tensor(tq) else tq, dtype=np.float64).reshape(-1)
    dev = legs[0].device
    tq_d = torch.as_tensor(tq_host.reshape(-1, 1)).float().to(dev)
    locs_d = torch.as_tensor(locs_cart).float().to(dev)
    dt = _dt_embed(kernel_sig_t, dt_embed)

    def readouts(i, xq):       # every leg's read-out [n_query, n_t, 1] at the queries `xq`, on the window that starts at source i's origin time
        for leg in legs:
            em = leg.embed(picks, srcs[i, 3], max_t, kernel_sig_t, dt)
            if em is not None:                                                                                          # :966-967
                yield leg.net.forward_fixed_source(em[0], em[1], None, None, None, locs_d, leg.x_grid_cart, xq, tq_d)[1]

    ranges = (lat_range, lon_range, depth_range)
    if source_batch > 1:
        def window(leg, i):
            return leg.embed(picks, srcs[i, 3], max_t, kernel_sig_t, dt)

        def draws():           # (source, its draw) in source order; a plain `rand` is called for every source, the rank's own or not
            for i in (range(b_lo, b_hi) if keyed is not None else range(srcs.shape[0])):
                draw = None if keyed is not None else rand(n_rand_query, 3)
                if b_lo <= i < b_hi:
                    yield i, draw

        refine_batch = _refine_batches_on_device_cloud(legs, srcs, window, tq_d.reshape(-1), X_offset_min, X_offset_range, ftrns1, ranges,
                                                       dev, ftrns2_device, n_rand_query, keyed, source_offset)
        nets = {id(leg.net): leg.net for leg in legs}.values()
        before = [(net, net.window_batch) for net in nets]
        found, batch = [], []
        try:
            for net in nets:
                net.window_batch = source_batch
            with torch.no_grad():
                for item in draws():
                    batch.append(item)
                    if len(batch) == source_batch:
                        found.append(refine_batch([i for i, _ in batch], [d for _, d in batch]))
                        batch = []
                if batch:
                    found.append(refine_batch([i for i, _ in batch], [d for _, d in batch]))
        finally:
            for net, n in before:      # (the setter waits for the tails issued here before it changes the batch size)
                if net.pending_windows == 0:
                    net.window_batch = n
        rows = torch.cat(found) if found else torch.zeros((0, 7), dtype=torch.float64, device=dev)
        return _refine_ending(rows, sp, blocks if sp is not None else None, merge_timeout, legs, (b_lo, b_hi), srcs, tq_host, ftrns2)
    cloud = (srcs, readouts, len(legs), tq_host.shape[0], X_offset_min, X_offset_range, ftrns1, ranges, dev)
    if ftrns2_device is not None:
        refine, to_geographic = _refine_on_device_cloud(*cloud, ftrns2_device, n_rand_query, keyed, source_offset), ftrns2
    else:
        refine, to_geographic = _refine_on_host_cloud(*cloud, ftrns2), (lambda x: x)       # (its rows are geographic already)
    found = []
    with torch.no_grad():
        if keyed is not None:                  # a draw indexed by source: only the rank's own sources, and no `rand` call at all
            for i in range(b_lo, b_hi):
                found.append(refine(i, None if ftrns2_device is not None else keyed.host(source_offset + i, n_rand_query)))
        else:
            for i in range(srcs.shape[0]):
                draw = rand(n_rand_query, 3)   # for another rank's source too, so that the stream is the one of one GPU
                if b_lo <= i < b_hi:
                    found.append(refine(i, draw))
    rows = torch.stack(found) if found else torch.zeros((0, 7), dtype=torch.float64, device=dev)
    return _refine_ending(rows, sp, blocks if sp is not None else None, merge_timeout, legs, (b_lo, b_hi), srcs, tq_host, to_geographic)


def _refine_ending(rows, sp, blocks, merge_timeout, legs, block, srcs, tq_host, to_geographic):
    """The end of `refine_sources`: this rank's device rows [hi - lo, 7] -> what the call returns."""
    if sp is not None and sp.collective:
        found = _gather_blocks(rows, blocks, sp.group, merge_timeout)
    else:
        found = rows.cpu().numpy()
    for leg in legs:       # a copy to the host has waited for the device (after the collective, so that a rank that raises here
        leg.check()        # leaves no other rank waiting): the verdicts of every window of this rank's pass are in
    if sp is not None and not sp.collective:
        return found, block
    return refined_from_found(found, srcs, tq_host, to_geographic)


def apply_windows_legs(legs, picks, x_query_cart, locs_cart, max_t, tsteps_abs=None, t_win=6.0, step_size="half", min_required_picks=1,
                       day_len=86400.0, kernel_sig_t=synthetic.KERNEL_SIG_T, dt_embed=None, times=None, tail_batch=16,
                       window_parallel=None, return_info=False, merge_timeout=60.0, merge="dense"):
    """The day's apply loop over several source grids into ONE `Out_2` (process_continuous_days.py:761-810, `for n in times_need: for
    x_grid_ind in x_grid_ind_list:`): every kept window runs on every leg of `legs` (`GridLeg`s, `use_subgraph` ones made with `pairs=`
    included; at most `engine.STACK_MAX_LEGS`, every leg with a model of its own), and all of them add into the same `Out_2`
    [n_query, len(tsteps_abs)], divided by `n_overlap * len(legs)` (:802-805). Returns (Out_2 on the device, window start times used) --
    the `Out_2` that `detect_refine_associate(legs, picks, Out_2, ...)` takes. `picks`: the day's `ResidentPicks` (uploaded once, shared
    by all legs); `x_query_cart` [Q, 3]: shared by all legs, each net caching its own kNN of the queries into its grid; `locs_cart`
    [S, 3]: the stations, as the per-source passes take them (the window path reads station positions from each model's adjacencies:
    here only the count is checked). Each leg brings its grid and its travel-time rows. The other arguments are those of
    `apply_windows_device`; the schedule is made once, from `picks.t_host`, and a window without a pick in the embedding range is
    skipped for every leg (:792-793).

    Per kept window, in window order, every leg in leg order embeds and pushes the window; when `tail_batch` windows are pending (or at
    the last one) every leg flushes its batched tail and ONE `genie_stack_windows_legs` launch adds all legs' read-outs, in (window,
    leg) order (`tail_batch=1`: every window gets a tail and a launch of its own): the summation order of the reference loop, which L
    single-grid runs added together afterwards, `(sum_w a_w) + (sum_w b_w)`, do not have -- and one dense `Out_2` instead of L. With
    one leg the result is `apply_windows_device(stack_on_device=True)` bit for bit.

    `window_parallel`: `(rank, world)` or a process group, as in `apply_windows_device`: rank r runs all legs of the windows
    `window_blocks(len(times), world)[r]` into a zero-initialised full-size `Out_2`; the tuple form returns that partial and the rank's
    `times`, the group form merges once (`_merge_partials`) and returns the full `times`. What is exact: a rank's partial is bit for bit
    what one GPU computes over that block of windows; the merged `Out_2` is bit-equal to one GPU in every column fed by one rank's
    windows only; in a column at a block boundary it is `fl(prefix) + fl(suffix)`. With more than one leg that also differs from one
    GPU on the default 'half' schedule, unlike the single-grid loop: a boundary column then has 2 L terms, split L | L, and two rounded
    sums of L terms added are not the running sum of 2 L. `return_info`: `window_parallel_info` of the run plus `rank`; its
    `exact_merge` keeps its meaning, independence from the order in which the collective adds the ranks. A source-node-sharded leg is
    refused (batched tails do not run on shards). No multi-GPU wall time has been measured. `merge="columns"`: as in
    `apply_windows_device` -- this rank's column band only, returned as a `BandedOut2`; the "dense" default is unchanged."""
    legs = list(legs)
    if not legs:
        raise ValueError("apply_windows_legs: no grid leg")
    if len(legs) > engine.STACK_MAX_LEGS:
        raise ValueError("apply_windows_legs: at most %d grid legs" % engine.STACK_MAX_LEGS)
    if any(getattr(leg.net, "is_sharded", False) for leg in legs):
        raise NotImplementedError("apply_windows_legs on a source-node-sharded leg: batched tails do not run on shards and the hybrid is "
                                  "not built; use an unsharded model per grid")
    wp = _rank_split(window_parallel, "window_parallel", False)
    dev = torch.device(picks.device)
    for l, leg in enumerate(legs):
        if torch.device(leg.device) != dev:
            raise ValueError("apply_windows_legs: leg %d lives on %s, the picks on %s" % (l, leg.device, dev))
        if leg.n_sta != picks.n_sta:
            raise ValueError("apply_windows_legs: leg %d has %d stations, the picks %d" % (l, leg.n_sta, picks.n_sta))
    if len({id(leg.net) for leg in legs}) != len(legs):
        raise ValueError("apply_windows_legs: two legs share one model (their pending windows would interleave); build one model per leg")
    if np.asarray(locs_cart).shape[0] != picks.n_sta:
        raise ValueError("apply_windows_legs: locs_cart has %d stations, the picks %d" % (np.asarray(locs_cart).shape[0], picks.n_sta))
    if len(picks) == 0:
        raise ValueError("apply_windows_legs: no pick of the model's stations")
    plan = _day_plan(picks.t_host, float(max_t), day_len, t_win, step_size, min_required_picks, tsteps_abs, times, kernel_sig_t, len(legs), wp,
                     return_info, merge)
    for leg in legs:
        leg.net.window_batch = tail_batch
    xq = torch.as_tensor(x_query_cart).float().to(dev)
    Out_2 = torch.zeros((xq.shape[0], plan.width), dtype=torch.float32, device=dev)
    return _run_day(plan, legs, picks, xq, Out_2, _fused_add(plan, Out_2), _dt_embed(kernel_sig_t, dt_embed), merge_timeout)


# ---- the online day loop: picks fed as they arrive, columns of Out_2 returned as they close ------------------------

def online_read_bounds(times, max_t, kernel_sig_t, t_win):
    """What the windows starting at `times` read of the pick axis, on the host: (first, embed_end, count_end), float64 arrays.
    * the embedding reads `t0 - 2 sigma < t < embed_end = t0 + max_t + 2 sigma`, both strict (`_embed_ranges`);
    * the `min_required_picks` count reads `t0 - t_win <= t <= count_end = t0 + max_t + t_win`, both inclusive, in the arithmetic of
      `windows_with_enough_picks` (centre `t0 + max_t / 2`, radius `t_win + max_t / 2`);
    * `first`: no pick with `t < first` is read at all -- the earlier of `t0 - 2 sigma` and the count's lower end."""
    times = np.asarray(times, dtype=np.float64)
    c, r = times + max_t / 2.0, t_win + max_t / 2.0
    return np.minimum(times - 2.0 * kernel_sig_t, c - r), times + max_t + 2.0 * kernel_sig_t, c + r


def online_ready(times, t_now, max_t, kernel_sig_t, t_win):
    """Boolean [n]: the windows whose every read pick has been fed, under the caller's promise that every pick with `t < t_now` has:
    `embed_end <= t_now` (the embedding's bound is strict, so a bound equal to `t_now` is ready) and `count_end < t_now` (the count's is
    inclusive: a pick exactly at `t_now` may still be missing). The later of the two decides."""
    _, embed_end, count_end = online_read_bounds(times, max_t, kernel_sig_t, t_win)
    return (embed_end <= t_now) & (count_end < t_now)


def online_frontiers(cols, n_cols):
    """int64 [n + 1]: entry k = the first column that a window k, k + 1, ... of the `cols` table (`window_cols_table`, -1 = no column)
    lists, `n_cols` past the last one: once windows 0 .. k - 1 have run, the columns below entry k are closed. Never decreasing in k."""
    cols = np.asarray(cols).astype(np.int64)
    first = np.where(cols >= 0, cols, int(n_cols)).min(axis=1, initial=int(n_cols))
    return np.minimum.accumulate(np.append(first, int(n_cols))[::-1])[::-1]


def online_batch_spans(cols, n_cols, tail_batch):
    """int64 [n]: entry k = the columns that are open at once when a batch of the loop starts at window k -- from the frontier of k
    (`online_frontiers`: everything below is closed before the batch starts) to the last column listed by any window up to the batch's
    end, window min(k + tail_batch, n) - 1. A batch never spans more than `tail_batch` windows of the schedule, skipped ones included."""
    cols = np.asarray(cols).astype(np.int64)
    n = cols.shape[0]
    last = np.maximum.accumulate(cols.max(axis=1, initial=-1)) if n else np.zeros(0, dtype=np.int64)
    end = np.minimum(np.arange(n) + int(tail_batch), n) - 1
    return np.maximum(last[end] - online_frontiers(cols, n_cols)[:n] + 1, 0)


def online_batches(start, end, tail_batch):
    """[(a, b)]: the windows [start, end) of the schedule that one `feed` runs, cut into its batches [a, b) of at most `tail_batch`
    windows, skipped ones included; after each batch the columns below `online_frontiers(...)[b]` close."""
    return [(a, min(a + int(tail_batch), end)) for a in range(start, end, int(tail_batch))]


def online_ring_min(cols, n_cols, tail_batch):
    """The smallest ring (in columns) in which no two open columns of `OnlineDay` ever share a slot, whichever way the windows become
    ready: the widest `online_batch_spans` entry (at least 1)."""
    return int(max(1, online_batch_spans(cols, n_cols, tail_batch).max(initial=1)))


def _tq_span(tq):
    """(tq_lo, tq_hi) = (min(tq, 0), max(tq, 0)) over the time offsets `tq`, float64: a refined time lies in [t_d + tq_lo, t_d + tq_hi]."""
    tq = np.asarray(tq.detach().cpu() if torch.is_tensor(tq) else tq, dtype=np.float64).reshape(-1)
    return float(min(tq.min(initial=0.0), 0.0)), float(max(tq.max(initial=0.0), 0.0))


def online_source_ready(t_det, t_now, tq, max_t, kernel_sig_t):
    """Boolean [n]: the detected sources (origin times `t_det`) whose refine AND association passes read nothing that can still arrive,
    under the promise of `online_ready` (every pick with `t < t_now` has been fed). The refine pass embeds the window that starts at
    `t_det`, the association pass the one that starts at the refined time `t_r = t_det + tq[j]` for a j not known beforehand; both
    read `t0 - 2 sigma < t < t0 + max_t + 2 sigma`, strict. The latest upper bound is the one of `t0 = t_det + tq_hi`, so the source is
    ready when `t_det + tq_hi + max_t + 2 sigma <= t_now` (equality allowed: the bound is strict). Evaluated in the operation order of
    `picks_in_embed_range`, so that float rounding cannot put a read bound above the tested one (rounding is monotonic)."""
    t_det = np.asarray(t_det, dtype=np.float64)
    return (t_det + _tq_span(tq)[1]) + max_t + 2.0 * kernel_sig_t <= t_now


def online_t_low(pending_t, held_cols, bound, closed, tsteps_abs):
    """`T_low`: no source that has not run yet -- released and waiting, or still to be detected -- has an origin time below it. The
    minimum of the waiting sources' times `pending_t`, the times of the detector's held candidate columns `held_cols`, T(`bound`)
    (`StreamPeaks.bound`: no later candidate falls below it) and T(`closed`) (the columns still open in the day's ring), with
    T(c) = tsteps_abs[c] and T(len(tsteps_abs)) = +inf. +inf when nothing is left."""
    ts = np.asarray(tsteps_abs, dtype=np.float64).reshape(-1)
    at = lambda c: float(ts[int(c)]) if int(c) < len(ts) else np.inf
    pending_t, held_cols = np.asarray(pending_t, dtype=np.float64).reshape(-1), np.asarray(held_cols).reshape(-1)
    return min(pending_t.min(initial=np.inf), at(held_cols.min()) if held_cols.size else np.inf, at(bound), at(closed))


def online_retain_from(pending_t, held_cols, bound, closed, tsteps_abs, tq, kernel_sig_t):
    """The time from which the pick store must keep everything (`OnlineDay.retain_from`) for the sources that have not run yet: a
    source at `t_d >= T_low` (`online_t_low`) is refined on `t > t_d - 2 sigma` and associated on `t > t_r - 2 sigma` with
    `t_r >= t_d + tq_lo`, so every pick with `t > T_low + tq_lo - 2 sigma` stays. Evaluated as `(T_low + tq_lo) - 2 sigma`, which no
    read bound `t0 - 2 sigma` with `t0 >= T_low + tq_lo` falls below."""
    return (online_t_low(pending_t, held_cols, bound, closed, tsteps_abs) + _tq_span(tq)[0]) - 2.0 * kernel_sig_t


def online_marching_final(t_refined, t_low, tq, tc_win):
    """How many of the refined sources (refined times `t_refined`, ASCENDING) have their verdict of the second LocalMarching fixed:
    the marching (`n_steps_max = 2`) lets a source see the refined sources within two hops, a hop spans at most `tc_win` in refined
    time, and every source not refined yet will have `t_r >= t_low + tq_lo` (`t_low` = `online_t_low` over everything not refined).
    Source i is final when `t_refined[i] + 2 tc_win < t_low + tq_lo`; these are a prefix, whose length is returned."""
    t_refined = np.asarray(t_refined, dtype=np.float64).reshape(-1)
    return int(np.searchsorted(t_refined + 2.0 * float(tc_win), t_low + _tq_span(tq)[0], side="left"))


def online_marching_verdicts(decided, rows, t_low, tq, tc_win, keep_flags):
    """One step of the second LocalMarching as the refined sources arrive. `rows` [n, 5]: the refined sources without a verdict,
    ASCENDING in refined time; `decided` [m, 5]: sources with a verdict (kept or not) that an undecided one may still reach; `t_low`:
    `online_t_low` over everything not refined yet; `keep_flags(srcs)` -> bool [len(srcs)]: the marching of the caller's choice
    (`n_steps_max = 2, use_directed = False`; `postproc.local_marching_keep_device`, or the host `postproc.local_marching`).
    The first `online_marching_final(...)` rows are final. Their verdicts are read from ONE marching over `decided` within `2 tc_win` of
    `rows[0]` plus all of `rows`: a final row's two-hop neighbourhood lies within `2 tc_win` of it, hence at or above
    `rows[0] - 2 tc_win` (every earlier source is in `decided`) and below every source still to come (all of it is in `rows`), and
    every edge among those nodes is present, so the row sees what it sees in the whole day's list. Returns (keep bool [n_final],
    the new `decided`): the final rows join `decided`, which is then cut to what the earliest source without a verdict -- `rows`'
    next one, or one still to come at `t_low + tq_lo` or later -- can reach."""
    rows, decided = np.asarray(rows, dtype=np.float64).reshape(-1, 5), np.asarray(decided, dtype=np.float64).reshape(-1, 5)
    n_final = online_marching_final(rows[:, 3], t_low, tq, tc_win)
    if n_final == 0:
        return np.zeros(0, dtype=bool), decided
    reach = 2.0 * float(tc_win)
    near = decided[decided[:, 3] >= rows[0, 3] - reach]
    keep = np.asarray(keep_flags(np.concatenate((near, rows))), dtype=bool)[len(near):len(near) + n_final]
    decided = np.concatenate((near, rows[:n_final]))
    first = min(rows[n_final, 3] if n_final < len(rows) else np.inf, t_low + _tq_span(tq)[0])
    return keep, decided[decided[:, 3] >= first - reach]


_OnlinePlan = collections.namedtuple("_OnlinePlan", "tsteps_abs times offsets h_cols frontiers tail_batch ring_min ring_cols scale")


def online_day_plan(tsteps_abs, times, max_t, t_win, step_size, tail_batch, n_grids, ring_cols=None):
    """What `OnlineDay` knows of its schedule before it touches a device, host arithmetic only: the axis, the candidate window starts
    (`times`, or the default ones: `window_schedule` for stand-in picks at both ends of the axis), the offsets, the column table
    `h_cols`, `online_frontiers`, `online_ring_min`, the ring's size and `scale`, the fp32 reciprocal of `n_overlap * n_grids`. The
    number of grid legs enters through `n_grids` and therefore through `scale` ALONE: the table, the frontiers, the ready rule and the
    ring minimum are functions of the schedule (none of `online_ready`, `online_frontiers`, `online_batch_spans`, `online_ring_min`
    takes a leg argument), because every leg runs every window and all legs of a window add into the same columns in one launch."""
    tsteps_abs = np.asarray(tsteps_abs, dtype=np.float64)
    # `window_schedule` for stand-in picks at both ends of the axis: the offsets, the overlap and the default window starts
    ends = [tsteps_abs[0] + t_win / 2.0 + max_t, tsteps_abs[-1] - t_win / 2.0]
    dt_win = window_schedule(ends, max_t, np.inf, t_win, 9, step_size)[4]
    tsteps, offsets, _, n_overlap, _ = window_schedule([ends[0], ends[1] + dt_win / 2.0], max_t, np.inf, t_win, 9, step_size)
    times = np.asarray(tsteps if times is None else times, dtype=np.float64).reshape(-1)
    if not is_ascending(times):
        raise ValueError("OnlineDay: times must ascend (windows run in the order in which they become ready)")
    h_cols = window_cols_table(tsteps_abs, times, offsets, step_size == "half", True)
    frontiers = online_frontiers(h_cols, len(tsteps_abs))
    tail_batch = int(tail_batch)
    if not 1 <= tail_batch <= engine.HipPath.MAX_BATCH:
        raise ValueError("OnlineDay: tail_batch must be in [1, %d]" % engine.HipPath.MAX_BATCH)
    ring_min = online_ring_min(h_cols, len(tsteps_abs), tail_batch)
    ring_cols = int(ring_min if ring_cols is None else ring_cols)
    if ring_cols < ring_min:
        raise ValueError("OnlineDay: ring_cols = %d is below the minimum of this schedule, %d columns (online_ring_min)" % (ring_cols, ring_min))
    return _OnlinePlan(tsteps_abs, times, offsets, h_cols, frontiers, tail_batch, ring_min, ring_cols, _stack_scale(n_overlap, n_grids)[1])


class OnlineDay(object):
    """The day's apply loop fed as the picks arrive: `feed(P_chunk, t_now)` runs every window that has become ready and returns the
    columns of `Out_2` that closed, `(first_col, block [Q, n] float32 on the device)` with n possibly 0 -- the shape
    `postproc.band_peaks` takes a band in; `finish()` does the same for everything left (`feed(None, inf)`); `closed` counts the
    columns returned so far. Memory is bounded: the picks live in a `PickStore` trimmed behind the windows, `Out_2` exists only as a
    ring of `ring_cols` open columns.

    `net`: the model (adjacencies set), its `GridLeg`, or a list / tuple of 1..`engine.STACK_MAX_LEGS` `GridLeg`s, one per source grid
    (below); `geom`: anything with `x_query` (Cartesian; and `x_grid`, read for a bare model only); `trv_times` [G, S, 2] (or [N, 2]
    rows with `pairs`, as `GridLeg` takes them; read for a bare model, and for the default `max_t` of one leg). `tsteps_abs`: the
    column axis, ascending, REQUIRED -- the offline default depends on the day's last pick. `times`: the candidate window starts, ascending; default: `_day_schedule`'s
    windows for picks spanning the axis, i.e. from `tsteps_abs[0] + t_win / 2` in steps of `step_size` while the window's centre lies on
    the axis. Per candidate, WHEN IT BECOMES READY, `windows_with_enough_picks(min_required_picks)` and the empty-range rule decide
    whether it runs; a window they drop counts as run. (Offline, an explicit `times=` is taken as filtered already: the two agree
    whenever every candidate passes the count, which `min_required_picks=1` with `t_win >= 2 kernel_sig_t` guarantees for every window
    with a pick to embed.) `P_chunk` [m, 5]: rows as `apply_windows_device` takes them -- station index in the model's order, or
    absolute with `ind_use` / `n_sta_all` as `ResidentPicks` takes them -- in any order, or None.

    The caller's promise: when `feed(P_chunk, t_now)` is called, every pick with `t < t_now` has been fed (picks at or after `t_now` may
    have been, too); `t_now` never decreases (ValueError). A window is ready when nothing it reads can still arrive (`online_ready`).
    `feed` runs the ready windows in ascending order through the body of the offline loop (`_WindowBody`: embedding, `push_window` /
    `flush_windows` in batches of at most `tail_batch`, the stacker stream), stacking into the ring (genie_stack_windows_ring); after
    each batch the columns no unrun window lists (`online_frontiers`) leave the ring (genie_ring_close). Then the store's `frozen_t`
    moves to the first time the next unrun window reads and the store is trimmed to it: a later pick older than that raises ValueError
    in `feed` (nothing changes; feed on). One synchronisation per `feed`, then the model's verdicts (`_check_verdicts`).
    `retain_from` (an attribute, default +inf: no effect): `feed` trims to the earlier of that first read time and `retain_from`, so a
    reader behind the windows (`OnlineCatalogue`: the refine and association passes of sources not yet run) sets, BEFORE each `feed`,
    the time from which it still needs picks -- and then picks are stored after the last window has run, too; `frozen_t` does not
    depend on it.
    `ring_cols`: default `online_ring_min` of the schedule, the least that can never alias; a smaller value raises ValueError.

    Equality contract: with the same `tsteps_abs`, `times` and options the blocks, concatenated, are the `Out_2` of
    `apply_windows_device(..., stack_on_device=True)` BIT FOR BIT, for `tail_batch` 1 and above 1 alike and however the picks are cut
    into chunks: a column's sum is one fp32 running sum over its windows in ascending order in both loops, and a window's read-out does
    not depend on how windows are grouped into batched tails (tests/test_hip_parity.py pins every window of a batched tail, batches of
    1, 3, 8 and 16, bit-equal to the plain forward). Not built (NotImplementedError): a source-node-sharded model, `window_parallel`,
    `merge="columns"`, two legs that share one model (their pending windows would interleave: build one model per leg).

    Several legs (the reference's `for window: for grid:` loop, process_continuous_days.py:761-810): every ready window runs on every
    leg in leg order, every leg flushes its batched tail, and ONE genie_stack_windows_ring launch per batch adds all legs' read-outs
    in (window, leg) order, scaled by `1 / (n_overlap * L)` (`n_grids` must be left at its default, or be L; with one leg it keeps its
    meaning). The legs share one device, one station set (one `PickStore`), one ring and one `max_t` (required). `lanes`: the legs;
    `lane` = `lanes[0]`. `window_batch` is set on every leg's model and checked at every `feed`; the verdicts of every leg are raised
    after the call's one wait. Nothing of the schedule depends on L -- `ring_min`, the frontiers, the ready rule, the trim and
    `retain_from` are those of one leg (`online_day_plan`) -- so the contract is the same sentence with
    `apply_windows_legs(legs, ResidentPicks(...), ..., tsteps_abs=, times=, tail_batch=)` as the twin: a column's sum is one fp32
    running sum over (window, leg) in both loops. `OnlineDay([leg])` IS `OnlineDay(leg)`.

    Detection on the closed blocks as they arrive: `postproc.OnlineDetector`
    (`det.push(*day.feed(P_chunk, t_now))`).

    A restart: `state_dict()` between any two `feed` calls (everything `feed` has changed, on the host) and `load_state_dict(state)` on
    a newly constructed object with the same arguments; from there on the blocks are the saved object's, bit for bit (DESIGN.md
    section 5.17)."""

    def __init__(self, net, geom, trv_times, tsteps_abs, times=None, t_win=6.0, step_size="half", min_required_picks=1, n_grids=1.0,
                 kernel_sig_t=synthetic.KERNEL_SIG_T, dt_embed=None, max_t=None, tail_batch=16, pairs=None, ring_cols=None, ind_use=None,
                 n_sta_all=None, window_parallel=None, merge="dense"):
        items = list(net) if isinstance(net, (list, tuple)) else [net]
        n_legs = len(items)
        if n_legs == 0:
            raise ValueError("OnlineDay: no grid leg")
        if n_legs > engine.STACK_MAX_LEGS:
            raise ValueError("OnlineDay: at most %d grid legs" % engine.STACK_MAX_LEGS)
        if n_legs > 1 and not all(isinstance(item, GridLeg) for item in items):
            raise ValueError("OnlineDay: a list of %d items holds a bare model, which has no grid and no travel-time table of its own; "
                             "pass one GridLeg per grid" % n_legs)
        models = [item.net if isinstance(item, GridLeg) else item for item in items]
        if any(getattr(model, "is_sharded", False) for model in models):
            raise NotImplementedError("OnlineDay on a source-node-sharded model: batched tails do not run on shards; use an unsharded model"
                                      + (" per grid" if n_legs > 1 else ""))
        if window_parallel is not None and window_parallel is not False:
            raise NotImplementedError("OnlineDay with window_parallel: the online loop runs on one GPU")
        if merge != "dense":
            raise NotImplementedError('OnlineDay with merge="%s": the online loop returns dense blocks of closed columns' % (merge,))
        if n_legs > 1:                            # the checks of `apply_windows_legs`, on the legs alone: nothing is allocated yet
            for l, leg in enumerate(items):
                if torch.device(leg.device) != torch.device(items[0].device):
                    raise ValueError("OnlineDay: leg %d lives on %s, leg 0 on %s" % (l, leg.device, items[0].device))
                if leg.n_sta != items[0].n_sta:
                    raise ValueError("OnlineDay: leg %d has %d stations, leg 0 has %d (one station set, one pick store)"
                                     % (l, leg.n_sta, items[0].n_sta))
            if len({id(model) for model in models}) != n_legs:
                raise NotImplementedError("OnlineDay: two legs share one model (their pending windows would interleave); build one model "
                                          "per leg")
            if len({bool(getattr(model, "use_phase_types", True)) for model in models}) != 1:
                raise ValueError("OnlineDay: the legs' models disagree on use_phase_types (one pick store serves all legs)")
            if n_grids != 1.0 and n_grids != n_legs:
                raise ValueError("OnlineDay: n_grids = %r with %d legs (the divisor is n_overlap * %d, as apply_windows_legs computes it; "
                                 "leave n_grids at its default)" % (n_grids, n_legs, n_legs))
            if max_t is None:
                raise ValueError("OnlineDay: max_t is required with several legs (one max_t for the day, whichever grids run)")
            n_grids = n_legs
        if tsteps_abs is None or not is_ascending(tsteps_abs) or len(tsteps_abs) == 0:
            raise ValueError("OnlineDay: tsteps_abs is required and must ascend (the offline default needs the day's last pick)")
        self.max_t = float(max_t if max_t is not None else np.ceil(np.asarray(trv_times).max() + 1.0))
        self.t_win, self.kernel_sig_t, self.min_required_picks = float(t_win), float(kernel_sig_t), min_required_picks
        plan = online_day_plan(tsteps_abs, times, self.max_t, t_win, step_size, tail_batch, n_grids, ring_cols)
        self.tsteps_abs, self.times, self.offsets, self.step_size = plan.tsteps_abs, plan.times, plan.offsets, step_size
        self.h_cols, self.frontiers, self.tail_batch = plan.h_cols, plan.frontiers, plan.tail_batch
        self.ring_min, self.ring_cols, self.scale = plan.ring_min, plan.ring_cols, plan.scale
        self.lanes = [item if isinstance(item, GridLeg) else GridLeg(item, geom.x_grid, trv_times, pairs=pairs) for item in items]
        self.lane = self.lanes[0]                 # (the one-leg name, kept for its readers)
        dev = self.lane.device
        for model in models:
            model.window_batch = self.tail_batch
        n_sta = self.lane.n_sta
        self.picks = PickStore(np.arange(n_sta) if ind_use is None else ind_use, n_sta if n_sta_all is None else n_sta_all, dev,
                               use_phase_types=getattr(models[0], "use_phase_types", True))
        self.dt_embed = _dt_embed(kernel_sig_t, dt_embed)
        self.t_now = -np.inf
        self.retain_from = np.inf                 # `feed` keeps every pick with t >= this, whatever the windows still read
        self.n_run = 0                            # candidate windows run so far (dropped ones included): the next one's index
        self.closed = 0                           # columns returned so far
        self.last_col = -1                        # the last column any window has fed
        self.times_used = []                      # the starts of the windows that ran
        with torch.no_grad(), torch.cuda.device(dev):
            self.ring = torch.zeros((np.asarray(geom.x_query).shape[0], self.ring_cols), dtype=torch.float32, device=dev)
            self.d_cols = torch.from_numpy(self.h_cols).to(dev)
            xq = torch.as_tensor(geom.x_query).float().to(dev)
            self.body = _WindowBody(self.lanes, xq, self.offsets, self.max_t, self.kernel_sig_t, self.dt_embed)

    def _close(self, blocks, upto):
        """On the stacker stream: the columns [closed, upto) leave the loop as blocks appended to `blocks` -- out of the ring (one
        genie_ring_close launch: the open columns never span more than the ring) up to the last column any window has fed so far,
        as zeros beyond it (columns no window feeds, whose slots may already belong to later columns)."""
        fed = min(upto, self.last_col + 1)
        if fed > self.closed:
            blocks.append(engine.ring_close(self.ring, self.closed, fed))
            self.closed = fed
        if upto > self.closed:
            blocks.append(torch.zeros((self.ring.shape[0], upto - self.closed), dtype=torch.float32, device=self.ring.device))
            self.closed = upto

    def feed(self, P_chunk, t_now):
        t_now = float(t_now)
        if not t_now >= self.t_now:
            raise ValueError("OnlineDay.feed: t_now = %r after t_now = %r (it never decreases)" % (t_now, self.t_now))
        n, first_col, blocks = len(self.times), self.closed, []
        for lane in self.lanes:
            if lane.net.window_batch != self.tail_batch:
                raise RuntimeError("OnlineDay.feed: the model's window_batch was changed to %d (this loop set %d)"
                                   % (lane.net.window_batch, self.tail_batch))
        if P_chunk is not None and (self.n_run < n or self.retain_from < np.inf):      # (after the last window only a reader behind
            self.picks.append(P_chunk)                       # the windows, `retain_from`, reads a pick) a pick older than frozen_t raises here
        self.t_now = t_now
        ready = online_ready(self.times[self.n_run:], t_now, self.max_t, self.kernel_sig_t, self.t_win)
        end = self.n_run + (int(np.argmin(ready)) if not ready.all() else len(ready))        # ascending times: the ready ones are a prefix
        cand = self.times[self.n_run:end]
        keep = np.isin(cand, windows_with_enough_picks(self.picks.t_host, cand, self.max_t, self.t_win, self.min_required_picks))
        lo, hi = _embed_ranges(self.picks.t_host, cand, self.max_t, self.kernel_sig_t)
        keep &= hi > lo                                                                       # process_continuous_days.py:792-793
        body, dev = self.body, self.ring.device
        with torch.no_grad(), torch.cuda.device(dev):
            body.main = torch.cuda.current_stream(dev)
            body.stacker.wait_stream(body.main)              # the uploads of this call's chunk, the ring's zeros
            with torch.cuda.stream(body.stacker):            # (the first call only: the columns before the first window's)
                self._close(blocks, int(self.frontiers[self.n_run]))
            for a, b in online_batches(self.n_run, end, self.tail_batch):
                ws = [w for w in range(a, b) if keep[w - self.n_run]]
                for w in ws:
                    k = w - self.n_run
                    body.window(self.picks, cand[k], int(lo[k]), int(hi[k]))
                if ws:
                    body.flush(lambda xs: self._add(xs, ws))
                    self.times_used.extend(self.times[ws])
                with torch.cuda.stream(body.stacker):
                    self._close(blocks, int(self.frontiers[b]))
            self.n_run = end
            with torch.cuda.stream(body.stacker):            # (after the last window frontiers[n] = the whole axis)
                block = blocks[0] if len(blocks) == 1 else (
                    torch.cat(blocks, dim=1) if blocks else torch.zeros((self.ring.shape[0], 0), dtype=torch.float32, device=dev))
            block.record_stream(body.main)
            body.join()
        body.main.synchronize()                              # this call's one wait
        for lane in self.lanes:
            _check_verdicts(lane.net)
        first_read = online_read_bounds(self.times[self.n_run:self.n_run + 1], self.max_t, self.kernel_sig_t, self.t_win)[0]
        first_read = float(first_read[0]) if self.n_run < n else np.inf
        self.picks.frozen_t = min(first_read, t_now)         # (a pick from t_now on that no window reads any more is not late: it is trimmed)
        self.picks.trim(np.nextafter(min(first_read, self.retain_from), -np.inf))
        return first_col, block

    def _add(self, xs, ws):
        """One genie_stack_windows_ring launch for the read-outs `xs` (one per leg, in leg order) of the candidate windows `ws`
        (ascending; contiguous unless the
        filters dropped one in between: then their rows of the table are gathered on the device)."""
        used = self.h_cols[ws]
        used = used[used >= 0]
        if used.size:
            self.last_col = max(self.last_col, int(used.max()))
            rows = self.d_cols[ws[0]:ws[-1] + 1] if ws[-1] - ws[0] + 1 == len(ws) else torch.cat([self.d_cols[w:w + 1] for w in ws])
            engine.stack_windows_ring(self.ring, xs, rows, self.scale, int(used.min()), int(used.max()))

    def finish(self):
        """Everything left: `feed(None, inf)`; afterwards `closed == len(tsteps_abs)`."""
        return self.feed(None, np.inf)

    def _fingerprint(self):
        """The schedule and options a saved day belongs to, in the order in which `load_state_dict` compares them."""
        return {"tsteps_abs": self.tsteps_abs, "times": self.times, "offsets": self.offsets, "step_size": self.step_size,
                "scale": self.scale, "tail_batch": self.tail_batch, "max_t": self.max_t, "kernel_sig_t": self.kernel_sig_t,
                "t_win": self.t_win, "min_required_picks": self.min_required_picks, "dt_embed": self.dt_embed,
                "n_query": int(self.ring.shape[0]), "n_legs": len(self.lanes)}

    def _state(self):
        """`state_dict()` before the copy to the host: the open columns are still a device tensor."""
        lo, hi = self.closed, max(self.closed, self.last_col + 1)
        with torch.no_grad():
            block = engine.ring_save(self.ring, lo, hi)                   # [closed, last_col + 1): the ring holds zeros everywhere else
        return {"fingerprint": self._fingerprint(), "t_now": float(self.t_now), "retain_from": float(self.retain_from),
                "n_run": int(self.n_run), "closed": int(self.closed), "last_col": int(self.last_col),
                "times_used": np.asarray(self.times_used, dtype=np.float64), "ring_block": block, "picks": self.picks.state_dict()}

    def state_dict(self):
        """Everything `feed` has changed, between any two `feed` calls: the counters, the open columns
        `[closed, last_col + 1)` of the ring as one dense CPU block (genie_ring_save and a copy of that block, not of the ring), the
        `PickStore`'s state and the fingerprint of the schedule. Python scalars, numpy arrays and CPU tensors only: it goes through
        `torch.save` / `torch.load(weights_only=False)`. One synchronisation; the object is left as it was."""
        return checkpoint.to_host(self._state())

    def _check_state(self, state):
        if self.n_run or self.closed or self.t_now != -np.inf or self.last_col != -1:
            raise RuntimeError("OnlineDay.load_state_dict: this day has been fed; a state is loaded into a newly constructed OnlineDay")
        checkpoint.check_fingerprint("OnlineDay", state, self._fingerprint())
        block, n_open = state["ring_block"], max(int(state["last_col"]) + 1 - int(state["closed"]), 0)
        if not (torch.is_tensor(block) and block.dtype == torch.float32 and tuple(block.shape) == (self.ring.shape[0], n_open)):
            raise ValueError("OnlineDay.load_state_dict: ring_block must be fp32 [%d, %d] (the open columns)" % (self.ring.shape[0], n_open))
        if n_open > self.ring.shape[1]:
            raise ValueError("OnlineDay.load_state_dict: ring_cols = %d is below the %d open columns of the state" % (self.ring.shape[1], n_open))
        self.picks._check_state(state["picks"])

    def _load_state(self, state):
        dev = self.ring.device
        with torch.no_grad(), torch.cuda.device(dev):
            engine.ring_load(self.ring, state["ring_block"].to(dev).contiguous(), int(state["closed"]))
        self.picks.load_state_dict(state["picks"])
        self.t_now, self.retain_from = float(state["t_now"]), float(state["retain_from"])
        self.n_run, self.closed, self.last_col = int(state["n_run"]), int(state["closed"]), int(state["last_col"])
        self.times_used = list(np.asarray(state["times_used"], dtype=np.float64))

    def load_state_dict(self, state):
        """Resume a saved day in a NEWLY CONSTRUCTED object (nothing fed: RuntimeError otherwise) built with the arguments of the one that
        saved it: a difference in the schedule or the options raises ValueError naming the first differing field, and nothing has
        changed. `ring_cols` may differ (any value the constructor accepts holds the open columns; genie_ring_load puts them in this
        ring's slots). From here on `feed` returns what the saved object would have returned, bit for bit."""
        self._check_state(state)
        self._load_state(state)


def _inside_region(X, ranges):
    """Boolean [n]: the rows of `X` [n, 3] (numpy array or tensor) strictly inside the three `ranges` (process_continuous_days.py:930-936)."""
    return ((X[:, 0] > ranges[0][0]) & (X[:, 0] < ranges[0][1]) & (X[:, 1] > ranges[1][0]) & (X[:, 1] < ranges[1][1])
            & (X[:, 2] > ranges[2][0]) & (X[:, 2] < ranges[2][1]))


def _staged_clouds(src_cart, off_rng, off_min, n_rand_query, dev):
    """`staged_cloud(i, draw)` of the device-cloud refine pass with a host draw: source i's cloud (Xc float64 [n, 3], its float32 rounding)
    from the host's `draw`, which crosses through one of two pinned buffers taken in turn."""
    off_rng_d, off_min_d = torch.as_tensor(off_rng, device=dev), torch.as_tensor(off_min, device=dev)
    src_cart_d = torch.from_numpy(src_cart).to(dev) if src_cart is not None else None
    stage, stage_ev = _pinned_pair(n_rand_query, dev), [None, None]

    def staged_cloud(i, draw):
        k = i % 2
        if stage_ev[k] is not None:
            stage_ev[k].synchronize()              # the copy that last read this staging buffer (two sources ago) has finished
        stage[k].numpy()[...] = draw                                                                              # the host's draw, float64
        r = stage[k].to(dev, non_blocking=True)
        stage_ev[k] = torch.cuda.Event()
        stage_ev[k].record(torch.cuda.current_stream(dev))       # the stream of `dev` the copy was issued on
        Xc_d = src_cart_d[i:i + 1] + (r * off_rng_d + off_min_d)                                                  # :929
        return Xc_d, Xc_d.float()
    return staged_cloud


def _refine_on_device_cloud(srcs, readouts, n_legs, n_t, X_offset_min, X_offset_range, ftrns1, ranges, dev, ftrns2_device, n_rand_query,
                            keyed=None, source_offset=0):
    """`refine(i, draw)` of `refine_sources(ftrns2_device=...)`: source i's row float64 [7] on the device = (query row, offset index,
    value, any query inside the region, the refined query's CARTESIAN position), from its draw `rand(n_rand_query, 3)` -- or, with
    `keyed` (a `PhiloxCloud`), from the cloud one kernel draws on the device for counter `source_offset + i` (`draw` is then None)."""
    from . import postproc
    if int(n_rand_query) < 1:
        raise ValueError("refine_sources: n_rand_query must be >= 1")
    # constants of the loop and every source's Cartesian position: made once
    off_rng = np.asarray(X_offset_range, dtype=np.float64).reshape(1, 3)
    off_min = np.asarray(X_offset_min, dtype=np.float64).reshape(1, 3)
    src_cart = np.ascontiguousarray(ftrns1(srcs[:, 0:3]), dtype=np.float64).reshape(-1, 3) if srcs.shape[0] else None
    # the staged path's device copies and pinned pair; the keyed path passes the same numbers by value
    staged_cloud = None if keyed is not None else _staged_clouds(src_cart, off_rng, off_min, n_rand_query, dev)
    if n_legs > postproc.REFINE_SELECT_MAX_LEGS:
        raise ValueError("refine_sources: at most %d grid legs with ftrns2_device" % postproc.REFINE_SELECT_MAX_LEGS)
    sel_scratch = postproc.refine_select_scratch(dev)

    def refine(i, draw):
        # Nothing here waits for the device (round 5, tools/sync_probe_day.py: eight waits per source before -- pageable copies, the
        # boolean-mask compaction, three tensor-indexed reads): the draw goes through pinned memory, the queries outside the region stay
        # in the cloud and are masked out of the argmax (a query's read-out depends on no other query: the same values and the same
        # refined query as after the reference's compaction), and the refined query's row is gathered on the device. The host draws
        # source i + 1's cloud while the GPU works on source i. A keyed draw has no host part at all: one launch makes the cloud's
        # float64 and float32 forms from (key, i), with no pinned pair, no copy and no event.
        if keyed is not None:
            Xc_d, xq = postproc.refine_cloud_device(keyed.key, source_offset + i, n_rand_query, src_cart[i], off_rng, off_min, dev)     # :929, :934
        else:
            Xc_d, xq = staged_cloud(i, draw)
        keep = _inside_region(ftrns2_device(Xc_d), ranges)
        # the legs' read-outs stay where the read-out kernel wrote them; one launch pair sums them, masks and selects
        xs = [x.contiguous() for x in readouts(i, xq)]
        sel = postproc.refine_select_device(xs, (xq.shape[0], n_t), keep, float(n_legs), scratch=sel_scratch)      # :972-978
        return torch.cat((sel, Xc_d.index_select(0, sel[0:1].long()).view(3)))
    return refine


REFINE_BATCH_MAX = 16      # sources per batched tail of `refine_sources(source_batch=)`: a tail batch holds at most 16 windows


def _check_source_batch(source_batch, ftrns2_device):
    """`source_batch` of `refine_sources` as an int: 1, or 2..REFINE_BATCH_MAX with `ftrns2_device`; ValueError otherwise."""
    if isinstance(source_batch, bool) or not isinstance(source_batch, (int, np.integer)) or not 1 <= int(source_batch) <= REFINE_BATCH_MAX:
        raise ValueError("refine_sources: source_batch must be an integer in [1, %d], got %r" % (REFINE_BATCH_MAX, source_batch))
    if int(source_batch) > 1 and ftrns2_device is None:
        raise ValueError("refine_sources: source_batch > 1 needs ftrns2_device (the batch runs on the device branch's clouds)")
    return int(source_batch)


def _refine_batches_on_device_cloud(legs, srcs, window, tq_d, X_offset_min, X_offset_range, ftrns1, ranges, dev, ftrns2_device,
                                    n_rand_query, keyed, source_offset):
    """`refine_batch(ids, draws)` of `refine_sources(source_batch=B)`: the rows float64 [len(ids), 7] of the consecutive sources `ids`, each
    the row `_refine_on_device_cloud` makes of that source alone, from one cloud launch, one batched tail per leg (`push_window` per
    source whose window holds a pick, `flush_windows_clouds` with every window at its own cloud) and one select launch pair.
    `window(leg, i)`: (Slice, Mask) of source i's window on `leg`, or None without a pick. `draws`: the sources' `rand` draws (None
    with `keyed`)."""
    from . import postproc
    if int(n_rand_query) < 1:
        raise ValueError("refine_sources: n_rand_query must be >= 1")
    n_legs, n_t = len(legs), int(tq_d.shape[0])
    if n_legs > postproc.REFINE_SELECT_MAX_LEGS:
        raise ValueError("refine_sources: at most %d grid legs with ftrns2_device" % postproc.REFINE_SELECT_MAX_LEGS)
    off_rng = np.asarray(X_offset_range, dtype=np.float64).reshape(1, 3)
    off_min = np.asarray(X_offset_min, dtype=np.float64).reshape(1, 3)
    src_cart = np.ascontiguousarray(ftrns1(srcs[:, 0:3]), dtype=np.float64).reshape(-1, 3) if srcs.shape[0] else None
    staged = None if keyed is not None else _staged_clouds(src_cart, off_rng, off_min, n_rand_query, dev)
    sel_scratch = postproc.refine_select_batch_scratch(dev, REFINE_BATCH_MAX)
    Q = int(n_rand_query)

    def refine_batch(ids, draws):
        nb = len(ids)
        if keyed is not None:                                                                                       # :929, :934
            Xc, xq = postproc.refine_cloud_batch_device(keyed.key, source_offset + ids[0], nb, Q, src_cart[ids[0]:ids[0] + nb], off_rng,
                                                        off_min, dev)
        else:
            clouds = [staged(i, draw) for i, draw in zip(ids, draws)]
            Xc, xq = torch.stack([c[0] for c in clouds]), torch.stack([c[1] for c in clouds])
        # the user's transform per source, on the slice the single form hands it: a batched call need not give the same bits
        keep = torch.stack([_inside_region(ftrns2_device(Xc[b]), ranges) for b in range(nb)])
        table = np.zeros((nb, n_legs), dtype=np.int64)
        held = []                                            # the read-outs the table points into, alive until the select is issued
        main = torch.cuda.current_stream(dev)
        for l, leg in enumerate(legs):
            pushed = []
            for b, i in enumerate(ids):
                em = window(leg, i)
                if em is not None:                                                                                  # :966-967
                    leg.net.push_window(em[0], em[1])
                    pushed.append(b)
            if pushed:
                _, x, done = leg.net.flush_windows_clouds(leg.x_grid_cart, xq, tq_d, pushed)
                main.wait_event(done)
                held.append(x)
                for k, b in enumerate(pushed):
                    table[b, l] = x[k].data_ptr()
        sel = postproc.refine_select_batch_device(torch.from_numpy(table).to(dev), (Q, n_t), keep, float(n_legs),
                                                  scratch=sel_scratch)                                              # :972-978
        rows = sel[:, 0].long() + torch.arange(nb, device=dev) * Q
        return torch.cat((sel, Xc.view(nb * Q, 3).index_select(0, rows)), dim=1)
    return refine_batch


def _refine_on_host_cloud(srcs, readouts, n_legs, n_t, X_offset_min, X_offset_range, ftrns1, ranges, dev, ftrns2):
    """`refine(i, draw)` of `refine_sources` without `ftrns2_device`, the reference's own statements: the cloud and its region filter in
    numpy, the refined query by torch's `max` / `argmax`. The row is the device branch's, except that its position is GEOGRAPHIC: the
    refined query's row of the batch transform `ftrns2(cloud)` (a second transform of that one row need not give the same bits)."""
    one = torch.ones(1, dtype=torch.float64, device=dev)

    def refine(i, draw):
        Xc = ftrns1(srcs[i, 0:3].reshape(1, -1)) + (draw * X_offset_range + X_offset_min)                          # :929
        X1 = ftrns2(Xc)
        inside = np.where(_inside_region(X1, ranges))[0]
        if inside.size == 0:
            return torch.zeros(7, dtype=torch.float64, device=dev)          # no query inside the region: `refined_from_found` raises
        X1_d = torch.from_numpy(np.ascontiguousarray(X1[inside], dtype=np.float64)).to(dev)
        xq = torch.from_numpy(np.ascontiguousarray(Xc[inside])).to(dev).float()                                 # torch.Tensor(...) :934 (rounded on the device)
        acc = torch.zeros((xq.shape[0], n_t), dtype=torch.float32, device=dev)
        for x in readouts(i, xq):
            acc += x[:, :, 0] / float(n_legs)                                                                       # :972
        ip = torch.argmax(acc.max(1)[0])                                                                            # :976 (first maximum)
        it = torch.argmax(acc[ip])                                                                                  # :977
        return torch.cat((torch.stack((ip.double(), it.double(), acc[ip, it].double())), one, X1_d[ip]))
    return refine


def associate_sources(legs, picks, srcs_refined, locs_cart, tq, max_t, trv_out_srcs, ftrns1, x_save, kernel_sig_t=synthetic.KERNEL_SIG_T,
                      dt_embed=None, t_win=10.0, source_parallel=None, pick_lists="torch"):
    """The association pass of the caller (process_continuous_days.py:1020-1065) on the device: for every refined source one 4-output
    `forward_fixed` per grid leg on the window that starts at its origin time, with the window's pick lists (`ResidentPicks.pick_inputs`
    = extract_pick_inputs_from_data), ONE spatial query `x_save` (lat, lon of the first node of the reference's coarse map; its depth
    replaced by the source's, :1046) and the source itself as the only candidate (`x_query_src = ftrns1(src)`, `tq_sample = 0`,
    `trv_out_q = trv_out_srcs[[i]]` [1, S, 2], :1052). Returns (Out_p_save, Out_s_save: lists of float32 device tensors [m_i] = the
    P / S association likelihood of every pick of the window, averaged over the legs (:1054-1055); Save_picks: list of host [m_i, 2]
    (relative time, station, :1042); lp_meta: list of host [m_i, 5]). A window without picks yields empty entries (:1049-1050).

    `source_parallel`: as in `refine_sources`; rank r runs the network for the block `window_blocks(len(srcs_refined), world)[r]`.
    `Save_picks` and `lp_meta` depend on the picks alone, so every rank makes them for ALL sources itself, without a collective.
    * tuple form: returns (Out_p, Out_s of this rank's block only, Save_picks, lp_meta of all sources, (lo, hi)).
    * group form: one `all_gather_object` of the blocks' ragged likelihoods through the host (a few thousand floats per source; an
      RCCL group carries them as byte tensors on the current device); every rank returns the four full lists of one GPU.

    `pick_lists`: "torch" (default) makes a window's pick lists with `picks.pick_inputs`, "device" with `picks.pick_inputs_device`
    (one launch per source, genie_pick_lists); the lists are the same bit for bit."""
    if pick_lists not in ("torch", "device"):
        raise ValueError('associate_sources: pick_lists must be "torch" or "device"')
    sp = _rank_split(source_parallel, "source_parallel", any(getattr(leg.net, "is_sharded", False) for leg in legs))
    srcs = np.asarray(srcs_refined, dtype=np.float64)
    b_lo, b_hi = window_blocks(srcs.shape[0], sp.world)[sp.rank] if sp is not None else (0, srcs.shape[0])
    dev = legs[0].device
    tq_d = torch.as_tensor(np.asarray(tq.detach().cpu() if torch.is_tensor(tq) else tq, dtype=np.float32).reshape(-1, 1)).to(dev)
    locs_d = torch.as_tensor(locs_cart).float().to(dev)
    trv_out_srcs = torch.as_tensor(trv_out_srcs).float().to(dev)
    dt = _dt_embed(kernel_sig_t, dt_embed)
    n_scale = float(len(legs))
    zero = torch.zeros(1, device=dev)
    x_save = np.array(x_save, dtype=np.float64).reshape(1, 3)
    Out_p, Out_s, Save_picks, lp_meta = [], [], [], []
    # the per-source positions of the loop, copied once (a pageable host-to-device copy per source made the host wait for the device)
    xs_all = np.repeat(x_save, max(srcs.shape[0], 1), axis=0)
    xs_all[: srcs.shape[0], 2] = srcs[:, 2]                                                                          # :1046
    xs_cart_all = torch.from_numpy(np.ascontiguousarray(ftrns1(xs_all))).float().to(dev)
    src_cart_all = torch.from_numpy(np.ascontiguousarray(ftrns1(srcs[:, 0:3]))).float().to(dev) if srcs.shape[0] else None
    pick_inputs = picks.pick_inputs_device if pick_lists == "device" else picks.pick_inputs
    with torch.no_grad():
        for i in range(srcs.shape[0]):
            tp, ip, ph, idx = pick_inputs(srcs[i, 3], max_t, kernel_sig_t, t_win)
            Save_picks.append((tp, ip))
            lp_meta.append(idx)
            if not b_lo <= i < b_hi:           # another rank's source: its pick lists only
                continue
            acc_p = torch.zeros(tp.shape[0], dtype=torch.float32, device=dev)
            acc_s = torch.zeros(tp.shape[0], dtype=torch.float32, device=dev)
            Out_p.append(acc_p)
            Out_s.append(acc_s)
            if tp.shape[0] == 0:
                continue                                                                                                # :1049-1050
            xs_cart, src_cart = xs_cart_all[i:i + 1], src_cart_all[i:i + 1]
            tpf, phf = tp.float(), ph.long().float().reshape(-1, 1)
            for leg in legs:
                em = leg.embed(picks, srcs[i, 3], max_t, kernel_sig_t, dt)
                if em is None:
                    continue
                out = leg.net.forward_fixed(em[0], em[1], tpf, ip, phf, locs_d, leg.x_grid_cart, xs_cart, src_cart, tq_d, zero,
                                            trv_out_srcs[i:i + 1])                                                      # :1052
                acc_p += out[2][0, :, 0] / n_scale                                                                      # :1054
                acc_s += out[3][0, :, 0] / n_scale                                                                      # :1055
    Save_picks = [np.stack((a.cpu().numpy(), b.cpu().numpy().astype(np.float64)), axis=1) for a, b in Save_picks]
    lp_meta = [picks.meta(ix) for ix in lp_meta]
    if srcs.shape[0]:
        torch.cuda.current_stream(dev).synchronize()      # (windows without picks copy nothing back)
    for leg in legs:       # device-side verdicts (a pick outside the time-pointer table, a station index outside the model) of every call above
        leg.check()
    if sp is not None and not sp.collective:
        return Out_p, Out_s, Save_picks, lp_meta, (b_lo, b_hi)
    if sp is not None:
        import torch.distributed as dist
        parts = [None] * sp.world
        with torch.cuda.device(dev):
            dist.all_gather_object(parts, ([o.cpu().numpy() for o in Out_p], [o.cpu().numpy() for o in Out_s]), group=sp.group)
        Out_p = [torch.from_numpy(o).to(dev) for part in parts for o in part[0]]
        Out_s = [torch.from_numpy(o).to(dev) for part in parts for o in part[1]]
    return Out_p, Out_s, Save_picks, lp_meta


def retained_after_marching(srcs_refined, ftrns1, tc_win, sp_win, scale_depth_clustering=0.2, scale_time_ref=3500.0, device=None):
    """The second LocalMarching of the caller and the match back to the refined list (process_continuous_days.py:1072-1085): the
    refined sources that survive it (`n_steps_max = 2, use_directed = False`), found as the nearest refined source of each survivor in
    (Cartesian position, `scale_time_ref` * origin time), `np.unique`d. Returns the retained row indices (ascending). `device`: run
    the marching there (`postproc.local_marching_device`, same survivors); the match back stays on the host either way."""
    from scipy.spatial import cKDTree
    from . import postproc
    srcs_refined = np.asarray(srcs_refined, dtype=np.float64)
    if len(srcs_refined) == 0:
        return np.zeros(0, dtype=np.int64)
    kw = dict(tc_win=tc_win, sp_win=sp_win, scale_depth=scale_depth_clustering, n_steps_max=2, use_directed=False)
    if device is None:
        kept = postproc.local_marching(srcs_refined, ftrns1, **kw)
    else:
        kept = postproc.local_marching_device(srcs_refined, ftrns1, device=device, **kw)
    tree = cKDTree(np.concatenate((ftrns1(srcs_refined), scale_time_ref * srcs_refined[:, [3]]), axis=1))
    return np.unique(tree.query(np.concatenate((ftrns1(kept), scale_time_ref * kept[:, [3]]), axis=1))[1])


def detect_refine_associate(legs, picks, Out_2, X_query, tsteps_abs, locs, trv, tq, max_t, ftrns1, ftrns2, lat_range, lon_range,
                            depth_range, X_offset_min, X_offset_range, n_rand_query, thresh, src_t_kernel, dt_win, break_win, tc_win,
                            sp_win, scale_depth_clustering=0.2, kernel_sig_t=synthetic.KERNEL_SIG_T, dt_embed=None, t_win_assoc=10.0,
                            rand=None, ftrns2_device=None, detect_on_device=False, source_parallel=None, max_unit_cols=None,
                            refine_batch=1):
    """Everything the caller does between the apply loop and the competitive assignment, with the network calls on the device
    (process_continuous_days.py:811-1105): peaks of the device-resident `Out_2` -> time groups -> LocalMarching (`postproc.
    detect_sources`, :811-891), the refine pass (`refine_sources`, :926-982), travel times of the refined sources (`trv(locs, srcs)`
    [n, S, 2], :1004), the association pass (`associate_sources`, :1006-1068: `X_save` = the first node of the 15 x 15 map of the region,
    :1008-1014), the second LocalMarching with its match back (`retained_after_marching`, :1072-1090), the travel times of the retained
    sources (:1092) and the final sort by origin time (:1097-1105). `locs` [S, 3] (lat, lon, depth) of the stations in use; `trv`: the
    travel-time callable of the reference, (float tensor [S, 3], float tensor [n, 3]) -> [n, S, 2]. Returns a dict: `srcs` (after the
    first marching), `srcs_refined` [m, 5], `trv_out_srcs` (device [m, S, 2]), `Out_p_save`, `Out_s_save` (lists of device tensors),
    `Save_picks`, `lp_meta` (lists of host arrays) -- the inputs of `competitive_assignment`, which is out of scope.
    `detect_on_device`: both LocalMarchings, the distance rule and the grouping run on the GPU (`postproc.detect_sources_device`,
    `retained_after_marching(device=...)`) instead of on the host; the sources are the same. `Out_2` may then be the `BandedOut2` of a
    window-parallel day run with `merge="columns"` (group form): detection goes through `postproc.detect_sources_banded`, same dict plus
    `detect_info`, that call's info (`detect_info["fallback"]` says whether the day fell back to the dense merge, and why).
    `source_parallel`: the two per-source passes split over GPUs (`refine_sources`, `associate_sources`: a process group, True for
    the default one, or `(rank, world)` -- which, having no transport, must have world 1 here). Detection, both LocalMarchings and the
    `trv` calls are cheap and deterministic and run replicated on every rank; the returned dict equals the one-GPU dict on every rank.
    `max_unit_cols`: detection in units of at most that many columns (`postproc.detect_sources_device(max_unit_cols=...)`, the offline
    twin of an `OnlineDetector` with the same argument); device detection on a dense `Out_2` only (ValueError otherwise).
    `refine_batch`: `refine_sources(source_batch=...)`, the sources one batched tail refines together; the dict does not depend on it."""
    from . import postproc
    refine_batch = _check_source_batch(refine_batch, ftrns2_device)
    if max_unit_cols is not None:
        if not detect_on_device:
            raise ValueError("detect_refine_associate: max_unit_cols needs detect_on_device=True (the host detection has no unit rule)")
        if isinstance(Out_2, BandedOut2):
            raise ValueError("detect_refine_associate: max_unit_cols is not available on a BandedOut2 (detect_sources_banded has no unit rule)")
    sp = _rank_split(source_parallel, "source_parallel", any(getattr(leg.net, "is_sharded", False) for leg in legs))
    if sp is not None and not sp.collective:
        if sp.world != 1:
            raise ValueError("detect_refine_associate: source_parallel = (rank, world) with world > 1 needs a process group (the "
                             "association pass reads every rank's refined sources)")
        source_parallel = None
    dev = legs[0].device
    empty = {"srcs": np.zeros((0, 5)), "srcs_refined": np.zeros((0, 5)), "trv_out_srcs": None, "Out_p_save": [], "Out_s_save": [],
             "Save_picks": [], "lp_meta": []}
    detect = postproc.detect_sources_device if detect_on_device else postproc.detect_sources
    banded = isinstance(Out_2, BandedOut2)
    if banded and not detect_on_device:
        raise ValueError("detect_refine_associate: a BandedOut2 is detected on the device (detect_on_device=True)")
    detect_info = {}                              # a banded day's info (its `fallback` above all) goes into the returned dict
    if banded:
        detect = postproc.detect_sources_banded
    units = {} if max_unit_cols is None else {"max_unit_cols": max_unit_cols}
    srcs = detect(Out_2, X_query, tsteps_abs, ftrns1, thresh, src_t_kernel, dt_win, break_win, tc_win, sp_win, scale_depth_clustering, **units)
    if banded:
        srcs, detect_info = srcs[0], {"detect_info": srcs[1]}
    if len(srcs) == 0:
        return dict(empty, **detect_info)                                                                               # :886-888
    locs = np.asarray(locs, dtype=np.float64)
    locs_cart = ftrns1(locs)
    locs_d = torch.as_tensor(locs).float().to(dev)
    srcs_refined, _ = refine_sources(legs, picks, srcs, locs_cart, tq, max_t, X_offset_min, X_offset_range, n_rand_query, ftrns1, ftrns2,
                                     lat_range, lon_range, depth_range, kernel_sig_t, dt_embed, rand, ftrns2_device,
                                     source_parallel=source_parallel, source_batch=refine_batch)
    with torch.no_grad():
        trv_out = trv(locs_d, torch.as_tensor(srcs_refined[:, 0:3]).float().to(dev)).detach()                           # :1004
    x_save = np.array([lat_range[0], lon_range[0], 0.0])                              # xx[0] of the meshgrid of :1008-1014
    Out_p, Out_s, Save_picks, lp_meta = associate_sources(legs, picks, srcs_refined, locs_cart, tq, max_t, trv_out, ftrns1, x_save,
                                                          kernel_sig_t, dt_embed, t_win_assoc, source_parallel=source_parallel)
    keep = retained_after_marching(srcs_refined, ftrns1, tc_win, sp_win, scale_depth_clustering,
                                   device=dev if detect_on_device else None)
    srcs_kept = srcs_refined[keep]
    with torch.no_grad():
        trv_kept = trv(locs_d, torch.as_tensor(srcs_kept[:, 0:3]).float().to(dev)).detach()                             # :1092
    order = np.argsort(srcs_kept[:, 3])                                                                                 # :1097
    pick = [int(keep[j]) for j in order]
    return dict({"srcs": srcs, "srcs_refined": srcs_kept[order], "trv_out_srcs": trv_kept[torch.as_tensor(order, device=trv_kept.device)],
                 "Out_p_save": [Out_p[j] for j in pick], "Out_s_save": [Out_s[j] for j in pick],
                 "Save_picks": [Save_picks[j] for j in pick], "lp_meta": [lp_meta[j] for j in pick]}, **detect_info)


# ---- the online catalogue: released sources refined and associated as they arrive ---------------------------------

class OnlineCatalogue(object):
    """The last two stages of the online day: `push(P_chunk, t_now)` feeds the day (`OnlineDay.feed`), detects on the closed columns
    (`OnlineDetector.push`), runs every released source whose reads are complete through `refine_sources` and `associate_sources` on the
    day's `PickStore`, and returns the sources whose verdict of the second LocalMarching has become final -- a dict with the keys of
    `detect_refine_associate`: `srcs` (the detections RELEASED in this call, [n, 5]), and for the sources that became FINAL in this
    call and survive the marching, in refined-time order: `srcs_refined` [m, 5], `trv_out_srcs` (device [m, S, 2]; [0, S, 2] when
    none), `Out_p_save`, `Out_s_save` (lists of device tensors), `Save_picks`, `lp_meta` (lists of host arrays). `finish()` does the
    same for everything left. `pending`: sources released but not run; `undecided`: sources refined but not final.

    Equality contract: with `day` and `det` built on the same axis and options as the offline calls, all returns concatenated are the
    dict of `apply_windows_device(stack_on_device=True)` -> `detect_refine_associate(detect_on_device=True,
    max_unit_cols=det.max_unit_cols, rand=PhiloxCloud(key), ftrns2_device=...)` BIT FOR BIT, however the picks are cut into chunks
    (refined times distinct, as the offline sorts assume). The catalogue takes the detector it is given: with forced unit cuts
    (`OnlineDetector(max_unit_cols=M)`) the units still come out in ascending time, so rules 1-5 stand as they are.
    Why, rule by rule:
    1. a source at `t_d` is refined on `t_d - 2 sigma < t < t_d + max_t + 2 sigma` and associated on the same range around
       `t_r = t_d + tq[j]`, whatever else the day holds; its cloud is keyed by its place in the day's detection list, which is the
       running count of released sources (`refine_sources(source_offset=...)`: units come out in ascending time);
    2. it runs once `online_source_ready` says nothing it reads can still arrive -- possibly pushes after its release;
    3. BEFORE each `day.feed`, `day.retain_from = online_retain_from(...)` keeps the picks every source not yet run can read;
       `lp_meta` is read inside the association call, before any later trim;
    4. the second LocalMarching (`n_steps_max = 2`) reaches two hops of at most `tc_win` each, so a refined source further than
       `2 tc_win` below every refined time still to come is final (`online_marching_final`). The verdicts are taken from
       `postproc.local_marching_keep_device` on the undecided sources plus the decided ones within `2 tc_win` of the earliest
       undecided one. A survivor is a row of the input, so the match back to the refined list is the row's own index: for distinct
       rows that is the nearest-neighbour (cKDTree) match of `retained_after_marching`, whose nearest row of a row is itself;
    5. `trv(locs, srcs)` is called on the few sources of a push, offline on all of them at once: THE CALLABLE'S ROWS MUST NOT DEPEND ON
       THE BATCH (row i a function of `srcs[i]` alone, bit for bit), as the straight-ray callable of `synthetic.Geometry` is.

    Several legs: the catalogue runs over `day.lanes` -- `refine_sources` and `associate_sources` take all of them, as
    `detect_refine_associate(legs, ...)` does offline, the verdicts of every leg are raised at the end of each call, and the device
    tensors live on the legs' one device. The twin is then `apply_windows_legs(legs, ...)` -> `detect_refine_associate(legs, ...)`. None
    of the rules reads the grid:
    1. every leg embeds the same pick range (`GridLeg.embed` -> `picks.embed_args(t0, max_t, sigma)`: one store, one `max_t`), and the
       cloud's key is the source's place in the list, not a leg's;
    2. `online_source_ready` takes `t_det`, `tq`, `max_t` and sigma, which the legs share;
    3. `online_retain_from` likewise; `lp_meta` comes from the store, once per source whatever L is;
    4. the marching sees refined sources only -- the mean over the legs was taken before;
    5. `trv(locs, srcs)` takes stations and sources, no grid.

    `rand` must be a `PhiloxCloud` and `ftrns2_device` must be given (ValueError): a stateful draw or the host cloud has no offline twin
    that a sub-list reproduces. `pick_lists`: how the association pass makes its pick lists (`associate_sources`; "device" here, one launch per source: at the
    few hundred picks of a window it takes about half the time of the torch statements, profiles/EXPERIMENTS.md). There is no
    `source_parallel`: a push carries a few sources. `refine_batch`: `refine_sources(source_batch=...)` for the sources of a push; results
    and saved state do not depend on it. Every block of `day` must go through this object (a `day.feed` of the caller's
    own loses columns: ValueError at the next call, nothing changed).

    A restart: `state_dict()` between any two `push` calls saves the day, the detector and this object in one call,
    `load_state_dict(state)` on newly constructed objects with the same arguments resumes all three or none."""

    def __init__(self, day, det, locs, trv, tq, ftrns1, ftrns2, lat_range, lon_range, depth_range, X_offset_min, X_offset_range,
                 n_rand_query, tc_win, sp_win, scale_depth_clustering=0.2, t_win_assoc=10.0, rand=None, ftrns2_device=None,
                 pick_lists="device", refine_batch=1):
        if not isinstance(rand, PhiloxCloud):
            raise ValueError("OnlineCatalogue: rand must be a PhiloxCloud (a source's draw must not depend on when it runs)")
        if ftrns2_device is None:
            raise ValueError("OnlineCatalogue: ftrns2_device is required (the keyed cloud is drawn on the device)")
        if pick_lists not in ("torch", "device"):
            raise ValueError('OnlineCatalogue: pick_lists must be "torch" or "device"')
        self.refine_batch = _check_source_batch(refine_batch, ftrns2_device)       # how the sources run, not what comes out: not saved
        if len(det.tsteps_abs) != len(day.tsteps_abs) or not np.array_equal(det.tsteps_abs, day.tsteps_abs):
            raise ValueError("OnlineCatalogue: day and det must share one tsteps_abs")
        self.day, self.det, self.legs = day, det, list(day.lanes)
        self.device = self.legs[0].device         # (`OnlineDay` has checked that the legs share one device)
        self.trv, self.ftrns1, self.ftrns2, self.ftrns2_device, self.rand = trv, ftrns1, ftrns2, ftrns2_device, rand
        self.tq = np.asarray(tq.detach().cpu() if torch.is_tensor(tq) else tq, dtype=np.float64).reshape(-1)
        self.ranges = (lat_range, lon_range, depth_range)
        self.offsets = (X_offset_min, X_offset_range)
        self.n_rand_query, self.tc_win, self.sp_win = n_rand_query, float(tc_win), float(sp_win)
        self.scale_depth_clustering, self.t_win_assoc, self.pick_lists = scale_depth_clustering, t_win_assoc, pick_lists
        locs = np.asarray(locs, dtype=np.float64)
        self.locs_cart = ftrns1(locs)
        self.locs_d = torch.as_tensor(locs).float().to(self.device)
        self.x_save = np.array([lat_range[0], lon_range[0], 0.0])                 # as `detect_refine_associate` takes it
        self.n_released = 0                       # sources released so far: the next one's place in the day's detection list
        self._pending = np.zeros((0, 5))          # released, not run (ascending origin time)
        self._rows = np.zeros((0, 5))             # refined, not final (ascending refined time), with their results in step:
        self._results = []                        #   (trv row, Out_p, Out_s, Save_picks, lp_meta) per row of `_rows`
        self._decided = np.zeros((0, 5))          # final rows, kept or not, that an undecided source may still reach

    pending = property(lambda self: int(self._pending.shape[0]))
    undecided = property(lambda self: int(self._rows.shape[0]))

    def _held_low(self):
        """What `online_t_low` reads of the detector's held columns: their minimum alone, as an array of one (or none)."""
        first = self.det.held_first_col
        return np.zeros(0, dtype=np.int64) if first is None else np.array([first], dtype=np.int64)

    def _t_low(self):
        return online_t_low(self._pending[:, 3], self._held_low(), self.det.peaks.bound, self.day.closed, self.day.tsteps_abs)

    def _run(self, srcs):
        """Refine and associate the sources `srcs` (the head of `_pending`), and file the results by refined time."""
        day, legs = self.day, self.legs
        rows, _ = refine_sources(legs, day.picks, srcs, self.locs_cart, self.tq, day.max_t, self.offsets[0], self.offsets[1],
                                 self.n_rand_query, self.ftrns1, self.ftrns2, *self.ranges, day.kernel_sig_t, day.dt_embed, self.rand,
                                 self.ftrns2_device, source_offset=self.n_released - self._pending.shape[0],
                                 source_batch=self.refine_batch)
        dev = self.device
        with torch.no_grad():
            trv_out = self.trv(self.locs_d, torch.as_tensor(rows[:, 0:3]).float().to(dev)).detach()
        res = associate_sources(legs, day.picks, rows, self.locs_cart, self.tq, day.max_t, trv_out, self.ftrns1, self.x_save,
                                day.kernel_sig_t, day.dt_embed, self.t_win_assoc, pick_lists=self.pick_lists)
        results = self._results + [(trv_out[i],) + tuple(r[i] for r in res) for i in range(rows.shape[0])]
        rows = np.concatenate((self._rows, rows))
        order = np.argsort(rows[:, 3], kind="stable")
        self._rows, self._results = rows[order], [results[i] for i in order]

    def _final(self):
        """Take the sources whose marching verdict is final out of the undecided ones; returns the kept ones' (rows, results)."""
        from . import postproc
        march = lambda srcs: postproc.local_marching_keep_device(srcs, self.ftrns1, tc_win=self.tc_win, sp_win=self.sp_win, n_steps_max=2,
                                                                 scale_depth=self.scale_depth_clustering, use_directed=False,
                                                                 device=self.device)
        keep, self._decided = online_marching_verdicts(self._decided, self._rows, self._t_low(), self.tq, self.tc_win, march)
        n = len(keep)
        rows, results = self._rows[:n][keep], [r for r, k in zip(self._results[:n], keep) if k]
        self._rows, self._results = self._rows[n:], self._results[n:]
        return rows, results

    def _step(self, P_chunk, t_now, last):
        day, det = self.day, self.det
        if det.seen != day.closed:
            raise ValueError("OnlineCatalogue: the detector has seen %d columns, the day has closed %d (every block of the day goes "
                             "through this object)" % (det.seen, day.closed))
        day.retain_from = online_retain_from(self._pending[:, 3], self._held_low(), det.peaks.bound, day.closed, day.tsteps_abs, self.tq,
                                             day.kernel_sig_t)
        srcs = det.push(*day.feed(P_chunk, t_now))
        if last:
            srcs = np.concatenate((srcs, det.finish()))
        self.n_released += srcs.shape[0]
        self._pending = np.concatenate((self._pending, srcs))
        ready = online_source_ready(self._pending[:, 3], day.t_now, self.tq, day.max_t, day.kernel_sig_t)
        n_ready = int(np.argmin(ready)) if not ready.all() else len(ready)        # ascending times: the ready ones are a prefix
        if n_ready:
            self._run(self._pending[:n_ready])
            self._pending = self._pending[n_ready:]
        rows, results = self._final()
        if last:                                  # nothing reads a pick any more
            day.retain_from = np.inf
            day.picks.trim(np.inf)
        for leg in self.legs:
            leg.check()
        n_sta = int(self.locs_d.shape[0])
        return {"srcs": srcs, "srcs_refined": rows,
                "trv_out_srcs": torch.stack([r[0] for r in results]) if results else torch.zeros((0, n_sta, 2), device=self.device),
                "Out_p_save": [r[1] for r in results], "Out_s_save": [r[2] for r in results],
                "Save_picks": [r[3] for r in results], "lp_meta": [r[4] for r in results]}

    def push(self, P_chunk, t_now):
        return self._step(P_chunk, t_now, False)

    def finish(self):
        """Everything left: the day's last windows, the detector's last unit, every waiting source, every verdict. Raises as
        `OnlineDetector.finish` does when the detector has not been given every column."""
        return self._step(None, np.inf, True)

    def _fingerprint(self):
        return {"philox_key": np.asarray(self.rand.key, dtype=np.uint64), "tq": self.tq, "lat_range": self.ranges[0],
                "lon_range": self.ranges[1], "depth_range": self.ranges[2], "X_offset_min": self.offsets[0], "X_offset_range": self.offsets[1],
                "n_rand_query": self.n_rand_query, "tc_win": self.tc_win, "sp_win": self.sp_win,
                "scale_depth_clustering": self.scale_depth_clustering, "t_win_assoc": self.t_win_assoc, "pick_lists": self.pick_lists,
                "locs_cart": self.locs_cart, "x_save": self.x_save}

    def state_dict(self):
        """`{"day": ..., "det": ..., "catalogue": ...}`: the states of the day, the detector and this object taken at one moment,
        between any two `push` calls. Of this object: `n_released`, the waiting, the undecided and the decided
        sources, and per undecided source its results -- the device tensors (travel-time row, the two likelihood vectors) as CPU tensors
        of the same dtype, shape and bytes. Every device tensor of the three states is queued for its copy first, then the host waits
        once. No model, no callable, no device tensor: it goes through `torch.save` / `torch.load(weights_only=False)`."""
        own = {"fingerprint": self._fingerprint(), "n_released": int(self.n_released), "pending": self._pending, "rows": self._rows,
               "decided": self._decided, "results": [tuple(r) for r in self._results]}
        return checkpoint.to_host({"day": self.day._state(), "det": self.det._state(), "catalogue": own})

    def load_state_dict(self, state):
        """Resume all three objects from one `state_dict()`, or none: this object, its day and its detector must be newly constructed
        (RuntimeError otherwise) with the arguments of the saved ones, and all three fingerprints are compared before anything changes
        (ValueError naming the first differing field). The results of the undecided sources go back onto the legs' device."""
        if not isinstance(state, dict) or sorted(state) != ["catalogue", "day", "det"]:
            raise ValueError('OnlineCatalogue.load_state_dict: a state has the keys "day", "det" and "catalogue"')
        if self.n_released or self.pending or self.undecided or self._decided.shape[0]:
            raise RuntimeError("OnlineCatalogue.load_state_dict: this catalogue has run; a state is loaded into a newly constructed one")
        own = state["catalogue"]
        self.day._check_state(state["day"])
        self.det._check_state(state["det"])
        checkpoint.check_fingerprint("OnlineCatalogue", own, self._fingerprint())
        self.day._load_state(state["day"])
        self.det._load_state(state["det"])
        dev = self.device
        f64 = lambda a: np.array(a, dtype=np.float64).reshape(-1, 5)
        self.n_released = int(own["n_released"])
        self._pending, self._rows, self._decided = f64(own["pending"]), f64(own["rows"]), f64(own["decided"])
        self._results = [tuple(x.to(dev) if torch.is_tensor(x) else np.array(x) for x in r) for r in own["results"]]
