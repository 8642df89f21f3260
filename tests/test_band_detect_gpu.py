"""GPU: a window-parallel day detected without the dense `Out_2` merge (`merge="columns"`, `apply.BandedOut2`,
`postproc.detect_sources_banded`, genie_band_peaks_count / _fill).

* the band candidate kernel against `row_select(x, th, 1)` on the full matrix: the ranks' triplets put together are the full
  matrix's, exactly, for every cut of the axis into two own ranges and for fixed cuts into three and five (own ranges of width 1 and 0
  among them); the edge flag rises exactly where a band cannot decide a flat top, and the triplets are then not used;
* every rank in this process (tuple form): each rank's completed band is bit-equal to the same columns of the rank-ordered sum of the
  dense partials, and detection from the bands equals `detect_sources_device` on that sum, row for row;
* one process per rank over gloo on one GPU (2 and 3 ranks) and a one-rank RCCL group: the sources and the `detect_refine_associate`
  dict of one GPU on every rank, the forced dense fallback included.
"""
import datetime
import functools
import os
import time

import numpy as np
import pytest
import torch

from genie_amd import apply, module, postproc, synthetic
from tests.peak_cases import THR, TOP, by_row_col as _by_row_col, matrix as _planted, trip as _trip
from tests.util import Case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_COLS = [3, 40, 64, 65, 257]       # 64 and 65: a band that ends exactly at, and one past, a chunk's last lane


# ---- the kernel against row_select on the full matrix ---------------------------------------------------------------------------------------

def _runs(x, thr):
    """Every maximal run of equal values >= thr of the full matrix: (row, start, end inclusive, lower on the left, lower on the right)."""
    rows, n = x.shape
    brk = np.ones((rows, n + 1), dtype=bool)
    brk[:, 1:n] = x[:, 1:] != x[:, :-1]
    out = []
    for r in range(rows):
        edges = np.flatnonzero(brk[r])
        s, e = edges[:-1], edges[1:] - 1
        v = x[r, s]
        keep = v >= thr
        s, e, v = s[keep], e[keep], v[keep]
        ll = (s > 0) & (x[r, np.maximum(s - 1, 0)] < v)
        rl = (e < n - 1) & (x[r, np.minimum(e + 1, n - 1)] < v)
        out.append(np.stack((np.full(s.shape, r), s, e, ll, rl), axis=1))
    return np.concatenate(out).astype(np.int64)


def _undecidable(runs, n, b_lo, b_hi, o_lo, o_hi):
    """Whether the band [b_lo, b_hi) of an axis of n columns can NOT decide the candidates of the own range [o_lo, o_hi): some run
    reaches an end of the band that is not an end of the axis (so that its true start / end is only bounded: start in [1, b_lo], end
    in [b_hi - 1, n - 2]), the neighbour on each side that the band does see is lower, and one of the midpoints the bounds admit lies
    in the own range; an empty own range holds no midpoint. This restates on the host the rule the kernel documents (the same bounds
    on the midpoint), so it pins the kernel to its specification band by band but is no independent oracle. The independent checks of
    the flag are `_spans` (read off the matrix: where it is False no rank may raise the flag), the planted flat tops (cuts inside
    them must raise it, cuts at their ends must not, a rank that owns nothing must not), and the triplets' equality with `row_select`
    wherever the flag stays down."""
    if o_lo >= o_hi:
        return False
    S, E, ll, rl = runs[:, 1], runs[:, 2], runs[:, 3].astype(bool), runs[:, 4].astype(bool)
    inside = (E >= b_lo) & (S < b_hi)
    s, e = np.maximum(S, b_lo), np.minimum(E, b_hi - 1)
    lk, rk = S > b_lo, E < b_hi - 1                                        # the band sees the column before the start / after the end
    lok = np.where(lk, ll, b_lo > 0)
    rok = np.where(rk, rl, b_hi < n)
    m_lo = (np.where(lk, s, 1) + e) // 2
    m_hi = (s + np.where(rk, e, n - 2)) // 2
    return bool((inside & lok & rok & ~(lk & rk) & (m_hi >= o_lo) & (m_lo < o_hi)).any())


def _spans(runs, cut):
    """A run >= thr holds both columns next to the cut: a flat stretch longer than the margin of 1 at that cut."""
    return bool(((runs[:, 1] < cut) & (runs[:, 2] >= cut)).any())


def _ranks(xd, n_cols, cuts, thr, margin=1):
    """The ranks' triplets (host arrays, concatenated in rank order) and flags for own ranges [cuts[k], cuts[k + 1])."""
    trip, flags, bands = [], [], []
    for o_lo, o_hi in zip(cuts[:-1], cuts[1:]):
        b_lo, b_hi = max(o_lo - margin, 0), min(o_hi + margin, n_cols)
        band = xd[:, b_lo:b_hi]
        assert band.shape[0] == 1 or band.stride(0) > band.shape[1]
        r, c, v, off, flag = postproc.band_peaks(band, b_lo, o_lo, o_hi, n_cols, thr)
        assert off.dtype == torch.int64 and off.numel() == xd.shape[0]
        cnt = torch.bincount(r.long(), minlength=xd.shape[0])
        assert torch.equal(off, torch.cumsum(cnt, 0) - cnt)                # the exclusive row offsets genie_peak_distance walks by
        trip.append(_trip(r, c, v))
        flags.append(bool(flag.item()))
        bands.append((b_lo, b_hi, o_lo, o_hi))
    return trip, flags, bands


@functools.lru_cache(maxsize=None)
def _case(rows, n_cols):
    x, xd = _planted(rows, n_cols, 100 * rows + n_cols, DEV, streamed=False)
    r, c, v = postproc.row_select(xd.contiguous(), THR, 1)                 # the reference: computed once per shape
    return x, xd, _trip(r, c, v), _runs(x, THR)


@pytest.mark.parametrize("n_cols", N_COLS)
@pytest.mark.parametrize("rows", [1, 3, 70])
def test_band_peaks_of_two_ranks_equal_row_select_at_every_cut(rows, n_cols):
    x, xd, want, runs = _case(rows, n_cols)
    assert len(want) >= 1 and (want[:, 1] == 1).any() and (want[:, 1] == n_cols - 2).any()
    assert n_cols < 40 or ((want[:, 2].view(np.float32) == np.float32(THR)).any() and 11 in want[:, 1] and 21 in want[:, 1])
    assert rows < 3 or not (want[:, 0] == 2).any()
    decided = raised = quiet = 0
    for cut in range(n_cols + 1):                                          # own ranges [0, cut) and [cut, n_cols): widths 0 and 1 included
        trip, flags, bands = _ranks(xd, n_cols, [0, cut, n_cols], THR)
        for (b_lo, b_hi, o_lo, o_hi), flag, t in zip(bands, flags, trip):
            assert flag == _undecidable(runs, n_cols, b_lo, b_hi, o_lo, o_hi), (cut, b_lo, b_hi)
            assert np.array_equal(t, _by_row_col(t))                       # row-major, columns ascending within a row
            assert ((t[:, 1] >= o_lo) & (t[:, 1] < o_hi)).all()
        if not _spans(runs, cut):                                          # no flat stretch >= thr longer than the margin at the cut:
            assert not any(flags), cut                                     # the flag must not rise
            quiet += 1
        if any(flags):
            raised += 1
            continue
        got = np.concatenate(trip)
        assert np.array_equal(_by_row_col(got), want), cut                 # no duplicate, no miss, the same bits
        decided += 1
    assert decided >= 2 and quiet >= 2                                     # (cuts 0 and n_cols leave one band = the whole axis)
    if n_cols >= 40:
        assert raised >= 3
        for cut in (11, 12, 13, 21, 22):                                   # the planted flat tops, wider than the margin at these cuts
            assert any(_ranks(xd, n_cols, [0, cut, n_cols], THR)[1]), cut
        if rows == 1:                                                      # (other rows' noise may flag these cuts; row 0 alone must not)
            for cut in (10, 14, 20, 23):                                   # the tops end exactly at o_hi - 1 / begin exactly at o_lo
                assert not any(_ranks(xd, n_cols, [0, cut, n_cols], THR)[1]), cut


@pytest.mark.parametrize("n_cols", N_COLS)
@pytest.mark.parametrize("rows", [1, 3, 70])
def test_band_peaks_of_three_and_five_ranks_equal_row_select(rows, n_cols):
    x, xd, want, runs = _case(rows, n_cols)
    if n_cols == 3:
        splits = [[0, 1, 2, 3], [0, 1, 1, 3], [0, 0, 1, 2, 3, 3], [0, 2, 2, 2, 3, 3]]
    else:                                                                   # cuts at the planted tops' ends, own ranges of width 1 and 0
        splits = [[0, 10, 14, n_cols], [0, 14, 15, n_cols], [0, 20, 20, n_cols], [0, 1, 10, 14, 23, n_cols],
                  [0, 10, 10, 11, n_cols - 1, n_cols], [0, 14, 20, 23, 23, n_cols]]
    decided = 0
    for cuts in splits:
        for margin in (1, 3, 70):
            trip, flags, bands = _ranks(xd, n_cols, cuts, THR, margin)
            for (b_lo, b_hi, o_lo, o_hi), flag, t in zip(bands, flags, trip):
                assert flag == _undecidable(runs, n_cols, b_lo, b_hi, o_lo, o_hi), (cuts, margin, b_lo, b_hi)
                assert o_lo < o_hi or (not flag and len(t) == 0), (cuts, margin)   # a rank that owns nothing reports and flags nothing
            if not any(flags):
                assert np.array_equal(_by_row_col(np.concatenate(trip)), want), (cuts, margin)
                decided += 1
    assert decided >= 2
    if n_cols >= 40:                          # an empty own range whose band [11, 13) lies inside the planted top 10..13: its two
        flags = _ranks(xd, n_cols, [0, 12, 12, n_cols], THR)[1]            # neighbours cannot decide the top and raise the flag, it must not
        assert flags[0] and not flags[1] and flags[2]
    if n_cols >= 40 and rows == 1:            # a margin wider than the planted tops decides every one of them
        assert not any(_ranks(xd, n_cols, [0, 12, 21, n_cols], THR, 6)[1])


@pytest.mark.parametrize("n_cols", [65, 257])
def test_band_peaks_on_runs_longer_than_a_chunk(n_cols):
    """Runs whose start a band reads back from the carry of an earlier chunk (the 8-level noise never yields one of 65 columns): a run
    over the whole axis (no peak; it begins at b_lo in every band) and a flat top on columns 2..n_cols - 3 (one peak; it begins inside
    the bands that see column 1). Two ranks at every cut, three ranks with a middle band that touches neither end of the axis."""
    x = np.zeros((2, n_cols), dtype=np.float32)
    x[0, :] = TOP
    x[1, 2:n_cols - 2] = TOP
    buf = torch.zeros((2, n_cols + 5), dtype=torch.float32, device=DEV)
    buf[:, 2:2 + n_cols] = torch.from_numpy(x).to(DEV)
    xd = buf[:, 2:2 + n_cols]
    want = _trip(*postproc.row_select(xd.contiguous(), THR, 1))
    assert want.tolist() == [[1, (2 + n_cols - 3) // 2, int(np.float32(TOP).view(np.int32))]]
    runs = _runs(x, THR)
    whole = xd[0:1]                                                         # the whole-axis run alone, read off the matrix, not off
    for cut in range(n_cols + 1):                                           # `_undecidable`: one of two ranks' bands always holds an end
        trip, flags, _ = _ranks(whole, n_cols, [0, cut, n_cols], THR)      # of the axis, so nothing is flagged and nothing reported
        assert not any(flags) and sum(len(t) for t in trip) == 0, cut
    for a, b in ((1, 2), (1, n_cols - 1), (20, 64), (63, 64), (3, n_cols - 3)):
        flags = _ranks(whole, n_cols, [0, a, b, n_cols], THR, margin=0)[1]  # the middle band sees neither end: it alone must flag
        assert flags == [False, True, False], (a, b)
    decided = raised = 0
    splits = [[0, cut, n_cols] for cut in range(n_cols + 1)] + [[0, 1, 2, n_cols], [0, 20, 64, n_cols], [0, 64, 65, n_cols], [0, 2, n_cols - 2, n_cols]]
    for cuts in splits:
        for margin in (1, 70):
            trip, flags, bands = _ranks(xd, n_cols, cuts, THR, margin)
            for (b_lo, b_hi, o_lo, o_hi), flag in zip(bands, flags):
                assert flag == _undecidable(runs, n_cols, b_lo, b_hi, o_lo, o_hi), (cuts, margin, b_lo, b_hi)
            raised += any(flags)
            if not any(flags):
                assert np.array_equal(_by_row_col(np.concatenate(trip)), want), (cuts, margin)
                decided += 1
    assert decided >= 4 and raised >= 4


def test_band_peaks_threshold_rounding_and_bad_arguments():
    x, xd, want, runs = _case(3, 40)
    r, c, v = postproc.row_select(xd.contiguous(), 0.3, 1)                 # 0.3 is no fp32 number: rounded as `row_select` rounds it
    trip, flags, _ = _ranks(xd, 40, [0, 40], 0.3)
    assert not flags[0] and np.array_equal(trip[0][:, 1], c.cpu().numpy()) and np.array_equal(trip[0][:, 0], r.cpu().numpy())
    with pytest.raises(Exception, match="genie_band_peaks_count"):
        postproc.band_peaks(xd[:, 5:20], 5, 3, 10, 40, THR)                # the own range leaves the band
    with pytest.raises(Exception, match="genie_band_peaks_count"):
        postproc.band_peaks(xd[:, 5:20], 30, 30, 35, 40, THR)              # the band leaves the axis
    with pytest.raises(ValueError):
        postproc.band_peaks(xd.t(), 0, 0, 3, 3, THR)                       # strided columns


# ---- every rank in this process (tuple form) ------------------------------------------------------------------------------------------------

def _net(geom, dev):
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=dev)
    net.load_state_dict({k: v.clone() for k, v in Case("cfg1_20x500").weights.items()})
    net.eval()
    net.set_adjacencies_base(torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src), torch.from_numpy(geom.edge_attr()).to(dev),
                             torch.from_numpy(geom.locs).float().to(dev), torch.from_numpy(geom.x_grid).float().to(dev))
    return net


@functools.lru_cache(maxsize=None)
def _day():
    """20 stations, 200 source nodes, 24 queries, picks over ~550 s: about 180 windows on the default 'half' schedule."""
    geom = synthetic.Geometry(20, 200, L=100e3, n_query=24, seed=11)
    P = synthetic.make_picks(geom, 1500, seed=12)
    P[:, 0] = P[:, 0] * 10.0 + 5000.0
    P = P[np.argsort(P[:, 0], kind="stable")]
    trv = geom.travel_times().astype(np.float32)
    return _net(geom, DEV), geom, P, trv, dict(max_t=float(np.ceil(trv.max() + 1.0)))


def _field(xq, ts, seed=23):
    """A few smooth space-time blobs on the queries `xq` and the axis `ts` (fp32 [Q, len(ts)]): sources for the detection to find,
    added to the stacked output of the random-weight model element by element (to a band and to the dense sum alike)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(xq), len(ts)), dtype=np.float32)
    span = ts[-1] - ts[0]
    for k, frac in enumerate((0.11, 0.13, 0.31, 0.4987, 0.52, 0.667, 0.81, 0.93)):
        c = xq[rng.integers(len(xq))]
        d = np.linalg.norm((xq[:, :3] - c[:3]) * np.array([1, 1, 0.3]), axis=1)
        out += (0.7 * np.exp(-0.5 * (d / 12e3) ** 2)[:, None] * np.exp(-0.5 * ((ts - (ts[0] + frac * span + 0.21)) / 3.0) ** 2)[None, :]).astype(np.float32)
    return out


DETECT = dict(thresh=0.15, src_t_kernel=5.0, dt_win=0.75, break_win=15.0, tc_win=6.75, sp_win=20e3)


def _detect_args(xq, ts):
    return (xq, ts, lambda x: x, DETECT["thresh"], DETECT["src_t_kernel"], DETECT["dt_win"], DETECT["break_win"], DETECT["tc_win"], DETECT["sp_win"])


def _complete_locally(bands):
    """The tuple form's exchange, every rank being here: each rank's strips are copied out of the senders' (still partial) bands, then
    every band is completed."""
    plan = bands[0].plan
    strips = [{p: bands[p].strip(a, b).clone() for p, a, b in plan["recv"][r]} for r in range(len(bands))]
    for r, band in enumerate(bands):
        assert not band.complete and band.rank == r and band.group is None
        band.add_strips(strips[r])
        assert band.complete
    return bands


def _check_bands_against_dense(run, world, xq, n_min):
    """`run(**kw)` -> (Out_2 or BandedOut2, times[, info]) of one rank. The dense partials summed in rank order are the reference."""
    tot, times, info = None, [], None
    for r in range(world):
        res = run(window_parallel=(r, world), return_info=True)
        tot = res[0].clone() if tot is None else tot + res[0]              # fp32, rank order, from the first partial (0 + p = p)
        times.append(res[1])
        info = res[2]
    assert len(np.concatenate(times)) >= n_min and float(tot.abs().max()) > 0
    res = [run(window_parallel=(r, world), merge="columns") for r in range(world)]
    assert all(np.array_equal(a[1], b) for a, b in zip(res, times))
    bands = _complete_locally([a[0] for a in res])
    n_cols = tot.shape[1]
    plan = bands[0].plan
    assert plan["own"][0][0] == 0 and plan["own"][-1][1] == n_cols == bands[0].n_cols
    for b in bands:
        assert tuple(b.band.shape) == (tot.shape[0], b.b_hi - b.b_lo) and b.band.is_cuda
        assert torch.equal(b.band, tot[:, b.b_lo:b.b_hi]), b.rank         # every column of the band: the rank-ordered sum's bits
        dense = b.dense()
        assert tuple(dense.shape) == tuple(tot.shape) and torch.equal(dense[:, b.b_lo:b.b_hi], b.band)
        assert not bool(dense[:, :b.b_lo].any()) and not bool(dense[:, b.b_hi:].any())
    if world > 1 and n_min >= 100:
        assert max(b.band.shape[1] for b in bands) < 0.75 * n_cols         # bands, not copies of the axis
    ts = np.arange(n_cols) * 0.75 + 4990.0
    field = torch.from_numpy(_field(xq, ts)).to(DEV)
    for b in bands:
        b.band += field[:, b.b_lo:b.b_hi]
    want = postproc.detect_sources_device(tot + field, *_detect_args(xq, ts))
    got, dinfo = postproc.detect_sources_banded(bands, *_detect_args(xq, ts))
    assert dinfo["fallback"] is None and len(dinfo["candidates"]) == world
    assert len(want) >= 3 and got.dtype == want.dtype and np.array_equal(got, want)
    return info, bands


@pytest.mark.parametrize("tail_batch", [1, 16])
@pytest.mark.parametrize("world", [2, 3, 5])
def test_completed_bands_are_the_rank_ordered_dense_sum_and_detect_alike(world, tail_batch):
    net, geom, P, trv, kw = _day()
    run = lambda **k: apply.apply_windows_device(net, geom, P, trv, tail_batch=tail_batch, **dict(kw, **k))
    info, bands = _check_bands_against_dense(run, world, geom.x_query, 100)
    assert info["exact_merge"]


def test_bands_of_a_tiny_day_whose_columns_three_ranks_feed():
    """24 windows at a 1 s stride over 8 ranks: six windows feed a column, three ranks among them, so `exact_merge` is False and a
    band adds two lower ranks' strips before its own part."""
    net, geom, P, trv, kw = _day()
    tsteps, offsets, step, n_overlap, dt_win = apply.window_schedule(P[:, 0], kw["max_t"], t_win=6.0, step_size="half")
    tsteps_abs = np.arange(tsteps.min() - 3.0, tsteps.max() + 3.0 + dt_win, dt_win)[:200]
    times = tsteps_abs[60] + 0.3 + 1.0 * np.arange(24)                     # (inside the stretch of the day that has picks)
    run = lambda **k: apply.apply_windows_device(net, geom, P, trv, tail_batch=4, tsteps_abs=tsteps_abs, times=times, **dict(kw, **k))
    info, bands = _check_bands_against_dense(run, 8, geom.x_query, 24)
    assert not info["exact_merge"] and info["ranks_per_column"].max() >= 3
    assert any(sum(1 for p, _, _ in bands[0].plan["recv"][r] if p < r) >= 2 for r in range(8))


def test_bands_of_a_two_leg_day():
    net, geom, P, trv, kw = _day()
    legs = [apply.GridLeg(net, geom.x_grid, trv), apply.GridLeg(_net(geom, DEV), geom.x_grid, trv)]
    picks = apply.ResidentPicks(P, np.arange(20), 20, DEV)
    run = lambda **k: apply.apply_windows_legs(legs, picks, geom.x_query, geom.locs, kw["max_t"], tail_batch=16, **k)
    _check_bands_against_dense(run, 3, geom.x_query, 100)


def test_columns_merge_refuses_what_it_cannot_split():
    net, geom, P, trv, kw = _day()
    with pytest.raises(ValueError, match="window_parallel"):
        apply.apply_windows_device(net, geom, P, trv, merge="columns", **kw)
    tsteps, offsets, step, n_overlap, dt_win = apply.window_schedule(P[:, 0], kw["max_t"], t_win=6.0, step_size="half")
    down = np.arange(tsteps.min() - 3.0, tsteps.max() + 3.0 + dt_win, dt_win)[::-1].copy()
    with pytest.raises(ValueError, match='merge="dense"'):
        apply.apply_windows_device(net, geom, P, trv, merge="columns", window_parallel=(0, 2), tsteps_abs=down, **kw)
    band = apply.apply_windows_device(net, geom, P, trv, merge="columns", window_parallel=(0, 2), **kw)[0]
    with pytest.raises(ValueError, match="all 2 ranks"):
        postproc.detect_sources_banded(band, *_detect_args(geom.x_query, np.arange(band.n_cols) * 0.75))
    with pytest.raises(ValueError, match="detect_on_device"):
        apply.detect_refine_associate([apply.GridLeg(net, geom.x_grid, trv)], None, band, *([None] * 20))


# ---- one process per rank ---------------------------------------------------------------------------------------------------------------------

def _group_day(s, **kw):
    """The day of tests/test_day_loops_gpu.py's `_Setup` (16 windows, 69 columns) on 150 queries: (Out_2 or BandedOut2, xq, ts, field)."""
    rng = np.random.default_rng(23)
    xq = np.c_[rng.uniform(0, 60e3, (150, 2)), rng.uniform(-30e3, 0, 150)]
    res = apply.apply_windows_legs([s.leg], s.picks, xq, s.locs, s.max_t, kernel_sig_t=s.sig, dt_embed=s.dt, return_info=True, **kw)
    plan = apply._day_plan(s.picks.t_host, s.max_t, 86400.0, 6.0, "half", 1, None, None, s.sig, 1.0, None, False)
    ts = plan.tsteps_abs
    return res, xq, ts, torch.from_numpy(_field(xq, ts)).to(DEV)


def _plant(out, b_lo, cut):
    """A constant stretch of 24 columns across the cut, above everything else in its row (the blobs reach 0.7 each): a flat top no band
    at that cut can decide."""
    lo, hi = np.clip([cut - 12 - b_lo, cut + 12 - b_lo], 0, out.shape[1])
    out[5, lo:hi] = 4.0
    return out


def _chain_dict(s, Out_2, xq, ts):
    from tests.test_source_parallel_gpu import IDENT, OFF_MIN, OFF_RNG, RANGES

    def trv(locs, srcs):
        d = torch.linalg.norm(locs[None, :, :] - srcs[:, None, :], dim=2)
        return torch.stack((d / 6000.0, d / 3500.0), dim=2)

    got = apply.detect_refine_associate([s.leg], s.picks, Out_2, xq, ts, s.locs, trv, s.tq, s.max_t, IDENT, IDENT, *RANGES, OFF_MIN, OFF_RNG,
                                        200, DETECT["thresh"], DETECT["src_t_kernel"], DETECT["dt_win"], DETECT["break_win"], DETECT["tc_win"],
                                        DETECT["sp_win"], rand=np.random.RandomState(3).rand, ftrns2_device=IDENT, kernel_sig_t=s.sig,
                                        dt_embed=s.dt, detect_on_device=True)
    torch.cuda.synchronize()
    if isinstance(Out_2, apply.BandedOut2):              # the banded detection's own info, handed through (a fallback would show here)
        assert got["detect_info"] == postproc.detect_sources_banded(Out_2, *_detect_args(xq, ts))[1] and got["detect_info"]["fallback"] is None
    else:
        assert "detect_info" not in got
    return {"srcs": got["srcs"], "srcs_refined": got["srcs_refined"], "trv_out_srcs": got["trv_out_srcs"].cpu().numpy(),
            "Out_p_save": [o.cpu().numpy() for o in got["Out_p_save"]], "Out_s_save": [o.cpu().numpy() for o in got["Out_s_save"]],
            "Save_picks": got["Save_picks"], "lp_meta": got["lp_meta"]}


@functools.lru_cache(maxsize=None)
def _one_gpu_day():
    """One GPU, dense: (Out_2 with the field, xq, ts, sources, the detect_refine_associate dict, times)."""
    from tests.test_day_loops_gpu import _Setup
    s = _Setup()
    (Out_2, times, info), xq, ts, field = _group_day(s)
    Out_2 = Out_2 + field
    return Out_2, xq, ts, postproc.detect_sources_device(Out_2, *_detect_args(xq, ts)), _chain_dict(s, Out_2, xq, ts), np.asarray(times)


def _one_gpu(cut):
    """(sources, dict, sources with the stretch planted across `cut`, times) of one GPU."""
    Out_2, xq, ts, srcs, chain, times = _one_gpu_day()
    planted = None if cut is None else postproc.detect_sources_device(_plant(Out_2.clone(), 0, cut), *_detect_args(xq, ts))
    return srcs, chain, planted, times


def _worker(rank, world, port, backend, ret):
    import torch.distributed as dist
    from tests.test_day_loops_gpu import _Setup
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(DEV)
    timeout = datetime.timedelta(seconds=60)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(DEV), timeout=timeout)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timeout)
    try:
        s = _Setup()
        (banded, times, info), xq, ts, field = _group_day(s, window_parallel=True, merge="columns")
        assert banded.complete and banded.rank == rank and banded.n_cols == len(ts)
        banded.band += field[:, banded.b_lo:banded.b_hi]
        srcs, dinfo = postproc.detect_sources_banded(banded, *_detect_args(xq, ts))
        chain = _chain_dict(s, banded, xq, ts)
        planted, pinfo = None, None
        if world > 1:
            cut = banded.plan["own"][1][0]
            forced = apply.BandedOut2(_plant(banded.band.clone(), banded.b_lo, cut), rank, banded.plan, complete=True, group=banded.group,
                                      timeout=banded.timeout)
            planted, pinfo = postproc.detect_sources_banded(forced, *_detect_args(xq, ts))
        torch.cuda.synchronize()
        ret[rank] = (srcs, dinfo, chain, planted, pinfo, np.asarray(times), banded.plan["own"], tuple(banded.band.shape), info["exact_merge"],
                     dist.get_backend())
    finally:
        dist.destroy_process_group()


def _run_group(world, backend, limit=240.0):
    import torch.multiprocessing as mp
    from tests.test_source_parallel_gpu import _free_port, _same_dict
    mgr = mp.Manager()
    ret = mgr.dict()
    ctx = mp.spawn(_worker, args=(world, _free_port(), backend, ret), nprocs=world, join=False)
    deadline = time.monotonic() + limit
    try:
        while not ctx.join(timeout=5.0):                  # returns as soon as a rank ends; raises what a rank raised
            assert time.monotonic() < deadline, "a rank of the %s group of %d is stuck" % (backend, world)
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
            p.join(10.0)
    assert len(ret) == world
    own = ret[0][6]
    cut = own[1][0] if world > 1 else None
    srcs, chain, planted, times = _one_gpu(cut)
    assert len(srcs) >= 3 and len(chain["srcs_refined"]) >= 2
    for rank in range(world):
        g_srcs, dinfo, g_chain, g_planted, pinfo, g_times, g_own, shape, exact, be = ret[rank]
        assert be == backend and g_own == own and exact
        assert np.array_equal(g_times, times)                               # every rank returns the full list
        assert shape[0] == 150 and (world == 1 or shape[1] < 69)            # a band, not the axis
        assert dinfo["fallback"] is None and sum(dinfo["candidates"]) > 0
        assert g_srcs.dtype == srcs.dtype and np.array_equal(g_srcs, srcs)  # the sources of one GPU, row for row
        _same_dict(g_chain, chain)
        if world > 1:
            assert pinfo["fallback"] == "flat top at a band edge" == postproc.BAND_FALLBACK
            assert np.array_equal(g_planted, planted) and not np.array_equal(planted, srcs)


def test_banded_day_two_processes_on_one_gpu_over_gloo():
    _run_group(2, "gloo")


def test_banded_day_three_processes_on_one_gpu_over_gloo():
    _run_group(3, "gloo")


def test_banded_day_world1_rccl():
    """A one-rank RCCL group: the device branch of the strip exchange (nothing to exchange) and a band that is the whole axis."""
    _run_group(1, "nccl")
