"""GPU: source detection on the closed columns of the online day loop as they arrive (`postproc.StreamPeaks`, `postproc.OnlineDetector`,
genie_stream_peaks_count / _fill).

* the streaming candidate kernel against `row_select(x, th, 1)` on the whole matrix: for every single cut of the axis, for random
  multi-block partitions (widths 0, 1, 63, 64, 65 and single columns among them), on contiguous blocks and on strided views, the pushes'
  triplets put together are the full matrix's, bit for bit, and a row's columns ascend from call to call;
* the bound of every push against its definition, restated on the host from the matrix;
* the detector on a synthetic field and behind the real online loop: the releases, concatenated, are `detect_sources_device` on the
  offline matrix, row for row, with releases before the axis has ended.
Everything compares exactly; there is no tolerance in this file."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from genie_amd import _lib, apply, module, postproc, synthetic
from tests.peak_cases import THR, TOP, by_row_col as _by_row_col, matrix as _planted, trip as _trip
from tests.util import Case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = [1, 4, 5, 9]                 # the kernel works four rows per workgroup
N_COLS = [1, 2, 3, 64, 65, 130]


# ---- the kernel against row_select on the full matrix ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(rows, n_cols):
    x, xd = _planted(rows, n_cols, 100 * rows + n_cols, DEV, streamed=True)
    r, c, v = postproc.row_select(xd.contiguous(), THR, 1)                 # the reference: computed once per shape
    return x, xd, _trip(r, c, v)


def _bound_of(x, seen, thr):
    """The bound after the columns [0, seen) of `x`, from its definition: `seen`, lowered to (start + seen - 1) // 2 for every row whose
    run through column seen - 1 goes on being open (seen < n_cols), reaches thr, rose and does not hold column 0."""
    n = x.shape[1]
    bound = seen
    if seen == 0 or seen == n:
        return bound
    for row in x:
        v = row[seen - 1]
        s = seen - 1
        while s > 0 and row[s - 1] == v:
            s -= 1
        if v >= thr and s > 0 and row[s - 1] < v:
            bound = min(bound, (s + seen - 1) // 2)
    return bound


def _stream(x, xd, cuts, thr=THR, contiguous=False):
    """Push the blocks [cuts[k], cuts[k + 1]) of `xd` through one StreamPeaks; checks every push's offsets and bound; returns the
    triplets in call order."""
    rows, n_cols = x.shape
    sp = postproc.StreamPeaks(rows, n_cols, thr, DEV)
    assert sp.seen == 0 and sp.bound == 0
    out, bounds = [np.zeros((0, 3), dtype=np.int32)], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        block = xd[:, a:b].contiguous() if contiguous else xd[:, a:b]
        assert contiguous or rows == 1 or b - a == 0 or block.stride(0) > block.shape[1]
        r, c, v, off = sp.push(a, block)
        assert sp.seen == b and r.dtype == c.dtype == torch.int32 and v.dtype == torch.float32 and r.is_cuda
        assert off.dtype == torch.int64 and off.numel() == rows
        cnt = torch.bincount(r.long(), minlength=rows)
        assert torch.equal(off, torch.cumsum(cnt, 0) - cnt)                # the exclusive row offsets genie_peak_distance walks by
        t = _trip(r, c, v)
        assert np.array_equal(t, _by_row_col(t))                           # row-major, columns ascending within a row
        for at, bd in bounds:
            assert (t[:, 1] >= bd).all(), (cuts, at, bd)                   # no later candidate lies below an earlier bound
        assert sp.bound == _bound_of(x, b, np.float32(thr)), (cuts, b)     # (== seen when no row ends the block in an open run >= thr)
        if b == 0 or b == n_cols or (x[:, b - 1] < np.float32(thr)).all():
            assert sp.bound == b
        bounds.append((b, sp.bound))
        out.append(t)
    assert sp.seen == n_cols and sp.bound == n_cols
    return np.concatenate(out)


def _check(got, want, what):
    assert np.array_equal(_by_row_col(got), want), what                    # no duplicate, no miss, the same bits
    assert np.array_equal(got[np.argsort(got[:, 0], kind="stable")], want), what     # within a row, across calls, columns ascend


@pytest.mark.parametrize("n_cols", N_COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_stream_peaks_equal_row_select_at_every_cut(rows, n_cols):
    x, xd, want = _case(rows, n_cols)
    if n_cols >= 64:
        assert {21, 41, 62} <= set(want[want[:, 0] == 0][:, 1]) and (want[:, 2].view(np.float32) == np.float32(THR)).any()
    if rows >= 2:
        assert (want[want[:, 0] == 1][:, 1] > 2).all() and (want[want[:, 0] == 1][:, 1] < n_cols - 3).all()
    assert rows < 4 or not (want[:, 0] == 3).any()
    for cut in range(n_cols + 1):                                          # widths 0 and n_cols included
        _check(_stream(x, xd, [0, cut, n_cols], contiguous=True), want, cut)


@pytest.mark.parametrize("n_cols", N_COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_stream_peaks_equal_row_select_on_multi_block_partitions(rows, n_cols):
    """Blocks that are strided views of a wider tensor."""
    x, xd, want = _case(rows, n_cols)
    rng = np.random.default_rng(7 * rows + n_cols)
    parts = [list(range(n_cols + 1))]                                      # single columns: every top of three columns spans three blocks
    if n_cols >= 64:
        parts += [[0, 20, 23, n_cols],                                     # the planted top 18..25 spans three blocks
                  [0, 26, n_cols], [0, 20, 26, 26, n_cols],                # ... and ends exactly on a block's last column
                  [0, 63, n_cols], [0, 64, n_cols], [0, 0, 1, 1, n_cols]]
    if n_cols == 130:
        parts += [[0, 65, 130], [0, 1, 64, 64, 129, 130], [0, 63, 127, 130], [0, 1, 66, 130]]      # widths 65, 63, 64, 1 and 0
    for _ in range(6):
        inner = np.sort(rng.integers(0, n_cols + 1, int(rng.integers(2, 9))))
        parts.append([0] + inner.tolist() + [n_cols])
    for cuts in parts:
        _check(_stream(x, xd, cuts), want, cuts)


@pytest.mark.parametrize("n_cols", N_COLS)
def test_a_flat_top_over_the_whole_axis_is_no_peak(n_cols):
    x = np.full((1, n_cols), TOP, dtype=np.float32)
    xd = torch.from_numpy(x).to(DEV)
    for cuts in ([0, n_cols], list(range(n_cols + 1)), [0, n_cols // 2, n_cols]):
        assert len(_stream(x, xd, cuts, contiguous=True)) == 0


def test_the_bound_on_hand_made_rows():
    x = np.zeros((3, 40), dtype=np.float32)
    x[0, 10:30] = 0.75                                                     # open from column 10 until it ends at 29: the peak is 19
    x[1, 5] = 1.0                                                          # decided in the first block
    x[1, 22:27] = 0.875                                                    # open at 25, ends at 26: the peak is 24
    x[2, 0:25] = 0.875                                                     # holds column 0: never a peak, never lowers the bound
    xd = torch.from_numpy(x).to(DEV)
    sp = postproc.StreamPeaks(3, 40, THR, DEV)
    t = _trip(*sp.push(0, xd[:, 0:20])[:3])
    assert t[:, :2].tolist() == [[1, 5]] and (sp.seen, sp.bound) == (20, (10 + 19) // 2)
    t = _trip(*sp.push(20, xd[:, 20:25])[:3])
    assert len(t) == 0 and (sp.seen, sp.bound) == (25, min((10 + 24) // 2, (22 + 24) // 2))
    t = _trip(*sp.push(25, xd[:, 25:25])[:3])                              # nothing arrives: nothing changes
    assert len(t) == 0 and (sp.seen, sp.bound) == (25, 17)
    t = _trip(*sp.push(25, xd[:, 25:28])[:3])                              # row 1 is decided, row 0 still open
    assert t[:, :2].tolist() == [[1, 24]] and (sp.seen, sp.bound) == (28, (10 + 27) // 2)
    t = _trip(*sp.push(28, xd[:, 28:40])[:3])
    assert t[:, :2].tolist() == [[0, 19]] and t[0, 2] == np.float32(0.75).view(np.int32) and (sp.seen, sp.bound) == (40, 40)


def test_count_and_fill_see_the_same_carry():
    """Blocks without a candidate skip FILL; the block that decides the carried run must still find the carry those calls left."""
    x = np.zeros((1, 12), dtype=np.float32)
    x[0, 1:5] = 0.75
    xd = torch.from_numpy(x).to(DEV)
    sp = postproc.StreamPeaks(1, 12, THR, DEV)
    assert sp.push(0, xd[:, 0:3])[0].numel() == 0 and sp.bound == (1 + 2) // 2
    assert sp.push(3, xd[:, 3:5])[0].numel() == 0 and sp.bound == (1 + 4) // 2
    t = _trip(*sp.push(5, xd[:, 5:8])[:3])
    assert t.tolist() == [[0, 2, int(np.float32(0.75).view(np.int32))]] and sp.bound == 8
    assert sp.push(8, xd[:, 8:12])[0].numel() == 0 and sp.bound == 12


def test_stream_peaks_threshold_rounding():
    x, xd, _ = _case(5, 65)
    r, c, v = postproc.row_select(xd.contiguous(), 0.3, 1)                 # 0.3 is no fp32 number: rounded as `row_select` rounds it
    _check(_stream(x, xd, [0, 17, 40, 65], thr=0.3), _trip(r, c, v), "thr 0.3")


# ---- the detector ---------------------------------------------------------------------------------------------------------------------------

DETECT = dict(thresh=0.15, src_t_kernel=5.0, dt_win=0.75, break_win=15.0, tc_win=6.75, sp_win=20e3)
BLOBS = (40, 46, 120, 123.5, 131, 260, 330, 333)


def _detect_args(xq, ts):
    return (xq, ts, lambda x: x, DETECT["thresh"], DETECT["src_t_kernel"], DETECT["dt_win"], DETECT["break_win"], DETECT["tc_win"], DETECT["sp_win"])


def _field(xq, ts, at, seed=23, bumps=None):
    """Smooth space-time blobs (those of tests/test_band_detect_gpu.py's `_field`) centred on the fractional columns `at` of the axis
    `ts`, quantised to 1/64 so that flat tops are common; `bumps` = (row, column): two narrow bumps (sigma = 1 column, unequal heights) 6
    columns apart on one row, of which the distance rule removes the lower."""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(xq), len(ts)), dtype=np.float64)
    col = np.arange(len(ts), dtype=np.float64)
    dt = ts[1] - ts[0]
    for a in at:
        c = xq[rng.integers(len(xq))]
        d = np.linalg.norm((xq[:, :3] - c[:3]) * np.array([1, 1, 0.3]), axis=1)
        out += 0.7 * np.exp(-0.5 * (d / 12e3) ** 2)[:, None] * np.exp(-0.5 * ((col - a) * dt / 3.0) ** 2)[None, :]
    if bumps is not None:
        out[bumps[0]] += 0.5 * np.exp(-0.5 * (col - bumps[1]) ** 2) + 0.40625 * np.exp(-0.5 * (col - bumps[1] - 6) ** 2)
    return (np.round(out * 64.0) / 64.0).astype(np.float32)


def _canon(s):
    """Rows in a canonical order: by time, then position, then height."""
    return s[np.lexsort((s[:, 4], s[:, 2], s[:, 1], s[:, 0], s[:, 3]))]


@functools.lru_cache(maxsize=None)
def _synthetic():
    geom = synthetic.Geometry(20, 200, L=100e3, n_query=24, seed=11)
    xq = np.asarray(geom.x_query, dtype=np.float64)
    ts = np.arange(400) * 0.75 + 4990.0
    full = torch.from_numpy(_field(xq, ts, BLOBS, bumps=(5, 200))).to(DEV)
    want = postproc.detect_sources_device(full, *_detect_args(xq, ts))
    # the offline stages, one by one: the distance rule and LocalMarching must each remove something, or the equality shows little
    d = int(1.5 * DETECT["src_t_kernel"] / DETECT["dt_win"])
    assert d == 10
    n_cand = postproc.row_select(full, DETECT["thresh"], 1)[0].numel()
    n_far = postproc.find_peaks_rows_device(full, DETECT["thresh"], d)[0].numel()
    assert n_cand > n_far > len(want) >= 3
    return xq, ts, full, want


def _detect_in_blocks(xq, ts, full, cuts):
    det = postproc.OnlineDetector(*_detect_args(xq, ts), device=DEV)
    assert det.held == 0 and det.seen == 0
    got, early, drops, t_last, new = [], 0, 0, -np.inf, []
    push = det.peaks.push
    det.peaks.push = lambda first, block: new.append(push(first, block)) or new[-1]       # (to count the candidates of each block)
    for a, b in zip(cuts[:-1], cuts[1:]):
        held = det.held
        s = det.push(a, full[:, a:b])
        n_new = new[-1][0].numel()
        assert s.dtype == np.float64 and s.ndim == 2 and s.shape[1] == 5 and det.seen == b
        assert np.array_equal(s[:, 3], np.sort(s[:, 3]))                   # sorted by time
        if len(s):
            assert t_last < s[0, 3]                                        # units come out in ascending time
            t_last = s[-1, 3]
        assert det.held <= held + n_new and (det.held < held + n_new) == (len(s) > 0)      # a release takes candidates out of `held`
        if len(s) and b < len(ts):
            early += 1
            drops += det.held < held
        got.append(s)
    assert drops >= min(early, 2)                                          # ... so that it drops, not only grows more slowly
    last = det.finish()
    assert det.held == 0 and len(last) == 0                                # the push that ended the axis released everything
    return np.concatenate(got + [last]), early


def test_detector_on_a_synthetic_field_equals_the_offline_detection():
    xq, ts, full, want = _synthetic()
    rng = np.random.default_rng(31)
    for trial in range(3):
        cuts = [0]
        while cuts[-1] < 400:
            cuts.append(min(cuts[-1] + int(rng.integers(0, 31)), 400))
        got, early = _detect_in_blocks(xq, ts, full, cuts)
        assert got.dtype == want.dtype == np.float64 and np.array_equal(_canon(got), _canon(want)), cuts
        assert early >= 2                                                  # sources before the axis has ended
    got, early = _detect_in_blocks(xq, ts, full, [0, 400])
    assert early == 0 and np.array_equal(_canon(got), _canon(want))


# ---- behind the real online loop ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _setup():
    """The small day of tests/test_online_day_gpu.py: 17 stations x 64 source nodes, 100 queries, 300 picks over ~100 s."""
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


def _cuts():
    """The irregular `t_now` values of tests/test_online_day_gpu.py: a repeated one, two neighbouring pick times, a jump of 30 s."""
    t = _setup()[2][:, 0]
    rng = np.random.default_rng(9)
    head = t[0] + np.cumsum(rng.uniform(0.2, 7.0, 8))
    k = int(np.searchsorted(t, head[-1])) + 2
    cuts = np.concatenate([head, [t[k], t[k + 1], t[k + 1]], t[k + 1] + 30.0 + np.cumsum(rng.uniform(0.5, 9.0, 6))])
    assert (np.diff(cuts) >= 0).all()
    return cuts


def test_detector_behind_the_online_day_loop():
    net, geom, P, trv, max_t, tsteps, ts = _setup()
    n_cols = len(ts)
    xq = np.asarray(geom.x_query, dtype=np.float64)
    field = torch.from_numpy(_field(xq, ts, [f * n_cols for f in (0.11, 0.13, 0.31, 0.4987, 0.52, 0.667, 0.81, 0.93)])).to(DEV)
    offline, _ = apply.apply_windows_device(net, geom, P, trv, tsteps_abs=ts, times=tsteps, max_t=max_t, tail_batch=16, stack_on_device=True)
    want = postproc.detect_sources_device(offline + field, *_detect_args(xq, ts))
    assert len(want) >= 3
    day = apply.OnlineDay(net, geom, trv, ts, times=tsteps, max_t=max_t, tail_batch=16)
    det = postproc.OnlineDetector(*_detect_args(xq, ts), device=DEV)
    got, lo = [], 0
    for t_now in _cuts():
        hi = int(np.searchsorted(P[:, 0], t_now, side="left"))
        first, block = day.feed(P[lo:hi], t_now)
        lo = hi
        got.append(det.push(first, block + field[:, first:first + block.shape[1]]))
    first, block = day.feed(P[lo:], np.inf)
    got.append(det.push(first, block + field[:, first:first + block.shape[1]]))
    got.append(det.finish())
    assert day.closed == n_cols == det.seen and det.held == 0
    got = np.concatenate(got)
    assert got.dtype == want.dtype and np.array_equal(_canon(got), _canon(want))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------

def test_refusals():
    xq, ts, full, _ = _synthetic()
    det = postproc.OnlineDetector(*_detect_args(xq, ts), device=DEV)
    det.push(0, full[:, 0:10])
    with pytest.raises(ValueError, match="next column"):
        det.push(11, full[:, 11:20])                                       # a gap
    with pytest.raises(ValueError, match="next column"):
        det.push(5, full[:, 5:20])                                         # an overlap
    with pytest.raises(ValueError, match="rows"):
        det.push(10, full[:5, 10:20])
    with pytest.raises(ValueError):
        det.push(10, full[:, 10:20].double())
    with pytest.raises(ValueError):
        det.push(10, full[:, 10:20].cpu())
    with pytest.raises(ValueError, match="contiguous"):
        det.push(10, full[:, 10:30:2])                                     # strided columns
    with pytest.raises(ValueError, match="finish"):
        det.finish()                                                       # before the axis has ended
    assert det.seen == 10                                                  # a refused push changes nothing
    det.push(10, full[:, 10:400])
    with pytest.raises(ValueError, match="leave the axis"):
        det.push(400, full[:, 0:1])                                        # after the end
    assert len(det.push(400, full[:, 400:400])) == 0 and len(det.finish()) == 0
    args = list(_detect_args(xq, ts))
    with pytest.raises(ValueError, match="0.01"):
        postproc.OnlineDetector(*(args[:3] + [0.01] + args[4:]), device=DEV)
    with pytest.raises(ValueError, match="distance"):
        postproc.OnlineDetector(*(args[:4] + [0.1] + args[5:]), device=DEV)           # src_t_kernel 0.1: d = 0
    with pytest.raises(ValueError, match="ascend"):
        postproc.OnlineDetector(*([xq, ts[::-1].copy()] + args[2:]), device=DEV)


def test_bad_arguments_return_err_arg_before_any_launch():
    lib = _lib.load()
    rows, width, n_cols = 3, 8, 40
    block = torch.zeros((rows, width), dtype=torch.float32, device=DEV)
    nbytes = int(lib.genie_stream_peaks_carry_bytes(rows))
    assert nbytes == 16 * rows and lib.genie_stream_peaks_carry_bytes(0) == 0
    cin, cout = (torch.zeros(nbytes // 8, dtype=torch.int64, device=DEV) for _ in range(2))
    counts = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    bound = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    off = torch.zeros(rows, dtype=torch.int64, device=DEV)
    o_r, o_c, o_v = (torch.zeros(4, dtype=dt, device=DEV) for dt in (torch.int32, torch.int32, torch.float32))
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    thr = ctypes.c_float(0.5)

    def count(block=block, rows=rows, width=width, stride=width, c0=0, n_cols=n_cols, cin=cin, cout=cout, counts=counts, bound=bound):
        return lib.genie_stream_peaks_count(p(block), rows, width, stride, c0, n_cols, thr, p(cin), p(cout), p(counts), p(bound), None)

    def fill(block=block, rows=rows, width=width, stride=width, c0=0, n_cols=n_cols, cin=cin, off=off, o_r=o_r, o_c=o_c, o_v=o_v):
        return lib.genie_stream_peaks_fill(p(block), rows, width, stride, c0, n_cols, thr, p(cin), p(off), p(o_r), p(o_c), p(o_v), None)

    GENIE_ERR_ARG = count(rows=-1)
    assert GENIE_ERR_ARG != 0
    for fn, name, nulls in ((count, b"genie_stream_peaks_count", ("block", "cin", "cout", "counts", "bound")),
                            (fill, b"genie_stream_peaks_fill", ("block", "cin", "off", "o_r", "o_c", "o_v"))):
        bad = [dict(rows=-1), dict(width=-1), dict(n_cols=-1), dict(c0=-1), dict(c0=n_cols - width + 1), dict(width=n_cols + 1, stride=n_cols + 1),
               dict(stride=width - 1), dict(n_cols=1 << 31)] + [{k: None} for k in nulls]
        for kw in bad:
            assert fn(**kw) == GENIE_ERR_ARG, (name, kw)
            assert name in lib.genie_last_error(), (name, kw)
        assert fn(width=1, stride=0, n_cols=n_cols) == 0                   # a single column: the stride is free
        assert fn(width=0, block=None) == 0 and fn(rows=0, block=None) == 0          # nothing to do: no launch
    torch.cuda.synchronize()
    bound.fill_(-7)
    assert count(width=0) == 0
    torch.cuda.synchronize()
    assert int(bound.item()) == -7                                         # width 0: the bound stays as it is
