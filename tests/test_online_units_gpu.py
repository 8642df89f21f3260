"""GPU: bounded online detection (`postproc.OnlineDetector(max_unit_cols=M)`, `postproc.detect_sources_device(max_unit_cols=M)`) and
the column-count kernel the detector's release rule reads (`genie_col_counts`).

The field: 37 rows (not a multiple of the candidate kernels' 4 rows per workgroup) x 700 columns, d = 6, break_win = 20 columns,
M = 40. A quiet stretch with isolated bumps (natural cuts only), then from column 200 to the end of the axis an ACTIVE stretch in which
every gap between candidate columns is below d -- no natural cut, so the unbounded detector holds all of it until the axis ends -- with
flat tops across the chunk edges 256, 320 and 448 of the 64-column scanner. The field is chosen on the host (`_design`: a numpy
restatement of the candidates, `online_units` on them) so that the host twin shows at least three forced cuts.
Everything compares exactly; there is no tolerance in this file."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from genie_amd import _lib, postproc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS, N_COLS, M = 37, 700, 40
ACTIVE = 200                                                                # the active stretch: columns [ACTIVE, N_COLS - 4)
DETECT = dict(thresh=0.15, src_t_kernel=3.0, dt_win=0.75, break_win=15.0, tc_win=6.75, sp_win=20e3)
D = int(1.5 * DETECT["src_t_kernel"] / DETECT["dt_win"])
TS = np.arange(N_COLS) * 0.75 + 4990.0
WIDTHS = [1, 8, 28, 65]


def _args(xq):
    return (xq, TS, lambda x: x, DETECT["thresh"], DETECT["src_t_kernel"], DETECT["dt_win"], DETECT["break_win"], DETECT["tc_win"], DETECT["sp_win"])


def _host_candidates(x, thr):
    """(row, column) of every mode-1 candidate of `row_select`, restated from scipy's local maxima: a run that rose and falls, at its
    midpoint, never one that holds the first or last column."""
    out = []
    for row, xr in enumerate(x):
        i, last = 1, len(xr) - 1
        while i < last:
            if xr[i - 1] < xr[i]:
                j = i + 1
                while j < last and xr[j] == xr[i]:
                    j += 1
                if xr[j] < xr[i] and xr[i] >= np.float32(thr):
                    out.append((row, (i + j - 1) // 2))
                i = j
            else:
                i += 1
    return np.array(out, dtype=np.int64).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def _design():
    """The field and what the host says about it (no GPU): x fp32 [ROWS, N_COLS], the query positions, the host twin's unit ends."""
    rng = np.random.default_rng(41)
    xq = np.c_[rng.uniform(0, 60e3, (ROWS, 2)), rng.uniform(-20e3, 0, ROWS)]
    x = np.zeros((ROWS, N_COLS), dtype=np.float32)

    def bump(row, col, h):                                                  # a three-column bump, heights in 1/64
        for k, f in ((-1, 0.5), (0, 1.0), (1, 0.5)):
            x[row, col + k] = max(x[row, col + k], np.float32(np.round(h * f * 64.0) / 64.0))

    for row, col, h in ((3, 30, 0.5), (20, 80, 0.75), (20, 84, 0.5), (36, 84, 0.625), (9, 120, 0.5), (10, 150, 0.875), (36, 153, 0.5)):
        bump(row, col, h)                                                   # the quiet stretch: natural cuts; 80 / 84 meet in the distance rule
    col = ACTIVE
    while col < N_COLS - 5:                                                 # the active stretch: a bump every 2 to 5 columns, on 1 to 3 rows
        for row in rng.choice(ROWS, int(rng.integers(1, 4)), replace=False):
            bump(int(row), col, float(rng.integers(16, 60)) / 64.0)
        col += int(rng.integers(2, D))
    for row, lo, hi, h in ((4, 253, 260, 0.96875), (17, 318, 323, 0.953125), (36, 440, 457, 0.984375)):
        x[row, lo - 3:hi + 3] = 0.0                                         # flat tops over the scanner's chunk edges 256, 320 and 448
        x[row, lo:hi] = h
    cand = _host_candidates(x, DETECT["thresh"])
    cols = np.unique(cand[:, 1])
    active = cols[cols >= ACTIVE]
    assert active.size > 100 and N_COLS - active[-1] < 20 and np.diff(active).max() < D         # no natural cut from ACTIVE to the end
    assert active[0] - cols[cols < ACTIVE][-1] >= 20                        # ... and a natural one before it
    assert {256, 320, 448} <= set(cand[:, 1].tolist())
    ends = postproc.online_units(cand[:, 1], N_COLS, TS, D, DETECT["break_win"], M)
    assert len(ends) >= 3 + 1 and (np.diff(ends[ends >= ACTIVE]) <= M + D).all()
    return x, xq, cand, ends


@functools.lru_cache(maxsize=None)
def _case():
    x, xq, cand, ends = _design()
    full = torch.from_numpy(x).to(DEV)
    r, c, _ = postproc.row_select(full, DETECT["thresh"], 1)
    got = np.stack((r.cpu().numpy(), c.cpu().numpy()), axis=1).astype(np.int64)
    assert np.array_equal(got, cand)                                        # the design's candidates are the device's
    want = postproc.detect_sources_device(full, *_args(xq), max_unit_cols=M)             # the references: computed once
    free = postproc.detect_sources_device(full, *_args(xq))
    assert want.dtype == np.float64 and want.shape[1] == 5 and np.array_equal(want[:, 3], np.sort(want[:, 3]))
    return full, xq, cand, want, free


def _blocks(width):
    return [(a, min(a + width, N_COLS)) for a in range(0, N_COLS, width)]


def _run(det, full, blocks, check=True):
    """Push the blocks; the invariant after every push; returns the pushes' sources and how many of them came before the axis ended."""
    out, early = [], 0
    for a, b in blocks:
        s = det.push(a, full[:, a:b])
        assert s.dtype == np.float64 and s.ndim == 2 and s.shape[1] == 5 and det.seen == b
        first, bound = det.held_first_col, det.peaks.bound
        assert (first is None) == (det.held == 0)
        if check and det.max_unit_cols is not None:
            assert first is None or first >= bound or bound - first < det.max_unit_cols, (a, b, first, bound)
        cols = det.held_cols
        assert cols.dtype == np.int64 and len(cols) == det.held and (first is None or cols[0] == first) and (np.diff(cols) >= 0).all()
        early += len(s) if b < N_COLS else 0
        out.append(s)
    return out, early


def test_without_the_argument_the_active_stretch_waits_for_the_end_of_the_axis():
    full, xq, cand, want, free = _case()
    det = postproc.OnlineDetector(*_args(xq), device=DEV)
    assert det.max_unit_cols is None and det.held_first_col is None
    blocks = _blocks(28)
    out, _ = _run(det, full, blocks[:-1])
    got = np.concatenate(out)
    assert len(got) >= 3 and (got[:, 3] < TS[ACTIVE]).all()                 # the quiet stretch came out; of the active one, nothing
    below = cand[(cand[:, 1] >= ACTIVE) & (cand[:, 1] < det.peaks.bound)]
    assert det.held >= len(below) > 200 and det.held_first_col == cand[cand[:, 1] >= ACTIVE][:, 1].min()      # ... it is all held
    out += _run(det, full, blocks[-1:])[0] + [det.finish()]
    assert det.held == 0 and np.array_equal(np.concatenate(out), free)


@pytest.mark.parametrize("width", WIDTHS + [N_COLS])
def test_bounded_detector_equals_the_bounded_offline_detection(width):
    """Blocks of one width, the whole axis in one push among them. (The push that ends the axis releases everything -- the bound is
    then the end of the axis -- so `finish()` finds nothing left; it is still part of the concatenation.)"""
    full, xq, cand, want, free = _case()
    assert not np.array_equal(want, free)                                   # the bounded result is another one
    det = postproc.OnlineDetector(*_args(xq), device=DEV, max_unit_cols=M)
    out, early = _run(det, full, _blocks(width))
    out.append(det.finish())
    assert det.held == 0 and det.held_first_col is None
    got = np.concatenate(out)
    assert got.dtype == want.dtype and np.array_equal(got, want), width
    if width < N_COLS:
        assert early >= 10 and (np.concatenate(out[:-2])[:, 3] >= TS[ACTIVE]).sum() >= 10      # the active stretch comes out as it goes


def test_held_stays_bounded_through_the_active_stretch():
    full, xq, cand, want, free = _case()
    det = postproc.OnlineDetector(*_args(xq), device=DEV, max_unit_cols=M)
    peak = 0
    for a, b in _blocks(8):
        det.push(a, full[:, a:b])
        lag = det.seen - det.peaks.bound
        assert det.held <= ROWS * -(-(M + lag) // 2)                         # the documented bound, after every push
        peak = max(peak, det.held)
    assert 0 < peak < (cand[:, 1] >= ACTIVE).sum() // 4                     # a fraction of what the unbounded detector holds


def test_a_limit_of_the_whole_axis_is_the_unbounded_detection():
    full, xq, cand, want, free = _case()
    assert np.array_equal(postproc.detect_sources_device(full, *_args(xq), max_unit_cols=N_COLS), free)
    det = postproc.OnlineDetector(*_args(xq), device=DEV, max_unit_cols=N_COLS + 5)
    out, _ = _run(det, full, _blocks(65))
    assert np.array_equal(np.concatenate(out + [det.finish()]), free)
    with pytest.raises(ValueError, match="max_unit_cols"):
        postproc.OnlineDetector(*_args(xq), device=DEV, max_unit_cols=D - 1)
    with pytest.raises(ValueError, match="max_unit_cols"):
        postproc.detect_sources_device(full, *_args(xq), max_unit_cols=D - 1)
    assert postproc.OnlineDetector(*_args(xq), device=DEV, max_unit_cols=D).max_unit_cols == D


# ---- the column counts ----------------------------------------------------------------------------------------------------------------------

def _col_counts(cols, ring):
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    return _lib.load().genie_col_counts(p(cols), int(cols.numel()), p(ring), int(ring.numel()), None)


@pytest.mark.parametrize("W", [1, 97, 1024])
def test_col_counts_accumulate_to_the_bincount(W):
    rng = np.random.default_rng(W)
    ring = torch.zeros(W, dtype=torch.int32, device=DEV)
    want = np.zeros(W, dtype=np.int64)
    for n in (0, 1, 255, 256, 257, 100000):
        for how in ("random", "equal"):
            cols = rng.integers(0, 5000, n) if how == "random" else np.full(n, 3 * W + W // 2)          # columns that wrap the ring;
            dcols = torch.from_numpy(cols.astype(np.int32)).to(DEV)                                       # one column: worst contention
            assert _col_counts(dcols, ring) == 0
            want += np.bincount(cols % W, minlength=W)
            torch.cuda.synchronize()
            assert np.array_equal(ring.cpu().numpy().astype(np.int64), want), (n, how)
    assert want.sum() == 2 * (1 + 255 + 256 + 257 + 100000)


def test_col_counts_bad_arguments_return_err_arg_before_any_launch():
    lib = _lib.load()
    ring = torch.zeros(8, dtype=torch.int32, device=DEV)
    cols = torch.zeros(4, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for args in ((p(cols), -1, p(ring), 8), (p(cols), 4, p(ring), 0), (p(cols), 4, p(ring), 1 << 31), (None, 4, p(ring), 8),
                 (p(cols), 4, None, 8), (p(cols), 1 << 31, p(ring), 8)):
        assert lib.genie_col_counts(*args, None) != 0 and b"genie_col_counts" in lib.genie_last_error(), args
    assert lib.genie_col_counts(None, 0, None, 8, None) == 0               # nothing to count: no launch
    torch.cuda.synchronize()
    assert int(ring.sum().item()) == 0


def test_a_ring_grown_mid_stream_changes_nothing():
    full, xq, cand, want, free = _case()
    for limit, ref in ((M, want), (None, free)):
        det = postproc.OnlineDetector(*_args(xq), device=DEV, max_unit_cols=limit, ring_cols=4)
        sizes = []
        out = []
        for a, b in _blocks(28):
            out.append(det.push(a, full[:, a:b]))
            sizes.append(int(det._ring.numel()))
            live = np.zeros(sizes[-1], dtype=np.int64)                      # the ring holds exactly the held columns' counts
            np.add.at(live, det.held_cols % sizes[-1], 1)
            assert np.array_equal(det._ring.cpu().numpy().astype(np.int64), live), (limit, a)
        assert sizes[-1] > 4 and len(set(sizes)) >= 2                       # it grew mid-stream
        assert np.array_equal(np.concatenate(out + [det.finish()]), ref)


# ---- save and resume ------------------------------------------------------------------------------------------------------------------------

def test_save_mid_stretch_and_resume():
    full, xq, cand, want, free = _case()
    blocks = _blocks(28)
    k = 15                                                                  # 420 columns in: the middle of the active stretch
    for limit in (M, None):
        det = postproc.OnlineDetector(*_args(xq), device=DEV, max_unit_cols=limit)
        head, _ = _run(det, full, blocks[:k])
        assert det.held > 0 and det.held_first_col >= ACTIVE
        state = det.state_dict()
        assert ("max_unit_cols" in state["fingerprint"]) == (limit is not None)
        assert sorted(state) == ["fingerprint", "held_col", "held_cols_sorted", "held_row", "held_val", "peaks"]
        assert np.array_equal(state["held_cols_sorted"], np.sort(state["held_col"].numpy().astype(np.int64)))
        new = postproc.OnlineDetector(*_args(xq), device=DEV, max_unit_cols=limit, ring_cols=16)
        new.load_state_dict(state)
        assert (new.held, new.seen, new.held_first_col) == (det.held, det.seen, det.held_first_col)
        assert np.array_equal(new.held_cols, det.held_cols)
        tail_old, _ = _run(det, full, blocks[k:])
        tail_new, _ = _run(new, full, blocks[k:])
        assert len(tail_old) == len(tail_new) and all(np.array_equal(a, b) for a, b in zip(tail_old, tail_new))
        assert np.array_equal(np.concatenate(head + tail_new + [new.finish()]), want if limit else free)
        for other in (M + 1, None) if limit else (M,):
            with pytest.raises(ValueError, match="max_unit_cols"):
                postproc.OnlineDetector(*_args(xq), device=DEV, max_unit_cols=other).load_state_dict(state)
