"""Downstream reduction of the apply loop: from the stacked query output `Out_2` to initial source candidates,
`/root/reference/Code/process_continuous_days.py:812-885` and `LocalMarching` (`process_utils.py:40-100`).

What runs where:
* `Out_2 [n_query, n_time]` stays on the GPU. The threshold pre-filter (`np.where(Out_2 > 0.01)`, :812-813) and the local-maximum /
  height stage of `scipy.signal.find_peaks` (:846) are HIP kernels (`genie_row_select_count` / `genie_row_select_fill`): only
  the sparse `(query, time step, value)` triplets cross to the host (a day of 10 000 queries x 115 200 steps is 4.6 GB dense).
* The remaining steps work on those few triplets on the host, restated from the libraries the reference calls: the distance
  rule of `find_peaks` (scipy `_select_by_peak_distance`), the grouping by `break_win` (:856-870) and `LocalMarching` (max
  propagation over a space-time radius graph, `process_utils.py:40-100`; pinned to the reference by tests/golden/localmarching.npz).
  `detect_sources` takes this path. A day with a thousand events has ~5 * 10^5 triplets and the host LocalMarching then takes about a
  minute (profiles/EXPERIMENTS.md, "Source detection on the device"), so:
* `find_peaks_rows_device`, `local_marching_device` and `detect_sources_device` run the same three steps as HIP kernels
  (`genie_peak_distance`, `genie_time_groups`, `genie_local_marching`, csrc/detect_kernels.hpp): triplets, the sort by time, groups and
  the march stay on the GPU, `ftrns1` is applied once to the query positions on the host, and only the surviving [n, 5] rows come
  back. The host functions are their oracle (equal index sets and rows); they differ only where scipy itself is unspecified: of two
  equal peak heights closer than the distance, the device keeps the later column.
* `detect_sources_banded` is `detect_sources_device` for a window-parallel day that keeps `Out_2` in column bands (`apply.BandedOut2`):
  the candidates per band (`genie_band_peaks_*`), one all-gather of the triplets, the other stages replicated; `row_select` on the
  full matrix is the oracle of the band kernel (equal triplets).
* `OnlineDetector` is `detect_sources_device` for an `Out_2` that arrives in blocks of closed columns (`apply.OnlineDay`): the
  candidates per block with a row's open run carried from block to block (`StreamPeaks`, `genie_stream_peaks_*`), the other stages on
  finished stretches of the axis (`online_units`, read from per-column candidate counts kept on the device, `genie_col_counts`);
  `detect_sources_device` on the whole matrix is its oracle (equal rows), with the same `max_unit_cols` when units are bounded.
* `refine_select_device` is the end of the refine pass per candidate source (process_continuous_days.py:972-978): the sum of the grid
  legs' query read-outs, the region mask and the nested first-maximum argmax in one launch pair (`genie_refine_select`,
  csrc/select_kernels.hpp); the torch statements of `apply.refine_sources` it replaces are its oracle (exact, ties included).
* `refine_cloud_device` is the beginning of that pass per source (:929, :934): the random query cloud around a candidate source, drawn
  on the device by a keyed Philox4x64-10 (`genie_refine_cloud`, csrc/cloud_kernels.hpp); numpy's `Generator(Philox(...)).random` and the
  numpy statement of the cloud are its oracle (bit for bit).
"""
import ctypes

import numpy as np
import torch
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

from . import _lib, checkpoint


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _fp32_threshold(threshold, mode):
    """The device compares in fp32 where numpy / scipy compare the fp32 entries with a float64 threshold: the fp32 value (a Python
    float) that gives the same decisions. Mode 0 (`>`): the largest fp32 <= threshold; mode 1 (`>=`): the smallest fp32 >= threshold."""
    th = np.float32(threshold)
    if mode == 0 and float(th) > float(threshold):
        th = np.nextafter(th, np.float32(-np.inf))
    elif mode == 1 and float(th) < float(threshold):
        th = np.nextafter(th, np.float32(np.inf))
    return float(th)


def _check_peak_args(who, thresh, distance):
    """What every entry point of the peak search asks of `find_peaks`' height and distance."""
    if distance is not None and distance < 1:
        raise ValueError("`distance` must be greater or equal to 1")          # scipy's own check
    if not thresh > 0.01:
        # the reference runs find_peaks on the array REBUILT from `Out_2 > 0.01` (everything else zero, process_continuous_days.py:812-846);
        # that equals find_peaks on Out_2 itself only for thresholds above the sparsification level
        raise ValueError("%s: the peak height must be > 0.01 (the reference's sparsification threshold)" % who)


def _count_scan_fill(rows, dev, count, fill, extra=None):
    """The two-pass selection every candidate kernel is driven by: `count(counts)` launches the pass that writes the rows' int32
    counts, `fill(offsets, out_row, out_col, out_val)` the pass that writes the triplets at the exclusive int64 row offsets (skipped
    when there are none). Returns (out_row, out_col, out_val, offsets), plus the host value of the device scalar `extra` (an int64
    tensor [1] that `count` wrote) when one is given: the total and `extra` cross in the ONE host read of the call."""
    with torch.cuda.device(dev):
        counts = torch.empty(rows, dtype=torch.int32, device=dev)
        count(counts)
        ends = torch.cumsum(counts.long(), 0)
        offsets = (ends - counts.long()).contiguous()
        total = ends[-1:] if rows else ends.new_zeros(1)
        host = rows > 0 or extra is not None              # (an empty matrix without `extra` costs no host read)
        n, *got = (total if extra is None else torch.cat((total, extra))).tolist() if host else [0]
        out_row = torch.empty(n, dtype=torch.int32, device=dev)
        out_col = torch.empty(n, dtype=torch.int32, device=dev)
        out_val = torch.empty(n, dtype=torch.float32, device=dev)
        if n:
            fill(offsets, out_row, out_col, out_val)
    return (out_row, out_col, out_val, offsets, *got)


def _row_select_offsets(x, threshold, mode):
    """`row_select` plus the exclusive int64 row offsets of its triplets (what `genie_peak_distance` walks rows by)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2):
        raise ValueError("row_select: x must be a 2-D fp32 GPU tensor")
    if not x.is_contiguous():
        raise ValueError("row_select: x must be contiguous (a silent copy of a multi-GB Out_2 is not what the caller wants)")
    lib = _lib.load()
    rows, cols = int(x.shape[0]), int(x.shape[1])
    head = (_ptr(x), rows, cols, ctypes.c_float(_fp32_threshold(threshold, mode)), int(mode))
    st = _stream(x.device)
    return _count_scan_fill(
        rows, x.device,
        lambda counts: _lib.check(lib.genie_row_select_count(*head, _ptr(counts), st), "genie_row_select_count"),
        lambda offsets, *out: _lib.check(lib.genie_row_select_fill(*head, _ptr(offsets), *map(_ptr, out), st), "genie_row_select_fill"))


def row_select(x, threshold, mode):
    """Device selection over the rows of a contiguous fp32 GPU matrix `x [rows, cols]`; mode 0: entries > threshold; mode 1:
    local maxima (flat tops -> midpoint, never the first / last column) with value >= threshold. Returns (row int32, col int32,
    value fp32) GPU tensors in row-major order. The only host round trip is the total count (one integer)."""
    return _row_select_offsets(x, threshold, mode)[:3]


def sparse_above(Out_2, thresh=0.01):
    """`iz1, iz2 = np.where(Out_2 > 0.01)`; `Out_2_sparse = [iz1, iz2, Out_2[iz1, iz2]]` (process_continuous_days.py:812-813),
    computed on the device; returns numpy (iz1, iz2, values)."""
    r, c, v = row_select(Out_2, thresh, 0)
    return r.cpu().numpy().astype(np.int64), c.cpu().numpy().astype(np.int64), v.cpu().numpy()


def select_by_peak_distance(peaks, priority, distance):
    """The distance rule of scipy.signal.find_peaks (`_select_by_peak_distance`): walking from the highest-priority peak down,
    a kept peak removes every other peak closer than ceil(distance) samples. `peaks` sorted ascending. Returns a bool mask."""
    peaks = np.asarray(peaks, dtype=np.int64)
    n = peaks.shape[0]
    d = int(np.ceil(distance))
    keep = np.ones(n, dtype=bool)
    order = np.argsort(priority)
    for i in range(n - 1, -1, -1):
        j = order[i]
        if not keep[j]:
            continue
        k = j - 1
        while k >= 0 and peaks[j] - peaks[k] < d:
            keep[k] = False
            k -= 1
        k = j + 1
        while k < n and peaks[k] - peaks[j] < d:
            keep[k] = False
            k += 1
    return keep


def find_peaks_rows(Out_2, height, distance):
    """`find_peaks(Out[i, :], height = thresh, distance = d)` for every row i (process_continuous_days.py:846): candidates (local
    maxima reaching `height`) on the device, the distance rule per row on the host. Returns numpy (row, col, peak height),
    rows ascending, columns ascending within a row."""
    _check_peak_args("find_peaks_rows", height, distance)
    r, c, v = row_select(Out_2, height, 1)
    r, c, v = r.cpu().numpy().astype(np.int64), c.cpu().numpy().astype(np.int64), v.cpu().numpy()
    if distance is None or r.size == 0:
        return r, c, v
    keep = np.ones(r.size, dtype=bool)
    starts = np.flatnonzero(np.r_[True, r[1:] != r[:-1]])
    stops = np.r_[starts[1:], r.size]
    for a, b in zip(starts, stops):
        if b - a > 1:
            keep[a:b] = select_by_peak_distance(c[a:b], v[a:b], distance)
    return r[keep], c[keep], v[keep]


def initial_sources(Out_2, X_query, tsteps_abs, thresh, src_t_kernel, dt_win):
    """`srcs_init` [n, 5] = (query position (3), time, peak height) of every peak of every query row, sorted by time
    (process_continuous_days.py:843-855)."""
    r, c, v = find_peaks_rows(Out_2, thresh, int(1.5 * src_t_kernel / dt_win))
    if r.size == 0:
        return np.zeros((0, 5))
    xq, ts = np.asarray(X_query, dtype=np.float64), np.asarray(tsteps_abs, dtype=np.float64)
    srcs = np.concatenate((xq[r, 0:3], ts[c].reshape(-1, 1), v.astype(np.float64).reshape(-1, 1)), axis=1)
    return srcs[np.argsort(srcs[:, 3])]


def group_sources(srcs_init, break_win):
    """Disjoint groups of time-sorted sources separated by gaps >= break_win (process_continuous_days.py:856-870)."""
    if len(srcs_init) == 0:
        return []
    ibreak = np.where(np.diff(srcs_init[:, 3]) >= break_win)[0]
    edges = np.r_[0, ibreak + 1, len(srcs_init)]
    return [srcs_init[a:b] for a, b in zip(edges[:-1], edges[1:]) if b > a]


def local_marching(srcs, ftrns1, tc_win=5, sp_win=35e3, n_steps_max=100, tol=1e-12, scale_depth=1.0, use_directed=True):
    """`LocalMarching.forward` (process_utils.py:46-100): sources (rows `[x0, x1, x2, t, value]`) linked when within `tc_win`
    in time AND `sp_win` in (depth-scaled) space; the value of every node is replaced by the maximum over its in-neighbours
    (itself included) until nothing changes or `n_steps_max` steps; a node survives when its value is still its own
    (`torch.isclose(..., rtol = tol)`, fp32, atol 1e-8). `use_directed` keeps only the edges that carry a value upwards
    (`value[target] <= value[source]`, :63-66). Returns the surviving rows of `srcs`, in index order (the reference orders them
    by connected component; every caller re-sorts by time, process_continuous_days.py:891)."""
    srcs = np.asarray(srcs, dtype=np.float64)
    n = srcs.shape[0]
    if n == 0:
        return srcs
    scale_vec = np.array([1.0, 1.0, scale_depth]).reshape(1, -1)
    xs = ftrns1(srcs[:, 0:3]) * scale_vec
    lp_t = cKDTree(srcs[:, 3].reshape(-1, 1)).query_ball_point(srcs[:, 3].reshape(-1, 1), r=tc_win)
    lp_x = cKDTree(xs).query_ball_point(xs, r=sp_win)
    src_l, dst_l = [], []
    for i in range(n):
        nb = np.array(sorted(set(lp_t[i]).intersection(lp_x[i])), dtype=np.int64)
        src_l.append(nb)
        dst_l.append(np.full(nb.size, i, dtype=np.int64))
    e0, e1 = np.concatenate(src_l), np.concatenate(dst_l)                    # edge j = e0 -> i = e1
    ncomp, comp = connected_components(coo_matrix((np.ones(e0.size), (e0, e1)), shape=(n, n)), directed=False)
    size = np.bincount(comp, minlength=ncomp)
    val0 = srcs[:, 4].astype(np.float32)
    if use_directed:
        m = val0[e1] <= val0[e0]
        e0, e1 = e0[m], e1[m]
    vals = val0.copy()
    active = size[comp] > 1                                                    # singletons are kept as they are (:72-73)
    for _ in range(int(n_steps_max)):
        new = np.zeros(n, dtype=np.float32)                                    # aggr = 'max' of an empty set is 0 (torch_scatter)
        np.maximum.at(new, e1, vals[e0])
        new = np.where(active, new, vals)
        done = float(np.abs(new - vals).max()) <= tol
        vals = new
        if done:
            break
    keep = ~active | (np.abs(val0 - vals) <= 1e-8 + tol * np.abs(vals))       # torch.isclose(vals_initial, vals, rtol = tol)
    return srcs[keep]


def detect_sources(Out_2, X_query, tsteps_abs, ftrns1, thresh, src_t_kernel, dt_win, break_win, tc_win, sp_win,
                   scale_depth_clustering=0.2):
    """process_continuous_days.py:843-891 in one call: peaks of the device-resident `Out_2` -> time groups -> LocalMarching
    (`n_steps_max = 2, use_directed = False`, :879) -> sources sorted by time, [n, 5]."""
    groups = group_sources(initial_sources(Out_2, X_query, tsteps_abs, thresh, src_t_kernel, dt_win), break_win)
    out = []
    for g in groups:
        if len(g) == 1:
            out.append(g)
        else:
            k = local_marching(g, ftrns1, tc_win=tc_win, sp_win=sp_win, scale_depth=scale_depth_clustering, n_steps_max=2,
                               use_directed=False)
            if len(k):
                out.append(k)
    if not out:
        return np.zeros((0, 5))
    srcs = np.vstack(out)
    return srcs[np.argsort(srcs[:, 3])]


# ------------------------------------------------------------------------------------------------
# The same three stages on the device (genie_peak_distance / genie_time_groups / genie_local_marching, csrc/detect_kernels.hpp).
# The host functions above stay as they are and are the oracle of these: index sets and surviving rows are equal, not close.
# ------------------------------------------------------------------------------------------------
def find_peaks_rows_device(Out_2, height, distance):
    """`find_peaks_rows` without the host: candidates and the distance rule both on the device. Returns GPU tensors (row int32,
    col int32, peak height fp32), rows ascending, columns ascending within a row. Equal to `find_peaks_rows` wherever the distance
    rule is decided by heights; of two EQUAL heights closer than ceil(distance) the later column is kept (scipy decides that case
    by an unstable sort, so its own answer is not specified)."""
    _check_peak_args("find_peaks_rows_device", height, distance)
    r, c, v, offsets = _row_select_offsets(Out_2, height, 1)
    if distance is None or r.numel() == 0:
        return r, c, v
    keep = _peak_distance_keep(offsets, c, v, distance)
    return r[keep], c[keep], v[keep]


def _peak_distance_keep(offsets, c, v, distance):
    """Keep flags (bool GPU tensor) of the distance rule on row-major peak triplets: `offsets` [rows] int64 exclusive row offsets,
    `c` int32 columns (ascending within a row), `v` fp32 heights."""
    keep = torch.empty(c.numel(), dtype=torch.uint8, device=c.device)
    with torch.cuda.device(c.device):
        _lib.check(_lib.load().genie_peak_distance(_ptr(offsets), int(offsets.numel()), int(c.numel()), _ptr(c), _ptr(v),
                                                   int(np.ceil(distance)), _ptr(keep), _stream(c.device)), "genie_peak_distance")
    return keep.bool()


def _distance_rule_unsorted(r, c, v, rows, n_cols, distance):
    """The distance rule on GPU peak triplets of a [rows, n_cols] matrix in ANY order: sorted once by (row, col), row offsets,
    `_peak_distance_keep`. Returns the surviving triplets, row-major."""
    if r.numel() == 0:
        return r, c, v
    order = torch.sort(r.long() * int(n_cols) + c.long(), stable=True)[1]
    r, c, v = r[order].contiguous(), c[order].contiguous(), v[order].contiguous()
    counts = torch.bincount(r.long(), minlength=rows)
    keep = _peak_distance_keep((torch.cumsum(counts, 0) - counts).contiguous(), c, v, distance)
    return r[keep], c[keep], v[keep]


def time_groups_device(t, break_win):
    """Group number (int32 GPU tensor) of every entry of the ascending fp64 GPU tensor `t`: a new group starts where the gap to the
    predecessor is >= break_win (`group_sources`)."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.dim() == 1 and t.is_contiguous()):
        raise ValueError("time_groups_device: t must be a contiguous 1-D fp64 GPU tensor")
    lib = _lib.load()
    n = int(t.numel())
    group = torch.empty(n, dtype=torch.int32, device=t.device)
    scratch = torch.empty(int(lib.genie_time_groups_scratch_ints(n)), dtype=torch.int32, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(lib.genie_time_groups(_ptr(t), n, ctypes.c_double(float(break_win)), _ptr(scratch), _ptr(group), _stream(t.device)),
                   "genie_time_groups")
    return group


def _marching_keep(xs, t, val, group, tc_win, sp_win, n_steps_max, tol, use_directed):
    """Keep flags (bool GPU tensor) of LocalMarching on device tensors already sorted by time: xs [n, 3] fp64, t [n] fp64,
    val [n] fp32, group [n] int32 or None."""
    lib = _lib.load()
    n = int(t.numel())
    xs, t, val = xs.contiguous(), t.contiguous(), val.contiguous()
    group = group.contiguous() if group is not None else None
    keep = torch.empty(n, dtype=torch.uint8, device=t.device)
    scratch = torch.empty(int(lib.genie_local_marching_scratch_bytes(n)), dtype=torch.uint8, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(lib.genie_local_marching(_ptr(xs), _ptr(t), _ptr(val), _ptr(group), n,
                                            ctypes.c_double(float(tc_win)), ctypes.c_double(float(sp_win)), int(n_steps_max),
                                            ctypes.c_double(float(tol)), int(bool(use_directed)), _ptr(scratch), _ptr(keep),
                                            _stream(t.device)), "genie_local_marching")
    return keep.bool()


def local_marching_device(srcs, ftrns1, tc_win=5, sp_win=35e3, n_steps_max=100, tol=1e-12, scale_depth=1.0, use_directed=True,
                          device=None):
    """`local_marching` with the graph and the march on the device: same arguments, same surviving rows of `srcs` in index order.
    `ftrns1` and the depth scale are applied on the host (one call); nodes are sorted by time on the device and the flags mapped back."""
    srcs = np.asarray(srcs, dtype=np.float64)
    return srcs[local_marching_keep_device(srcs, ftrns1, tc_win, sp_win, n_steps_max, tol, scale_depth, use_directed, device)]


def local_marching_keep_device(srcs, ftrns1, tc_win=5, sp_win=35e3, n_steps_max=100, tol=1e-12, scale_depth=1.0, use_directed=True,
                               device=None):
    """The keep flags of `local_marching_device` (host bool [n], in the order of `srcs`): its survivors are `srcs[flags]`."""
    srcs = np.asarray(srcs, dtype=np.float64)
    n = srcs.shape[0]
    if n == 0:
        return np.zeros(0, dtype=bool)
    dev = torch.device("cuda" if device is None else device)
    xs = np.asarray(ftrns1(srcs[:, 0:3]), dtype=np.float64) * np.array([1.0, 1.0, scale_depth]).reshape(1, -1)
    xs_d = torch.from_numpy(np.ascontiguousarray(xs)).to(dev)
    t_d, order = torch.sort(torch.from_numpy(np.ascontiguousarray(srcs[:, 3])).to(dev), stable=True)
    val_d = torch.from_numpy(srcs[:, 4].astype(np.float32)).to(dev)
    keep_sorted = _marching_keep(xs_d[order], t_d, val_d[order], None, tc_win, sp_win, n_steps_max, tol, use_directed)
    keep = torch.empty_like(keep_sorted)
    keep[order] = keep_sorted
    return keep.cpu().numpy()


def detect_sources_device(Out_2, X_query, tsteps_abs, ftrns1, thresh, src_t_kernel, dt_win, break_win, tc_win, sp_win,
                          scale_depth_clustering=0.2, max_unit_cols=None):
    """`detect_sources` with every stage on the device: peaks and distance rule (`find_peaks_rows_device`), a stable sort by time,
    the time groups, LocalMarching within the groups (`n_steps_max = 2, use_directed = False`). `ftrns1` is applied once to the
    query positions on the host (every candidate sits on a query row). Only the surviving rows cross to the host: [n, 5], sorted by
    time, equal to the rows `detect_sources` returns (sources of equal time may come in another order).
    `max_unit_cols=M` (an integer >= the peak distance in columns; ValueError otherwise): the offline twin of
    `OnlineDetector(max_unit_cols=M)`. The candidates are cut into the units of `online_units` on the whole axis, every unit goes
    through the distance rule, the time groups and LocalMarching on its own, and the units' sources are concatenated in ascending time.
    Not the unbounded result: across a forced cut two peaks of a row closer than the distance both survive, and no time group and no
    march crosses it. M >= the number of columns gives the unbounded result."""
    d = int(1.5 * src_t_kernel / dt_win)
    if max_unit_cols is None:
        r, c, v = find_peaks_rows_device(Out_2, thresh, d)
        return _sources_from_peaks(r, c, v, X_query, tsteps_abs, ftrns1, break_win, tc_win, sp_win, scale_depth_clustering)
    _check_peak_args("detect_sources_device", thresh, d)
    _check_max_unit_cols("detect_sources_device", max_unit_cols, d)
    r, c, v = row_select(Out_2, thresh, 1)
    n_cols, rows = int(Out_2.shape[1]), int(Out_2.shape[0])
    if len(np.asarray(tsteps_abs).reshape(-1)) != n_cols:
        raise ValueError("detect_sources_device: tsteps_abs has %d entries, Out_2 %d columns" % (len(np.asarray(tsteps_abs).reshape(-1)), n_cols))
    out, prev = [np.zeros((0, 5))], -1
    for end in online_units(c.cpu().numpy(), n_cols, tsteps_abs, d, break_win, max_unit_cols).tolist():
        go = (c > prev) & (c <= end)
        u = _distance_rule_unsorted(r[go], c[go], v[go], rows, n_cols, d)
        out.append(_sources_from_peaks(*u, X_query, tsteps_abs, ftrns1, break_win, tc_win, sp_win, scale_depth_clustering))
        prev = end
    return np.concatenate(out)


def _sources_from_peaks(r, c, v, X_query, tsteps_abs, ftrns1, break_win, tc_win, sp_win, scale_depth_clustering):
    """The part of `detect_sources_device` after the peaks: GPU triplets (row, col, height) -> surviving sources [n, 5] on the host."""
    if r.numel() == 0:
        return np.zeros((0, 5))
    dev = r.device
    xq = np.asarray(X_query, dtype=np.float64)
    xs_q = np.asarray(ftrns1(xq[:, 0:3]), dtype=np.float64) * np.array([1.0, 1.0, scale_depth_clustering]).reshape(1, -1)
    ts_d = torch.from_numpy(np.ascontiguousarray(np.asarray(tsteps_abs, dtype=np.float64))).to(dev)
    t, order = torch.sort(ts_d[c.long()], stable=True)
    r, v = r[order].long(), v[order]
    group = time_groups_device(t, break_win)
    keep = _marching_keep(torch.from_numpy(np.ascontiguousarray(xs_q)).to(dev)[r], t, v, group, tc_win, sp_win, 2, 1e-12, False)
    xq_d = torch.from_numpy(np.ascontiguousarray(xq[:, 0:3])).to(dev)
    srcs = torch.cat((xq_d[r[keep]], t[keep].reshape(-1, 1), v[keep].double().reshape(-1, 1)), dim=1)
    return srcs.cpu().numpy()


# ------------------------------------------------------------------------------------------------
# Detection from column bands: a window-parallel day whose `Out_2` stays distributed (`apply.BandedOut2`, merge="columns").
# Only the candidate step of find_peaks is local (a pixel's two neighbours, or the extent of its flat top), so that is what runs per
# band (genie_band_peaks_*, csrc/detect_kernels.hpp); the distance rule is greedy along a whole row and the time groups and
# LocalMarching are global, so they run replicated on the gathered triplets, with the kernels above.
# ------------------------------------------------------------------------------------------------
BAND_FALLBACK = "flat top at a band edge"


def band_peaks(band, b_lo, o_lo, o_hi, n_cols, threshold):
    """The mode-1 candidates of `row_select` on the full matrix whose column lies in [o_lo, o_hi), found on the column band `band`
    [rows, width] = the global columns [b_lo, b_lo + width) of an axis of `n_cols` (an fp32 GPU matrix; rows may be strided, columns
    not). Returns (row int32, GLOBAL col int32, value fp32, exclusive int64 row offsets, flag): GPU tensors, row-major, columns ascending
    within a row; `flag` (int32 GPU tensor [1]) is non-zero when a flat top reached an end of the band that is not an end of the axis
    and could not be decided there -- the triplets are then incomplete and must not be used. Own ranges that partition the axis give
    every candidate of the full matrix exactly once."""
    if not (torch.is_tensor(band) and band.is_cuda and band.dtype == torch.float32 and band.dim() == 2):
        raise ValueError("band_peaks: band must be a 2-D fp32 GPU tensor")
    if band.shape[1] > 1 and band.stride(1) != 1:
        raise ValueError("band_peaks: the columns of band must be contiguous")
    lib = _lib.load()
    rows, width = int(band.shape[0]), int(band.shape[1])
    stride = int(band.stride(0)) if rows > 1 else width
    head = (_ptr(band), rows, width, stride, int(b_lo), int(o_lo), int(o_hi), int(n_cols), ctypes.c_float(_fp32_threshold(threshold, 1)))
    dev = band.device
    st = _stream(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    return _count_scan_fill(
        rows, dev,
        lambda counts: _lib.check(lib.genie_band_peaks_count(*head, _ptr(counts), _ptr(flag), st), "genie_band_peaks_count"),
        lambda offsets, *out: _lib.check(lib.genie_band_peaks_fill(*head, _ptr(offsets), *map(_ptr, out), _ptr(flag), st),
                                         "genie_band_peaks_fill")) + (flag,)


def detect_sources_banded(banded, X_query, tsteps_abs, ftrns1, thresh, src_t_kernel, dt_win, break_win, tc_win, sp_win,
                          scale_depth_clustering=0.2, group=None):
    """`detect_sources_device` of a day whose `Out_2` stays distributed in column bands: `banded` = this rank's completed
    `apply.BandedOut2` (group form of `merge="columns"`), or the list of ALL ranks' completed bands in rank order (every rank in one
    process: nothing is gathered). Returns (srcs [n, 5] as `detect_sources_device` returns them, info).
    * each rank finds the candidates it owns on its band (`band_peaks`);
    * with a group (`group`, default: the one the band came over; True = the default group) ONE `all_gather_object` carries the ranks'
      ragged triplets and edge flags through the host, as `apply.associate_sources` moves its ragged lists (a few thousand rows);
    * the lists are concatenated in rank order (row-major within a rank, not across ranks), sorted once on the device by (row, col),
      and the distance rule, the time groups and LocalMarching run replicated on the whole list (`_peak_distance_keep`,
      `_sources_from_peaks`): identical sources on every rank, those of one GPU on the merged `Out_2`.
    * if any rank's flat top reached a band edge undecided, EVERY rank falls back to the dense merge for this day: the ranks' own
      columns, one non-zero term per element, are summed into a full-size matrix (`_merge_partials`) and `detect_sources_device`
      runs on it; `info["fallback"]` is then "flat top at a band edge" (otherwise None).
    `info` also holds `candidates` (per rank) and `gathered_bytes` (what the all-gather moved per rank)."""
    from . import apply
    distance = int(1.5 * src_t_kernel / dt_win)
    _check_peak_args("detect_sources_banded", thresh, distance)
    bands = list(banded) if isinstance(banded, (list, tuple)) else [banded]
    if not bands or not all(isinstance(b, apply.BandedOut2) for b in bands):
        raise ValueError("detect_sources_banded: an apply.BandedOut2 (or the list of every rank's) expected")
    first = bands[0]
    if group is None:
        group = first.group
    world = first.plan["world"]
    if (len(bands) > 1 or group is None) and [b.rank for b in bands] != list(range(world)):
        raise ValueError("detect_sources_banded: without a process group the bands of all %d ranks are needed, in rank order" % world)
    for b in bands:
        if not b.complete and b.plan["recv"][b.rank]:
            raise ValueError("detect_sources_banded: the band of rank %d still lacks the other ranks' strips (BandedOut2.add_strips)" % b.rank)
    dev, n_cols, rows = first.band.device, first.n_cols, int(first.band.shape[0])
    found = [band_peaks(b.band, b.b_lo, b.o_lo, b.o_hi, b.n_cols, thresh) for b in bands]
    if len(bands) == 1 and world > 1:                                       # one all-gather of (row, col, value, flag) per rank
        import torch.distributed as dist
        r, c, v, _, flag = found[0]
        parts = [None] * world
        with torch.cuda.device(dev):
            dist.all_gather_object(parts, (r.cpu().numpy(), c.cpu().numpy(), v.cpu().numpy(), int(flag.item())),
                                   group=None if group is True else group)
    else:
        parts = [(r, c, v, int(flag.item())) for r, c, v, _, flag in found]
    info = {"fallback": None, "candidates": [int(len(p[0])) for p in parts], "gathered_bytes": [12 * int(len(p[0])) + 4 for p in parts]}
    args = (X_query, tsteps_abs, ftrns1, thresh, src_t_kernel, dt_win, break_win, tc_win, sp_win, scale_depth_clustering)
    if any(p[3] for p in parts):                                            # the same decision on every rank: all of them saw all flags
        info["fallback"] = BAND_FALLBACK
        dense = bands[0].own_dense()
        for b in bands[1:]:
            dense += b.own_dense()
        if len(bands) == 1 and world > 1:
            apply._merge_partials(dense, None if group is True else group, first.timeout)
        return detect_sources_device(dense, *args), info
    as_dev = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev).to(dt)
    r = torch.cat([as_dev(p[0], torch.int32) for p in parts])
    c = torch.cat([as_dev(p[1], torch.int32) for p in parts])
    v = torch.cat([as_dev(p[2], torch.float32) for p in parts])
    r, c, v = _distance_rule_unsorted(r, c, v, rows, n_cols, distance)
    return _sources_from_peaks(r, c, v, X_query, tsteps_abs, ftrns1, break_win, tc_win, sp_win, scale_depth_clustering), info


# ------------------------------------------------------------------------------------------------
# Detection from the closed columns of the online day loop (`apply.OnlineDay.feed` -> `(first_col, block)`), as they arrive.
# The candidate step carries a row's open run from block to block (genie_stream_peaks_*, csrc/detect_kernels.hpp: every flat top is
# decided exactly, there is no flag); the distance rule, the time groups and LocalMarching run, with the kernels above, on finished
# stretches of the axis that `online_release` hands over as soon as nothing later can change them.
# ------------------------------------------------------------------------------------------------
class StreamPeaks(object):
    """The mode-1 candidates of `row_select` on a matrix [rows, n_cols] that arrives in column blocks: owner of the two carry buffers
    of genie_stream_peaks_count / _fill. `push(first_col, block)` takes the next block (fp32 GPU matrix [rows, width] of the global
    columns [first_col, first_col + width); rows may be strided, columns not; width 0 is allowed and changes nothing) and returns
    (row int32, GLOBAL col int32, value fp32, exclusive int64 row offsets), GPU tensors of the kind `band_peaks` returns: every peak
    whose run ended with this block, among them a run carried in from earlier blocks (first in its row; its midpoint may lie several
    blocks back). Over all pushes the triplets are those of `row_select(full, threshold, 1)`; within a row the columns ascend, across
    calls too. `seen`: the next column expected. `bound` (a Python int, read together with the count: one host read per push): no
    candidate of any later push has a column below it; `n_cols` once the axis has ended. `state_dict()` / `load_state_dict(state)`:
    `seen`, `bound` and the carry the next push reads, into a new stream of the same rows, axis and threshold."""

    def __init__(self, rows, n_cols, threshold, device):
        self.rows, self.n_cols = int(rows), int(n_cols)
        if self.rows < 0 or not 0 <= self.n_cols < 1 << 31:
            raise ValueError("StreamPeaks: rows >= 0 and 0 <= n_cols < 2**31 required")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("StreamPeaks: a GPU device is required")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.threshold = _fp32_threshold(threshold, 1)
        self.seen, self.bound = 0, 0
        nbytes = max(int(_lib.load().genie_stream_peaks_carry_bytes(self.rows)), 16)
        self._carry = [torch.zeros(nbytes // 8, dtype=torch.int64, device=self.device) for _ in range(2)]     # [in, out]
        self._bound = torch.zeros(1, dtype=torch.int64, device=self.device)

    def push(self, first_col, block):
        if not (torch.is_tensor(block) and block.is_cuda and block.dtype == torch.float32 and block.dim() == 2):
            raise ValueError("StreamPeaks.push: block must be a 2-D fp32 GPU tensor")
        if block.device != self.device:
            raise ValueError("StreamPeaks.push: block is on %s, the stream on %s" % (block.device, self.device))
        rows, width = int(block.shape[0]), int(block.shape[1])
        if rows != self.rows:
            raise ValueError("StreamPeaks.push: block has %d rows, the stream %d" % (rows, self.rows))
        if int(first_col) != self.seen:
            raise ValueError("StreamPeaks.push: first_col = %d, but the next column of the stream is %d (blocks arrive in order, without gaps)"
                             % (int(first_col), self.seen))
        if self.seen + width > self.n_cols:
            raise ValueError("StreamPeaks.push: columns [%d, %d) leave the axis of %d columns" % (self.seen, self.seen + width, self.n_cols))
        if width > 1 and block.stride(1) != 1:
            raise ValueError("StreamPeaks.push: the columns of block must be contiguous")
        dev = self.device
        empty = lambda dt: torch.empty(0, dtype=dt, device=dev)
        if rows == 0 or width == 0:
            self.seen += width
            if rows == 0:
                self.bound = self.seen
            return empty(torch.int32), empty(torch.int32), empty(torch.float32), torch.zeros(rows, dtype=torch.int64, device=dev)
        lib = _lib.load()
        stride = int(block.stride(0)) if rows > 1 else width
        carry_in, carry_out = self._carry
        head = (_ptr(block), rows, width, stride, self.seen, self.n_cols, ctypes.c_float(self.threshold), _ptr(carry_in))
        st = _stream(dev)
        out_row, out_col, out_val, offsets, bound = _count_scan_fill(
            rows, dev,
            lambda counts: _lib.check(lib.genie_stream_peaks_count(*head, _ptr(carry_out), _ptr(counts), _ptr(self._bound), st),
                                      "genie_stream_peaks_count"),
            lambda offsets, *out: _lib.check(lib.genie_stream_peaks_fill(*head, _ptr(offsets), *map(_ptr, out), st), "genie_stream_peaks_fill"),
            extra=self._bound)                            # the count and the bound: the one host read of a push
        self._carry = [carry_out, carry_in]               # (FILL has read carry_in on this stream before the next COUNT overwrites it)
        self.seen += width
        self.bound = int(bound)
        return out_row, out_col, out_val, offsets

    def _fingerprint(self):
        return {"rows": self.rows, "n_cols": self.n_cols, "thresh": self.threshold}

    def _state(self):
        """`seen`, `bound` and the carry the next push reads (every row's open run across the last block edge; the other buffer of
        the pair is the next push's output, and the device `bound` is set by every push before it is read)."""
        return {"fingerprint": self._fingerprint(), "seen": int(self.seen), "bound": int(self.bound), "carry": self._carry[0]}

    def state_dict(self):
        return checkpoint.to_host(self._state())

    def _check_state(self, state):
        if self.seen:
            raise RuntimeError("StreamPeaks.load_state_dict: this stream has been pushed to; a state is loaded into a new one")
        checkpoint.check_fingerprint("StreamPeaks", state, self._fingerprint())
        carry = state["carry"]
        if not (torch.is_tensor(carry) and carry.dtype == torch.int64 and carry.shape == self._carry[0].shape):
            raise ValueError("StreamPeaks.load_state_dict: carry must be int64 [%d]" % self._carry[0].shape[0])

    def _load_state(self, state):
        self._carry[0].copy_(state["carry"])
        self.seen, self.bound = int(state["seen"]), int(state["bound"])

    def load_state_dict(self, state):
        """Into a stream nothing has been pushed to (RuntimeError otherwise) of the same rows, axis and threshold (ValueError naming
        the field otherwise, nothing changed); the next `push` continues the saved stream."""
        self._check_state(state)
        self._load_state(state)


def online_release(cols, bound, tsteps_abs, d, break_win):
    """How many of the held candidates' columns `cols` (ascending, repeats allowed) are final: the pure host rule of `OnlineDetector`.
    Let c_1 < ... < c_m be the distinct held columns below `bound` and c_{m+1} = `bound` (no later candidate has a column below it,
    `StreamPeaks.bound`; a held column at or above the bound waits behind it). A cut after c_i is valid when
        c_{i+1} - c_i >= d   and   tsteps_abs[c_{i+1}] - tsteps_abs[c_i] >= break_win;
    with `bound == len(tsteps_abs)` the axis has ended, nothing comes after c_m, and the last cut is always valid. Everything up to the
    LAST valid cut goes as one unit: returned is the number of entries of `cols` at or before it (0: nothing may go)."""
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    ts = np.asarray(tsteps_abs, dtype=np.float64)
    bound, n_cols = int(bound), len(ts)
    c = np.unique(cols[cols < bound])
    if c.size == 0:
        return 0
    if bound >= n_cols:
        return int(cols.size)                             # the axis has ended (every column is below n_cols)
    nxt = np.r_[c[1:], bound]
    valid = (nxt - c >= int(d)) & (ts[nxt] - ts[c] >= float(break_win))
    if not valid.any():
        return 0
    return int(np.searchsorted(cols, c[np.flatnonzero(valid)[-1]], side="right"))


def _check_max_unit_cols(who, max_unit_cols, d):
    if max_unit_cols is None:
        return None
    if int(max_unit_cols) != max_unit_cols or max_unit_cols < 1 or max_unit_cols < d:
        raise ValueError("%s: max_unit_cols must be an integer >= 1 and >= the peak distance (%d columns), or None" % (who, d))
    return int(max_unit_cols)


def online_units(cols, bound, tsteps_abs, d, break_win, max_unit_cols=None):
    """The unit rule of the detection, offline and online: the LAST COLUMN of every unit of the candidate columns `cols` (any order,
    repeats allowed) that is final under `bound`, ascending (int64, possibly empty). The unit of an entry holds the candidates of the
    columns after the entry before it (or from the start) up to it; every unit goes through the offline stages on its own, and every
    column above the last entry waits. `bound` as in `online_release`; `bound == len(tsteps_abs)` is the ended axis -- the one-shot
    form, which returns the units of the whole list.

    On the distinct columns c_1 < ... < c_m below the bound, with c_{m+1} = `bound`: a cut after c_i is NATURAL when
    c_{i+1} - c_i >= d and tsteps_abs[c_{i+1}] - tsteps_abs[c_i] >= break_win (after c_m always, once the axis has ended).
    * `max_unit_cols=None`: the rule of `online_release` -- at most one entry, the column before the last natural cut.
    * `max_unit_cols=M` (M >= d, M >= 1; ValueError otherwise): a piece starts at s = c_1. A natural cut after a column in [s, s + M)
      ends it (the FIRST such cut; the next piece starts at the next column). Without one, the piece ends after the last column below
      s + M -- a FORCED cut -- as soon as all of [s, s + M) is known: a column at or beyond s + M is there, or `bound >= s + M`. The next
      piece starts at the first column at or beyond s + M and the rule repeats; a piece that is neither ended nor known to its limit
      waits, with everything after it. Entries: the column before every forced cut, and the column before the last natural cut after
      the last forced one (pieces between natural cuts go as one unit: merging across a natural cut changes nothing, `OnlineDetector`).
    The pieces do not depend on the bound: a piece that starts at s is decided by the columns in [s, s + M) and the natural cuts among
    them alone. When the cut at the limit is taken with the bound standing in for an unknown c_{m+1} >= bound >= s + M, it is a cut
    whether that gap later proves natural (the piece ended by itself) or not (it is forced): the unit is the same, only its name is
    not -- which is why no count of forced cuts is returned."""
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    ts = np.asarray(tsteps_abs, dtype=np.float64).reshape(-1)
    bound, n_cols, d = int(bound), len(ts), int(d)
    M = _check_max_unit_cols("online_units", max_unit_cols, d)
    c = np.unique(cols[cols < bound])
    m = c.size
    none = np.zeros(0, dtype=np.int64)
    if m == 0:
        return none
    ended = bound >= n_cols
    nxt = np.r_[c[1:], min(bound, n_cols - 1)]
    natural = (nxt - c >= d) & (ts[nxt] - ts[c] >= float(break_win))
    natural[-1] |= ended                                                    # (the index was clamped for that case only)
    if M is None:
        return c[np.flatnonzero(natural)[-1:]]
    ends, i, last_natural = [], 0, -1
    while i < m:
        lim = c[i] + M
        j = int(np.searchsorted(c, lim, side="left")) - 1                   # the last column below the limit (>= i)
        nat = np.flatnonzero(natural[i:j + 1])
        if nat.size:
            last_natural = i + int(nat[0])
            i = last_natural + 1
        elif j + 1 < m or bound >= lim:
            ends.append(c[j])
            i, last_natural = j + 1, -1
        else:
            break
    if last_natural >= 0:
        ends.append(c[last_natural])
    return np.asarray(ends, dtype=np.int64)


class OnlineDetector(object):
    """`detect_sources_device` on an `Out_2` that arrives in blocks of closed columns: `det.push(*day.feed(P_chunk, t_now))` returns the
    sources [n, 5] (float64, sorted by time, possibly none) that became FINAL with this block, `det.finish()` the rest (ValueError
    unless every column has been pushed). All returns concatenated are the rows `detect_sources_device` finds on the offline `Out_2`,
    exactly and however the axis is cut into blocks. `held`: the candidates still waiting; `held_first_col`: the lowest column among
    them (None when nothing is held); `seen`: the next column expected.

    A push runs the streaming candidate kernel on the block (`StreamPeaks`: flat tops across block edges are carried, never flagged),
    adds the new candidates to the held ones and asks `online_units` for the cuts: with d = int(1.5 src_t_kernel / dt_win),
    a cut between two consecutive distinct candidate columns -- or between the last one and the stream's bound, below which no later
    candidate can fall -- is valid when they are >= d columns AND >= break_win seconds apart. Everything before the last valid cut is
    one unit and goes through the offline stages, unchanged: sort by (row, col), row offsets, `_peak_distance_keep`,
    `_sources_from_peaks`.

    The rule needs which columns are occupied, not the candidates: the detector owns a ring of per-column candidate counts on the device
    (`genie_col_counts` adds the new candidates' columns behind the FILL pass, on its stream), whose live columns run from the first
    held column -- or the previous bound -- to `seen`. A push that found candidates reads that window (at most two slices, one copy of a
    few hundred integers) instead of the candidates' columns; released slots are cleared; a window wider than the ring (`ring_cols`; a
    lagging bound) grows it, rebuilt from the held columns by one launch of the same kernel. The host work of a push does not grow
    with `held`; `held_cols` is rebuilt from the counts when asked.

    Why the result does not depend on when blocks arrive: (1) the distance rule only ever pairs peaks of a row closer than d columns, so
    no peak of a unit meets a peak outside it; (2) the time groups are cut on the candidates that SURVIVE the rule, but removing
    candidates only widens gaps: two candidates that are consecutive before the rule and >= break_win apart (tsteps_abs ascends, so
    consecutive in column is consecutive in time) separate two groups after it, whatever the rule removes on either side, so no group
    spans a cut; (3) LocalMarching never leaves a group. Hence the full pipeline on a union of units is the concatenation of the
    pipeline on each unit, units come out in ascending time, and releasing late only merges units -- the offline call is the one
    unit of everything.

    `max_unit_cols=None`: candidates that never leave a gap of d columns and break_win seconds are held until `finish()`; memory is
    then bounded by the activity, and `held` shows it.

    `max_unit_cols=M` (an integer >= d; ValueError otherwise) bounds it with FORCED cuts, under a contract of its own: all returns
    concatenated are `detect_sources_device(Out_2, ..., max_unit_cols=M)`, exactly and however the axis is cut into blocks. That is NOT
    the unbounded result: a piece of the axis that starts at the candidate column s and has no natural cut in [s, s + M) is cut after its
    last candidate column below s + M, the next piece starts at the first candidate column at or beyond s + M, and every unit between two
    forced cuts goes through the offline stages on its own (`online_units`). Across a forced cut two peaks of one row closer than d
    both survive, and neither a time group nor LocalMarching crosses it. M >= n_cols gives the unbounded result.
    Why arrival does not matter here either. The detector takes no state for it: s is the first held column below the bound. (a) The
    decision for s depends only on the candidates in [s, s + M) and the natural cuts among them, and it is taken when they are all
    known: a candidate at or beyond s + M has arrived, or `bound >= s + M`. (b) With the bound standing in for the unknown next column,
    the cut at the limit is taken whether or not that gap later proves natural; natural or forced, the unit before it is the same set
    of candidates, and running two units apart that a natural cut separates changes nothing (1-3 above). So which cuts count as
    forced may depend on arrival -- no such count is exposed -- the sources cannot. (c) Everything after a cut restarts from the first
    candidate at or beyond it, and that candidate is below the bound when it is used, so it is the first of ALL candidates there. By
    induction over the pieces, online and offline cut the same units. A push, and `finish()`, run every piece they complete as a
    separate unit, in ascending time.
    Invariant, after every push: no held column lies below `peaks.bound`, or `peaks.bound - held_first_col < M`. A row's candidates are
    at least two columns apart, so after a push `held <= rows * ceil((M + lag) / 2)` with lag = `seen - peaks.bound`, and inside a
    push of a block B columns wide `held <= rows * ceil((M + B + lag) / 2)`. lag is about half the longest run of equal values at or above the threshold that is
    still open at the block's end (a column or two on a smooth field); the one exception that remains is a long run of exactly equal
    values above the threshold, which holds the bound back at its midpoint for as long as it lasts ("The
    bound").

    Besides `StreamPeaks`' one host read per push, a push that found candidates reads the ring's window.

    A restart: `state_dict()` between any two pushes (the held candidates and the `StreamPeaks` carry, on the host) and
    `load_state_dict(state)` on a newly constructed detector with the same arguments."""

    def __init__(self, X_query, tsteps_abs, ftrns1, thresh, src_t_kernel, dt_win, break_win, tc_win, sp_win, scale_depth_clustering=0.2,
                 device="cuda", max_unit_cols=None, ring_cols=1024):
        self.distance = int(1.5 * src_t_kernel / dt_win)
        _check_peak_args("OnlineDetector", thresh, self.distance)
        self.max_unit_cols = _check_max_unit_cols("OnlineDetector", max_unit_cols, self.distance)
        if int(ring_cols) < 1:
            raise ValueError("OnlineDetector: ring_cols >= 1 required")
        self.tsteps_abs = np.asarray(tsteps_abs, dtype=np.float64).reshape(-1)
        if self.tsteps_abs.size > 1 and not np.all(self.tsteps_abs[1:] >= self.tsteps_abs[:-1]):
            raise ValueError("OnlineDetector: tsteps_abs must ascend")
        self.X_query = np.asarray(X_query, dtype=np.float64)
        self.n_cols, self.break_win = len(self.tsteps_abs), float(break_win)
        self._tail = (ftrns1, break_win, tc_win, sp_win, scale_depth_clustering)
        self.peaks = StreamPeaks(self.X_query.shape[0], self.n_cols, thresh, device)
        dev = self.peaks.device
        self._r = torch.empty(0, dtype=torch.int32, device=dev)
        self._c = torch.empty(0, dtype=torch.int32, device=dev)
        self._v = torch.empty(0, dtype=torch.float32, device=dev)
        self._ring = torch.zeros(int(ring_cols), dtype=torch.int32, device=dev)    # candidates per column, slot = column mod its length
        self._win_lo = 0                                  # the host's copy of the ring's live window as the last push left it:
        self._win = np.zeros(0, dtype=np.int64)           #   the counts of the columns [_win_lo, ...), the first one held (or empty)

    @property
    def seen(self):
        return self.peaks.seen

    @property
    def held(self):
        return int(self._c.numel())

    @property
    def held_first_col(self):
        """The lowest column of a held candidate (an int), None when nothing is held."""
        return int(self._win_lo) if self._win.size else None

    @property
    def held_cols(self):
        """The columns of the held candidates (host int64, ascending, repeats included), rebuilt from the column counts."""
        return np.repeat(self._win_lo + np.arange(self._win.size, dtype=np.int64), self._win)

    def _run_unit(self, r, c, v):
        """The offline stages on one released unit (GPU triplets in any order)."""
        r, c, v = _distance_rule_unsorted(r, c, v, self.peaks.rows, self.n_cols, self.distance)
        return _sources_from_peaks(r, c, v, self.X_query, self.tsteps_abs, *self._tail)

    def _slices(self, lo, n):
        """The ring's slots of the columns [lo, lo + n), n <= its length: one or two contiguous slices."""
        W = int(self._ring.numel())
        a = lo % W
        return (self._ring[a:a + n],) if a + n <= W else (self._ring[a:], self._ring[:a + n - W])

    def _count(self, cols, span):
        """Add the candidates' columns `cols` (int32 GPU tensor) to the ring; a live window of `span` columns that the ring cannot
        hold grows it first, and it is then rebuilt from ALL held columns (which `cols` must be part of by now)."""
        W = int(self._ring.numel())
        if span > W:
            while W < span:
                W *= 2
            self._ring = torch.zeros(W, dtype=torch.int32, device=self._ring.device)
            cols = self._c
        dev = self._ring.device
        with torch.cuda.device(dev):
            _lib.check(_lib.load().genie_col_counts(_ptr(cols.contiguous()), int(cols.numel()), _ptr(self._ring), W, _stream(dev)),
                       "genie_col_counts")

    def _set_window(self, lo, counts):
        """Keep the counts of the columns [lo, ...) from their first occupied column on."""
        held = np.flatnonzero(counts)
        k = int(held[0]) if held.size else len(counts)
        self._win_lo, self._win = lo + k, counts[k:]

    def _release(self):
        """The units that are final under the stream's bound, each through the offline stages on its own; they leave the held
        candidates, the ring and the window."""
        lo, counts = self._win_lo, self._win
        ends = online_units(lo + np.flatnonzero(counts), self.peaks.bound, self.tsteps_abs, self.distance, self.break_win, self.max_unit_cols)
        if ends.size == 0:
            return np.zeros((0, 5))
        out, prev = [], -1
        for end in ends.tolist():
            go = (self._c > prev) & (self._c <= end)
            out.append(self._run_unit(self._r[go], self._c[go], self._v[go]))
            prev = end
        stay = self._c > prev
        self._r, self._c, self._v = self._r[stay], self._c[stay], self._v[stay]
        for part in self._slices(lo, prev + 1 - lo):
            part.zero_()
        self._set_window(prev + 1, counts[prev + 1 - lo:])
        return np.concatenate(out)

    def push(self, first_col, block):
        first, bound = self.held_first_col, self.peaks.bound
        lo = bound if first is None else min(first, bound)                  # no candidate of this push has a column below the bound
        r, c, v, _ = self.peaks.push(first_col, block)
        if r.numel():
            self._r, self._c, self._v = torch.cat((self._r, r)), torch.cat((self._c, c)), torch.cat((self._v, v))
            span = self.peaks.seen - lo
            self._count(c, span)
            self._set_window(lo, torch.cat(self._slices(lo, span)).cpu().numpy().astype(np.int64))
        return self._release()

    def finish(self):
        if self.peaks.seen != self.n_cols:
            raise ValueError("OnlineDetector.finish: %d of %d columns have been pushed" % (self.peaks.seen, self.n_cols))
        return self._release()

    def _fingerprint(self):
        _, break_win, tc_win, sp_win, scale_depth = self._tail
        own = {"tsteps_abs": self.tsteps_abs, "X_query": self.X_query, "distance": self.distance, "break_win": break_win, "tc_win": tc_win,
               "sp_win": sp_win, "scale_depth_clustering": scale_depth}
        if self.max_unit_cols is not None:                # (a state saved before the argument existed has no such field)
            own["max_unit_cols"] = self.max_unit_cols
        return own

    def _state(self):
        return {"fingerprint": self._fingerprint(), "peaks": self.peaks._state(), "held_row": self._r, "held_col": self._c,
                "held_val": self._v, "held_cols_sorted": self.held_cols}

    def state_dict(self):
        """Everything `push` has changed, between any two pushes: the held candidates (row, column, value as
        CPU tensors in their device order, and the sorted host columns), the `StreamPeaks` state (`seen`, `bound`, the scanner's carry
        across the last block edge) and the fingerprint of the axis, the queries, the threshold and the windows. One synchronisation;
        the object is left as it was."""
        return checkpoint.to_host(self._state())

    def _check_state(self, state):
        if self.held:
            raise RuntimeError("OnlineDetector.load_state_dict: this detector holds candidates; a state is loaded into a new one")
        checkpoint.check_fingerprint("OnlineDetector", state, self._fingerprint())
        self.peaks._check_state(state["peaks"])
        r, c, v, cols = state["held_row"], state["held_col"], state["held_val"], np.asarray(state["held_cols_sorted"])
        if not (all(torch.is_tensor(x) and x.dim() == 1 and x.shape == r.shape for x in (r, c, v)) and r.dtype == c.dtype == torch.int32
                and v.dtype == torch.float32 and cols.dtype == np.int64 and cols.shape == tuple(r.shape)):
            raise ValueError("OnlineDetector.load_state_dict: the held candidates are (int32, int32, fp32) tensors and int64 columns [n]")

    def _load_state(self, state):
        dev = self.peaks.device
        self.peaks._load_state(state["peaks"])
        self._r, self._c, self._v = (state[k].to(dev) for k in ("held_row", "held_col", "held_val"))
        cols = np.array(state["held_cols_sorted"], dtype=np.int64)
        if cols.size:                                     # the ring and its window, from the held columns
            self._ring.zero_()
            self._count(self._c, self.peaks.seen - int(cols[0]))
            self._set_window(int(cols[0]), np.bincount(cols - cols[0]))

    def load_state_dict(self, state):
        """Resume a saved detector in a newly constructed one (nothing pushed: RuntimeError otherwise) built with the same arguments
        (ValueError naming the first differing field otherwise, nothing changed): all returns from here on are the saved object's."""
        self._check_state(state)
        self._load_state(state)


# ------------------------------------------------------------------------------------------------
# The refine pass's selection of the refined source (genie_refine_select, csrc/select_kernels.hpp).
# ------------------------------------------------------------------------------------------------
REFINE_SELECT_MAX_LEGS = 32


def refine_select_scratch(device):
    """The scratch buffer of `refine_select_device` (uint8 GPU tensor, a few KB): a loop over sources allocates it once."""
    return torch.empty(int(_lib.load().genie_refine_select_scratch_bytes()), dtype=torch.uint8, device=device)


def refine_select_device(xs, shape, keep, n_scale, device=None, scratch=None):
    """The refined source of one query cloud in one launch pair: with `acc = sum over xs, in order, of x / n_scale` (fp32, from zero; the
    statements `acc += x[:, :, 0] / n_scale` of `apply.refine_sources`) and rows where `keep` is False counted as -inf, returns the fp64 GPU
    tensor (ip, it, acc[ip, it], any_kept): `ip = argmax(acc.max(1)[0])`, `it = argmax(acc[ip])`, first maximum in both, bit for bit.
    `xs`: the read-outs of the legs that produced a window, fp32 GPU tensors [Q, n_t] or [Q, n_t, 1], contiguous (their storage is
    read in place); an empty list is an all-zero `acc`. `shape` = (Q, n_t); `keep`: bool / uint8 GPU tensor [Q] or None (all kept);
    `n_scale`: the number of legs of the average. Nothing here waits for the device."""
    Q, n_t = int(shape[0]), int(shape[1])
    xs = list(xs)
    if len(xs) > REFINE_SELECT_MAX_LEGS:
        raise ValueError("refine_select_device: at most %d read-outs per call" % REFINE_SELECT_MAX_LEGS)
    for x in xs:
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() == Q * n_t
                and tuple(x.shape[:2]) == (Q, n_t)):
            raise ValueError("refine_select_device: every read-out must be a contiguous fp32 GPU tensor [%d, %d] or [%d, %d, 1]" % (Q, n_t, Q, n_t))
    if keep is not None:
        if not (torch.is_tensor(keep) and keep.is_cuda and keep.dtype in (torch.bool, torch.uint8) and tuple(keep.shape) == (Q,)):
            raise ValueError("refine_select_device: keep must be a bool or uint8 GPU tensor [%d]" % Q)
        keep = keep.contiguous()
    dev = xs[0].device if xs else (keep.device if keep is not None else torch.device("cuda" if device is None else device))
    lib = _lib.load()
    if scratch is None:
        scratch = refine_select_scratch(dev)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    ptrs = (ctypes.c_void_p * max(len(xs), 1))(*[x.data_ptr() for x in xs])
    with torch.cuda.device(dev):
        _lib.check(lib.genie_refine_select(ptrs, len(xs), Q, n_t, _ptr(keep), float(n_scale), _ptr(scratch), _ptr(out), _stream(dev)),
                   "genie_refine_select")
    return out


# ------------------------------------------------------------------------------------------------
# The refine pass's query cloud, drawn on the device (genie_refine_cloud, csrc/cloud_kernels.hpp).
# ------------------------------------------------------------------------------------------------
REFINE_CLOUD_SWEEP = 1024 * 256 * 4       # elements one sweep of the capped grid covers (RC_MAX_WG x RC_BLOCK x 4): beyond it threads stride


def philox_key_words(key):
    """The two 64-bit key words (low, high) of a Philox4x64 key given as an int below 2**128 or as a pair of 64-bit words -- what
    `np.random.Philox(key=...)` makes of either form."""
    if isinstance(key, (int, np.integer)):
        key = int(key)
        if not 0 <= key < 1 << 128:
            raise ValueError("Philox key: an int key must lie in [0, 2**128)")
        return key & 0xFFFFFFFFFFFFFFFF, key >> 64
    words = [int(k) for k in np.asarray(key, dtype=object).reshape(-1)]
    if len(words) != 2 or not all(0 <= k < 1 << 64 for k in words):
        raise ValueError("Philox key: a pair of words in [0, 2**64) or an int below 2**128")
    return words[0], words[1]


def refine_cloud_device(key, source, n_query, src_cart, off_range, off_min, device, want_draw=False):
    """The query cloud of candidate source number `source` in one launch on the current stream of `device`: with
    `r = np.random.Generator(np.random.Philox(key=key, counter=[0, source, 0, 0])).random((n_query, 3))`, returns
    (Xc = src_cart + (r * off_range + off_min) float64 [n_query, 3], xq = Xc rounded to float32[, r]) as GPU tensors carrying the bits of
    those numpy statements. `key`: an int below 2**128 or a pair of 64-bit words; `src_cart`, `off_range`, `off_min`: three host numbers
    each (they travel in the kernel arguments). Nothing is copied to the device and nothing waits for it."""
    k0, k1 = philox_key_words(key)
    source, n = int(source), int(n_query)
    if not 0 <= source < 1 << 64:
        raise ValueError("refine_cloud_device: source must lie in [0, 2**64)")
    if n < 0:
        raise ValueError("refine_cloud_device: n_query must be >= 0")
    vec = [float(v) for a in (src_cart, off_range, off_min) for v in np.asarray(a, dtype=np.float64).reshape(3)]
    dev = torch.device(device)
    Xc = torch.empty((n, 3), dtype=torch.float64, device=dev)
    xq = torch.empty((n, 3), dtype=torch.float32, device=dev)
    r = torch.empty((n, 3), dtype=torch.float64, device=dev) if want_draw else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().genie_refine_cloud(k0, k1, source, n, *vec, _ptr(r), _ptr(Xc), _ptr(xq), _stream(dev)), "genie_refine_cloud")
    return (Xc, xq, r) if want_draw else (Xc, xq)


# ------------------------------------------------------------------------------------------------
# The two kernels above for a batch of sources in one launch (pair) each: `apply.refine_sources(source_batch=B)`.
# ------------------------------------------------------------------------------------------------
def refine_select_batch_scratch(device, n_batch):
    """The scratch buffer of `refine_select_batch_device` for up to `n_batch` sources (uint8 GPU tensor, `n_batch` times the single form's)."""
    return torch.empty(int(n_batch) * int(_lib.load().genie_refine_select_scratch_bytes()), dtype=torch.uint8, device=device)


def refine_select_batch_device(table, shape, keep, n_scale, scratch=None):
    """`refine_select_device` of B sources in one launch pair (genie_refine_select_batch): fp64 GPU tensor [B, 4] whose row b carries the
    bits the single form gives for source b's read-outs. `table`: int64 GPU tensor [B, n_legs] of device addresses, entry (b, l) = the
    `data_ptr()` of leg l's contiguous fp32 read-out [Q, n_t] (or [Q, n_t, 1]) of source b, or 0 where that leg produced no window for
    it; the caller keeps those tensors alive and orders their producers before the current stream. `shape` = (Q, n_t); `keep`: bool /
    uint8 GPU tensor [B, Q] or None (all kept); `n_scale`: the number of legs of the average. Nothing here waits for the device."""
    Q, n_t = int(shape[0]), int(shape[1])
    if not (torch.is_tensor(table) and table.is_cuda and table.dtype == torch.int64 and table.dim() == 2 and table.is_contiguous()
            and table.shape[0] >= 1):
        raise ValueError("refine_select_batch_device: table must be a contiguous int64 GPU tensor [B, n_legs] with B >= 1")
    B, n_legs = int(table.shape[0]), int(table.shape[1])
    if n_legs > REFINE_SELECT_MAX_LEGS:
        raise ValueError("refine_select_batch_device: at most %d read-outs per source" % REFINE_SELECT_MAX_LEGS)
    dev = table.device
    if keep is not None:
        if not (torch.is_tensor(keep) and keep.is_cuda and keep.dtype in (torch.bool, torch.uint8) and tuple(keep.shape) == (B, Q)):
            raise ValueError("refine_select_batch_device: keep must be a bool or uint8 GPU tensor [%d, %d]" % (B, Q))
        keep = keep.contiguous()
    lib = _lib.load()
    need = B * int(lib.genie_refine_select_scratch_bytes())
    if scratch is None:
        scratch = refine_select_batch_scratch(dev, B)
    elif scratch.numel() < need:
        raise ValueError("refine_select_batch_device: scratch holds %d bytes, %d sources need %d" % (scratch.numel(), B, need))
    out = torch.empty((B, 4), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.genie_refine_select_batch(_ptr(table), B, n_legs, Q, n_t, _ptr(keep), float(n_scale), _ptr(scratch), _ptr(out),
                                                 _stream(dev)), "genie_refine_select_batch")
    return out


def refine_cloud_batch_device(key, source0, n_batch, n_query, src_cart, off_range, off_min, device):
    """The query clouds of the candidate sources `source0 .. source0 + n_batch - 1` in one launch (genie_refine_cloud_batch): (Xc float64
    [n_batch, n_query, 3], xq = Xc rounded to float32), row block b bit-equal to `refine_cloud_device(key, source0 + b, n_query,
    src_cart[b], off_range, off_min, device)`. `src_cart`: host numbers [n_batch, 3] (one small copy to the device, in stream order);
    `off_range`, `off_min`: three host numbers each."""
    k0, k1 = philox_key_words(key)
    source0, B, n = int(source0), int(n_batch), int(n_query)
    if B < 1:
        raise ValueError("refine_cloud_batch_device: n_batch must be >= 1")
    if not (0 <= source0 and source0 + B - 1 < 1 << 64):
        raise ValueError("refine_cloud_batch_device: sources must lie in [0, 2**64)")
    if n < 0:
        raise ValueError("refine_cloud_batch_device: n_query must be >= 0")
    src = np.ascontiguousarray(np.asarray(src_cart, dtype=np.float64).reshape(B, 3))
    vec = [float(v) for a in (off_range, off_min) for v in np.asarray(a, dtype=np.float64).reshape(3)]
    dev = torch.device(device)
    src_d = torch.from_numpy(src).to(dev)
    Xc = torch.empty((B, n, 3), dtype=torch.float64, device=dev)
    xq = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().genie_refine_cloud_batch(k0, k1, source0, B, n, _ptr(src_d), *vec, _ptr(Xc), _ptr(xq), _stream(dev)),
                   "genie_refine_cloud_batch")
    return Xc, xq
