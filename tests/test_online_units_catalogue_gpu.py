"""GPU: the online catalogue behind a BOUNDED detector (`postproc.OnlineDetector(max_unit_cols=M)`) against its offline twin,
`apply_windows_device(stack_on_device=True)` -> `detect_refine_associate(detect_on_device=True, max_unit_cols=M, rand=PhiloxCloud(key),
ftrns2_device=...)`, on the small day of tests/test_online_catalogue_gpu.py (169 columns, d = 4 columns, break_win = 2.5 s) with two
active stretches added to its field: three-column bumps every 3 columns (below d, and below break_win) over columns 47..71 and 89..113,
which M = 8 cuts into three units each. Every key of the concatenated online dicts equals the twin's, `np.array_equal` / `torch.equal`."""
import functools

import numpy as np
import pytest
import torch

from genie_amd import apply, postproc
from tests.test_online_catalogue_gpu import DETECT, DEV, IDENT, KEY, _chain_args, _chunks, _concat, _detect_args, _field, _setup

pytestmark = pytest.mark.gpu

M = 8
STRETCHES = (47, 89)                                                        # nine bumps each: first, first + 3, ..., first + 24


@functools.lru_cache(maxsize=None)
def _active_field():
    """The blobs of the base test plus the two active stretches. The bumps of a stretch sit on three neighbouring query rows; the first
    bump of every unit of M columns is the highest, so that the units' sources are 9 columns apart: further than the 6 s the refine
    pass can move two sources towards each other (refined times stay distinct, as the offline sorts assume)."""
    _, geom, _, _, _, _, ts = _setup()
    xq = np.asarray(geom.x_query, dtype=np.float64)
    rows = np.argsort(np.linalg.norm(xq - xq[50], axis=1), kind="stable")[:3]
    extra = np.zeros((len(xq), len(ts)), dtype=np.float32)
    k = 0
    for first in STRETCHES:
        for i in range(9):
            col, h = first + 3 * i, (52 + k) / 64.0 if i % 3 == 0 else (24 + k) / 64.0         # distinct heights, in 1/64
            extra[rows[i % 3], col - 1:col + 2] = np.float32(h) * np.array([0.5, 1.0, 0.5], dtype=np.float32)
            k += 1
    return _field() + torch.from_numpy(extra).to(DEV)


@functools.lru_cache(maxsize=None)
def _twin():
    net, geom, P, trv_t, max_t, tsteps, ts = _setup()
    xq = np.asarray(geom.x_query, dtype=np.float64)
    Out_2, _ = apply.apply_windows_device(net, geom, P, trv_t, tsteps_abs=ts, times=tsteps, max_t=max_t, tail_batch=16, stack_on_device=True)
    Out_2 = Out_2 + _active_field()
    leg = apply.GridLeg(net, geom.x_grid, trv_t)
    picks = apply.ResidentPicks(P, np.arange(geom.n_sta), geom.n_sta, DEV)
    a = _chain_args()
    run = lambda **kw: apply.detect_refine_associate([leg], picks, Out_2, xq, ts, a[0], a[1], a[2], max_t, *a[3:], DETECT["thresh"],
                                                     DETECT["src_t_kernel"], DETECT["dt_win"], DETECT["break_win"], DETECT["tc_win"],
                                                     DETECT["sp_win"], rand=apply.PhiloxCloud(KEY), ftrns2_device=IDENT,
                                                     detect_on_device=True, **kw)
    want = run(max_unit_cols=M)
    torch.cuda.synchronize()
    # the fixture's own requirements: forced cuts, and a detection list that the limit changes
    _, c, _ = postproc.row_select(Out_2.contiguous(), DETECT["thresh"], 1)
    d = int(1.5 * DETECT["src_t_kernel"] / DETECT["dt_win"])
    cols = c.cpu().numpy()
    ends = postproc.online_units(cols, len(ts), ts, d, DETECT["break_win"], M)
    free = postproc.detect_sources_device(Out_2.contiguous(), *_detect_args(xq, ts))
    print("twin: %d detections (%d without the limit), %d retained, unit ends %s" % (len(want["srcs"]), len(free), len(want["srcs_refined"]), ends))
    assert len(ends) > len(postproc.online_units(cols, len(ts), ts, d, DETECT["break_win"], None)) + 3
    assert not np.array_equal(want["srcs"], free)
    assert len(want["srcs_refined"]) >= 3 and len(np.unique(want["srcs_refined"][:, 3])) == len(want["srcs_refined"])
    return want


def _catalogue():
    net, geom, P, trv_t, max_t, tsteps, ts = _setup()
    xq = np.asarray(geom.x_query, dtype=np.float64)
    day = apply.OnlineDay(net, geom, trv_t, ts, times=tsteps, max_t=max_t, tail_batch=16)
    feed, field = day.feed, _active_field()
    day.feed = lambda P_chunk, t_now: (lambda first, block: (first, block + field[:, first:first + block.shape[1]]))(*feed(P_chunk, t_now))
    det = postproc.OnlineDetector(*_detect_args(xq, ts), device=DEV, max_unit_cols=M)
    a = _chain_args()
    return day, det, apply.OnlineCatalogue(day, det, *a, DETECT["tc_win"], DETECT["sp_win"], rand=apply.PhiloxCloud(KEY), ftrns2_device=IDENT)


@pytest.mark.parametrize("how", ["second", "random"])
def test_online_catalogue_behind_a_bounded_detector_equals_the_offline_twin(how):
    want = _twin()
    day, det, cat = _catalogue()
    parts, early = [], 0
    for rows, t_now in _chunks(how):
        parts.append(cat.push(rows, t_now))
        early += len(parts[-1]["srcs"])
        first, bound = det.held_first_col, det.peaks.bound
        assert first is None or first >= bound or bound - first < M        # the detector's invariant, behind the real loop
    parts.append(cat.finish())
    assert cat.pending == 0 and cat.undecided == 0 and det.held == 0 and day.closed == len(_setup()[6])
    got = _concat(parts)
    for key in ("srcs", "srcs_refined"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    assert torch.equal(got["trv_out_srcs"], want["trv_out_srcs"])
    for key in ("Out_p_save", "Out_s_save"):
        assert len(got[key]) == len(want[key])
        assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(got[key], want[key])), key
    for key in ("Save_picks", "lp_meta"):
        assert len(got[key]) == len(want[key])
        assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got[key], want[key])), key
    assert sorted(got) == sorted(want)
    assert early >= 3 and len(day.picks) == 0                               # sources of the stretches were released along the way
