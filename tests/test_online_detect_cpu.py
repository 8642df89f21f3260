"""CPU: the host side of online detection (`postproc.online_release`, the release rule of `postproc.OnlineDetector`) and the C ABI of the
streaming candidate kernel (genie_stream_peaks_*: declared in the header, bound in `_lib.SYMBOLS`).

The decomposition the detector rests on is checked here with the host stages alone: the distance rule, the time groups and LocalMarching
on a whole candidate list against the same stages unit by unit, for units that `online_release` cuts under random sequences of bounds."""
import os
import re

import numpy as np

from genie_amd import _lib, postproc

HEADER = os.path.join(_lib.REPO, "include", "genie_hip.h")
STREAM_SYMBOLS = ("genie_stream_peaks_count", "genie_stream_peaks_fill")


def test_stream_peaks_abi_is_declared_and_bound():
    text = open(HEADER).read()
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    for name in STREAM_SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name + " is not declared in include/genie_hip.h"
        assert name in bound, name + " is not in _lib.SYMBOLS"
        assert len(bound[name]) == len(m.group(1).split(",")), name + ": the binding and the declaration differ in their argument count"
    assert re.search(r"\bsize_t\s+genie_stream_peaks_carry_bytes\s*\(\s*int\s+rows\s*\)\s*;", text) and "genie_stream_peaks_carry_bytes" in bound
    declared = set(re.findall(r"\b(genie_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(bound)                                           # the header and the binding name the same entry points


def test_online_release_on_hand_made_lists():
    rel = postproc.online_release
    ts = np.arange(100) * 0.75                                              # d = 10 columns = 7.5 s; break_win = 15 s = 20 columns
    d, bw = 10, 15.0
    assert rel([], 50, ts, d, bw) == 0 and rel(np.zeros(0, dtype=np.int64), 100, ts, d, bw) == 0       # nothing held
    # one column: it goes once the bound is d columns and break_win seconds on, or the axis has ended
    assert rel([30], 49, ts, d, bw) == 0 and rel([30], 50, ts, d, bw) == 1 and rel([30, 30, 30], 50, ts, d, bw) == 3
    assert rel([99], 100, ts, d, bw) == 1 and rel([98, 99], 100, ts, d, bw) == 2                       # bound == n_cols
    # the column gap alone (break_win 0): exactly d and d - 1
    assert rel([10, 20, 29], 29, ts, d, 0.0) == 1 and rel([10, 19, 29], 28, ts, d, 0.0) == 0 and rel([10, 19, 29], 29, ts, d, 0.0) == 2
    assert rel([10, 20, 29], 39, ts, d, 0.0) == 3 and rel([10, 20, 29], 38, ts, d, 0.0) == 1
    # both: the gap of 20 columns is exactly break_win, 19 columns is not (d alone would cut there)
    assert rel([10, 30], 31, ts, d, bw) == 1 and rel([10, 29], 31, ts, d, bw) == 0
    # everything up to the LAST valid cut goes as one unit, invalid cuts before it included
    assert rel([10, 12, 40, 45, 70], 71, ts, d, bw) == 4 and rel([10, 12, 40, 45, 70], 90, ts, d, bw) == 5
    # a bound inside the gap holds the cut back, a bound beyond it does not
    assert rel([10, 60], 25, ts, d, bw) == 0 and rel([10, 60], 30, ts, d, bw) == 1 and rel([10, 60], 61, ts, d, bw) == 1
    # a held column at or above the bound (another row's run is still open further back) waits, and does not cut
    assert rel([10, 60], 45, ts, d, bw) == 1 and rel([40, 60], 45, ts, d, bw) == 0 and rel([10, 60], 10, ts, d, bw) == 0
    # a non-uniform axis: the time gap is exactly break_win / just below it while the column gap stays 12 >= d
    tn = np.arange(100) * 0.75
    tn[50:] += 15.0 - 12 * 0.75                                             # columns 40 -> 52 are exactly 15 s apart
    assert tn[52] - tn[40] == 15.0 and rel([40, 52], 53, tn, d, bw) == 1
    tn[50:] -= 2.0 ** -20
    assert tn[52] - tn[40] < 15.0 and rel([40, 52], 53, tn, d, bw) == 0
    assert rel([40, 52], 100, tn, d, bw) == 2                               # the axis has ended: the last cut is always valid


def _pipeline(r, c, v, xq, ts, d, break_win, tc_win, sp_win):
    """The host stages after the candidates (`detect_sources` without `row_select`): (rows [n, 5] in canonical order, how many the
    distance rule removed, how many LocalMarching removed)."""
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    keep = np.ones(r.size, dtype=bool)
    for row in np.unique(r):
        m = np.flatnonzero(r == row)
        keep[m] = postproc.select_by_peak_distance(c[m], v[m], d)
    n_rule = int((~keep).sum())
    r, c, v = r[keep], c[keep], v[keep]
    srcs = np.concatenate((xq[r], ts[c].reshape(-1, 1), v.astype(np.float64).reshape(-1, 1)), axis=1)
    srcs = srcs[np.argsort(srcs[:, 3], kind="stable")]
    out = [np.zeros((0, 5))]
    for g in postproc.group_sources(srcs, break_win):
        out.append(g if len(g) == 1 else postproc.local_marching(g, lambda x: x, tc_win=tc_win, sp_win=sp_win, scale_depth=0.2, n_steps_max=2,
                                                                 use_directed=False))
    out = np.vstack(out)
    return out[np.lexsort((out[:, 4], out[:, 2], out[:, 1], out[:, 0], out[:, 3]))], n_rule, len(srcs) - len(out)


def test_the_pipeline_on_released_units_is_the_pipeline_on_the_whole_list():
    rng = np.random.default_rng(17)
    rows, n_cols, d, bw, tc, sp = 6, 400, 10, 15.0, 6.75, 20e3
    ts = np.arange(n_cols) * 0.75 + 4990.0
    xq = np.c_[rng.uniform(0, 30e3, (rows, 2)), rng.uniform(-20e3, 0, rows)]
    # bursts of candidates separated by quiet stretches of at least 20 columns; distinct heights (scipy leaves equal heights within d open)
    cells = set()
    for lo, hi in ((5, 40), (70, 95), (130, 190), (215, 222), (260, 300), (330, 395)):
        for _ in range(int(0.25 * (hi - lo)) + 2):
            cells.add((int(rng.integers(rows)), int(rng.integers(lo, hi))))
    cells = np.array(sorted(cells), dtype=np.int64)
    r, c = cells[:, 0], cells[:, 1]
    v = (0.2 + rng.permutation(len(r)) / 1024.0).astype(np.float32)
    want, n_rule, n_march = _pipeline(r, c, v, xq, ts, d, bw, tc, sp)
    assert n_rule >= 1 and n_march >= 1 and len(want) >= 6                  # otherwise the equality shows nothing
    for trial in range(8):
        # a stream: the bound climbs in random steps; everything below it has been emitted, and so has a random part of what lies up to
        # 25 columns beyond (other rows' runs that are already decided)
        emitted, released = np.zeros(len(r), dtype=bool), np.zeros(len(r), dtype=bool)
        bound, units, early = 0, [], 0
        while bound < n_cols:
            bound = min(bound + int(rng.integers(1, 40)), n_cols)
            emitted |= (c < bound) | ((c < bound + 25) & (rng.random(len(r)) < 0.5))
            held = np.flatnonzero(emitted & ~released)
            held = held[np.argsort(c[held], kind="stable")]
            k = postproc.online_release(c[held], bound, ts, d, bw)
            assert 0 <= k <= len(held)
            if k:
                unit = held[:k]
                assert k == len(held) or c[held[k]] > c[unit[-1]]           # a column is never split
                released[unit] = True
                units.append(_pipeline(r[unit], c[unit], v[unit], xq, ts, d, bw, tc, sp)[0])
                early += bound < n_cols
        assert released.all() and early >= 2                                # at least two units before the axis ended
        got = np.vstack(units)
        assert np.array_equal(got[np.lexsort((got[:, 4], got[:, 2], got[:, 1], got[:, 0], got[:, 3]))], want), trial
