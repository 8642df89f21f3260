"""CPU: the unit rule of bounded online detection (`postproc.online_units`: natural cuts, and forced cuts after `max_unit_cols` columns),
the refusals of `max_unit_cols` that are raised before any device use, and the C ABI of the column-count kernel.

As tests/test_online_detect_cpu.py does for the unbounded rule, the decomposition is checked with the host stages alone: the stages unit by
unit for units cut while the bound climbs in random steps, against the same stages on the units of the whole list (the one-shot twin)."""
import inspect
import os
import re

import numpy as np
import pytest

from genie_amd import _lib, apply, postproc
from tests.test_online_detect_cpu import _pipeline

HEADER = os.path.join(_lib.REPO, "include", "genie_hip.h")
TS = np.arange(100) * 0.75                                                  # d = 10 columns; break_win = 15 s = 20 columns
D, BW = 10, 15.0


def _units(cols, bound, M, ts=TS, d=D, bw=BW):
    return postproc.online_units(cols, bound, ts, d, bw, M).tolist()


def test_col_counts_abi_is_declared_and_bound():
    text = open(HEADER).read()
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    m = re.search(r"\bint\s+genie_col_counts\s*\(([^;]*)\)\s*;", text)
    assert m and "genie_col_counts" in bound and len(bound["genie_col_counts"]) == len(m.group(1).split(",")) == 5


def test_without_a_limit_the_units_are_online_release():
    rng = np.random.default_rng(5)
    cases = [([], 50), ([30], 49), ([30], 50), ([30, 30, 30], 50), ([99], 100), ([98, 99], 100), ([10, 12, 40, 45, 70], 71),
             ([10, 12, 40, 45, 70], 90), ([10, 60], 25), ([10, 60], 30), ([10, 60], 61), ([10, 60], 45), ([40, 60], 45), ([10, 60], 10)]
    for _ in range(300):
        cols = np.sort(rng.integers(0, 100, int(rng.integers(0, 25))))
        cases.append((cols.tolist(), int(rng.integers(0, 101))))
    some = 0
    for cols, bound in cases:
        for bw in (BW, 0.0):
            ends = _units(cols, bound, None, bw=bw)
            assert len(ends) <= 1                                           # one unit: everything up to the last natural cut
            k = int(np.searchsorted(cols, ends[0], side="right")) if ends else 0
            assert k == postproc.online_release(cols, bound, TS, D, bw), (cols, bound, bw)
            some += k > 0
    assert some > 50


def test_only_natural_gaps_give_the_unbounded_units():
    for bound, want in ((71, [45]), (90, [70]), (100, [70]), (41, [12]), (32, [12]), (31, [])):
        cols = [c for c in (10, 12, 40, 45, 70) if c < bound or bound == 100]
        assert _units(cols, bound, 40) == want == _units(cols, bound, None), bound
    assert _units([10, 12, 40, 45, 70], 100, 100) == [70]


def test_a_gapless_run_is_cut_at_the_limit_and_again_from_the_next_piece():
    M = 20
    run = np.arange(10, 10 + 3 * M)                                         # every gap is 1 < d: no natural cut inside
    assert _units(run, 100, M) == [29, 49, 69]                              # s = 10: after 29; s' = 30: after 49; the axis has ended
    assert _units(run, 100, None) == [69]
    assert _units(run[run < 30], 30, M) == [29] and _units(run[run < 29], 29, M) == []        # taken once bound >= s + M, not before
    assert _units(run[run < 31], 29, M) == []                               # a column at or above the bound waits, and decides nothing
    assert _units(run[run < 50], 50, M) == [29, 49] and _units(run[run < 49], 49, M) == [29]
    assert _units(run[run < 69], 69, M) == [29, 49]                         # 50..68 wait: bound < 70 = s'' + M and no natural cut yet
    assert _units(run, 70, M) == [29, 49, 69] == _units(run, 89, M)         # the cut at the limit, whether or not it proves natural
    stride = np.arange(10, 70, 4)                                           # 10, 14, ..., 66: the limit falls between candidates
    assert _units(stride, 100, M) == [26, 46, 66] and _units(stride, 100, 21) == [30, 54, 66]


def test_a_candidate_exactly_at_the_limit_starts_the_next_piece():
    cols = [10, 14, 18, 22, 26, 30, 34, 38]
    assert _units(cols, 39, 20) == [26]                                     # 30 = s + M is not part of the first piece
    assert _units(cols, 39, 21) == [30]
    assert _units(cols[:6], 31, 20) == [26] and _units(cols[:5], 30, 20) == [26] and _units(cols[:5], 29, 20) == []
    assert _units(cols, 49, 20) == [26] and _units(cols, 50, 20) == [26, 38]                  # s' = 30: after the last column below 50,
    assert _units(cols + [49], 50, 20) == [26, 49] and _units(cols + [50], 51, 20) == [26, 38]            # and 50 starts the third piece


def test_a_natural_gap_inside_the_limit_wins():
    M = 40
    cols = [10, 12] + list(range(35, 90, 3))                                # 12 -> 35 is natural (23 columns); 35, 38, ..., 89 gapless
    assert _units(cols, 100, M) == [74, 89]                                 # the piece after the gap starts at 35: forced after 74 < 75
    assert _units(list(range(10, 90, 3)), 100, M) == [49, 88]               # without the gap the cut falls at 10 + M
    assert _units([c for c in cols if c < 60], 60, M) == [12]               # the natural cut goes at once, the piece from 35 waits
    assert _units([c for c in cols if c < 75], 75, M) == [74]               # ... and goes with it as one list when both are due


def test_limit_below_the_distance_or_one_is_refused():
    for M in (D - 1, 0, -3, 9.5):
        with pytest.raises(ValueError, match="max_unit_cols"):
            _units([10, 20], 50, M)
    with pytest.raises(ValueError, match="max_unit_cols"):
        postproc.online_units([3], 10, TS, 1, 0.0, 0)
    assert _units([10, 20], 50, D) == [10, 20] and postproc.online_units([3], 10, TS, 1, 0.0, 1).tolist() == [3]


def test_a_limit_of_the_whole_axis_is_no_limit():
    rng = np.random.default_rng(8)
    for _ in range(300):
        cols = rng.integers(0, 100, int(rng.integers(0, 40)))
        bound = int(rng.integers(0, 101))
        for M in (100, 101, 1000):
            assert _units(cols, bound, M) == _units(cols, bound, None)


# ---- replay: streaming units against the one-shot twin, host stages per unit ----------------------------------------------------------------

ROWS, N_COLS, M_REPLAY, TC, SP = 5, 240, 24, 6.75, 20e3
TS_REPLAY = np.arange(N_COLS) * 0.75 + 4990.0


def _canon(s):
    return s[np.lexsort((s[:, 4], s[:, 2], s[:, 1], s[:, 0], s[:, 3]))]


def _candidates(rng):
    """A random candidate set: two or three dense stretches (every gap below d, 30 to 90 columns long) among sparse ones."""
    cells = set()
    at = int(rng.integers(0, 15))
    while at < N_COLS - 5:
        if rng.random() < 0.6:                                              # a dense stretch
            hi = min(at + int(rng.integers(30, 90)), N_COLS - 1)
            while at < hi:
                for row in rng.choice(ROWS, int(rng.integers(1, 3)), replace=False):
                    cells.add((int(row), at))
                at += int(rng.integers(1, D))
        else:
            cells.add((int(rng.integers(ROWS)), at))
        at += int(rng.integers(D, 45))
    cells = np.array(sorted(cells), dtype=np.int64)
    v = (0.2 + rng.permutation(len(cells)) / 4096.0).astype(np.float32)     # distinct heights
    return cells[:, 0], cells[:, 1], v


def _run_units(r, c, v, xq, index_lists, cache):
    out = [np.zeros((0, 5))]
    for idx in index_lists:
        key = tuple(idx.tolist())
        if key not in cache:
            cache[key] = _pipeline(r[idx], c[idx], v[idx], xq, TS_REPLAY, D, BW, TC, SP)[0]
        out.append(cache[key])
    return _canon(np.vstack(out))


def _split(c, idx, ends):
    """The index lists of the units that end at the columns `ends`, out of the candidates `idx`."""
    lists, prev = [], -1
    for e in ends:
        lists.append(idx[(c[idx] > prev) & (c[idx] <= e)])
        prev = e
    return lists, prev


def test_streamed_units_equal_the_one_shot_units():
    rng = np.random.default_rng(2024)
    xq = np.c_[rng.uniform(0, 30e3, (ROWS, 2)), rng.uniform(-20e3, 0, ROWS)]
    forced_sets = differs = early = 0
    for trial in range(200):
        r, c, v = _candidates(rng)
        every = np.arange(len(c))
        cache = {}
        ends = postproc.online_units(c, N_COLS, TS_REPLAY, D, BW, M_REPLAY).tolist()
        lists, last = _split(c, every, ends)
        assert last == c.max() and sum(len(x) for x in lists) == len(c)     # the one-shot form leaves nothing behind
        want = _run_units(r, c, v, xq, lists, cache)
        forced_sets += len(ends) >= 3
        differs += not np.array_equal(want, _run_units(r, c, v, xq, [every], cache))
        for _ in range(2):
            emitted, released, bound, units = np.zeros(len(c), dtype=bool), np.zeros(len(c), dtype=bool), 0, []
            while bound < N_COLS:
                bound = min(bound + int(rng.integers(1, 40)), N_COLS)
                emitted |= (c < bound) | ((c < bound + 12) & (rng.random(len(c)) < 0.5))
                held = np.flatnonzero(emitted & ~released)
                got, last = _split(c, held, postproc.online_units(c[held], bound, TS_REPLAY, D, BW, M_REPLAY).tolist())
                for idx in got:
                    assert len(idx)
                    released[idx] = True
                units += got
                early += bool(got) and bound < N_COLS
                below = c[emitted & ~released]
                below = below[below < bound]
                assert below.size == 0 or bound - below.min() < M_REPLAY, (trial, bound)          # the invariant, after every step
            assert released.all()
            assert np.array_equal(_run_units(r, c, v, xq, units, cache), want), trial
    assert forced_sets >= 100 and differs >= 20 and early >= 400           # otherwise the equality shows little


def test_two_peaks_of_a_row_across_a_forced_cut_both_survive():
    """Where the bounded result provably is not the unbounded one: row 0 holds peaks at columns 26 and 32, closer than d = 10. One list:
    the distance rule removes the lower one (26). M = 20: the cut falls after column 28 < 10 + M, and both survive."""
    r = np.array([0, 1, 0, 1, 0, 1, 0, 1], dtype=np.int64)
    c = np.array([10, 14, 18, 22, 26, 28, 32, 38], dtype=np.int64)
    v = np.array([0.9, 0.3, 0.5, 0.3, 0.6, 0.3, 0.8, 0.3], dtype=np.float32)          # row 0: 26 beats 18, 32 beats 26
    xq = np.array([[0.0, 0.0, 0.0], [25e3, 0.0, 0.0]])
    args = (xq, TS, D, BW, 0.1, 1.0)                                        # windows so small that LocalMarching joins nothing
    whole = _pipeline(r, c, v, *args)[0]
    assert postproc.online_units(c, 100, TS, D, BW, 20).tolist() == [28, 38]
    a, b = c <= 28, c > 28
    units = np.vstack((_pipeline(r[a], c[a], v[a], *args)[0], _pipeline(r[b], c[b], v[b], *args)[0]))
    row0 = lambda s: sorted(s[s[:, 0] == 0.0][:, 3].tolist())
    assert row0(whole) == [TS[10], TS[32]]                                  # 18 falls to 10 (and to 26), 26 falls to 32
    assert row0(units) == [TS[10], TS[26], TS[32]]                          # 26 never meets 32
    assert len(units) == len(whole) + 1


# ---- the argument, where it is refused before any device use ----------------------------------------------------------------------------------

def test_detect_refine_associate_refuses_the_limit_off_the_dense_device_path():
    assert inspect.signature(apply.detect_refine_associate).parameters["max_unit_cols"].default is None
    assert inspect.signature(postproc.detect_sources_device).parameters["max_unit_cols"].default is None
    assert inspect.signature(postproc.OnlineDetector.__init__).parameters["max_unit_cols"].default is None
    assert "max_unit_cols" not in inspect.signature(postproc.detect_sources).parameters
    assert "max_unit_cols" not in inspect.signature(postproc.detect_sources_banded).parameters
    rest = [None] * 20
    with pytest.raises(ValueError, match="detect_on_device"):
        apply.detect_refine_associate(None, None, None, *rest, max_unit_cols=40)
    banded = object.__new__(apply.BandedOut2)
    with pytest.raises(ValueError, match="BandedOut2"):
        apply.detect_refine_associate(None, None, banded, *rest, detect_on_device=True, max_unit_cols=40)
