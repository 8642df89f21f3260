"""GPU: saving and resuming the online objects. The ring checkpoint kernels (`engine.ring_save` /
`engine.ring_load`) against torch gathers; `OnlineDay`, `OnlineDetector` and `OnlineCatalogue` saved between two calls, sent through
`torch.save` / `torch.load`, loaded into newly constructed objects and fed on NEXT TO the objects that were saved: every later return
of the resumed object is the continuing one's, bit for bit, and everything concatenated is the offline day. The set-ups are the ones of
tests/test_online_day_gpu.py and tests/test_online_catalogue_gpu.py.

`step_size` 1.0 below is the 1 s stride of window starts of tests/test_online_day_gpu.py (`_times`: anything but "half"); the
schedule's own `step_size` argument takes the reference's three names only."""
import io

import numpy as np
import pytest
import torch

from genie_amd import _lib, apply, engine, postproc, synthetic
from tests import test_online_catalogue_gpu as cat_t
from tests import test_online_day_gpu as day_t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GENIE_OK, GENIE_ERR_ARG = 0, -1


def _through_torch_save(state):
    buf = io.BytesIO()
    torch.save(state, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


def _host_only(x):
    """True when `x` (nested dicts, lists, tuples) holds Python scalars, strings, None, numpy arrays and CPU tensors only."""
    if torch.is_tensor(x):
        return not x.is_cuda
    if isinstance(x, dict):
        return all(isinstance(k, str) and _host_only(v) for k, v in x.items())
    if isinstance(x, (list, tuple)):
        return all(_host_only(v) for v in x)
    return x is None or isinstance(x, (bool, int, float, str, np.ndarray, np.generic))


# ---- 1. the ring kernels ----------------------------------------------------------------------------------------------------------------------

def _ring(Q, W):
    return (torch.arange(Q * W, dtype=torch.float32, device=DEV).reshape(Q, W) + 1.0) * 0.5          # distinct, non-zero, exact in fp32


# Q = 5, W = 7: [5, 10) wraps the ring's end, [14, 21) and [3, 10) are the full width (the second wraps), [4, 4) is empty, [500, 504) and
# [502, 507) start in the hundreds (500 % 7 = 3; 502 % 7 = 5: wraps). Q = 300, W = 67, 65 columns: 19 500 elements = 76 full workgroups
# and a last one of 44 threads (a partial last wave); 130 % 67 = 63: wraps.
RING_CASES = [(5, 7, 5, 10, (7, 11)), (5, 7, 14, 21, (7, 11)), (5, 7, 3, 10, (7, 11)), (5, 7, 4, 4, (7, 11)), (5, 7, 500, 504, (7, 11)),
              (5, 7, 502, 507, (7, 11)), (300, 67, 130, 195, (67, 71)), (300, 67, 400, 465, (65, 200))]


@pytest.mark.parametrize("Q,W,c_lo,c_hi,widths", RING_CASES)
def test_ring_save_reads_the_block_and_ring_load_puts_it_back(Q, W, c_lo, c_hi, widths):
    ring = _ring(Q, W)
    before = ring.clone()
    block = engine.ring_save(ring, c_lo, c_hi)
    torch.cuda.synchronize()
    cols = torch.arange(c_lo, c_hi, device=DEV)
    assert block.shape == (Q, c_hi - c_lo) and block.dtype == torch.float32 and block.is_contiguous()
    assert torch.equal(block, before[:, cols % W])                       # the torch gather of ring[:, (c_lo + j) % W]
    assert torch.equal(ring, before)                                     # the ring is only read
    for W2 in widths:
        ring2 = torch.zeros((Q, W2), dtype=torch.float32, device=DEV)
        assert engine.ring_load(ring2, block, c_lo) is ring2
        torch.cuda.synchronize()
        want = torch.zeros_like(ring2)
        want[:, cols % W2] = block
        assert torch.equal(ring2, want)                                  # exactly those slots, no others
        closed = engine.ring_close(ring2, c_lo, c_hi)
        torch.cuda.synchronize()
        assert torch.equal(closed, block) and not bool(ring2.any())      # the closed block is the saved one; every other slot still zero


@pytest.mark.parametrize("Q,W,c_lo", [(5, 7, 3), (5, 7, 500), (300, 67, 130)])
def test_ring_save_and_load_refuse_bad_arguments_and_write_nothing(Q, W, c_lo):
    lib = _lib.load()
    ring = _ring(Q, W)
    before = ring.clone()
    out = torch.full((Q, W + 1), -7.0, dtype=torch.float32, device=DEV)
    for name in ("genie_ring_save", "genie_ring_load"):
        fn = getattr(lib, name)
        assert fn(ring.data_ptr(), Q, W, c_lo, c_lo + W + 1, out.data_ptr(), None) == GENIE_ERR_ARG       # more columns than slots
        assert name.encode() in lib.genie_last_error()
        assert fn(None, Q, W, c_lo, c_lo + 2, out.data_ptr(), None) == GENIE_ERR_ARG                       # a null pointer, a range
        assert fn(ring.data_ptr(), Q, W, c_lo, c_lo + 2, None, None) == GENIE_ERR_ARG
        assert b"null" in lib.genie_last_error()
        assert fn(ring.data_ptr(), Q, W, c_lo + 1, c_lo, out.data_ptr(), None) == GENIE_ERR_ARG            # c_hi < c_lo
        assert fn(ring.data_ptr(), Q, 0, c_lo, c_lo, out.data_ptr(), None) == GENIE_ERR_ARG                # no slots
        assert fn(None, 0, W, c_lo, c_lo + 2, None, None) == GENIE_OK                                      # Q = 0: nothing to do
        assert fn(None, Q, W, c_lo, c_lo, None, None) == GENIE_OK                                          # an empty range
    torch.cuda.synchronize()
    assert torch.equal(ring, before) and bool((out == -7.0).all())
    with pytest.raises(ValueError, match="ring_save"):
        engine.ring_save(ring, c_lo, c_lo + W + 1)
    with pytest.raises(ValueError, match="ring_load"):
        engine.ring_load(ring, out, c_lo)                                # W + 1 columns
    with pytest.raises(ValueError, match="ring_load"):
        engine.ring_load(ring, out[:, :2], c_lo)                         # not contiguous
    with pytest.raises(ValueError, match="ring_load"):
        engine.ring_load(ring, out[:1, :2].contiguous(), c_lo)           # another row count
    with pytest.raises(ValueError, match="ring_load"):
        engine.ring_load(ring, out[:, :2].contiguous().cpu(), c_lo)
    with pytest.raises(ValueError, match="ring_save"):
        engine.ring_save(ring.double(), c_lo, c_lo + 1)
    empty = torch.zeros((0, W), dtype=torch.float32, device=DEV)
    assert engine.ring_save(empty, c_lo, c_lo + 3).shape == (0, 3)
    assert engine.ring_load(empty, torch.zeros((0, 3), dtype=torch.float32, device=DEV), c_lo) is empty
    torch.cuda.synchronize()
    assert torch.equal(ring, before)


# ---- 2., 3. the day -----------------------------------------------------------------------------------------------------------------------------

def _day_chunks():
    """[(rows of P, t_now)]: the irregular cuts of tests/test_online_day_gpu.py, then one `t_now` behind the last window's reads, at
    which every window has run while `finish` has not been called."""
    _, _, P, _, max_t, _, _ = day_t._setup()
    cuts = list(day_t._cuts()) + [float(P[-1, 0]) + max_t + 30.0]
    out, lo = [], 0
    for t_now in cuts:
        hi = int(np.searchsorted(P[:, 0], t_now, side="left"))
        out.append((P[lo:max(lo, hi)], float(t_now)))
        lo = max(lo, hi)
    assert lo == len(P)
    return out


def _early_cut_ok(day):
    """Windows run and unrun, open columns in the ring, a retained pick older than `t_now`: nothing of the state is empty."""
    return 0 < day.n_run < len(day.times) and day.last_col + 1 > day.closed and len(day.picks) > 0 and day.picks.t_host.min() < day.t_now


def _assert_same_day(new, old):
    assert (new.closed, new.n_run, new.last_col, new.t_now) == (old.closed, old.n_run, old.last_col, old.t_now)
    assert np.array_equal(new.times_used, old.times_used) and len(new.times_used) == len(old.times_used)
    assert new.picks.frozen_t == old.picks.frozen_t and new.picks.n_fed == old.picks.n_fed
    assert np.array_equal(new.picks.t_host, old.picks.t_host)
    for f in ("t", "sta", "phase", "index"):
        assert torch.equal(getattr(new.picks, f), getattr(old.picks, f)), f


@pytest.mark.parametrize("tail_batch", [1, 16])
@pytest.mark.parametrize("step_size", ["half", 1.0])
def test_a_saved_day_resumes_bit_equal(step_size, tail_batch):
    """Two cuts. The early one is the first call after which nothing of the state is empty (`_early_cut_ok`, asserted again on the
    saved state: open non-zero columns, a retained pick older than `t_now`, windows unrun). The late one follows the last window and
    precedes `finish`: the `feed` that runs the last window closes the whole axis (`frontiers[n]` is its end), so there the ring block
    is [Q, 0] by construction and the counters and the store carry the state. At each cut the state goes through `torch.save` into two
    new objects, ring of `ring_min` and of `ring_min + 3` columns, which are fed on next to the saved one."""
    want, used = day_t._offline(step_size, tail_batch)
    chunks = _day_chunks()
    day = day_t._online(step_size, tail_batch)
    blocks, resumed, cuts_taken = [], [], []                             # resumed: (object, index of its first chunk, its blocks)
    for i, (rows, t_now) in enumerate(chunks):
        first, block = day.feed(rows, t_now)
        blocks.append(block)
        for new, _, theirs in resumed:
            first_n, block_n = new.feed(rows, t_now)
            assert first_n == first and torch.equal(block_n, block), (i, first_n, first)
            _assert_same_day(new, day)
            theirs.append(block_n)
        early = not cuts_taken and _early_cut_ok(day)
        late = i == len(chunks) - 1
        if not (early or late):
            continue
        cuts_taken.append(i)
        before = (day.ring.clone(), day.n_run, day.closed, day.last_col, day.t_now, len(day.picks), day.picks.frozen_t)
        state = day.state_dict()
        assert _host_only(state)
        after = (day.ring, day.n_run, day.closed, day.last_col, day.t_now, len(day.picks), day.picks.frozen_t)
        assert torch.equal(before[0], after[0]) and before[1:] == after[1:]                  # the saved object is left as it was
        if early:                                                        # not an empty state: open non-zero columns, a pick behind t_now
            assert day.last_col + 1 > day.closed and state["ring_block"].shape == (want.shape[0], day.last_col + 1 - day.closed)
            assert bool(state["ring_block"].any())
            assert (state["picks"]["t"] < day.t_now).any() and day.n_run < len(day.times)
        else:                                                            # every window has run: the whole axis has closed in that call
            assert day.n_run == len(day.times) and day.closed == len(day.tsteps_abs) and state["ring_block"].shape[1] == 0
        loaded = _through_torch_save(state)
        for ring_cols in (None, day.ring_min + 3):
            new = day_t._online(step_size, tail_batch, ring_cols=ring_cols)
            assert new.ring_cols == (day.ring_min if ring_cols is None else day.ring_min + 3)
            new.load_state_dict(loaded)
            _assert_same_day(new, day)
            resumed.append((new, i + 1, []))
    assert len(cuts_taken) == 2 and cuts_taken[0] < len(chunks) - 2, cuts_taken
    first, block = day.finish()
    blocks.append(block)
    assert day.closed == len(day.tsteps_abs) and np.array_equal(day.times_used, used)
    assert torch.equal(torch.cat(blocks, dim=1), want)
    for new, start, theirs in resumed:
        first_n, block_n = new.finish()
        assert first_n == first and torch.equal(block_n, block)
        _assert_same_day(new, day)
        assert torch.equal(torch.cat(blocks[:start] + theirs + [block_n], dim=1), want)      # saved + resumed = the offline day


def _fed_day(tail_batch=16):
    """A day fed up to the first cut at which nothing of its state is empty; returns (day, the chunks, the next chunk's index)."""
    chunks = _day_chunks()
    day = day_t._online("half", tail_batch)
    for i, (rows, t_now) in enumerate(chunks):
        day.feed(rows, t_now)
        if _early_cut_ok(day):
            return day, chunks, i + 1
    raise AssertionError("no cut with open columns and retained picks")


def test_a_late_pick_is_refused_after_the_resume_as_before_it():
    day, chunks, nxt = _fed_day()
    new = day_t._online("half", 16)
    new.load_state_dict(_through_torch_save(day.state_dict()))
    frozen = day.picks.frozen_t
    assert np.isfinite(frozen) and new.picks.frozen_t == frozen
    rows, t_now = chunks[nxt]
    bad = np.concatenate((rows, rows[:1])) if len(rows) else day_t._setup()[2][:1].copy()
    bad[-1, 0] = frozen - 1.0
    said = []
    for d in (day, new):
        state = (d.n_run, d.closed, d.t_now, len(d.picks))
        with pytest.raises(ValueError) as err:
            d.feed(bad, t_now)
        assert repr(float(frozen)) in str(err.value) and state == (d.n_run, d.closed, d.t_now, len(d.picks))
        said.append(str(err.value))
    assert said[0] == said[1]
    a, b = day.feed(rows, t_now), new.feed(rows, t_now)                  # the feed goes on, in step
    assert a[0] == b[0] and torch.equal(a[1], b[1])


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------------

def _untouched(day):
    return (day.n_run, day.closed, day.last_col, len(day.picks), day.picks.n_fed) == (0, 0, -1, 0, 0) and day.t_now == -np.inf \
        and not bool(day.ring.any())


def test_a_day_refuses_a_state_of_another_schedule_and_stays_as_it_was():
    net, geom, P, trv, max_t, _, tsteps_abs = day_t._setup()
    day, chunks, nxt = _fed_day()
    state = _through_torch_save(day.state_dict())
    n_open = state["ring_block"].shape[1]
    assert n_open >= 2
    others = (("tsteps_abs", apply.OnlineDay(net, geom, trv, tsteps_abs + 1e-6, times=day_t._times("half"), max_t=max_t, tail_batch=16)),
              ("times", day_t._online("half", 16, times=day_t._times("half")[:-1])),
              ("tail_batch", day_t._online("half", 8)),
              ("kernel_sig_t", day_t._online("half", 16, kernel_sig_t=synthetic.KERNEL_SIG_T * 1.25)),
              ("min_required_picks", day_t._online("half", 16, min_required_picks=2)))
    for field, other in others:
        with pytest.raises(ValueError, match=r"another %s " % field):
            other.load_state_dict(state)
        assert _untouched(other), field
    small = day_t._online("half", 16)
    small.ring = small.ring[:, :n_open - 1].contiguous()                 # (the constructor admits no ring below ring_min)
    with pytest.raises(ValueError, match="ring_cols = %d" % (n_open - 1)):
        small.load_state_dict(state)
    assert _untouched(small)
    broken = dict(state, picks=dict(state["picks"], t=state["picks"]["t"][::-1].copy()))
    fresh = day_t._online("half", 16)
    with pytest.raises(ValueError, match="time-sorted"):
        fresh.load_state_dict(broken)                                    # the last check fails: the ring has not been written
    assert _untouched(fresh)
    before = (day.ring.clone(), day.n_run, day.closed, len(day.picks))
    with pytest.raises(RuntimeError, match="has been fed"):
        day.load_state_dict(state)                                       # an object that has been fed
    assert torch.equal(day.ring, before[0]) and before[1:] == (day.n_run, day.closed, len(day.picks))
    fresh.load_state_dict(state)                                         # and the state itself loads
    a, b = day.feed(*chunks[nxt]), fresh.feed(*chunks[nxt])
    assert a[0] == b[0] and torch.equal(a[1], b[1])


# ---- 4. detector and catalogue ------------------------------------------------------------------------------------------------------------------

def _assert_same_return(got, want):
    assert sorted(got) == sorted(want)
    for key in ("srcs", "srcs_refined"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    assert got["trv_out_srcs"].dtype == want["trv_out_srcs"].dtype and torch.equal(got["trv_out_srcs"], want["trv_out_srcs"])
    for key in ("Out_p_save", "Out_s_save"):
        assert len(got[key]) == len(want[key])
        assert all(a.dtype == b.dtype and a.device == b.device and torch.equal(a, b) for a, b in zip(got[key], want[key])), key
    for key in ("Save_picks", "lp_meta"):
        assert len(got[key]) == len(want[key])
        assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got[key], want[key])), key


def test_a_saved_catalogue_resumes_bit_equal_and_all_or_nothing():
    want = cat_t._twin()
    chunks = cat_t._chunks("random")
    day, det, cat = cat_t._catalogue("device")
    parts, resumed, cut = [], None, None                                 # resumed: (day, det, catalogue), and its returns
    for i, (rows, t_now) in enumerate(chunks):
        parts.append(cat.push(rows, t_now))
        if resumed is not None:
            theirs.append(resumed[2].push(rows, t_now))
            _assert_same_return(theirs[-1], parts[-1])
            assert (resumed[2].pending, resumed[2].undecided, resumed[1].held, resumed[1].seen, resumed[0].closed) == \
                (cat.pending, cat.undecided, det.held, det.seen, day.closed)
        if cut is None and cat.undecided > 0 and i < len(chunks) - 1:
            cut = i
            assert cat.pending > 0 or cat.undecided > 0
            assert len(cat._results) == cat.undecided and all(r[k].is_cuda for r in cat._results for k in (0, 1, 2))
            assert any(r[1].numel() > 0 for r in cat._results)           # a likelihood vector with content travels
            rows_before, seen_before = cat._rows.copy(), det.seen
            state = cat.state_dict()
            assert sorted(state) == ["catalogue", "day", "det"] and _host_only(state)
            assert np.array_equal(cat._rows, rows_before) and det.seen == seen_before == day.closed
            for r, s in zip(cat._results, state["catalogue"]["results"]):
                for k in (0, 1, 2):
                    assert s[k].dtype == r[k].dtype and s[k].shape == r[k].shape and torch.equal(s[k], r[k].cpu())
            loaded = _through_torch_save(state)
            # all three or none: the day's and the detector's states fit, the catalogue's Philox key does not
            day_x, det_x, cat_x = cat_t._catalogue("device", rand=apply.PhiloxCloud(cat_t.KEY + 1))
            with pytest.raises(ValueError, match="another philox_key "):
                cat_x.load_state_dict(loaded)
            assert _untouched(day_x) and det_x.seen == 0 and det_x.held == 0 and cat_x.n_released == 0 and cat_x.undecided == 0
            xq = np.asarray(cat_t._setup()[1].x_query, dtype=np.float64)
            args = list(cat_t._detect_args(xq, cat_t._setup()[6]))
            args[3] = cat_t.DETECT["thresh"] * 1.5
            det_y = postproc.OnlineDetector(*args, device=DEV)
            with pytest.raises(ValueError, match="another thresh "):
                det_y.load_state_dict(loaded["det"])
            assert det_y.seen == 0 and det_y.held == 0
            with pytest.raises(RuntimeError):
                cat.load_state_dict(loaded)                              # objects that have run
            with pytest.raises(RuntimeError):
                det.load_state_dict(loaded["det"])
            resumed, theirs = cat_t._catalogue("device"), []
            resumed[2].load_state_dict(loaded)
            assert all(r[k].device == cat._results[0][k].device for r in resumed[2]._results for k in (0, 1, 2))
            assert resumed[1].held == det.held and np.array_equal(resumed[1].held_cols, det.held_cols)
            assert resumed[1].peaks.bound == det.peaks.bound and resumed[0].retain_from == day.retain_from
    assert cut is not None
    parts.append(cat.finish())
    theirs.append(resumed[2].finish())
    _assert_same_return(theirs[-1], parts[-1])
    assert sum(len(p["srcs_refined"]) for p in theirs) >= 1              # a source that was undecided at the cut came out of the resumed one
    for whole in (parts, parts[:cut + 1] + theirs):
        _assert_same_return(cat_t._concat(whole), want)
