"""GPU: a window's pick lists in one launch (genie_pick_lists through `engine.pick_lists` / `ResidentPicks.pick_inputs_device`) against
`ResidentPicks.pick_inputs`, the torch statements that stay its oracle: `torch.equal` on all four outputs, no tolerance.

Range sizes 0, 1, 255, 256, 257 and 1 000 (the kernel places chunks of 256 picks) x station sets of 1, 2 and 2 000 stations, every pick
on one station, every pick on the last station, many equal times, the ball query on (`kernel_sig_t = 6`, `t_win = 10`) and off, and a
`PickStore` after a merge and after a trim (a nonzero base)."""
import ctypes

import numpy as np
import pytest
import torch

from genie_amd import _lib, apply, engine

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [0, 1, 255, 256, 257, 1000]
MAX_T = 20.0
T0 = 5000.0


def _picks(n, n_sta, seed, sig, mode="spread", ties=False):
    """`n` picks inside the embedding range of the window at T0 for `sig` (with sigma 6 about a tenth of them outside the ball query
    of `t_win = 10`), plus 40 outside the range on both sides."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(T0 - 2.0 * sig + 0.1, T0 + MAX_T + 2.0 * sig - 0.1, n)
    if ties:
        t = np.round(t / 4.0) * 4.0                    # a handful of distinct times: the order within a station is the caller's
    sta = {"spread": rng.integers(0, n_sta, n), "one": np.full(n, n_sta // 2), "last": np.full(n, n_sta - 1)}[mode]
    far = np.concatenate((rng.uniform(T0 - 400.0, T0 - 13.0, 20), rng.uniform(T0 + MAX_T + 13.0, T0 + 400.0, 20)))
    P = np.zeros((n + 40, 5))
    P[:, 0] = np.concatenate((t, far))
    P[:, 1] = np.concatenate((sta, rng.integers(0, n_sta, 40)))
    P[:, 3] = rng.random(n + 40)
    P[:, 4] = rng.integers(0, 2, n + 40)
    return P[rng.permutation(n + 40)]                  # the caller's order is no time order


def _same(picks, sig, t_win=10.0, t0=T0):
    want = picks.pick_inputs(t0, MAX_T, sig, t_win)
    got = picks.pick_inputs_device(t0, MAX_T, sig, t_win)
    assert len(got) == 4
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.device == w.device and g.shape == w.shape
        assert torch.equal(g, w)
    return want


@pytest.mark.parametrize("sig", [3.0, 6.0])            # 2 sigma <= t_win: no ball query; 2 sigma > t_win: the ball query cuts
@pytest.mark.parametrize("n_sta", [1, 2, 2000])
@pytest.mark.parametrize("n", SIZES)
def test_pick_lists_equal_pick_inputs(n, n_sta, sig):
    picks = apply.ResidentPicks(_picks(n, n_sta, 7 * n + n_sta, sig), np.arange(n_sta), n_sta, DEV)
    lo, hi = picks.embed_range(T0, MAX_T, sig)
    assert hi - lo == n
    tp = _same(picks, sig)[0]
    if sig == 6.0 and n >= 255:
        assert 0 < tp.shape[0] < n                     # the ball query removed something, not everything
    elif sig == 3.0:
        assert tp.shape[0] == n


@pytest.mark.parametrize("sig", [3.0, 6.0])
@pytest.mark.parametrize("mode,ties", [("one", False), ("last", False), ("spread", True), ("one", True)])
@pytest.mark.parametrize("n", SIZES)
def test_pick_lists_on_one_station_and_on_equal_times(n, mode, ties, sig):
    picks = apply.ResidentPicks(_picks(n, 37, 11 * n + 3, sig, mode=mode, ties=ties), np.arange(37), 37, DEV)
    tp, ip, _, idx = _same(picks, sig)
    if n >= 255:
        if mode != "spread":
            assert len(torch.unique(ip)) == 1 and int(ip[0]) == {"one": 18, "last": 36}[mode]
        if ties:
            assert len(torch.unique(tp)) <= 12 and not torch.equal(idx, torch.sort(idx)[0])


def test_pick_lists_of_a_store_after_a_merge_and_a_trim():
    """The model's stations are a subset of the file's; the second chunk is older than the first (a merge), then the store is trimmed
    (its live picks start at a nonzero base of the buffers)."""
    n_all, ind_use = 50, np.arange(3, 50, 2)
    P = _picks(1000, n_all, 5, 6.0)
    late = P[:, 0] >= T0 + 4.0
    P = np.concatenate((P[late], P[~late]))           # feed order: `index` counts the rows fed
    store = apply.PickStore(ind_use, n_all, DEV, capacity=64)
    store.append(P[:int(late.sum())])
    store.append(P[int(late.sum()):])
    whole = apply.ResidentPicks(P, ind_use, n_all, DEV)
    for sig, t0 in ((3.0, T0), (6.0, T0)):
        for g, w in zip(_same(store, sig, t0=t0), whole.pick_inputs(t0, MAX_T, sig)):
            assert torch.equal(g, w)
    store.trim(T0 - 1.0)
    assert store._base > 0
    for sig, t0 in ((3.0, T0 + 7.0), (6.0, T0 + 12.0)):   # windows that read nothing at or before T0 - 1
        want = _same(store, sig, t0=t0)
        assert want[0].shape[0] > 100
        for g, w in zip(want, whole.pick_inputs(t0, MAX_T, sig)):
            assert torch.equal(g, w)


def test_the_count_on_the_device_and_the_refusals():
    n_sta = 9
    picks = apply.ResidentPicks(_picks(600, n_sta, 2, 6.0), np.arange(n_sta), n_sta, DEV)
    lo, hi = picks.embed_range(T0, MAX_T, 6.0)
    run = (picks.t[lo:hi], picks.sta[lo:hi], picks.phase[lo:hi], picks.index[lo:hi])
    ball = (T0 + MAX_T / 2.0, 10.0 + MAX_T / 2.0)
    want = picks.pick_inputs(T0, MAX_T, 6.0, 10.0)
    out = engine.pick_lists(run, n_sta, T0, ball)
    m = int(out[4].item())
    assert m == want[0].shape[0] and all(torch.equal(o[:m], w) for o, w in zip(out, want))
    assert int(engine.pick_lists(run, n_sta, T0, None)[4].item()) == hi - lo
    assert int(engine.pick_lists(tuple(x[:0] for x in run), n_sta, T0, None)[4].item()) == 0
    # a station set beyond the LDS table: None from the wrapper, GENIE_ERR_ARG from the library, and the store falls back to torch
    big = engine.pick_lists_max_sta() + 1
    assert engine.pick_lists_max_sta() >= 2000 and engine.pick_lists(run, big, T0, None) is None
    wide = apply.ResidentPicks(_picks(300, big, 4, 3.0), np.arange(big), big, DEV)
    _same(wide, 3.0)
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    args = lambda n, n_sta: ([p(x) for x in run] + [n, n_sta, ctypes.c_double(T0), 0, ctypes.c_double(0.0), ctypes.c_double(0.0)]
                             + [p(o) for o in out] + [None])
    assert lib.genie_pick_lists(*args(hi - lo, big)) != 0 and b"genie_pick_lists" in lib.genie_last_error()
    assert lib.genie_pick_lists(*args(-1, n_sta)) != 0 and lib.genie_pick_lists(*args(hi - lo, 0)) != 0
    with pytest.raises(ValueError):
        engine.pick_lists((run[0].float(),) + run[1:], n_sta, T0, None)
    with pytest.raises(ValueError):
        apply.ResidentPicks(_picks(5, 3, 1, 3.0), np.arange(3), 3, "cpu").pick_inputs_device(T0, MAX_T, 3.0)
    torch.cuda.synchronize()
