"""GPU: the refine pass over batches of sources (`apply.refine_sources(source_batch=B)`): the batched tail with a query set per window
(`flush_windows_clouds`, genie_tail_batched_q), the two batch kernels (`postproc.refine_select_batch_device`,
`postproc.refine_cloud_batch_device`) and the pass itself, each against the form it batches -- per-window `forward_fixed_source`, the
single kernels, `source_batch=1` -- with `torch.equal` / `np.array_equal`: the batched tail is bit-identical by construction, the kNN
search is exact and the selection keeps its order, so no tolerance applies.

The model carries the assoc_7x45 weights on 9 stations x 53 source nodes (a second leg: 45 nodes over the same stations), the picks come
from `genie_amd.synthetic`."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from genie_amd import apply, graph, module, postproc, synthetic
from tests.util import GOLDEN_DIR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDENT = lambda x: x                                                                        # noqa: E731
RANGES = ((0.0, 60e3), (0.0, 60e3), (-40e3, 2e3))
OFF_MIN, OFF_RNG = np.array([[-5e3, -5e3, -3e3]]), np.array([[10e3, 10e3, 6e3]])
N_QUERY = 150
KEY = 0x5EED0123456789ABCDEF
S, SEED = 9, 91
QUIET_T, HALF_QUIET = 30000.0, 1           # a stretch of the day without picks; the source the second leg has no window for


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV)


def _leg(G, weights, max_t, cls=apply.GridLeg):
    geom = synthetic.Geometry(S, G, L=60e3, n_query=8, seed=SEED)
    trv = geom.travel_times().astype(np.float32)
    assert float(trv.max()) < max_t
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV)
    net.load_state_dict({k: v.clone() for k, v in weights.items()}, strict=True)
    net.eval()
    sig = synthetic.KERNEL_SIG_T
    edges_p, edges_s, dt_partition = graph.time_pointers(trv, max_t=max_t, dt=sig / 5.0, k=10, win=2.0 * sig)
    net.set_adjacencies_base(torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src), torch.from_numpy(geom.edge_attr()).to(DEV),
                             _t(geom.locs), _t(geom.x_grid), torch.from_numpy(edges_p).to(DEV), torch.from_numpy(edges_s).to(DEV),
                             _t(dt_partition), _t(trv.reshape(-1, 2)))
    return cls(net, geom.x_grid, trv), geom, trv


class _HalfQuietLeg(apply.GridLeg):
    """A leg that has no window for the source at `quiet_t` while the other leg has one (in the field: a grid whose stations were down).
    The passes under test see `embed` return None for it, as they do for a window without picks."""
    quiet_t = None

    def embed(self, picks, t0, max_t, kernel_sig_t, dt):
        return None if float(t0) == self.quiet_t else super().embed(picks, t0, max_t, kernel_sig_t, dt)


@functools.lru_cache(maxsize=None)
def _setup():
    from oracle import genie_oracle as O
    w = O.weights_from_npz(np.load(os.path.join(GOLDEN_DIR, "assoc_7x45.npz")))
    geom = synthetic.Geometry(S, 53, L=60e3, n_query=8, seed=SEED)
    P = synthetic.make_picks(geom, 400, seed=SEED + 1)
    P[:, 0] = P[:, 0] * 0.5 + 7000.0
    P = P[np.argsort(P[:, 0], kind="stable")]
    max_t = float(np.ceil(max(synthetic.Geometry(S, G, L=60e3, n_query=8, seed=SEED).travel_times().max() for G in (53, 45)) + 1.0))
    s = types.SimpleNamespace(P=P, max_t=max_t, sig=3.0, dt=0.3, tq=np.arange(-3.0, 3.75, 0.75).reshape(-1, 1))
    s.leg, s.geom, s.trv = _leg(53, w, max_t)
    s.leg_b, geom_b, _ = _leg(45, w, max_t, _HalfQuietLeg)
    assert np.array_equal(geom_b.locs, geom.locs)
    s.locs = geom.locs
    s.picks = apply.ResidentPicks(P, np.arange(S), S, DEV)
    return s


def _candidates(s, n):
    """n candidates: near the picks (origin times spread over the busy stretch), the last but one in a stretch without picks (no leg
    produces a window), the last at the region's corner (part of its cloud is masked). Source HALF_QUIET has no window on leg b."""
    rng = np.random.default_rng(5)
    t = np.quantile(s.P[:, 0], np.linspace(0.05, 0.8, n)) - 2.0
    srcs = np.c_[s.geom.x_grid[rng.integers(0, s.geom.x_grid.shape[0], n)], t, np.full(n, 0.5)]
    srcs[n - 2] = [20e3, 30e3, -5e3, QUIET_T, 0.5]
    srcs[n - 1, 0:3] = [500.0, 59.6e3, 1500.0]
    s.leg_b.quiet_t = float(srcs[HALF_QUIET, 3])
    return srcs


def _rand(how):
    return apply.PhiloxCloud(KEY) if how == "keyed" else np.random.RandomState(77).rand


def _refine(n, n_legs, how, **kw):
    s = _setup()
    legs = [s.leg, s.leg_b][:n_legs]
    return apply.refine_sources(legs, s.picks, _candidates(s, n), s.locs, s.tq, s.max_t, OFF_MIN, OFF_RNG, N_QUERY, IDENT, IDENT, *RANGES,
                                kernel_sig_t=s.sig, dt_embed=s.dt, rand=_rand(how), ftrns2_device=IDENT, **kw)


@functools.lru_cache(maxsize=None)
def _one_by_one(n, n_legs, how):
    """`source_batch=1`, the yardstick, in tuple form of a world of one (the rows) and in plain form."""
    rows, block = _refine(n, n_legs, how, source_parallel=(0, 1))
    assert block == (0, n) and rows[:, 3].all() and len(np.unique(rows[:, 0])) > 2
    assert rows[n - 2, 0] == 0 and rows[n - 2, 1] == 0 and rows[n - 2, 2] == 0          # the quiet source: all-zero read-out
    return rows, _refine(n, n_legs, how)


# ---------------------------------------------------------------------------------------------------------------- flush_windows_clouds
@functools.lru_cache(maxsize=None)
def _windows(n):
    """n windows of the busy stretch: (Slice, Mask) each, all different."""
    s = _setup()
    out = [s.leg.embed(s.picks, t0, s.max_t, s.sig, s.dt) for t0 in np.quantile(s.P[:, 0], np.linspace(0.05, 0.8, n)) - 2.0]
    assert all(em is not None for em in out) and (n == 1 or not torch.equal(out[0][0], out[-1][0]))
    return out


@pytest.fixture
def batch16():
    net = _setup().leg.net
    before = net.window_batch
    net.window_batch = 16
    yield net
    net.window_batch = before


def _qsets(n):
    """(n_sets, qset): n_sets > n, a permutation of the sets, and from two windows on two windows that share one set."""
    n_sets = n + 2
    qset = list(np.random.default_rng(n).permutation(n_sets)[:n])
    if n >= 2:
        qset[-1] = qset[0]
    return n_sets, [int(q) for q in qset]


@pytest.mark.parametrize("n", [1, 2, 3, 16])
@pytest.mark.parametrize("Q", [1, 16, 37])
def test_flush_windows_clouds_equals_the_per_window_calls(batch16, Q, n):
    """Q = 37: a 16-query tile straddles two windows, so the lanes of one tile read different sets; Q = 1: less than a tile."""
    s, net = _setup(), batch16
    n_sets, qset = _qsets(n)
    rng = np.random.default_rng(100 * Q + n)
    sets = _t(np.c_[rng.uniform(0, 60e3, (n_sets * Q, 2)), rng.uniform(-30e3, 0, n_sets * Q)].reshape(n_sets, Q, 3))
    x_grid, tq, locs = s.leg.x_grid_cart, _t(s.tq), _t(s.locs)
    with torch.no_grad():
        want = []
        for (Sl, M), q in zip(_windows(n), qset):
            y, x = net.forward_fixed_source(Sl, M, None, None, None, locs, x_grid, sets[q].clone(), tq)
            want.append((y.clone(), x.clone()))
        for Sl, M in _windows(n):
            net.push_window(Sl, M)
        y, x, done = net.flush_windows_clouds(x_grid, sets, tq, qset)
        done.synchronize()
    assert tuple(y.shape) == (n, 53, 9, 1) and tuple(x.shape) == (n, Q, 9, 1) and net.pending_windows == 0
    for w in range(n):
        assert torch.equal(y[w], want[w][0]) and torch.equal(x[w], want[w][1]), w
    assert float(x.abs().max()) > 0 and (n == 1 or not torch.equal(x[0], x[-1]))         # (one set, two windows)
    if n >= 3:                                                                          # (one window, two sets)
        with torch.no_grad():
            other = net.forward_fixed_source(*_windows(n)[0], None, None, None, locs, x_grid, sets[qset[1]].clone(), tq)[1]
        assert qset[0] != qset[1] and not torch.equal(want[0][1], other)


@pytest.mark.parametrize("Q", [16, 37])
def test_flush_windows_clouds_on_one_shared_set_equals_flush_windows(batch16, Q):
    s, net = _setup(), batch16
    rng = np.random.default_rng(Q)
    sets = _t(np.c_[rng.uniform(0, 60e3, (3 * Q, 2)), rng.uniform(-30e3, 0, 3 * Q)].reshape(3, Q, 3))
    tq = _t(s.tq)
    with torch.no_grad():
        for Sl, M in _windows(3):
            net.push_window(Sl, M)
        y0, x0, done = net.flush_windows(s.leg.x_grid_cart, sets[1].clone(), tq)
        done.synchronize()
        for Sl, M in _windows(3):
            net.push_window(Sl, M)
        y1, x1, done = net.flush_windows_clouds(s.leg.x_grid_cart, sets, tq, [1, 1, 1])
        done.synchronize()
    assert torch.equal(y0, y1) and torch.equal(x0, x1) and float(x0.abs().max()) > 0


def test_qset_is_checked_before_any_launch(batch16):
    s, net = _setup(), batch16
    sets, tq = _t(np.zeros((2, 5, 3))), _t(s.tq)
    with torch.no_grad():
        for Sl, M in _windows(2):
            net.push_window(Sl, M)
        for bad in ([0], [0, 1, 1], [0, 2], [-1, 0], [0.0, 1.0], [[0, 1]]):
            with pytest.raises(ValueError, match="qset"):
                net.flush_windows_clouds(s.leg.x_grid_cart, sets, tq, bad)
            assert net.pending_windows == 2                                             # nothing was flushed
        with pytest.raises(ValueError, match="n_sets"):
            net.flush_windows_clouds(s.leg.x_grid_cart, sets[0], tq, [0, 0])
        _, _, done = net.flush_windows_clouds(s.leg.x_grid_cart, sets, tq, np.array([1, 0]))
        done.synchronize()
    lib = net._hip.lib
    z = torch.zeros(64, device=DEV)
    p = lambda t: t.data_ptr()                                                          # noqa: E731
    tail = (5, 10, p(z), 9, p(z), p(z), p(z), net._hip._ws_ptr, None)
    for args, msg in (((net._hip.ctx, 0, 1, p(z), 2, None, p(z), p(z)) + tail, b"null query-set table"),
                      ((net._hip.ctx, 0, 1, p(z), 0, p(z), p(z), p(z)) + tail, b"n_sets >= 1"),
                      ((net._hip.ctx, 0, 1, p(z), 2 ** 30, p(z), p(z), p(z)) + tail, b"must fit an int")):
        assert lib.genie_tail_batched_q(*args) == -1 and msg in lib.genie_last_error()


# ---------------------------------------------------------------------------------------------------------------- the two batch kernels
@pytest.mark.parametrize("n_legs", [2, 3])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_select_batch_rows_are_the_single_form_rows(B, n_legs):
    """Q x n_t = 300 x 9 elements: two workgroups per source. Values on a grid of 1/8: ties at the maximum, in rows and between rows.
    Source 0 keeps no query, source 1 (from B = 3) has no leg at all, the others lose legs at random (never leg order)."""
    Q, n_t = 300, 9
    rng = np.random.default_rng(10 * B + n_legs)
    xs = [[torch.from_numpy((rng.integers(0, 6, (Q, n_t, 1)) / 8.0).astype(np.float32)).to(DEV) for _ in range(n_legs)] for _ in range(B)]
    has = rng.random((B, n_legs)) < 0.7
    has[0] = True
    if B >= 3:
        has[1] = False
        has[2] = [True] + [False] * (n_legs - 1)
    keep = torch.from_numpy(rng.random((B, Q)) < 0.6).to(DEV)
    keep[0] = False
    table = torch.tensor([[xs[b][l].data_ptr() if has[b, l] else 0 for l in range(n_legs)] for b in range(B)], dtype=torch.int64, device=DEV)
    got = postproc.refine_select_batch_device(table, (Q, n_t), keep, float(n_legs))
    none = postproc.refine_select_batch_device(table, (Q, n_t), None, float(n_legs))
    assert tuple(got.shape) == (B, 4) and got.dtype == torch.float64
    for b in range(B):
        used = [xs[b][l] for l in range(n_legs) if has[b, l]]
        assert torch.equal(got[b], postproc.refine_select_device(used, (Q, n_t), keep[b], float(n_legs), device=DEV)), b
        assert torch.equal(none[b], postproc.refine_select_device(used, (Q, n_t), None, float(n_legs), device=DEV)), b
    assert got[0].tolist() == [0.0, 0.0, -np.inf, 0.0]
    if B >= 3:
        assert got[1, 2] == 0.0 and got[1, 3] == 1.0 and got[1, 1] == 0.0               # all-zero acc: the first kept query, column 0
    mx = sum(x[:, :, 0] for x in xs[0]) / n_legs
    assert int((mx == mx.max()).sum()) > 1                                              # the maximum is tied


@pytest.mark.parametrize("Q", [1, 37, 300])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_cloud_batch_row_blocks_are_the_single_form_clouds(B, Q):
    """3 Q = 111 is no multiple of 4 (the row blocks are not 16-byte aligned: element stores), 900 is (vector stores)."""
    s0 = 5
    src = np.random.default_rng(B).uniform(-1e5, 1e5, (B, 3))
    Xc, xq = postproc.refine_cloud_batch_device(KEY, s0, B, Q, src, OFF_RNG, OFF_MIN, DEV)
    assert tuple(Xc.shape) == tuple(xq.shape) == (B, Q, 3) and Xc.dtype == torch.float64 and xq.dtype == torch.float32
    for b in range(B):
        w_c, w_q = postproc.refine_cloud_device(KEY, s0 + b, Q, src[b], OFF_RNG, OFF_MIN, DEV)
        assert torch.equal(Xc[b], w_c) and torch.equal(xq[b], w_q), b
    assert B == 1 or not torch.equal(Xc[0] - torch.from_numpy(src[0]).to(DEV), Xc[1] - torch.from_numpy(src[1]).to(DEV))


# ---------------------------------------------------------------------------------------------------------------- refine_sources
@pytest.mark.parametrize("how", ["keyed", "plain"])
@pytest.mark.parametrize("n_legs", [1, 2])
@pytest.mark.parametrize("n,B", [(5, 2), (5, 3), (5, 16), (17, 2), (17, 3), (17, 16)])
def test_refine_in_batches_equals_one_by_one(n, B, n_legs, how):
    """5 and 17 sources in batches of 2, 3 and 16: a short last batch, one batch, a full batch and one source."""
    s = _setup()
    rows, (want, order) = _one_by_one(n, n_legs, how)
    nets = [s.leg.net, s.leg_b.net]
    nets[0].window_batch, nets[1].window_batch = 4, 1
    got, got_order = _refine(n, n_legs, how, source_batch=B)
    assert np.array_equal(got, want) and np.array_equal(got_order, order)
    assert (nets[0].window_batch, nets[1].window_batch) == (4, 1) and nets[0].pending_windows == nets[1].pending_windows == 0
    got_rows, block = _refine(n, n_legs, how, source_batch=B, source_parallel=(0, 1))
    assert block == (0, n) and got_rows.tobytes() == rows.tobytes()
    nets[0].window_batch = 1


@pytest.mark.parametrize("B", [2, 3])
def test_refine_in_batches_on_two_ranks_and_with_an_offset(B):
    n = 17
    for how in ("keyed", "plain"):
        parts = []
        for r in range(2):
            want, block = _refine(n, 2, how, source_parallel=(r, 2))
            got, got_block = _refine(n, 2, how, source_parallel=(r, 2), source_batch=B)
            assert got_block == block == apply.window_blocks(n, 2)[r] and got.tobytes() == want.tobytes()
            parts.append(got)
        assert np.concatenate(parts).tobytes() == _one_by_one(n, 2, how)[0].tobytes()
    want = _refine(5, 2, "keyed", source_offset=7)
    got = _refine(5, 2, "keyed", source_offset=7, source_batch=B)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(want[0], _one_by_one(5, 2, "keyed")[1][0])                 # the offset draws other clouds


def test_a_day_after_a_batched_refine_is_unchanged():
    s = _setup()
    net = s.leg.net
    tsteps, _, _, _, dt_win = apply.window_schedule(s.P[:, 0], s.max_t, t_win=6.0, step_size="half")
    ts = np.arange(tsteps.min() - 3.0, tsteps.max() + 3.0 + dt_win, dt_win)
    day = lambda: apply.apply_windows_device(net, s.geom, s.P, s.trv, tsteps_abs=ts, times=tsteps[:40], max_t=s.max_t, tail_batch=16,   # noqa: E731
                                             stack_on_device=True)[0].clone()
    before = day()
    _refine(5, 1, "keyed", source_batch=3)
    after = day()
    assert torch.equal(before, after) and float(before.abs().max()) > 0
    net.window_batch = 1


def test_a_failing_batch_leaves_the_window_batch_as_it_was():
    s = _setup()
    s.leg.net.window_batch = 4

    def broken(x):
        raise KeyError("transform")

    with pytest.raises(KeyError):
        apply.refine_sources([s.leg], s.picks, _candidates(s, 5), s.locs, s.tq, s.max_t, OFF_MIN, OFF_RNG, N_QUERY, IDENT, IDENT, *RANGES,
                             kernel_sig_t=s.sig, dt_embed=s.dt, rand=_rand("keyed"), ftrns2_device=broken, source_batch=3)
    assert s.leg.net.window_batch == 4 and s.leg.net.pending_windows == 0
    s.leg.net.window_batch = 1


# ---------------------------------------------------------------------------------------------------------------- the pass-throughs
def test_detect_refine_associate_does_not_depend_on_refine_batch():
    from tests.test_source_parallel_gpu import _chain, _same_dict
    s = _setup()
    want = _chain(s)
    assert len(want["srcs"]) >= 3 and sum(o.size > 0 for o in want["Out_p_save"]) >= 2
    _same_dict(_chain(s, refine_batch=3), want)


def test_online_catalogue_does_not_depend_on_refine_batch():
    from tests import test_online_catalogue_gpu as cat_t
    P = cat_t._setup()[2]
    runs = []
    for batch in (1, 3):
        day, det, cat = cat_t._catalogue("device", refine_batch=batch)
        parts = [cat.push(P, float(P[0, 0])), cat.finish()]
        state = cat.state_dict()["catalogue"]
        assert "refine_batch" not in state and "refine_batch" not in state["fingerprint"]
        runs.append(cat_t._concat(parts))
    one, three = runs
    assert len(one["srcs_refined"]) >= 3
    for key in ("srcs", "srcs_refined"):
        assert np.array_equal(one[key], three[key]), key
    assert torch.equal(one["trv_out_srcs"], three["trv_out_srcs"])
    for key in ("Out_p_save", "Out_s_save"):
        assert len(one[key]) == len(three[key]) and all(torch.equal(a, b) for a, b in zip(one[key], three[key])), key
    for key in ("Save_picks", "lp_meta"):
        assert len(one[key]) == len(three[key]) and all(np.array_equal(a, b) for a, b in zip(one[key], three[key])), key
