"""GPU: the host side of the G-sized tail (Bipartite read-out, SpatialAggregation x3, the two read-out heads). Every C-ABI entry
point that launches the tail kernels must give the same bits whichever form it is asked in: chained or layer by layer, one window
or a batch, any launch grid, plain or latent, inference or training forward. Shapes: 40 source nodes (one workgroup, last 16-node
tile partial) and 257 (several workgroups, five virtual blocks of the grid-wide mean, odd tail); 17 / 16384 / 16385 queries (a
partial query tile and both sides of the query read-out's prefetch switch); 1 and 9 query times. All comparisons are bitwise
except the backward's against the oracle."""
import functools

import numpy as np
import pytest
import torch

from genie_amd import _lib, engine
from tests.util import Case, max_abs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ["tiny_6x40", "odd_33x257"]
P = engine._ptr


def make_engine(c, weights=None):
    sta_nbr, src_nbr = c.tables()
    hp = engine.HipPath(c.S, c.G, engine.csr_from_table(sta_nbr), engine.csr_from_table(src_nbr),
                        grid_order=engine.morton_order(c.x_grid.numpy()), device=DEV)
    hp.set_weights({k: v.to(DEV) for k, v in (weights or c.weights).items()})
    return hp


def queries(c, n_query, seed=11):
    """`n_query` points in the bounding box of the fixture's source grid."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = c.x_grid.min(0)[0].float(), c.x_grid.max(0)[0].float()
    return lo + (hi - lo) * torch.rand((n_query, 3), generator=g)


@functools.lru_cache(maxsize=None)
def setup(name):
    """Device inputs of a fixture: three windows (the fixture's own and two with its rows rolled), positions, queries, kNN table."""
    c = Case(name)
    wins = [(c.Slice.roll(7 * k, 0).contiguous().to(DEV), c.Mask.roll(7 * k, 0).contiguous().to(DEV)) for k in range(3)]
    pos, xq, tq = c.x_grid.float().to(DEV), c.x_query.float().to(DEV), c.t_query.float().reshape(-1).to(DEV)
    return c, wins, c.edge_attr.to(DEV), pos, xq, engine.knn_device(pos, xq, 10), tq


def per_window(hp, win, ea, pos, xq, knn, tq):
    """(x_spatial, y, x) of one window by the per-window calls."""
    xs = hp.path_fwd(win[0], win[1], ea, pos)[0]
    return xs, hp.readout_grid(xs, tq), hp.readout_query(xs, pos, xq, knn, tq)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The per-window results of the fixture's three windows with the default tail precision and launch grids: computed once."""
    c, wins, ea, pos, xq, knn, tq = setup(name)
    hp = make_engine(c)
    out = [per_window(hp, w, ea, pos, xq, knn, tq) for w in wins]
    torch.cuda.synchronize()
    return out


def tail_batched(hp, nwin, pos, xq, knn, tq, with_query=True):
    """genie_tail_batched over the `nwin` windows pushed last, on the current stream: (x_spatial [n, G, 30], y, x or None)."""
    bt = hp._bt
    assert bt["n"] == nwin
    nq = xq.shape[0]
    xs = torch.empty((nwin, hp.n_grid, 30), dtype=torch.float32, device=DEV)
    y = torch.empty((nwin, hp.n_grid, tq.numel(), 1), dtype=torch.float32, device=DEV)
    x = torch.empty((nwin, nq, tq.numel(), 1), dtype=torch.float32, device=DEV) if with_query else None
    _lib.check(hp.lib.genie_tail_batched(hp.ctx, bt["group"] * hp.window_batch, nwin, P(pos), P(xq) if with_query else None,
                                         P(knn) if with_query else None, nq if with_query else 0, 10, P(tq), tq.numel(), P(xs), P(y),
                                         P(x), hp._ws_ptr, engine._stream()), "genie_tail_batched")
    bt["n"] = 0
    return xs, y, x


@pytest.mark.parametrize("wide", [1, 0])
@pytest.mark.parametrize("name", CASES)
def test_chained_layers_equal_the_layers_one_by_one(name, wide):
    """genie_spatial_agg3_fwd = three genie_spatial_agg_fwd calls; genie_path_fwd = stage 1 + stage 2 / Bipartite read-out + the chain;
    fp64 and fp32 tail chains."""
    c, wins, ea, pos, xq, knn, tq = setup(name)
    hp = make_engine(c)
    hp.set_tail_precision(wide)
    Slice, Mask = wins[0]
    xs, _, bip = hp.path_fwd(Slice, Mask, ea, pos, want_bip=True)
    hp.da_stage1(Slice, Mask)
    _, bip2 = hp.da_stage2_bipartite(Mask, ea)
    chain = hp.spatial_agg3(bip2, pos)
    single = hp.spatial_agg(3, hp.spatial_agg(2, hp.spatial_agg(1, bip2, pos), pos), pos)
    assert torch.equal(bip, bip2)
    assert torch.equal(chain, single)
    assert torch.equal(xs, chain)
    assert bool(torch.isfinite(xs).all()) and float(xs.abs().max()) > 0
    if wide:
        assert torch.equal(xs, reference(name)[0][0])


@pytest.mark.parametrize("with_query", [True, False])
@pytest.mark.parametrize("nwin", [1, 2, 3])
@pytest.mark.parametrize("name", CASES)
def test_batched_tail_equals_the_per_window_calls(name, nwin, with_query):
    c, wins, ea, pos, xq, knn, tq = setup(name)
    ref = reference(name)
    hp = make_engine(c)
    hp.set_window_batch(nwin)
    for k in range(nwin):
        hp.window_push(wins[k][0], wins[k][1], ea)
    xs, y, x = tail_batched(hp, nwin, pos, xq, knn, tq, with_query)
    for k in range(nwin):
        assert torch.equal(xs[k], ref[k][0]), k
        assert torch.equal(y[k], ref[k][1]), k
        if with_query:
            assert torch.equal(x[k], ref[k][2]), k


@pytest.mark.parametrize("nwin", [1, 2, 3])
@pytest.mark.parametrize("name", CASES)
def test_windows_flush_equals_the_per_window_calls(name, nwin):
    """Two rounds of window_push / windows_flush (rotating slot groups, alternating side streams)."""
    c, wins, ea, pos, xq, knn, tq = setup(name)
    ref = reference(name)
    hp = make_engine(c)
    hp.set_window_batch(nwin)
    for rnd in range(2):
        for k in range(nwin):
            assert hp.window_push(wins[k][0], wins[k][1], ea) == k + 1
        y, x, done = hp.windows_flush(pos, xq, knn, tq)
        done.synchronize()
        for k in range(nwin):
            assert torch.equal(y[k], ref[k][1]) and torch.equal(x[k], ref[k][2]), (rnd, k)


@pytest.mark.parametrize("name", CASES)
def test_results_do_not_depend_on_the_launch_grid(name):
    c, wins, ea, pos, xq, knn, tq = setup(name)
    ref = reference(name)[0]
    hp = make_engine(c)
    for ro, sa in ((1, 1), (1024, 1024)):
        _lib.check(hp.lib.genie_set_tail_grid(hp.ctx, ro, sa), "genie_set_tail_grid")
        got = per_window(hp, wins[0], ea, pos, xq, knn, tq)
        for g, r in zip(got, ref):
            assert torch.equal(g, r), (ro, sa)


@pytest.mark.parametrize("name", CASES)
def test_latent_entry_points_equal_the_plain_ones(name):
    c, wins, ea, pos, xq, knn, tq = setup(name)
    xs, y, x = reference(name)[0]
    hp = make_engine(c)
    y2, ylat = hp.readout_grid_latent(xs, tq)
    assert torch.equal(y2, y)
    assert bool(torch.isfinite(ylat).all()) and float(ylat.abs().max()) > 0
    nq = xq.shape[0]
    x2 = torch.empty((nq, tq.numel(), 1), dtype=torch.float32, device=DEV)
    lat = torch.empty((nq, 30), dtype=torch.float32, device=DEV)
    _lib.check(hp.lib.genie_readout_query_latent(hp.ctx, P(xs), P(pos), P(xq), P(knn), nq, 10, P(tq), tq.numel(), P(x2), P(lat), hp._ws_ptr,
                                                 engine._stream()), "genie_readout_query_latent")
    assert torch.equal(x2, x)
    assert torch.equal(hp.spatial_attention(xs, pos, xq, knn, tq), lat)
    assert bool(torch.isfinite(lat).all()) and float(lat.abs().max()) > 0


@pytest.mark.parametrize("n_t", [1, 9])
@pytest.mark.parametrize("n_query", [17, 16384, 16385])
def test_query_counts_around_the_prefetch_switch(n_query, n_t):
    """The per-window query read-out takes its prefetching form up to 16384 queries, the batch never does: same bits either way, for
    the plain and the latent entry point, and the grid read-out's too at 1 and 9 query times."""
    c, wins, ea, pos, _, _, tq9 = setup("tiny_6x40")
    xq = queries(c, n_query).to(DEV)
    knn = engine.knn_device(pos, xq, 10)
    tq = tq9[4:5].contiguous() if n_t == 1 else tq9
    hp = make_engine(c)
    ref = [per_window(hp, w, ea, pos, xq, knn, tq) for w in wins[:2]]
    x2 = torch.empty_like(ref[0][2])
    lat = torch.empty((n_query, 30), dtype=torch.float32, device=DEV)
    _lib.check(hp.lib.genie_readout_query_latent(hp.ctx, P(ref[0][0]), P(pos), P(xq), P(knn), n_query, 10, P(tq), n_t, P(x2), P(lat),
                                                 hp._ws_ptr, engine._stream()), "genie_readout_query_latent")
    assert torch.equal(x2, ref[0][2])
    assert torch.equal(hp.readout_grid_latent(ref[0][0], tq)[0], ref[0][1])
    hp.set_window_batch(2)
    for k in range(2):
        hp.window_push(wins[k][0], wins[k][1], ea)
    xs, y, x = tail_batched(hp, 2, pos, xq, knn, tq)
    for k in range(2):
        assert torch.equal(xs[k], ref[k][0]) and torch.equal(y[k], ref[k][1]) and torch.equal(x[k], ref[k][2]), k
    assert tuple(x.shape) == (2, n_query, n_t, 1) and bool(torch.isfinite(x).all())
    if n_t == 9 and n_query == 17:
        assert torch.equal(ref[0][0], reference("tiny_6x40")[0][0]) and torch.equal(ref[0][1], reference("tiny_6x40")[0][1])


def train_forward(hp, s):
    c, wins, ea, pos, xq, knn, tq = s
    y, x, xs, ylat, _, save, tsave = hp.path_train_fwd(wins[0][0], wins[0][1], ea, pos, xq, knn, tq, want_y_latent=True)
    return y, x, xs, ylat, tsave


@pytest.mark.parametrize("name", CASES)
def test_training_forward_equals_the_fp32_inference_tail(name):
    """genie_tail_train_fwd runs the inference tail's kernels in their fp32 form on the station sums genie_da_train_fwd left in the
    workspace: with set_tail_precision(0) the inference calls on those same sums return the same bits. (The stages in front differ:
    the whole inference path is compared at a tolerance in test_train_gpu.py.)"""
    s = setup(name)
    c, wins, ea, pos, xq, knn, tq = s
    hp = make_engine(c)
    hp.set_tail_precision(0)
    y, x, xs, ylat, tsave = train_forward(hp, s)
    xs_i = hp.spatial_agg3(hp.bipartite_readout(), pos)
    y_i, ylat_i = hp.readout_grid_latent(xs_i, tq)
    x_i = hp.readout_query(xs_i, pos, xq, knn, tq)
    full = per_window(hp, wins[0], ea, pos, xq, knn, tq)
    print("training forward vs whole inference path: x_spatial %.2e y %.2e x %.2e" % (max_abs(xs, full[0]), max_abs(y, full[1]), max_abs(x, full[2])))
    assert torch.equal(xs, xs_i)
    assert torch.equal(y, y_i) and torch.equal(ylat, ylat_i)
    assert torch.equal(x, x_i)


def test_training_forward_first_on_a_second_context():
    """The dynamic-LDS limit of the read-out kernels is raised per context: a second context on the device whose FIRST tail call is
    the training forward (no inference read-out before it) gives the first context's results."""
    s = setup("odd_33x257")
    a = make_engine(s[0])
    per_window(a, s[1][0], *s[2:])
    want = train_forward(a, s)
    b = make_engine(s[0])
    got = train_forward(b, s)
    torch.cuda.synchronize()
    for g, w in zip(got[:4], want[:4]):          # y, x, x_spatial, y_latent (tsave has padding that nothing writes)
        assert torch.equal(g, w)
        assert bool(torch.isfinite(g).all())


@pytest.mark.parametrize("name", CASES)
def test_tail_backward_is_deterministic_and_matches_the_oracle(name):
    """genie_tail_train_bwd twice on the same inputs: equal gradient blobs and d r. Against the oracle's autograd of the tail (r -> y, x,
    float64, random N(0, 1) cotangents, the scaled `o1` weights) every gradient is within 1e-4 of its own scale, the bound of
    test_train_gpu.py for gradients behind an fp32 forward."""
    from oracle import genie_oracle as O
    s = setup(name)
    c, wins, ea, pos, xq, knn, tq = s
    w0 = Case("o1_20x500").weights
    hp = make_engine(c, w0)
    y, x, xs, ylat, tsave = train_forward(hp, s)
    G, Q, T = c.G, xq.shape[0], tq.numel()
    rng = np.random.default_rng(5)
    cy, cx = torch.from_numpy(rng.normal(0, 1, (G, T)).astype(np.float32)), torch.from_numpy(rng.normal(0, 1, (Q, T)).astype(np.float32))
    d_r, blob = hp.tail_train_bwd(pos, xq, knn, tq, tsave, cy.to(DEV), cx.to(DEV))
    d_r2, blob2 = hp.tail_train_bwd(pos, xq, knn, tq, tsave, cy.to(DEV), cx.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(blob, blob2) and torch.equal(d_r, d_r2)
    d64 = lambda t: t.detach().double().cpu()
    r = d64(tsave[:32 * G].view(G, 32)[:, :30]).clone().requires_grad_(True)
    w = {k: v.double().clone().requires_grad_(v.is_floating_point()) for k, v in w0.items()}
    sa = O.act(O.linear(r, w, "Bipartite_ReadIn.fc2"), w, "Bipartite_ReadIn.activate2")
    xg = d64(pos)
    for k in (1, 2, 3):
        sa = O.spatial_aggregation(w, sa, c.A_src_src, xg, "SpatialAggregation%d" % k)
    yo = O.temporal_attention(w, O.spatial_direct(w, sa), d64(tq).reshape(-1, 1))
    edges = torch.stack([knn.cpu().long().reshape(-1), torch.arange(Q).repeat_interleave(10)])
    xo = O.temporal_attention(w, O.spatial_attention(w, sa, d64(xq), xg, edge_index=edges), d64(tq).reshape(-1, 1))
    print("training forward vs float64 oracle tail, %s: y %.2e x %.2e" % (name, max_abs(y.cpu(), yo.detach()), max_abs(x.cpu(), xo.detach())))
    ((yo[:, :, 0] * cy.double()).sum() + (xo[:, :, 0] * cx.double()).sum()).backward()
    worst, checked = 0.0, 0
    grads = [("d r", d_r[:, :30].cpu(), r.grad)]
    for k, n, off in zip(hp.w_names, hp.w_numel, hp.w_off):
        if k in w and w[k].grad is not None:
            grads.append((k, blob[off:off + n].cpu().view_as(w[k]), w[k].grad))
    for k, got, want in grads:
        sc = float(want.abs().max())
        err = max_abs(got, want)
        worst = max(worst, err / max(sc, 1e-300))
        checked += 1
    print("tail gradients vs float64 oracle, %s: %d tensors, worst relative error %.2e" % (name, checked, worst))
    for k, got, want in grads:
        sc = float(want.abs().max())
        assert max_abs(got, want) <= 1e-4 * sc, (k, max_abs(got, want), sc)
    assert checked >= 50
