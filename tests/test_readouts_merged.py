"""GPU: genie_readouts (k_ro_pre_m, then both read-out heads in ONE launch, k_readouts_m) gives the bits of genie_readout_grid +
genie_readout_query. Random weights, random x_spatial. Grid sizes 16 (a single tile), 40 (one workgroup, last tile partial) and 250
(four workgroups, last tile partial); 1 / 17 / 64 / 300 queries (one query, a partial last tile, and fewer, as many and more query
workgroups than the grid has: the merged launch puts the query workgroups in front); 1 and 10 query times. All comparisons are bitwise."""
import functools

import pytest
import torch

from genie_amd import _lib, engine, graph, module, synthetic
from tests.util import Case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = engine._ptr


@functools.lru_cache(maxsize=None)
def random_weights():
    g = torch.Generator().manual_seed(23)
    return {k: (0.3 * torch.randn(v.shape, generator=g)).to(DEV) for k, v in Case("tiny_6x40").weights.items()}


@functools.lru_cache(maxsize=None)
def setup(G):
    """An engine over `G` source nodes, their positions, and two different x_spatial."""
    geom = synthetic.Geometry(6, G, L=100e3, n_query=1, seed=G)
    hp = engine.HipPath(6, G, engine.csr_from_edges(torch.from_numpy(geom.A_sta_sta), 6),
                        engine.csr_from_edges(torch.from_numpy(geom.A_src_src), G), device=DEV)
    hp.set_weights(random_weights())
    g = torch.Generator().manual_seed(100 + G)
    xs = [torch.randn((G, 30), generator=g).to(DEV) for _ in range(2)]
    return hp, torch.from_numpy(geom.x_grid).float().to(DEV), xs


@functools.lru_cache(maxsize=None)
def queries(G, Q):
    hp, pos, _ = setup(G)
    g = torch.Generator().manual_seed(1000 * G + Q)
    lo, hi = pos.min(0)[0].cpu(), pos.max(0)[0].cpu()
    xq = (lo + (hi - lo) * torch.rand((Q, 3), generator=g)).to(DEV)
    return xq, engine.knn_device(pos, xq, 10)


def times(n_t):
    return torch.linspace(-3.0, 3.0, n_t, device=DEV) if n_t > 1 else torch.tensor([0.75], device=DEV)


def two_calls(hp, xs, pos, xq, knn, tq):
    return hp.readout_grid(xs, tq), hp.readout_query(xs, pos, xq, knn, tq)


def merged(hp, xs, pos, xq, knn, tq):
    """genie_readouts through the C ABI on the current stream."""
    y = torch.empty((hp.n_grid, tq.numel(), 1), dtype=torch.float32, device=DEV)
    x = torch.empty((xq.shape[0], tq.numel(), 1), dtype=torch.float32, device=DEV)
    _lib.check(hp.lib.genie_readouts(hp.ctx, P(xs), P(pos), P(xq), P(knn), xq.shape[0], 10, P(tq), tq.numel(), P(y), P(x), hp._ws_ptr,
                                     engine._stream()), "genie_readouts")
    return y, x


def check(got, want):
    for a, b in zip(got, want):
        assert bool(torch.isfinite(b).all()) and float(b.abs().max()) > 0
        assert torch.equal(a, b)


@pytest.mark.parametrize("n_t", [1, 10])
@pytest.mark.parametrize("Q", [1, 17, 64, 300])
@pytest.mark.parametrize("G", [16, 40, 250])
def test_one_launch_equals_the_two_calls(G, Q, n_t):
    hp, pos, xs = setup(G)
    xq, knn = queries(G, Q)
    tq = times(n_t)
    check(merged(hp, xs[0], pos, xq, knn, tq), two_calls(hp, xs[0], pos, xq, knn, tq))


def test_on_a_side_stream():
    hp, pos, xs = setup(250)
    xq, knn = queries(250, 300)
    tq = times(10)
    want = two_calls(hp, xs[0], pos, xq, knn, tq)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        got = merged(hp, xs[0], pos, xq, knn, tq)
    s.synchronize()
    check(got, want)


def test_two_windows_back_to_back_reuse_the_cv_buffer():
    """Two different windows through the same workspace slot, no synchronisation in between: the second call's k_ro_pre_m overwrites
    the table the first call's query head gathers from, in stream order."""
    hp, pos, xs = setup(250)
    xq, knn = queries(250, 300)
    tq = times(10)
    want = [two_calls(hp, x, pos, xq, knn, tq) for x in xs]
    torch.cuda.synchronize()
    got = [merged(hp, x, pos, xq, knn, tq) for x in xs]
    torch.cuda.synchronize()
    assert not torch.equal(want[0][1], want[1][1])
    for g, w in zip(got, want):
        check(g, w)


def test_forward_fixed_source_equals_path_and_the_two_read_outs():
    """The literal call on the smallest synthetic config: byte-equal to path_fwd + readout_grid + readout_query."""
    c = Case("cfg1_20x500")
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV)
    net.load_state_dict({k: v.clone() for k, v in c.weights.items()}, strict=True)
    net.eval()
    A_in_sta, A_in_src, A_src_in_prod, A_src_in_sta = c.product_edges()
    ea = graph.GraphEdges(x=c.edge_attr.to(DEV), edge_index=A_src_in_prod.to(DEV))
    locs, pos = c.locs.float().to(DEV), c.x_grid.float().to(DEV)
    net.set_adjacencies(A_in_sta.to(DEV), A_in_src.to(DEV), ea, ea, A_src_in_sta.to(DEV), c.A_src_src.to(DEV), None, None, None, None, locs, pos)
    Slice, Mask, xq, tq = c.Slice.to(DEV), c.Mask.to(DEV), c.x_query.float().to(DEV), c.t_query.float().to(DEV)
    with torch.no_grad():
        y, x = net.forward_fixed_source(Slice, Mask, None, None, None, locs, pos, xq, tq)
        hp = net._hip
        xs = hp.path_fwd(Slice, Mask, net._edge_attr, pos)[0]
        knn = engine.knn_device(pos, xq, 10)
        want = two_calls(hp, xs, pos, xq, knn, tq)
    torch.cuda.synchronize()
    check((y, x), want)
