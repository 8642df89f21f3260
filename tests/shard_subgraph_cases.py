"""Irregular product graphs (`use_subgraph`) for the source-node-shard tests (test_shard_subgraph_cpu.py / _gpu.py): the graph of a
golden fixture and two hand-made ones, each as a `Graph` with the product-level CSRs the way `module._set_adjacencies_subgraph` builds
them (pure numpy / CPU torch: importable without a GPU)."""
import collections
import functools

import numpy as np
import torch

from genie_amd import engine, graph

Graph = collections.namedtuple("Graph", "S G pairs seg sta_csr src_csr A_sta_sta A_src_src locs x_grid A_in_sta A_in_src A_src_in_prod")


def _graph(S, G, A_sta_sta, A_src_src, pairs, locs, x_grid):
    pairs = np.asarray(pairs, dtype=np.int64)
    A1, A2, A3 = graph.subgraph_product_edges(A_sta_sta, A_src_src, pairs)
    n = pairs.shape[1]
    seg = np.concatenate(([0], np.cumsum(np.bincount(pairs[1], minlength=G)))).astype(np.int64)
    csr = lambda A: tuple(t.numpy() for t in engine.csr_from_edges(A, n))
    return Graph(S, G, pairs, seg, csr(A1), csr(A2), np.asarray(A_sta_sta), np.asarray(A_src_src), np.asarray(locs, dtype=np.float32),
                 np.asarray(x_grid, dtype=np.float32), A1, A2, A3)


@functools.lru_cache(maxsize=None)
def fixture_graph(name):
    from tests.util import Case
    c = Case(name)
    return _graph(c.S, c.G, c.A_sta_sta.numpy(), c.A_src_src.numpy(), c.z["pairs"], c.locs.numpy(), c.x_grid.numpy())


def _ring_edges(n, k):
    """In-edges of node i from i + 1 .. i + k (mod n): [2, n * k], row 0 = neighbour, row 1 = centre."""
    i = np.repeat(np.arange(n), k)
    j = (i + np.tile(np.arange(1, k + 1), n)) % n
    return np.stack((j, i))


@functools.lru_cache(maxsize=None)
def handmade_graph():
    """10 source nodes, 6 stations. Station 5 has no product node; source node 3 has a single row; the source nodes 0 .. 4 have
    neighbours among themselves only (with the identity order the first rank of two lists no row of another rank), 5 .. 9 also reach
    back into 0 .. 4."""
    S, G = 6, 10
    A_sta = _ring_edges(S, 2)
    src_edges = []
    for i in range(G):
        nb = [(i + 1) % 5, (i + 2) % 5] if i < 5 else [5 + (i + 1) % 5, i - 5, (i - 3) % 5]
        src_edges += [(j, i) for j in nb if j != i]
    A_src = np.asarray(src_edges, dtype=np.int64).T
    stations = {0: [0, 1, 2, 3], 1: [0, 2, 4], 2: [1, 2, 3, 4], 3: [2], 4: [0, 1, 2, 3, 4], 5: [0, 1, 2], 6: [2, 3, 4], 7: [0, 4],
                8: [0, 1, 2, 3, 4], 9: [1, 2, 3]}
    pairs = np.asarray([(s, g) for g in range(G) for s in stations[g]], dtype=np.int64).T
    rng = np.random.default_rng(5)
    return _graph(S, G, A_sta, A_src, pairs, rng.uniform(-1e5, 1e5, (S, 3)), rng.uniform(-1e5, 1e5, (G, 3)))


@functools.lru_cache(maxsize=None)
def straddle_graph():
    """Row counts per source node around the 16-row tile of the stage kernels: 1, 15, 16, 17 and 33 rows, in an order that puts a
    node's rows at every offset inside a tile. 34 stations (8 ring neighbours), 12 source nodes (4 ring neighbours)."""
    S, G = 34, 12
    counts = [1, 15, 16, 17, 33, 16, 1, 33, 17, 15, 16, 1]
    pairs = np.asarray([(s, g) for g in range(G) for s in sorted((3 * g + np.arange(counts[g])) % S)], dtype=np.int64).T
    rng = np.random.default_rng(11)
    return _graph(S, G, _ring_edges(S, 8), _ring_edges(G, 4), pairs, rng.uniform(-1e5, 1e5, (S, 3)), rng.uniform(-1e5, 1e5, (G, 3)))


@functools.lru_cache(maxsize=None)
def geometry_graph(S=24, G=120, seed=77):
    """A synthetic network (`synthetic.Geometry`: picks and travel times for the apply loop) whose source nodes keep their 3 .. 7
    nearest stations. Returns (geom, Graph)."""
    from genie_amd import synthetic
    geom = synthetic.Geometry(S, G, L=150e3, n_query=20, seed=seed)
    d = np.linalg.norm(geom.x_grid[:, None, :2] - geom.locs[None, :, :2], axis=2)
    rank = np.argsort(np.argsort(d, axis=1), axis=1)
    src_i, sta_i = np.nonzero(rank < (3 + np.arange(G) % 5)[:, None])
    return geom, _graph(S, G, geom.A_sta_sta, geom.A_src_src, np.stack((sta_i, src_i)), geom.locs, geom.x_grid)


def plan_of(g, world, rank, order=None):
    from genie_amd import dist as gdist
    return gdist.SubgraphShardPlan(g.seg, g.src_csr, g.sta_csr, g.G, world, rank, order)


def random_inputs(g, seed):
    """Plain finite random Slice / Mask / edge_attr rows with O(1) values, as the `subgraph_*` fixtures use."""
    gen = torch.Generator().manual_seed(seed)
    n = g.pairs.shape[1]
    Slice = torch.rand((n, 4), generator=gen)
    Mask = (torch.rand((n, 4), generator=gen) > 0.4).float()
    ea = torch.randn((n, 3), generator=gen) * 0.5
    return Slice * Mask, Mask, ea
