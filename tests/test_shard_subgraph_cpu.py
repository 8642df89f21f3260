"""CPU: the shard plan of an irregular product graph (`dist.SubgraphShardPlan`, pure numpy): ownership by source node, the ragged halo
of rows, row counts that mirror between ranks, the local numbering and CSRs -- on the product graph of the `subgraph_14x50` fixture and
on a hand-made graph (a station without a product node, a source node with one row, a rank that lists no foreign row), at worlds 1, 2, 3
and 5."""
import numpy as np
import pytest

from genie_amd import engine
from tests import shard_subgraph_cases as cases

WORLDS = [1, 2, 3, 5]


def _graph(name):
    if name == "handmade":
        return cases.handmade_graph(), None                    # identity order: what the graph's docstring promises holds
    g = cases.fixture_graph(name)
    return g, engine.sfc_order(g.x_grid)


def _plans(name, world):
    g, order = _graph(name)
    return g, [cases.plan_of(g, world, r, order) for r in range(world)]


def _edges(g):
    rp, col = g.src_csr
    return np.repeat(np.arange(rp.size - 1), np.diff(rp)), col.astype(np.int64)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", ["subgraph_14x50", "handmade"])
def test_owned_rows_partition_and_local_numbering(name, world):
    g, plans = _plans(name, world)
    n_prod = int(g.seg[-1])
    assert np.array_equal(np.sort(np.concatenate([p.own_rows for p in plans])), np.arange(n_prod))
    src_of = g.pairs[1]
    for p in plans:
        assert p.n_prod == n_prod and p.n_rows_own == p.own_rows.size and p.n_rows_ext == p.n_rows_own + p.n_rows_halo
        # ownership by source node, in the order's blocks; the processing order is a permutation of the owned nodes in four classes
        assert np.array_equal(np.sort(p.own_proc), np.sort(p.own_global)) and np.array_equal(p.own_proc, p.own_global[p.proc_order])
        assert (p.owner[src_of[p.own_rows]] == p.rank).all() and (p.owner[src_of[p.halo_rows]] != p.rank).all()
        # owned rows: node after node in processing order, every node's rows in the global row order
        want = np.concatenate([np.arange(g.seg[n], g.seg[n + 1]) for n in p.own_proc]) if p.n_own else np.zeros(0, np.int64)
        assert np.array_equal(p.own_rows, want)
        assert np.array_equal(np.diff(p.seg_rowptr), np.diff(g.seg)[p.own_proc]) and p.seg_rowptr[-1] == p.n_rows_own
        (s0, s1), (n0, n1) = p.r_send, p.r_need
        assert 0 == s0 <= n0 <= s1 <= n1 <= p.n_own


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", ["subgraph_14x50", "handmade"])
def test_halo_is_exactly_the_foreign_rows_listed(name, world):
    g, plans = _plans(name, world)
    centre, col = _edges(g)
    for p in plans:
        mine = np.isin(centre, p.own_rows)
        listed = np.unique(col[mine])
        foreign = listed[~np.isin(listed, p.own_rows)]
        assert np.array_equal(np.sort(p.halo_rows), foreign)                      # exactly: no row more, none twice
        assert np.unique(p.halo_rows).size == p.halo_rows.size
        # every neighbour column of an owned row resolves to a local row, station neighbours to owned rows
        assert p.src_col.size == int(mine.sum()) and (p.src_col >= 0).all() and (p.src_col < p.n_rows_ext).all()
        assert (p.sta_col >= 0).all() and (p.sta_col < p.n_rows_own).all()
        assert np.array_equal(p.ext_rows[p.src_col], np.concatenate([col[centre == r] for r in p.own_rows]))     # same edges, same order
        # grouped by owner, in the owner's row order
        own_of = p.owner[g.pairs[1][p.halo_rows]]
        assert (np.diff(own_of) >= 0).all()
        for q, other in enumerate(plans):
            rows = p.halo_rows[own_of == q]
            assert np.array_equal(rows, p.need[p.rank][q])
            assert (np.diff(other.row_to_local[rows]) > 0).all()
        # classes: NEED nodes are those with a halo neighbour, SEND nodes those with a row in another rank's halo
        need_nodes = {int(n) for n in np.unique(np.searchsorted(p.seg_rowptr, np.repeat(np.arange(p.n_rows_own), np.diff(p.src_rowptr))
                                                                  [p.src_col >= p.n_rows_own], side="right") - 1)}
        assert need_nodes == set(range(p.r_need[0], p.r_need[1]))
        sent = np.concatenate([q.need[q.rank][p.rank] for q in plans])
        send_nodes = {int(n) for n in np.unique(np.searchsorted(p.seg_rowptr, p.row_to_local[sent], side="right") - 1)}
        assert send_nodes == set(range(p.r_send[0], p.r_send[1]))


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", ["subgraph_14x50", "handmade"])
def test_send_lists_mirror_receive_lists(name, world):
    g, plans = _plans(name, world)
    for p in plans:
        assert sum(p.recv_counts) == p.n_rows_halo and p.send_counts[p.rank] == 0 == p.recv_counts[p.rank]
        for q in plans:
            assert p.send_counts[q.rank] == q.recv_counts[p.rank]
            # the rows p sends to q, as global rows, are q's halo block of p, row for row
            ro = np.concatenate(([0], np.cumsum(q.recv_counts)))
            assert np.array_equal(p.own_rows[p.send_rows[q.rank]], q.halo_rows[ro[p.rank]:ro[p.rank + 1]])


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", ["subgraph_14x50", "handmade"])
def test_gathered_halo_rows_give_the_global_neighbour_mean(name, world):
    """Numpy restatement of the device path: exchange the halo rows, then the per-row neighbour mean over the local CSR."""
    g, plans = _plans(name, world)
    centre, col = _edges(g)
    n_prod = int(g.seg[-1])
    x = np.random.default_rng(3).standard_normal((n_prod, 5)).astype(np.float32)

    def mean(rowptr, cols, rows):
        acc = np.zeros((rowptr.size - 1, rows.shape[1]), dtype=np.float32)
        np.add.at(acc, np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr)), rows[cols])          # in edge order
        return acc / np.maximum(np.diff(rowptr), 1).astype(np.float32)[:, None]
    want = mean(g.src_csr[0].astype(np.int64), col, x)
    for p in plans:
        local = np.full((p.n_rows_ext, 5), np.nan, dtype=np.float32)
        local[: p.n_rows_own] = x[p.own_rows]
        ro = np.concatenate(([0], np.cumsum(p.recv_counts)))
        for q in plans:              # what q packs for p lands behind p's owned rows, grouped by owner
            if q.rank != p.rank:
                local[p.n_rows_own + ro[q.rank]: p.n_rows_own + ro[q.rank + 1]] = x[q.own_rows][q.send_rows[p.rank]]
        got = mean(p.src_rowptr.astype(np.int64), p.src_col.astype(np.int64), local)
        assert np.array_equal(got, want[p.own_rows])


def test_handmade_graph_has_its_edge_cases():
    g, plans = _plans("handmade", 2)
    assert 5 not in g.pairs[0] and g.S == 6                                       # a station without a product node
    assert int(np.diff(g.seg)[3]) == 1                                            # a source node with a single row
    assert plans[0].n_rows_halo == 0 and plans[0].r_need == (plans[0].r_need[0],) * 2 and sum(plans[0].send_counts) > 0
    assert plans[1].n_rows_halo > 0 and sum(plans[1].send_counts) == 0
    g, plans = _plans("handmade", 1)
    assert plans[0].n_rows_halo == 0 and np.array_equal(plans[0].own_rows, np.arange(int(g.seg[-1])))
