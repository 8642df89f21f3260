"""GPU: packed station tail tiles of k_stage1_h2 (genie_amd/csrc/tile_items.hpp). With n_sta mod 16 in 1 .. 8 the half-empty last
station tiles of two adjacent source nodes share one 16-lane row; `genie_set_tail_packing(ctx, 0)` keeps the padded item table. Both
forms must give the same bits everywhere: c / wu / wv after stage 1, x_latent and the Bipartite station sums after stage 2 (which
reads the message mask of the split pass), the spatial aggregation and both read-outs. Sparse windows (two picks per station, as
bench.py's `sparse_window`), so that Mask rows gate and all-zero rows sit inside mixed tiles."""
import numpy as np
import pytest
import torch

from genie_amd import engine, graph, synthetic
from tests.util import Case, max_abs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel_tol(ref, scale=1e-5):       # the tolerance of tests/test_hip_parity.py
    return scale * max(1.0, float(ref.abs().max()))


class Shape:
    """Geometry, kNN tables (8 station / 15 source neighbours: the f16x2 kernels' graphs), one sparse window. G < 16 has no 15 distinct
    neighbours: the source table then lists the other nodes cyclically, repeats and the node itself included (byte equality only)."""

    def __init__(self, S, G):
        self.S, self.G = S, G
        self.geom = geom = synthetic.Geometry(S, max(G, 16), L=150e3, n_query=24, seed=S + G)
        if G >= 16:
            self.A_src = torch.from_numpy(geom.A_src_src)
            self.src_csr = engine.csr_from_edges(self.A_src, G)
            self.x_grid = geom.x_grid
        else:
            tab = (np.arange(G)[:, None] + 1 + np.arange(15)[None, :]) % G
            self.A_src = None
            self.src_csr = engine.csr_from_table(torch.from_numpy(tab))
            self.x_grid = geom.x_grid[:G]
        self.A_sta = torch.from_numpy(geom.A_sta_sta)
        self.sta_csr = engine.csr_from_edges(self.A_sta, S)
        rng = np.random.default_rng(S * 131 + G)
        if G >= 16:
            win = synthetic.make_window(geom, 2 * S, seed=9, window=7)
            self.Slice, self.Mask = torch.from_numpy(win["Slice"]), torch.from_numpy(win["Mask"])
            self.ea = torch.from_numpy(geom.edge_attr())
        else:       # the same kind of rows on S x G product nodes: a third of the Mask rows all zero
            live = (rng.random((S * G, 1)) < 0.67)
            self.Mask = torch.from_numpy(((rng.random((S * G, 4)) < 0.5) & live).astype(np.float32))
            self.Slice = torch.from_numpy((rng.random((S * G, 4)) * self.Mask.numpy()).astype(np.float32))
            self.ea = torch.from_numpy(rng.normal(0, 1, (S * G, 3)).astype(np.float32))
        self.weights = Case("cfg1_20x500").weights

    def engine(self, pack):
        hp = engine.HipPath(self.S, self.G, self.sta_csr, self.src_csr, grid_order=engine.sfc_order(self.x_grid), device=DEV,
                            sta_order=engine.sfc_order(self.geom.locs))
        hp.set_tail_packing(pack)
        hp.set_weights({k: v.to(DEV) for k, v in self.weights.items()})
        return hp

    def dev(self):
        return self.Slice.to(DEV), self.Mask.to(DEV), self.ea.to(DEV), torch.from_numpy(self.x_grid).float().to(DEV)


def run_all(sh, pack):
    hp = sh.engine(pack)
    Slice, Mask, ea, pos = sh.dev()
    hp.da_stage1(Slice, Mask)
    got = {"c": hp.export(0).clone(), "wu": hp.export(1).clone(), "wv": hp.export(2).clone()}
    x_latent, bip = hp.da_stage2_bipartite(Mask, ea, want_x_latent=True)
    got["x_latent"], got["bip"] = x_latent.clone(), bip.clone()
    out, xl, bip2 = hp.path_fwd(Slice, Mask, ea, pos, True, True)
    got["sa3"], got["x_latent_path"], got["bip_path"] = out, xl, bip2
    tq = (torch.arange(5, dtype=torch.float32) * 1.7 - 3.0).to(DEV)
    got["y"] = hp.readout_grid(out, tq)
    if sh.G >= 10:
        from genie_amd.module import knn_query_edges
        xq = torch.from_numpy(sh.geom.x_query).float().to(DEV)
        table = knn_query_edges(pos, xq, 10)[0].view(xq.shape[0], -1).to(torch.int32).contiguous()
        got["x"] = hp.readout_query(out, pos, xq, table, tq)
    assert hp.stage_precision()["f16x2_active"]            # k_stage1_h2 / k_stage2_h2u ran
    torch.cuda.synchronize()
    return got


_shapes = {}


def shape(S, G):
    if (S, G) not in _shapes:
        _shapes[(S, G)] = Shape(S, G)
    return _shapes[(S, G)]


# r = 8 (the full half) with odd chunks that leave unpartnered nodes; r = 3; G = 2: the eight chunks of a range hold one node or none,
# so nothing pairs (every tail tile stays padded, in the packing kernel); G = 16: one pair per chunk, all tail tiles mixed; r = 0 and
# r = 13: nothing to pack, the same kernel and item table under either setting
@pytest.mark.parametrize("S,G", [(24, 33), (19, 40), (17, 2), (17, 16), (16, 20), (32, 20), (29, 20)])
def test_packed_tail_tiles_are_bitwise_equal_to_padded_ones(S, G):
    sh = shape(S, G)
    padded = run_all(sh, False)
    packed = run_all(sh, True)
    assert set(padded) == set(packed)
    for k in padded:
        assert torch.isfinite(padded[k]).all(), k
        assert torch.equal(padded[k], packed[k]), (k, max_abs(padded[k].cpu(), packed[k].cpu()))
    assert float(padded["bip"].abs().max()) > 0 and float(padded["wv"].abs().max()) > 0
    m = sh.Mask.max(1)[0]
    assert 0.0 < float((m == 0).float().mean()) < 1.0       # the gate selects: all-zero Mask rows and live ones


def test_packed_tail_tiles_against_the_oracle():
    """S = 19 (r = 3), G = 40: x_latent, the Bipartite input and the spatial aggregation against the oracle, to the tolerance of
    tests/test_hip_parity.py -- a fault shared by the packed and the padded item tables cannot hide behind their equality."""
    from oracle import genie_oracle as O
    sh = shape(19, 40)
    got = run_all(sh, True)
    w = sh.weights
    A_in_sta, A_in_src, A_src_in_prod, _ = graph.cartesian_product_edges(sh.A_sta, sh.A_src, sh.S, sh.G)
    da = O.data_aggregation(w, sh.Slice, sh.Mask, A_in_sta, A_in_src, full=True)
    o_bip = O.bipartite_read_in(w, da["x_latent"], sh.ea, A_src_in_prod, sh.Mask)
    o = o_bip
    pos = torch.from_numpy(sh.x_grid).float()
    for l in (1, 2, 3):
        o = O.spatial_aggregation(w, o, sh.A_src, pos, "SpatialAggregation%d" % l)
    assert max_abs(got["x_latent"].cpu(), da["x_latent"]) <= rel_tol(da["x_latent"])
    assert max_abs(got["bip"].cpu(), o_bip) <= rel_tol(o_bip)
    assert max_abs(got["sa3"].cpu(), o) <= rel_tol(o)


@pytest.mark.parametrize("S,G,cut", [(19, 40, 5), (24, 33, 16), (24, 33, 17)])
def test_range_launches_cut_next_to_a_pair(S, G, cut):
    """The sharded path's range launches (genie_da_stage1_range / genie_da_stage2_partials_range over [0, cut) and [cut, G)): pairs
    are formed inside the chunks of a launched range, so an odd cut, which falls inside a pair of the whole-grid table, splits none.
    Stage-1 rows, x_latent and the Bipartite read-out of the two ranges equal the whole-grid call bit for bit."""
    sh = shape(S, G)
    whole = run_all(sh, True)
    hp = sh.engine(True)
    Slice, Mask, ea, _ = sh.dev()
    for k, (b, e) in enumerate(((0, cut), (cut, G))):
        hp.da_stage1_range(Slice, Mask, b, e, k == 0)
    got = {"c": hp.export(0).clone(), "wu": hp.export(1).clone(), "wv": hp.export(2).clone()}
    xl = torch.zeros((S * G, 30), dtype=torch.float32, device=DEV)
    for b, e in ((0, cut), (cut, G)):
        hp.da_stage2_partials_range(Mask, ea, b, e, xl)
    got["x_latent"], got["bip"] = xl, hp.bipartite_readout()
    torch.cuda.synchronize()
    for k in got:
        assert torch.equal(got[k], whole[k]), (k, max_abs(got[k].cpu(), whole[k].cpu()))
