"""GPU: k_stage2_h2u with union rows carried in LDS from block to block of a group (genie_amd/csrc/s2u_plan.hpp) through
`forward_fixed_source` on small synthetic geometries: two station tiles with the second partial (S = 20), three tiles on a grid
that is no multiple of 8 (S = 33, G = 500: short blocks, empty node slots, several blocks per XCD chunk, so rows ARE carried).
Outputs against the CPU oracle within the 1e-5 absolute of tests/test_hip_parity.py for (y, x); run-to-run, pipelined-to-literal and
sharded-to-unsharded equality bit for bit. S = 17, G = 16 is the smallest grid whose kNN graph has 15 neighbours per node, which is
what selects k_stage2_h2u: two nodes per XCD chunk. G = 9 reaches the kernel with a neighbour table of repeated rows (see its test)."""
import pytest
import torch

from genie_amd import engine, graph, module, synthetic
from tests.util import Case, max_abs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(20, 300), (33, 500), (17, 16)]
_cache = {}


def _case(S, G):
    """Geometry, window, model and the oracle's (y, x) of a shape: computed once, shared by the tests, left unchanged."""
    if (S, G) in _cache:
        return _cache[(S, G)]
    from oracle import genie_oracle as O
    geom = synthetic.Geometry(S, G, L=200e3, n_query=40, seed=300 + S)
    win = synthetic.make_window(geom, 12 * S, seed=301 + S)
    w = Case("cfg1_20x500").weights
    Slice, Mask = torch.from_numpy(win["Slice"]), torch.from_numpy(win["Mask"])
    ea = torch.from_numpy(geom.edge_attr())
    pos = torch.from_numpy(geom.x_grid).float()
    locs = torch.from_numpy(geom.locs).float()
    xq, tq = torch.from_numpy(geom.x_query).float(), torch.from_numpy(geom.t_query).float()
    A_sta, A_src = torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src)
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV)
    net.load_state_dict({k: v.clone() for k, v in w.items()})
    net.eval()
    net.set_adjacencies_base(A_sta, A_src, ea.to(DEV), locs.to(DEV), pos.to(DEV))
    A_in_sta, A_in_src, A_src_in_prod, _ = graph.cartesian_product_edges(A_sta, A_src, S, G)
    with torch.no_grad():
        yo, xo = O.forward_fixed_source(w, Slice, Mask, A_in_sta, A_in_src, ea, A_src_in_prod, A_src, pos, xq, tq)
    args = (Slice.to(DEV), Mask.to(DEV), None, None, None, locs.to(DEV), pos.to(DEV), xq.to(DEV), tq.to(DEV))
    _cache[(S, G)] = dict(geom=geom, w=w, net=net, args=args, oracle=(yo, xo), Slice=Slice, Mask=Mask, ea=ea, pos=pos)
    return _cache[(S, G)]


@pytest.mark.parametrize("S,G", SHAPES)
def test_outputs_match_the_oracle_and_repeat_bit_for_bit(S, G):
    c = _case(S, G)
    with torch.no_grad():
        y, x = c["net"].forward_fixed_source(*c["args"])
        y2, x2 = c["net"].forward_fixed_source(*c["args"])
    torch.cuda.synchronize()
    yo, xo = c["oracle"]
    ey, ex = max_abs(y.cpu(), yo), max_abs(x.cpu(), xo)
    print("S %d G %d: max|y - oracle| %.3g  max|x - oracle| %.3g (max|y| %.3g)" % (S, G, ey, ex, float(yo.abs().max())))
    assert y.shape == tuple(yo.shape) and x.shape == tuple(xo.shape)
    assert ey <= 1e-5 and ex <= 1e-5                  # fp32 max-abs tolerance of the outputs (tests/test_hip_parity.py)
    assert torch.equal(y, y2) and torch.equal(x, x2)
    assert c["net"]._hip.stage_precision()["f16x2_active"], "the f16x2 stage kernels (k_stage2_h2u) are what this test is about"


@pytest.mark.parametrize("S,G", SHAPES)
def test_pipelined_form_is_bit_equal_to_the_literal_one(S, G):
    c = _case(S, G)
    net = c["net"]
    with torch.no_grad():
        y, x = net.forward_fixed_source(*c["args"])
        outs = [net.forward_fixed_source_pipelined(*c["args"]) for _ in range(3)]       # (three windows: every slot copy of the rows)
    for yp, xp, done in outs:
        done.wait()
    torch.cuda.synchronize()
    for yp, xp, _ in outs:
        assert torch.equal(yp, y) and torch.equal(xp, x)


def test_sharded_sub_range_launches_are_bit_equal_to_the_unsharded_kernel():
    """Two virtual ranks on one GPU (halo rows by direct copies, as tests/test_hip_parity.py emulates a world), stage 2 in the three
    sub-range launches of the overlapped schedule (genie_amd/dist.py: before the halo positions, after them, the halo positions):
    every range has its own block table whose groups start at the range's own chunk boundaries."""
    from genie_amd import dist as gdist
    S, G, W = 33, 500, 2
    c = _case(S, G)
    geom, Slice, Mask, ea, pos = c["geom"], c["Slice"], c["Mask"], c["ea"], c["pos"]
    wd = {k: v.to(DEV) for k, v in c["w"].items()}
    sta_csr = engine.csr_from_edges(torch.from_numpy(geom.A_sta_sta), S)
    hp = engine.HipPath(S, G, sta_csr, engine.csr_from_edges(torch.from_numpy(geom.A_src_src), G),
                        grid_order=engine.sfc_order(geom.x_grid), device=DEV, sta_order=engine.sfc_order(geom.locs))
    hp.set_weights(wd)
    _, _, bip_ref = hp.path_fwd(Slice.to(DEV), Mask.to(DEV), ea.to(DEV), pos.to(DEV), False, True)
    ranks = [gdist.ShardedPath(S, G, sta_csr, geom.A_src_src, geom.x_grid, W, r, DEV, pos_sta=geom.locs) for r in range(W)]
    rows = []
    for sp in ranks:
        sp.set_weights(wd)
        ext = torch.from_numpy(sp.plan.ext_global)
        r = (ext.view(-1, 1) * S + torch.arange(S).view(1, -1)).reshape(-1)
        rows.append(r)
        sp._S, sp._M = sp.local.da_stage1(Slice[r].to(DEV), Mask[r].to(DEV))
    for sp in ranks:                                  # halo exchange by direct copies
        p, wv = sp.plan, sp.wv_view()
        off = p.n_own
        for q in range(W):
            need = p.need[p.rank][q]
            if need.size == 0:
                continue
            src = ranks[q]
            loc = torch.from_numpy(src.plan.global_to_local[need]).to(DEV)
            blocks = src.wv_view()[: src.plan.n_own * S].view(src.plan.n_own, S * 16).index_select(0, loc)
            wv[off * S:(off + need.size) * S] = blocks.view(-1, 16)
            off += need.size
        assert off == p.n_ext
    bip = torch.empty((G, 15), device=DEV)
    n_ranges = 0
    for sp, r in zip(ranks, rows):
        p, lp = sp.plan, sp.local
        (n0, n1), n = p.r_need, p.n_own
        ea_own = ea[r[: n * S]].to(DEV).contiguous()
        Mask_own = sp._M[: n * S]
        lp.set_static_edge_attr(ea_own)
        for b, e in ((0, n0), (n1, n), (n0, n1)):
            lp.da_stage2_partials_range(Mask_own, ea_own, b, e)
            n_ranges += e > b
        bip[torch.from_numpy(p.own_global).to(DEV)] = lp.bipartite_readout()
    torch.cuda.synchronize()
    assert n_ranges >= 3, "the plan must give real sub-ranges"
    assert torch.equal(bip, bip_ref)


def test_grid_of_nine_source_nodes():
    """G = 9. A 9-node grid has 8 neighbours per node, and a source graph of in-degree other than 15 takes the generic stage
    kernels: k_stage2_h2u would never run. So every node lists its 8 neighbours cyclically up to 15 entries (a mean over repeated
    rows; tests/s2u_plan_check.cpp builds its small tables the same way): the union of a block has 8 rows, a chunk holds one or two
    nodes. The f16x2 route is asserted; the path output, x_latent and the Bipartite output against the structured oracle on the same
    table within the 1e-5 x max(1, max|ref|) of tests/test_hip_parity.py for these intermediates; two runs bit-equal. (Through
    `HipPath.path_fwd`: the query read-out of `forward_fixed_source` reads the 10 nearest grid nodes of a query and refuses nine.)"""
    import numpy as np
    from oracle import genie_oracle as O
    S, G = 17, 9
    geom = synthetic.Geometry(S, G, L=200e3, n_query=40, seed=300 + S)
    win = synthetic.make_window(geom, 12 * S, seed=301 + S)
    w = Case("cfg1_20x500").weights
    sta_nbr = graph.neighbour_table(geom.A_sta_sta, S)
    nbr8 = np.asarray(graph.neighbour_table(geom.A_src_src, G))
    assert nbr8.shape == (G, 8)
    src_nbr = torch.from_numpy(np.ascontiguousarray(nbr8[:, np.arange(15) % 8])).to(torch.int32)
    A_src = torch.stack((src_nbr.reshape(-1).long(), torch.arange(G).repeat_interleave(15)))
    hp = engine.HipPath(S, G, engine.csr_from_table(sta_nbr), engine.csr_from_table(src_nbr), grid_order=engine.morton_order(geom.x_grid),
                        device=DEV, sta_order=engine.sfc_order(geom.locs))
    hp.set_weights({k: v.to(DEV) for k, v in w.items()})
    Slice, Mask = torch.from_numpy(win["Slice"]), torch.from_numpy(win["Mask"])
    ea = torch.from_numpy(geom.edge_attr())
    pos = torch.from_numpy(geom.x_grid).float()
    runs = [hp.path_fwd(Slice.to(DEV), Mask.to(DEV), ea.to(DEV), pos.to(DEV), want_x_latent=True, want_bip=True) for _ in range(2)]
    torch.cuda.synchronize()
    assert hp.stage_precision()["f16x2_active"], "the f16x2 stage kernels (k_stage2_h2u) are what this test is about"
    out, x_latent, bip = runs[0]
    da = O.data_aggregation_structured(w, Slice, Mask, sta_nbr, src_nbr.long(), S, G, full=True)
    o_bip = O.bipartite_read_in_structured(w, da["x_latent"], ea, Mask, S, G)
    o = o_bip
    for l in (1, 2, 3):
        o = O.spatial_aggregation(w, o, A_src, pos, "SpatialAggregation%d" % l)
    tol = lambda ref: 1e-5 * max(1.0, float(ref.abs().max()))
    assert max_abs(x_latent.cpu(), da["x_latent"]) <= tol(da["x_latent"])
    assert max_abs(bip.cpu(), o_bip) <= tol(o_bip)
    assert max_abs(out.cpu(), o) <= tol(o)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
