"""GPU: k_stage2_h2u with its read-once streams (c, message mask, edge fragments) loaded non-temporally, behind k_stage1_h2 storing
c non-temporally. The change adds no second plan or grid to compare with, so x_latent and the Bipartite output (the read-out of the
kernel's per-tile partials) are held to the structured oracle within the 1e-5 x max(1, max|ref|) that tests/test_hip_parity.py
applies to these intermediates, and two runs to each other bit for bit.
Shapes: S = 16 (one full station tile), 17 (one lane in the last tile), 33 (three tiles); G = 40 (five nodes = one block = one
group per XCD chunk), 500 (62 or 63 nodes per chunk: two groups, rows carried inside them, the second group short)."""
import pytest
import torch

from genie_amd import engine, graph, synthetic
from tests.util import Case, max_abs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("G", [40, 500])
@pytest.mark.parametrize("S", [16, 17, 33])
def test_partials_match_the_oracle(S, G):
    from oracle import genie_oracle as O
    geom = synthetic.Geometry(S, G, L=200e3, n_query=40, seed=500 + S)
    win = synthetic.make_window(geom, 12 * S, seed=501 + S)
    w = Case("cfg1_20x500").weights
    sta_nbr = graph.neighbour_table(geom.A_sta_sta, S)
    src_nbr = graph.neighbour_table(geom.A_src_src, G)
    assert tuple(sta_nbr.shape) == (S, 8) and tuple(src_nbr.shape) == (G, 15)
    hp = engine.HipPath(S, G, engine.csr_from_table(sta_nbr), engine.csr_from_table(src_nbr), grid_order=engine.sfc_order(geom.x_grid),
                        device=DEV, sta_order=engine.sfc_order(geom.locs))
    hp.set_weights({k: v.to(DEV) for k, v in w.items()})
    Slice, Mask = torch.from_numpy(win["Slice"]), torch.from_numpy(win["Mask"])
    ea = torch.from_numpy(geom.edge_attr())
    pos = torch.from_numpy(geom.x_grid).float()
    hp.set_static_edge_attr(ea.to(DEV))
    runs = [hp.path_fwd(Slice.to(DEV), Mask.to(DEV), ea.to(DEV), pos.to(DEV), want_x_latent=True, want_bip=True) for _ in range(2)]
    torch.cuda.synchronize()
    assert hp.stage_precision()["f16x2_active"], "the f16x2 stage kernels (k_stage1_h2, k_stage2_h2u) are what this test is about"
    _, x_latent, bip = runs[0]
    da = O.data_aggregation_structured(w, Slice, Mask, sta_nbr, src_nbr.long(), S, G, full=True)
    o_bip = O.bipartite_read_in_structured(w, da["x_latent"], ea, Mask, S, G)
    tol = lambda ref: 1e-5 * max(1.0, float(ref.abs().max()))
    ex, eb = max_abs(x_latent.cpu(), da["x_latent"]), max_abs(bip.cpu(), o_bip)
    print("S %d G %d: max|x_latent - oracle| %.3g (tol %.3g)  max|bip - oracle| %.3g (tol %.3g)" % (S, G, ex, tol(da["x_latent"]), eb, tol(o_bip)))
    assert ex <= tol(da["x_latent"])
    assert eb <= tol(o_bip)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
