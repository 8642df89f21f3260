"""GPU: the association heads' time-pointer tables built on the device (`engine.time_pointers_device`, genie_time_pointers) against
their exact yardsticks -- the reference's own tables (tests/golden/assoc_7x45.npz), `graph.time_pointers` on tie-laden travel times, the
irregular-graph rule restated below -- and through the class (`time_pointers=` of `set_adjacencies_base` /
`set_adjacencies_subgraph_from_positions`). Every comparison is exact: `np.array_equal` on tables and on `dt_partition`."""
import functools
import os

import numpy as np
import pytest
import torch

from genie_amd import engine, graph, module, synthetic
from tests.util import GOLDEN_DIR, Case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIG = synthetic.KERNEL_SIG_T
TP = dict(dt=SIG / 5.0, k=10, win=2.0 * SIG)          # train_GENIE_model.py:1364


def _tables(got):
    torch.cuda.synchronize()
    ep, es, dtp = got
    assert ep.dtype == torch.int32 and es.dtype == torch.int32 and ep.is_cuda and es.is_cuda
    assert isinstance(dtp, np.ndarray) and dtp.dtype == np.float64
    return ep.cpu().numpy(), es.cpu().numpy(), dtp


def _same(got, want, what=None):
    ep, es, dtp = _tables(got)
    assert np.array_equal(dtp, want[2]), what
    assert ep.shape == want[0].shape and es.shape == want[1].shape, what
    assert np.array_equal(ep, want[0]) and np.array_equal(es, want[1]), what


def test_device_tables_equal_the_reference_fixture():
    """The fixture's A_edges_p / A_edges_s are the output of the reference's assemble_time_pointers_for_stations itself
    (oracle/make_golden.py), the case of tests/test_assoc_cpu.py::test_time_pointers_match_the_reference_tables."""
    z = np.load(os.path.join(GOLDEN_DIR, "assoc_7x45.npz"))
    S, G = int(z["n_sta"]), int(z["n_grid"])
    tl = np.asarray(z["tlatent"])
    kw = dict(max_t=float(z["max_t"]), dt=3.0 / 5.0, k=10, win=6.0)
    host = graph.time_pointers(tl.reshape(G, S, 2), **kw)
    for form in (torch.from_numpy(tl).to(DEV), tl.reshape(G, S, 2)):           # [P, 2] on the device; the host function's [G, S, 2] array
        ep, es, dtp = _tables(engine.time_pointers_device(form, S, device=DEV, **kw))
        assert np.array_equal(ep, z["A_edges_p"]) and np.array_equal(es, z["A_edges_s"])
        assert np.array_equal(dtp, host[2]) and np.allclose(dtp, z["dt_partition"])


def _tie_trv(n_src, n_sta, quantum, seed=0):
    rng = np.random.default_rng([seed, n_src, n_sta])
    trv = rng.uniform(0, 60, (n_src, n_sta, 2)).astype(np.float32)
    if quantum:
        trv = (np.round(trv / quantum) * quantum).astype(np.float32)
    return trv


@pytest.mark.parametrize("dt", [0.6, 0.5])
@pytest.mark.parametrize("n_src,n_sta,k,quantum", [(500, 5, 10, None), (37, 4, 10, 1.0), (8, 3, 10, 1.0), (300, 4, 10, 0.5), (1000, 2, 3, 1.0),
                                                   (1, 3, 10, None), (1, 1, 1, 1.0), (200, 3, 32, 2.0)])
def test_device_tables_equal_the_host_builder_also_on_ties(n_src, n_sta, k, quantum, dt):
    """The cases of test_time_pointers_equal_the_full_ranking_also_on_ties (many equal travel times, travel times equal to time steps,
    k clipped to G at (8, 3, 10)), a single source node, and k = 32 at a quantum of 2 s (about six nodes per distinct travel time)."""
    trv = _tie_trv(n_src, n_sta, quantum)
    kw = dict(max_t=float(np.ceil(trv.max())), dt=dt, k=k, win=6.0)
    _same(engine.time_pointers_device(torch.from_numpy(trv.reshape(-1, 2)).to(DEV), n_sta, **kw), graph.time_pointers(trv, **kw), (n_src, n_sta, k, dt))


@pytest.mark.parametrize("dt", [0.6, 0.5])
def test_a_column_of_equal_travel_times(dt):
    """Every source node of station 0 has the same P travel time (a time step at dt = 0.5, between two at 0.6) and of station 1 the same
    S travel time: every time step of those columns lists the k lowest ids; the other columns are ordinary."""
    trv = _tie_trv(257, 3, None, seed=5)
    trv[:, 0, 0] = 7.0
    trv[:, 1, 1] = 33.5
    kw = dict(max_t=float(np.ceil(trv.max())), dt=dt, k=10, win=6.0)
    want = graph.time_pointers(trv, **kw)
    assert np.array_equal(want[0].reshape(3, -1, 10)[0], np.tile(np.arange(10) * 3, (len(want[2]), 1)))
    _same(engine.time_pointers_device(trv, 3, device=DEV, **kw), want)


def test_no_size_limit_three_stations_70000_source_nodes():
    """The kernels keep a station's candidates in global memory and have no internal size limit: the one large case instead (more than
    2^16 candidates per station, about 600 per bin)."""
    trv = _tie_trv(70000, 3, None, seed=7)
    trv[::997] = np.round(trv[::997])                  # (some ties and travel times on time steps at this size too)
    kw = dict(max_t=float(np.ceil(trv.max())), dt=0.5, k=10, win=6.0)
    _same(engine.time_pointers_device(torch.from_numpy(trv).to(DEV), 3, **kw), graph.time_pointers(trv, **kw))


def test_max_t_none_takes_the_largest_travel_time():
    trv = _tie_trv(300, 4, None, seed=9)
    _same(engine.time_pointers_device(torch.from_numpy(trv).to(DEV), 4, dt=0.6, k=10, win=6.0), graph.time_pointers(trv, dt=0.6, k=10, win=6.0))


def test_two_runs_give_identical_tables():
    trv = torch.from_numpy(_tie_trv(500, 5, 0.5).reshape(-1, 2)).to(DEV)
    a = _tables(engine.time_pointers_device(trv, 5, max_t=60.0, dt=0.6, k=10, win=6.0))
    b = _tables(engine.time_pointers_device(trv, 5, max_t=60.0, dt=0.6, k=10, win=6.0))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- irregular product graphs ---------------------------------------------------------------------------------------------------
def _irregular_tables(trv, pairs, max_t, dt, k, win):
    """The rule of the irregular form, restated: per station and time step the k product nodes OF THAT STATION nearest in travel time
    (float64 distance, stable: equal distances to the lower node id), rank j of a station with n < k nodes = rank j mod n."""
    dtp = np.arange(-win, win + max_t + dt, dt)
    S = trv.shape[1]
    out = []
    for ph in range(2):
        tab = np.zeros((S, dtp.size, k), dtype=np.int64)
        for i in range(S):
            nodes = np.nonzero(pairs[0] == i)[0]
            tt = trv[pairs[1][nodes], i, ph].astype(np.float64)
            order = np.argsort(np.abs(tt[None, :] - dtp[:, None]), axis=1, kind="stable")
            tab[i] = nodes[np.take(order, np.arange(k) % nodes.size, axis=1)]
        out.append(tab.reshape(-1))
    return out[0], out[1], dtp


def _draw_pairs(geom, seed):
    """Product nodes as tests/test_fuzz_gpu.py draws them (each source node keeps its 1-5 nearest stations, every station keeps a source
    node, random extras), then station 0 cut to its 3 nearest source nodes (fewer than k = 10: cycling) and station 1 to exactly 10."""
    rng = np.random.default_rng(seed)
    S, G = geom.n_sta, geom.n_grid
    d = np.linalg.norm(geom.x_grid[:, None, :2] - geom.locs[None, :, :2], axis=2)          # [G, S]
    keep = np.zeros(d.shape, dtype=bool)
    keep[np.arange(G)[:, None], np.argsort(d, axis=1)[:, :int(rng.integers(1, min(6, S) + 1))]] = True
    keep[np.argmin(d, axis=0), np.arange(S)] = True
    keep |= rng.random(d.shape) < 0.5
    for i, n in ((0, 3), (1, 10)):
        keep[:, i] = False
        keep[np.argsort(d[:, i], kind="stable")[:n], i] = True
    keep[~keep.any(axis=1), 2] = True                                                      # every source node keeps a station
    src_i, sta_i = np.nonzero(keep)
    pairs = np.stack((sta_i, src_i))
    n_of = np.bincount(sta_i, minlength=S)
    assert n_of[0] == 3 and n_of[1] == 10 and n_of.min() >= 1 and n_of.max() > 10
    return pairs


@functools.lru_cache(maxsize=None)
def _irregular_case(S, G):
    geom = synthetic.Geometry(S, G, n_query=8, seed=40 + S)
    trv = geom.travel_times().astype(np.float32)
    trv[::3] = np.round(trv[::3])                                                          # ties
    pairs = _draw_pairs(geom, 900 + S)
    kw = dict(max_t=float(np.ceil(trv.max())), **TP)
    return trv, pairs, kw, _irregular_tables(trv, pairs, kw["max_t"], kw["dt"], kw["k"], kw["win"])


@pytest.mark.parametrize("S,G", [(14, 50), (5, 16)])
@pytest.mark.parametrize("where", ["host_pairs", "device_pairs"])
def test_irregular_tables_equal_the_restated_rule(S, G, where):
    trv, pairs, kw, want = _irregular_case(S, G)
    rows = trv[pairs[1], pairs[0]]                                                         # [N, 2] in product-node order
    prs = torch.from_numpy(pairs)
    if where == "device_pairs":                                                            # (the empty-station verdict comes from the device)
        _same(engine.time_pointers_device(torch.from_numpy(rows).to(DEV), S, pairs=prs.to(DEV), **kw), want)
    else:
        _same(engine.time_pointers_device(trv, S, pairs=prs, device=DEV, **kw), want)     # [G, S, 2] gathered at the pairs


def test_a_station_without_a_product_node_is_found_on_the_device():
    trv, pairs, kw, _ = _irregular_case(5, 16)
    sel = pairs[0] != 3
    prs, rows = torch.from_numpy(pairs[:, sel]).to(DEV), torch.from_numpy(trv[pairs[1][sel], pairs[0][sel]]).to(DEV)
    with pytest.raises(ValueError, match="without a product node"):
        engine.time_pointers_device(rows, 5, pairs=prs, **kw)


# ---- through the class ----------------------------------------------------------------------------------------------------------
def _net():
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV)
    net.load_state_dict({k: v.clone() for k, v in Case("cfg1_20x500").weights.items()}, strict=True)
    return net


def _t(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)


def _four_outputs(net, geom, smp, Slice, Mask):
    """(eval outputs, train outputs, parameter gradients of a fixed cotangent) of forward_fixed on the model as it stands."""
    args = (_t(Slice), _t(Mask), _t(smp["tpick"]), _t(smp["ipick"], torch.long), _t(smp["phase_label"]), _t(geom.locs), _t(geom.x_grid),
            _t(geom.x_query), _t(smp["x_query_src"]), _t(geom.t_query), _t(smp["tq_sample"]), _t(smp["trv_out_q"]))
    net.eval()
    with torch.no_grad():
        out_e = net.forward_fixed(*args)
    net.train()
    net.zero_grad(set_to_none=True)
    out_t = net.forward_fixed(*args)
    gen = torch.Generator().manual_seed(3)
    sum((o * torch.randn(o.shape, generator=gen).to(DEV)).sum() for o in out_t).backward()
    torch.cuda.synchronize()
    return out_e, [o.detach() for o in out_t], {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}


def _assert_same_runs(a, b):
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)
    assert a[2].keys() == b[2].keys() and len(a[2]) >= 80
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    assert a[0][2].shape[1] > 0 and float(a[0][2].abs().max()) > 0          # picks reached the association heads


def _int32_tables_are_used_in_place(net):
    assert net.A_edges_p.dtype == torch.int32 and net.A_edges_p.is_cuda
    assert net._a_edges_i32[0].data_ptr() == net.A_edges_p.data_ptr() and net._a_edges_i32[1].data_ptr() == net.A_edges_s.data_ptr()


def test_forward_fixed_is_bit_equal_with_host_and_device_tables():
    S, G = 7, 45
    geom = synthetic.Geometry(S, G, n_query=20, seed=11)
    smp = synthetic.training_sample(geom, 120, n_src=4, seed=5)
    trv = smp["tlatent"].reshape(G, S, 2)
    kw = dict(max_t=float(np.ceil(trv.max())), **TP)
    ep, es, dtp = graph.time_pointers(trv, **kw)
    assert np.array_equal(ep, smp["A_edges_p"]) and np.array_equal(es, smp["A_edges_s"])          # the sample's own tables
    base = (torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src), _t(geom.edge_attr()), _t(geom.locs), _t(geom.x_grid))
    host = _net()
    host.set_adjacencies_base(*base, A_edges_p=_t(ep, torch.long), A_edges_s=_t(es, torch.long), dt_partition=dtp, tlatent=_t(smp["tlatent"]))
    dev = _net()
    dev.set_adjacencies_base(*base, tlatent=_t(smp["tlatent"]), time_pointers=kw)
    assert np.array_equal(dev.dt_partition, dtp) and np.array_equal(dev.A_edges_p.cpu().numpy(), ep)
    _assert_same_runs(_four_outputs(host, geom, smp, smp["Slice"], smp["Mask"]), _four_outputs(dev, geom, smp, smp["Slice"], smp["Mask"]))
    _int32_tables_are_used_in_place(dev)


def test_forward_fixed_is_bit_equal_on_an_irregular_graph():
    S, G = 7, 45
    geom = synthetic.Geometry(S, G, n_query=20, seed=11)
    smp = synthetic.training_sample(geom, 120, n_src=4, seed=5)
    trv = smp["tlatent"].reshape(G, S, 2)
    kw = dict(max_t=float(np.ceil(trv.max())), **TP)
    sub = dict(max_deg_offset=0.0, k_nearest_pairs=3)          # every source node with its 3 nearest stations
    dev = _net()
    _, _, prs = dev.set_adjacencies_subgraph_from_positions(_t(geom.locs), _t(geom.x_grid), tlatent=trv, time_pointers=kw, **sub)
    pairs = prs.cpu().numpy()
    n_of = np.bincount(pairs[0], minlength=S)
    assert pairs.shape[1] == 3 * G and n_of.min() >= 1
    ep, es, dtp = _irregular_tables(trv, pairs, kw["max_t"], kw["dt"], kw["k"], kw["win"])
    assert np.array_equal(dev.A_edges_p.cpu().numpy(), ep) and np.array_equal(dev.A_edges_s.cpu().numpy(), es)
    assert np.array_equal(dev.dt_partition, dtp)
    host = _net()
    _, _, prs_h = host.set_adjacencies_subgraph_from_positions(_t(geom.locs), _t(geom.x_grid), **sub)
    assert torch.equal(prs_h, prs)
    host.A_edges_p, host.A_edges_s, host.dt_partition = _t(ep, torch.long), _t(es, torch.long), dtp
    host.tlatent = _t(trv[pairs[1], pairs[0]])
    rows = pairs[1] * S + pairs[0]
    Slice, Mask = smp["Slice"][rows], smp["Mask"][rows]
    _assert_same_runs(_four_outputs(host, geom, smp, Slice, Mask), _four_outputs(dev, geom, smp, Slice, Mask))
    _int32_tables_are_used_in_place(dev)
