"""GPU: source-node shards of an IRREGULAR product graph (`use_subgraph`): `dist.SubgraphShardPlan` + the extended irregular context
(genie_ctx_create_subgraph_ext) + the row-range stage launches, against the unsharded `use_subgraph` context, bit for bit.

* one process, virtual ranks (`emulate=True`; the halo rows of `wv` are fed from the unsharded run): every rank of worlds 1, 2, 3 on the
  graphs of `subgraph_14x50` and `subgraph_edges_14x50` and on a graph whose source nodes have 1, 15, 16, 17 and 33 rows (the 16-row
  tile of the stage kernels), both stage-1 kernels, both schedules;
* the drop-in class at world 1 against the unsharded class and the fixture;
* 2 and 3 processes sharing one GPU over gloo, and a world-size-1 RCCL group: `forward_fixed_source[_pipelined]` with full inputs and
  with `ShardRows`, and `apply.apply_windows_device`, `torch.equal` to one GPU on every rank;
* what an irregular shard refuses names the call."""
import functools
import multiprocessing
import os
import socket

import numpy as np
import pytest
import torch

from tests import shard_subgraph_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RANKS = [(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3)]
CHILD_TIMEOUT = 150.0


def _named(name):
    return {"straddle": cases.straddle_graph, "handmade": cases.handmade_graph}.get(name, lambda: cases.fixture_graph(name))()


def _weights():
    from tests.util import Case
    return Case("subgraph_14x50").weights


def _sub(g):
    t = torch.from_numpy
    return {"n_prod": int(g.seg[-1]), "sta_csr": tuple(t(a) for a in g.sta_csr), "src_csr": tuple(t(a) for a in g.src_csr),
            "seg_rowptr": t(g.seg.astype(np.int32))}


def _wv_rows(hp, n_rows):
    """The wv rows [n_rows, pitch] a context's stage 1 left in its workspace."""
    pitch = int(hp.lib.genie_ws_v_pitch(hp.ctx))
    off = int(hp.lib.genie_ws_v_ptr(hp.ctx, hp._ws_ptr)) - hp.ws.data_ptr()
    return hp.ws[off: off + 4 * n_rows * pitch].view(torch.float32).view(n_rows, pitch)


@functools.lru_cache(maxsize=None)
def _whole(name, precision):
    """The unsharded `use_subgraph` context on random inputs: wv after stage 1, x_latent, and the Bipartite output of both stage-2
    routes (with and without x_latent). Computed once per (graph, precision), shared, left unchanged."""
    from genie_amd import engine
    g = _named(name)
    n = int(g.seg[-1])
    hp = engine.HipPath(g.S, g.G, None, engine.csr_from_edges(g.A_src_src, g.G), grid_order=engine.sfc_order(g.x_grid), device=DEV,
                        subgraph=_sub(g), stage_precision=precision)
    hp.set_weights({k: v.to(DEV) for k, v in _weights().items()})
    Slice, Mask, ea = [t.to(DEV) for t in cases.random_inputs(g, 7)]
    hp.da_stage1(Slice, Mask)
    wv = _wv_rows(hp, n).clone()
    x_latent, bip_xl = hp.da_stage2_bipartite(Mask, ea, want_x_latent=True)
    hp.da_stage1(Slice, Mask)
    _, bip = hp.da_stage2_bipartite(Mask, ea)
    torch.cuda.synchronize()
    assert precision == "auto" or not hp.stage_precision()["f16x2_active"]
    assert float(bip.abs().max()) > 1e-3 and bool(torch.isfinite(wv).all())
    return g, (Slice, Mask, ea), wv, x_latent, bip_xl.clone(), bip.clone()


@pytest.mark.parametrize("rank,world", RANKS)
@pytest.mark.parametrize("name,precision", [("subgraph_14x50", "auto"), ("subgraph_edges_14x50", "auto"), ("straddle", "auto"),
                                            ("straddle", "f32"), ("subgraph_14x50", "f32")])
def test_virtual_rank_rows_equal_the_unsharded_context(name, precision, rank, world):
    from genie_amd import dist as gdist, engine
    g, (Slice, Mask, ea), wv, x_latent, bip_xl, bip = _whole(name, precision)
    wd = {k: v.to(DEV) for k, v in _weights().items()}
    for overlap in (True, False):
        sp = gdist.ShardedPath(g.S, g.G, None, g.A_src_src, g.x_grid, world, rank, DEV, emulate=True, subgraph=_sub(g), overlap=overlap)
        sp.local.set_stage_precision(precision)
        sp.set_weights(wd)
        p = sp.plan
        ref = cases.plan_of(g, world, rank, engine.sfc_order(g.x_grid))
        assert np.array_equal(p.own_rows, ref.own_rows) and np.array_equal(p.halo_rows, ref.halo_rows)
        own, ext = sp.row_index(own_only=True), sp.row_index()
        halo = ext[p.n_rows_own:]
        # the emulated exchange delivers nothing meaningful: the halo rows come from the unsharded run's wv
        sp.transport.all_to_all_rows = lambda recv, send, rc, sc: recv.copy_(wv[halo]) if recv.shape[0] else None
        sp.local.ws.fill_(255)                                                       # NaN-poisoned workspace
        xl = torch.full((p.n_rows_own, 30), float("nan"), device=DEV)
        got_xl = sp.front(Slice[ext], Mask[ext], ea[own], x_latent_out=xl)           # stage 2 with x_latent (k_stage2<PCSR> + segment sums)
        got_wv = sp.wv_view()[: p.n_rows_own].clone()
        got = sp.front(Slice[ext], Mask[ext], ea[own])                               # the inference route (k_stage2_pseg)
        torch.cuda.synchronize()
        nodes = torch.as_tensor(p.own_global, device=DEV)
        assert torch.equal(got_wv, wv[own]), (overlap, "wv")
        assert torch.equal(xl, x_latent[own]), (overlap, "x_latent")
        assert torch.equal(got_xl, bip_xl[nodes]), (overlap, "bip next to x_latent")
        assert torch.equal(got, bip[nodes]), (overlap, "bip")
        sp.local.check_input_range()


def _model(g, weights, dev=DEV, **kw):
    """The drop-in class with the irregular lists of `g` (the reference's 12 arguments)."""
    from genie_amd import graph, module
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=dev, **kw)
    net.load_state_dict({k: v.clone() for k, v in weights.items()}, strict=True)
    return net.eval()


def _adj(g, ea, dev=DEV):
    from genie_amd import graph
    e = graph.GraphEdges(x=ea.to(dev), edge_index=g.A_src_in_prod.to(dev))
    t = lambda a: torch.as_tensor(a).to(dev)
    return (g.A_in_sta.to(dev), g.A_in_src.to(dev), e, e, t(g.pairs), t(g.A_src_src), None, None, None, None, t(g.locs).float(),
            t(g.x_grid).float())


def test_world1_drop_in_equals_the_unsharded_model_and_the_fixture():
    from tests.util import Case, max_abs
    c = Case("subgraph_14x50")
    g = cases.fixture_graph("subgraph_14x50")
    t = lambda a: a.float().to(DEV)
    call = (t(c.Slice), t(c.Mask), None, None, None, t(c.locs), t(c.x_grid), t(c.x_query), t(c.t_query))
    outs = []
    for kw in ({}, {"shard": (0, 1)}):
        net = _model(g, c.weights, **kw)
        net.set_adjacencies(*_adj(g, c.edge_attr))
        with torch.no_grad():
            outs.append(tuple(o.clone() for o in net.forward_fixed_source(*call)))
    assert net.is_sharded and net._shard.irregular and net.shard_plan.n_rows_halo == 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert max_abs(outs[1][0].cpu(), c.ref("y")) <= 1e-5 and max_abs(outs[1][1].cpu(), c.ref("x")) <= 1e-5


def test_refusals_name_the_call():
    """What an irregular shard does not serve raises NotImplementedError naming the call (a virtual rank of two: no collective runs)."""
    g = cases.fixture_graph("subgraph_14x50")
    w = _weights()
    _, Mask, ea = cases.random_inputs(g, 7)
    adj = _adj(g, ea)
    net = _model(g, w, shard=(0, 2), shard_emulate=True)
    net.set_adjacencies(*adj)
    n = int(g.seg[-1])
    S4 = torch.zeros((n, 4), device=DEV)
    q = adj[11][:3]
    tq = torch.zeros(3, device=DEV)
    ff = (S4, S4, None, None, None, adj[10], adj[11], q, q[:2], tq, None, None)

    def message(fn):
        with pytest.raises(NotImplementedError) as e, torch.enable_grad():
            fn()
        return str(e.value)
    assert "forward_fixed" in message(lambda: net.forward_fixed(*ff)) and "use_subgraph" in message(lambda: net.forward_fixed(*ff))
    fwd = message(lambda: net.forward(S4, S4, *adj[:10], None, None, None, adj[10], adj[11], q, q[:2], tq, None, None))
    assert "forward" in fwd and "use_subgraph" in fwd
    assert "training step" in message(lambda: net.train().forward_fixed_source(*ff[:8], tq))
    net.eval()
    assert "window_batch" in message(lambda: setattr(net, "window_batch", 2))
    assert "time_pointers" in message(lambda: net._shard.time_pointers(torch.zeros((n, 2), device=DEV)))
    assert "assoc_fwd" in message(lambda: net._shard.assoc_fwd(None, None, None, None, None))
    assert "callable" in message(lambda: net.node_rows(lambda ids: None))
    m = message(lambda: net.set_adjacencies_subgraph_from_positions(adj[10], adj[11]))
    assert "set_adjacencies_subgraph_from_positions" in m and "use_subgraph" in m
    for kw in ("use_updated_model_definition", "use_absolute_pos"):
        from genie_amd import module
        var = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV, shard=(0, 2), shard_emulate=True, **{kw: True}).eval()
        assert kw in message(lambda: var.set_adjacencies(*adj)) and var._hip is None
    # the library: sub-ranges stay refused on an unsharded irregular context, and an extended one checks its columns
    from genie_amd import _lib, engine
    hp = engine.HipPath(g.S, g.G, None, engine.csr_from_edges(g.A_src_src, g.G), device=DEV, subgraph=_sub(g))
    with pytest.raises(_lib.GenieHipError, match="unsharded irregular"):
        hp.da_stage1_range(S4, S4, 0, 1, True)
    p = cases.plan_of(g, 2, 0)
    t = torch.from_numpy
    bad = p.src_col.copy()
    bad[0] = p.n_rows_ext                                                            # one past the halo rows
    with pytest.raises(_lib.GenieHipError, match="outside the local rows"):
        engine.HipPath(g.S, p.n_own, None, None, device=DEV, subgraph={
            "n_prod": p.n_rows_own, "n_prod_ext": p.n_rows_ext, "sta_csr": (t(p.sta_rowptr), t(p.sta_col)),
            "src_csr": (t(p.src_rowptr), t(bad)), "seg_rowptr": t(p.seg_rowptr)})


# ---- one process per rank -------------------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, backend, ret):
    import torch.distributed as dist
    from genie_amd import apply, dist as gdist, synthetic
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(DEV)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(DEV))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tests.util import Case
        geom, g = cases.geometry_graph()
        w = Case("o1_20x500").weights                                                # weights with O(1) outputs
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV)
        ea = torch.from_numpy(geom.edge_attr().reshape(g.G, g.S, 3)[g.pairs[1], g.pairs[0]]).float()
        adj = _adj(g, ea)
        locs, xg, xq, tq = adj[10], adj[11], t(geom.x_query), t(geom.t_query)
        wins = [[a.to(DEV) for a in cases.random_inputs(g, 20 + k)[:2]] for k in range(3)]
        ref_net = _model(g, w)
        ref_net.set_adjacencies(*adj)
        with torch.no_grad():
            refs = [tuple(o.clone() for o in ref_net.forward_fixed_source(s, m, None, None, None, locs, xg, xq, tq)) for s, m in wins]
        P = synthetic.make_picks(geom, 900, seed=72)
        P[:, 0] = P[:, 0] * 0.25 + 5000.0
        P = P[np.argsort(P[:, 0], kind="stable")]
        trv = geom.travel_times().astype(np.float32)
        max_t = float(np.ceil(trv.max() + 1.0))
        Out_ref, times_ref = apply.apply_windows_device(ref_net, geom, P, trv, min_required_picks=5, max_t=max_t, tail_batch=1, pairs=g.pairs)
        torch.cuda.synchronize()
        res = {"nontrivial": float(refs[0][0].abs().max()) > 0.05 and float(Out_ref.abs().max()) > 0 and len(times_ref) >= 3}
        for overlap, halo in ((True, "a2a"), (False, "a2a"), (True, "p2p")):
            net = _model(g, w, process_group=True, shard_overlap=overlap, shard_halo=halo)
            net.set_adjacencies(*adj)
            p = net.shard_plan
            net._shard.local.ws.fill_(255)                                           # NaN-poisoned workspace
            with torch.no_grad():
                outs = [net.forward_fixed_source(s, m, None, None, None, locs, xg, xq, tq) for s, m in wins]       # full inputs
                ok = all(torch.equal(y, y0) and torch.equal(x, x0) for (y, x), (y0, x0) in zip(outs, refs))
                outs = [net.forward_fixed_source_pipelined(s, m, None, None, None, locs, xg, xq, tq) for s, m in wins]
                net._hip.wait_tails()
                torch.cuda.synchronize()
                ok_piped = all(torch.equal(y, y0) and torch.equal(x, x0) for (y, x, _), (y0, x0) in zip(outs, refs))
                rows = net._shard.row_index()
                s, m = wins[1]
                y, x = net.forward_fixed_source(gdist.ShardRows(s[rows]), gdist.ShardRows(m[rows]), None, None, None, locs, xg, xq, tq)
                ok_local = torch.equal(y, refs[1][0]) and torch.equal(x, refs[1][1])
            Out, times = apply.apply_windows_device(net, geom, P, trv, min_required_picks=5, max_t=max_t, pairs=g.pairs)
            torch.cuda.synchronize()
            ok_apply = np.array_equal(times, times_ref) and torch.equal(Out, Out_ref)
            res[(overlap, halo)] = (ok, ok_piped, ok_local, ok_apply)
            dist.barrier()
        res["plan"] = (p.n_rows_own, p.n_rows_halo, p.r_send, p.r_need, p.n_own)
        res["device_collectives"] = bool(net._shard.transport.on and net._shard.transport.device_collectives)
        ret[rank] = res
    finally:
        dist.destroy_process_group()


def _run(world, backend):
    """One child per rank, each under its own timeout: a child that outlives it is killed and fails the test."""
    ctx = multiprocessing.get_context("spawn")
    mgr = ctx.Manager()
    ret = mgr.dict()
    port = _free_port()
    kids = [ctx.Process(target=_worker, args=(r, world, port, backend, ret)) for r in range(world)]
    for k in kids:
        k.start()
    late = []
    for r, k in enumerate(kids):
        k.join(CHILD_TIMEOUT)
        if k.is_alive():
            late.append(r)
    for k in kids:
        if k.is_alive():
            k.kill()
            k.join()
    assert not late, "rank(s) %s did not finish within %.0f s" % (late, CHILD_TIMEOUT)
    assert [k.exitcode for k in kids] == [0] * world and len(ret) == world
    for rank in range(world):
        r = ret[rank]
        assert r["nontrivial"]
        if world > 1:
            assert r["plan"][1] > 0, "the test graph must give every rank halo rows"
        for k in ((True, "a2a"), (False, "a2a"), (True, "p2p")):
            assert r[k] == (True,) * 4, (rank, k, r[k], "(full inputs, pipelined, ShardRows, apply loop)")
    return ret


def test_two_processes_on_one_gpu_bit_equal_to_unsharded():
    _run(2, "gloo")


def test_three_processes_on_one_gpu_bit_equal_to_unsharded():
    _run(3, "gloo")


def test_world1_rccl_group_bit_equal_to_unsharded():
    ret = _run(1, "nccl")
    assert ret[0]["device_collectives"], "the nccl (RCCL) process group must select the device-collective transport"
