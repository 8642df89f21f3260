"""GPU: the 4-output `forward_fixed` / `forward` and the association pass on a source-node-sharded model (genie_amd/dist.py): the
P-sized association heads on the shard with one halo exchange per layer (genie_assoc_fwd_part), the pick-sized heads fed from rows
that live on several ranks (genie_lslc_rows, one ragged all-gather, genie_lslc_fwd_rows). The yardstick is always the UNSHARDED model on
the same inputs, compared with `torch.equal`.

Ranks on one GPU as in tests/test_dist_gpu.py: 2 and 3 processes over gloo (host-staged transport, every kernel and buffer of the sharded
schedule for real), one process with a world-1 RCCL group (the device-collective branch), and virtual ranks inside this process for the
new kernel alone. The RCCL path with more than one rank needs more than one GPU and does not run here."""
import functools
import os

import numpy as np
import pytest
import torch

from tests.test_sharded_assoc_cpu import K, _free_port, assert_case_exercises_the_exchange, sample_case, spawn_with_limit

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = ((7, 45), (9, 53))


def _t(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)


def _net(weights, **kw):
    from genie_amd import module
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV, **kw)
    net.load_state_dict({k: v.clone() for k, v in weights.items()}, strict=True)
    return net.eval()


def _base_args(geom, smp):
    return ((torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src), _t(geom.edge_attr()), _t(geom.locs), _t(geom.x_grid)),
            dict(A_edges_p=_t(smp["A_edges_p"], torch.long), A_edges_s=_t(smp["A_edges_s"], torch.long), dt_partition=smp["dt_partition"],
                 tlatent=_t(smp["tlatent"])))


def _call_args(geom, smp, Slice, Mask, picks=slice(None)):
    return (Slice, Mask, _t(smp["tpick"][picks]), _t(smp["ipick"][picks], torch.long), _t(smp["phase_label"][picks]), _t(geom.locs),
            _t(geom.x_grid), _t(geom.x_query), _t(smp["x_query_src"]), _t(geom.t_query), _t(smp["tq_sample"]), _t(smp["trv_out_q"]))


def _same(a, b):
    return len(a) == len(b) == 4 and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def _body(rank, world, res):
    """Everything one rank checks against the unsharded model built in the same process."""
    from genie_amd import apply, dist as gdist, graph
    from tests.util import Case
    weights = Case("cfg1_20x500").weights
    with torch.no_grad():
        for S, G in SHAPES:
            geom, smp, _, _, _ = sample_case(S, G, world)
            base, tables = _base_args(geom, smp)
            for phase_types in (True, False):
                ref, net = _net(weights, use_phase_types=phase_types), _net(weights, use_phase_types=phase_types, process_group=True)
                ref.set_adjacencies_base(*base, **tables)
                net.set_adjacencies_base(*base, **tables)
                assert net.is_sharded and (net.shard_plan.rank, net.shard_plan.world) == (rank, world)
                Slice, Mask = _t(smp["Slice"]), _t(smp["Mask"])
                want = [o.clone() for o in ref.forward_fixed(*_call_args(geom, smp, Slice, Mask))]
                net._shard.local.ws.fill_(255)                                          # NaN-poisoned workspace
                got = net.forward_fixed(*_call_args(geom, smp, Slice, Mask))
                tag = (S, G, phase_types)
                res[("fixed", tag)] = _same(got, want)
                res[("nontrivial", tag)] = want[2].shape[1] > 0 and float(want[2].abs().max()) > 0 and float(want[3].abs().max()) > 0
                if not phase_types:
                    continue
                rows = net._shard.row_index()                                           # the rank's local rows, as embed_window hands them over
                got = net.forward_fixed(*_call_args(geom, smp, gdist.ShardRows(Slice[rows]), gdist.ShardRows(Mask[rows])))
                res[("local rows", tag)] = _same(got, want)
                none = slice(0, 0)                                                      # a window without picks
                got, w0 = net.forward_fixed(*_call_args(geom, smp, Slice, Mask, none)), ref.forward_fixed(*_call_args(geom, smp, Slice, Mask, none))
                res[("no picks", tag)] = _same(got, w0) and tuple(got[2].shape) == (3, 0, 1)
                if (S, G) != SHAPES[0]:
                    continue
                # `forward`: the graphs passed per call (22 arguments)
                A_in_sta, A_in_src, A_src_in_prod, A_src_in_sta = graph.cartesian_product_edges(geom.A_sta_sta, geom.A_src_src, S, G)
                ea = graph.GraphEdges(x=_t(geom.edge_attr()), edge_index=A_src_in_prod.to(DEV))
                adj = (A_in_sta.to(DEV), A_in_src.to(DEV), ea, ea, A_src_in_sta.to(DEV), torch.from_numpy(geom.A_src_src).to(DEV),
                       tables["A_edges_p"], tables["A_edges_s"], tables["dt_partition"], tables["tlatent"])
                call = _call_args(geom, smp, Slice, Mask)
                fwd = _net(weights, process_group=True)
                ok = True
                for _ in range(2):                                                      # the build, then the cached graphs
                    ok = ok and _same(fwd.forward(Slice, Mask, *adj, *call[2:]), want)
                res[("forward", tag)] = ok
                # what stays refused names itself
                refused = {}
                for what, fn in (("train", lambda: net.train().forward_fixed(*call)),
                                 ("push_window", lambda: net.eval().push_window(Slice, Mask)),
                                 ("use_subgraph", lambda: net.set_adjacencies_subgraph_from_positions(_t(geom.locs), _t(geom.x_grid))),
                                 ("time_pointers", lambda: net.set_adjacencies_base(*base, tlatent=tables["tlatent"],
                                                                                     time_pointers=dict(max_t=5.0, dt=1.0, k=10, win=1.0)))):
                    try:
                        with torch.enable_grad():
                            fn()
                        refused[what] = "no error"
                    except NotImplementedError as e:
                        refused[what] = str(e)
                    net.eval()
                for kw in (dict(use_updated_model_definition=True), dict(use_absolute_pos=True)):
                    from genie_amd import module
                    var = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV, process_group=True, **kw).eval()
                    var.set_adjacencies_base(*base, **tables)
                    try:
                        var.forward_fixed(*call)
                        refused[list(kw)[0]] = "no error"
                    except NotImplementedError as e:
                        refused[list(kw)[0]] = str(e)
                res["refused"] = refused
        # through the caller: the association pass on a sharded leg, one of the two sources in a stretch without picks
        from tests.test_day_loops_gpu import _Setup
        s = _Setup()
        net = _net(s.w, process_group=True)
        net.set_adjacencies_base(torch.from_numpy(s.A_sta_sta), torch.from_numpy(s.geom_all.A_src_src), _t(s.ea), _t(s.locs), _t(s.geom_all.x_grid),
                                 torch.from_numpy(s.A_edges_p).to(DEV), torch.from_numpy(s.A_edges_s).to(DEV), _t(s.dt_partition),
                                 _t(s.trv_use.reshape(-1, 2)))
        leg = apply.GridLeg(net, s.geom_all.x_grid, s.trv_use)
        srcs = np.array([list(s.geom_all.x_grid[7]) + [7002.0, 0.5], [20e3, 30e3, -5e3, 30000.0, 0.5]])
        d = np.linalg.norm(srcs[:, None, 0:3] - s.locs[None, :, :], axis=2)
        trv_out = np.stack((d / 6000.0, d / 3500.0), axis=2).astype(np.float32)
        ident = lambda x: x                                                                 # noqa: E731
        outs = [apply.associate_sources([lg], s.picks, srcs, s.locs, s.tq, s.max_t, trv_out, ident, np.array([1000.0, 2000.0, 0.0]),
                                        kernel_sig_t=s.sig, dt_embed=s.dt) for lg in (s.leg, leg)]
    (p0, s0, sp0, lm0), (p1, s1, sp1, lm1) = outs
    res["associate"] = (len(p1) == 2 and all(torch.equal(a, b) for a, b in zip(p0 + s0, p1 + s1))
                        and all(np.array_equal(a, b) for a, b in zip(sp0 + lm0, sp1 + lm1)))
    res["associate shape"] = (int(p0[0].numel()) > 0 and float(p0[0].abs().max()) > 0, int(p0[1].numel()) == 0)


def _worker(rank, world, port, backend, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(DEV)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(DEV))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = {}
        _body(rank, world, res)
        torch.cuda.synchronize()
        ret[rank] = res
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def _ranks(world, backend="gloo"):
    import torch.multiprocessing as mp
    for S, G in SHAPES:                                        # conditions on the inputs, before anything is spawned
        if world > 1:
            _, _, _, plans, owners = sample_case(S, G, world)
            assert_case_exercises_the_exchange(plans, owners)
    ret = mp.Manager().dict()
    spawn_with_limit(_worker, (world, _free_port(), backend, ret), world, 240.0)
    assert len(ret) == world
    return [ret[r] for r in range(world)]


@pytest.mark.parametrize("world", [2, 3])
def test_four_outputs_bit_equal_to_the_unsharded_model_on_every_rank(world):
    """Fails with NotImplementedError without the sharded `forward_fixed`."""
    for rank, r in enumerate(_ranks(world)):
        for S, G in SHAPES:
            assert r[("nontrivial", (S, G, True))], (rank, S, G)
            assert r[("fixed", (S, G, True))], (rank, S, G)
            assert r[("local rows", (S, G, True))], (rank, S, G)
            assert r[("no picks", (S, G, True))], (rank, S, G)


@pytest.mark.parametrize("world", [2, 3])
def test_callers_on_a_sharded_model(world):
    for rank, r in enumerate(_ranks(world)):
        assert r[("forward", SHAPES[0] + (True,))], (rank, "forward (22 arguments) != forward_fixed of the unsharded model")
        for S, G in SHAPES:
            assert r[("fixed", (S, G, False))] and r[("nontrivial", (S, G, False))], (rank, S, G, "use_phase_types=False")
        assert r["associate shape"] == (True, True), (rank, r["associate shape"])
        assert r["associate"], (rank, "associate_sources on a sharded leg != the unsharded leg")


def test_refusals_name_the_call():
    for r in _ranks(2):
        got = r["refused"]
        for what, word in (("train", "training step"), ("push_window", "push_window"), ("use_subgraph", "use_subgraph"),
                           ("time_pointers", "time_pointers"), ("use_updated_model_definition", "use_updated_model_definition"),
                           ("use_absolute_pos", "use_absolute_pos")):
            assert word in got[what], (what, got[what])


def test_world1_rccl_group():
    r = _ranks(1, "nccl")[0]
    for S, G in SHAPES:
        assert r[("fixed", (S, G, True))] and r[("local rows", (S, G, True))] and r[("no picks", (S, G, True))], (S, G)
    assert r["associate"]


# ---- the new kernel alone: virtual ranks inside this process ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _whole_s(S, G):
    """An association embedding `s` [P, 30] of the whole product graph and the context that made it (the unsharded model)."""
    from tests.util import Case
    geom, smp, base, _, _ = sample_case(S, G, 3)
    ref = _net(Case("cfg1_20x500").weights)
    b, tables = _base_args(geom, smp)
    ref.set_adjacencies_base(*b, **tables)
    ref._hip.sync_weights(ref._path_params, ref._weight_split())             # (the heads' parameters: the unsharded lslc_fwd below)
    s = torch.randn((S * G, 30), generator=torch.Generator().manual_seed(4)).to(DEV)
    s[5, 3] = -0.0
    return geom, smp, ref, s, tables


def _rank_lists(S, G, world, tpick, ipick):
    from genie_amd import dist as gdist, engine
    geom, smp, ref, s, tables = _whole_s(S, G)
    hp = ref._hip
    ep, es = tables["A_edges_p"].to(torch.int32), tables["A_edges_s"].to(torch.int32)
    order = engine.sfc_order(geom.x_grid)
    lists = []
    for r in range(world):
        plan = gdist.ShardPlan(geom.A_src_src, G, world, r, order)
        sp = gdist.ShardedPath(S, G, engine.csr_from_edges(torch.from_numpy(geom.A_sta_sta), S), geom.A_src_src, geom.x_grid, world, r, DEV,
                               pos_sta=geom.locs, emulate=True)
        assert np.array_equal(sp.plan.own_global, plan.own_global)
        s_own = s[sp.row_index(own_only=True)].contiguous()
        count, rows = sp.local.lslc_rows(s_own, sp.node_local, ep, es, smp["dt_partition"], tpick, ipick, tables["tlatent"])
        lists.append((sp, rows[: int(count.item())].clone()))
    return s, ep, es, tables["tlatent"], lists


@pytest.mark.parametrize("n", [37, 16, 1])
def test_rank_lists_are_a_permutation_of_the_torch_gather(n):
    S, G = SHAPES[0]
    geom, smp, ref, _, _ = _whole_s(S, G)
    tpick, ipick = _t(smp["tpick"][:n]), _t(smp["ipick"][:n], torch.int32)
    s, ep, es, tl, lists = _rank_lists(S, G, 3, tpick, ipick)
    dtp = smp["dt_partition"]
    ti = np.floor((smp["tpick"][:n] - dtp[0]) / (dtp[1] - dtp[0])).astype(np.int64)
    base = torch.from_numpy(smp["ipick"][:n].astype(np.int64) * len(dtp) + ti).to(DEV)
    idx = (base.view(-1, 1) * K + torch.arange(K, device=DEV)).reshape(-1)
    e = torch.cat((ep[idx], es[idx])).long()                                            # entry number -> product node, both heads
    want = torch.cat((s[e], torch.cat((tl[e[: n * K], 0], tl[e[n * K:], 1])).view(-1, 1)), 1)
    rows = torch.cat([r for _, r in lists])
    keys = rows[:, 31].contiguous().view(torch.int32).long()
    assert rows.shape[0] == 2 * n * K and torch.equal(torch.sort(keys)[0], torch.arange(2 * n * K, device=DEV))     # every pair exactly once
    assert torch.equal(rows[:, :31].view(torch.int32), want[keys].view(torch.int32))                               # row bits, -0.0 included
    for sp, _ in lists:
        sp.local.check_index_flags(synchronize=True)                                    # nothing reported


def test_zero_picks_and_a_pick_outside_the_table():
    S, G = SHAPES[0]
    geom, smp, ref, _, tables = _whole_s(S, G)
    s, ep, es, tl, lists = _rank_lists(S, G, 2, _t(smp["tpick"][:0]), _t(smp["ipick"][:0], torch.int32))
    assert all(r.shape == (0, 32) for _, r in lists)
    tpick = _t(smp["tpick"][:5]).clone()
    tpick[3] = float(smp["dt_partition"][-1]) + 50.0                                    # outside dt_partition: clamped and reported
    s, ep, es, tl, lists = _rank_lists(S, G, 2, tpick, _t(smp["ipick"][:5], torch.int32))
    assert sum(int(r.shape[0]) for _, r in lists) == 2 * 5 * K                          # the clamped entry still has its owners
    for sp, _ in lists:
        with pytest.raises(IndexError, match="outside the time-pointer table"):
            sp.local.check_index_flags(synchronize=True)
    # ... as the unsharded call reports it
    hp = ref._hip
    hp.lslc_fwd(0, s, ep, smp["dt_partition"], tpick, _t(smp["ipick"][:5], torch.int32), _t(smp["phase_label"][:5]), tl, 0, 1.0)
    with pytest.raises(IndexError, match="outside the time-pointer table"):
        hp.check_index_flags(synchronize=True)
