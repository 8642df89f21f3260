"""GPU: a source-node-sharded model set up from each rank's own travel-time rows -- the distributed time-pointer build
(genie_time_pointers_candidates, one all-gather, genie_time_pointers_merge), the pick-sized heads fed with the travel time of every
listed row from the row's owner (genie_lslc_rows_own), and the four outputs under every model definition. Yardsticks, all exact
(`torch.equal` / `np.array_equal`): `graph.time_pointers`, the unsharded `engine.time_pointers_device`, the unsharded model.

Ranks on one GPU as in tests/test_sharded_assoc_gpu.py: 2 and 3 processes over gloo, one process with a world-1 RCCL group; every child
is a fresh process under one time limit. On the parent of this change `time_pointers=` on a shard raises NotImplementedError."""
import functools
import os

import numpy as np
import pytest
import torch

from tests.test_shard_time_pointers_cpu import CASES, case, cross_rank_ties_at_k, own_rows, plans
from tests.test_sharded_assoc_cpu import _free_port, assert_case_exercises_the_exchange, sample_case, spawn_with_limit

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = ((7, 45), (9, 53))
# The two other model definitions: the public `forward` / `forward_fixed` refuse them on a shard (tests/test_sharded_assoc_gpu.py pins
# that), so their four outputs are taken behind the guard (`_sharded_four_outputs`, the very computation the default definition runs).
DEFINITIONS = ({}, {"use_updated_model_definition": True}, {"use_absolute_pos": True})


def _t(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)


def _tp_kw(smp):
    from genie_amd import synthetic
    sig = synthetic.KERNEL_SIG_T
    return dict(max_t=float(np.ceil(smp["tlatent"].max())), dt=sig / 5.0, k=10, win=2.0 * sig)      # (synthetic.training_sample's tables)


def _base(geom):
    return (torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src), _t(geom.edge_attr()), _t(geom.locs), _t(geom.x_grid))


def _call_args(geom, smp, Slice, Mask, picks=slice(None)):
    return (Slice, Mask, _t(smp["tpick"][picks]), _t(smp["ipick"][picks], torch.long), _t(smp["phase_label"][picks]), _t(geom.locs),
            _t(geom.x_grid), _t(geom.x_query), _t(smp["x_query_src"]), _t(geom.t_query), _t(smp["tq_sample"]), _t(smp["trv_out_q"]))


def _same(a, b):
    return len(a) == len(b) == 4 and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def _pair(seed, **kw):
    """(unsharded model, sharded model) with the same seeded parameters."""
    from genie_amd import module
    torch.manual_seed(seed)
    ref = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV, **kw).eval()
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV, process_group=True, **kw).eval()
    net.load_state_dict({k: v.clone() for k, v in ref.state_dict().items()}, strict=True)
    return ref, net


def _tables_equal(got, want):
    return (got[0].dtype == torch.int32 and np.array_equal(got[0].cpu().numpy(), np.asarray(want[0]).astype(np.int64))
            and np.array_equal(got[1].cpu().numpy(), np.asarray(want[1]).astype(np.int64)) and np.array_equal(np.asarray(got[2]), want[2]))


def _body(rank, world, res):
    from genie_amd import apply, dist as gdist, engine, graph
    tr = gdist.Transport(None, world)
    # ---- the tables alone: the driver with its two kernels, every case, against the host builder and the unsharded device builder
    for name, (S, G, k, _, worlds) in CASES.items():
        if world not in worlds:
            continue
        trv, kw, _, _ = case(name)
        p = plans(name, world)[rank]
        for max_t in (kw["max_t"], None):
            kw2 = dict(kw, max_t=max_t)
            got = gdist.shard_time_pointers(own_rows(trv, p).to(DEV), p.own_global, S, G, tr, **kw2)
            one = engine.time_pointers_device(_t(trv.reshape(-1, 2)), S, **kw2)
            res[("tables", name, max_t is None)] = (_tables_equal(got, graph.time_pointers(trv, **kw2))
                                                    and torch.equal(got[0], one[0]) and torch.equal(got[1], one[1])
                                                    and got[0].numel() == S * len(got[2]) * min(k, G))
    if world > 1:            # a NaN in the rows of rank 1 only: every rank raises
        trv, kw, _, _ = case("7x45")
        p = plans("7x45", world)[rank]
        rows = own_rows(trv, p).to(DEV)
        if rank == 1:
            rows[3, 1] = float("nan")
        try:
            gdist.shard_time_pointers(rows, p.own_global, 7, 45, tr, **dict(kw, max_t=None))
            res["nan"] = "no error"
        except ValueError as e:
            res["nan"] = str(e)
    with torch.no_grad():
        for si, (S, G) in enumerate(SHAPES):
            geom, smp, _, _, _ = sample_case(S, G, world)
            base, tp, tl = _base(geom), _tp_kw(smp), smp["tlatent"]
            Slice, Mask = _t(smp["Slice"]), _t(smp["Mask"])
            call = _call_args(geom, smp, Slice, Mask)
            for kw in DEFINITIONS + ({"use_phase_types": False},):
                tag = (S, G, tuple(kw))
                ref, net = _pair(7 + si, **kw)
                ref.set_adjacencies_base(*base, tlatent=_t(tl), time_pointers=tp)
                net.set_adjacencies_base(*base)
                # ---- through the class: the rank's own rows only, as a ShardRows or a callable over source-node ids
                forms = {"ShardRows": lambda: net.node_rows(tl.reshape(G, S, 2))}
                if not kw and si == 0:
                    forms["callable"] = lambda: (lambda ids: tl.reshape(G, S, 2)[ids])
                    forms["callable, flat rows"] = lambda: (lambda ids: _t(tl.reshape(G, S, 2)[ids].reshape(-1, 2)))
                    forms["max_t=None"] = lambda: net.node_rows(tl)
                    # the whole table, cut down to the rank's rows by the shard itself (`ShardedPath.time_pointers`)
                    for what, whole in (("whole [P, 2] on the device", _t(tl)), ("whole [P, 2] on the host", torch.from_numpy(tl))):
                        ep, es, dtp, own = net._shard.time_pointers(whole, **tp)
                        res[("form", tag, what)] = (torch.equal(ep, ref.A_edges_p) and torch.equal(es, ref.A_edges_s)
                                                    and np.array_equal(dtp, ref.dt_partition) and own.own_only
                                                    and torch.equal(own.t, _t(tl)[net._shard.row_index(own_only=True)]))
                for what, form in forms.items():
                    tpw = dict(tp, max_t=None) if what == "max_t=None" else tp
                    net.set_adjacencies_base(*base, tlatent=form(), time_pointers=tpw)
                    want = ref if what != "max_t=None" else None
                    if want is None:
                        want = _pair(7, **kw)[0]
                        want.set_adjacencies_base(*base, tlatent=_t(tl), time_pointers=tpw)
                    own = net.tlatent
                    res[("form", tag, what)] = (torch.equal(net.A_edges_p, want.A_edges_p) and torch.equal(net.A_edges_s, want.A_edges_s)
                                                and np.array_equal(net.dt_partition, want.dt_partition)
                                                and isinstance(own, gdist.ShardRows) and own.own_only
                                                and tuple(own.shape) == (net.shard_plan.n_own * S, 2)
                                                and torch.equal(own.t, _t(tl)[net._shard.row_index(own_only=True)]))
                net.set_adjacencies_base(*base, tlatent=net.node_rows(tl), time_pointers=tp)
                res[("host tables", tag)] = _tables_equal((net.A_edges_p, net.A_edges_s, net.dt_partition),
                                                          graph.time_pointers(tl.reshape(G, S, 2), **tp))
                # ---- the four outputs
                variant = "use_updated_model_definition" in kw or "use_absolute_pos" in kw
                fixed = (lambda *c: net._sharded_four_outputs(*c[:5], *c[6:])) if variant else net.forward_fixed
                want = [o.clone() for o in ref.forward_fixed(*call)]
                net._shard.local.ws.fill_(255)                                          # NaN-poisoned workspace
                res[("fixed", tag)] = _same(fixed(*call), want)
                res[("nontrivial", tag)] = want[2].shape[1] > 0 and float(want[2].abs().max()) > 0 and float(want[3].abs().max()) > 0
                none = slice(0, 0)                                                      # a window without picks
                got, w0 = fixed(*_call_args(geom, smp, Slice, Mask, none)), ref.forward_fixed(*_call_args(geom, smp, Slice, Mask, none))
                res[("no picks", tag)] = _same(got, w0) and tuple(got[2].shape) == (3, 0, 1)
                if si != 0 or "use_phase_types" in kw or variant:
                    continue
                # `forward`: the graphs passed per call (22 arguments), the tables and this rank's travel-time rows with them
                A_in_sta, A_in_src, A_src_in_prod, A_src_in_sta = graph.cartesian_product_edges(geom.A_sta_sta, geom.A_src_src, S, G)
                ea = graph.GraphEdges(x=_t(geom.edge_attr()), edge_index=A_src_in_prod.to(DEV))
                adj = (A_in_sta.to(DEV), A_in_src.to(DEV), ea, ea, A_src_in_sta.to(DEV), torch.from_numpy(geom.A_src_src).to(DEV),
                       net.A_edges_p, net.A_edges_s, net.dt_partition, net.tlatent)
                fwd = _pair(7 + si, **kw)[1]
                ok = True
                for _ in range(2):                                                      # the build, then the cached graphs
                    ok = ok and _same(fwd.forward(Slice, Mask, *adj, *call[2:]), want)
                res[("forward", tag)] = ok
                if kw:
                    continue
                # caller-supplied tables of the whole graph keep working as they did
                net.set_adjacencies_base(*base, A_edges_p=ref.A_edges_p.long(), A_edges_s=ref.A_edges_s.long(), dt_partition=ref.dt_partition,
                                         tlatent=_t(tl))
                res["whole-graph tables"] = _same(net.forward_fixed(*call), want)
                # what stays refused names itself
                refused = {}
                net.set_adjacencies_base(*base, tlatent=net.node_rows(tl), time_pointers=tp)
                for what, fn in (("train", lambda: net.train().forward_fixed(*call)),
                                 ("use_subgraph", lambda: net.set_adjacencies_subgraph_from_positions(_t(geom.locs), _t(geom.x_grid))),
                                 ("window_batch", lambda: setattr(net, "window_batch", 2))):
                    try:
                        with torch.enable_grad():
                            fn()
                        refused[what] = "no error"
                    except NotImplementedError as e:
                        refused[what] = str(e)
                    net.eval()
                res["refused"] = refused
        # through the caller: the association pass on a sharded leg set up from the rank's rows, against one GPU
        from tests.test_day_loops_gpu import _Setup
        s = _Setup()
        net = _pair(3)[1]
        net.load_state_dict({k: v.clone() for k, v in s.w.items()}, strict=True)
        base = (torch.from_numpy(s.A_sta_sta), torch.from_numpy(s.geom_all.A_src_src), _t(s.ea), _t(s.locs), _t(s.geom_all.x_grid))
        net.set_adjacencies_base(*base)                                                     # (the shard plan: node_rows needs it)
        net.set_adjacencies_base(*base, tlatent=net.node_rows(s.trv_use), time_pointers=dict(max_t=s.max_t, dt=s.sig / 5.0, k=10, win=2.0 * s.sig))
        res["associate tables"] = (np.array_equal(net.A_edges_p.cpu().numpy(), np.asarray(s.A_edges_p)) and
                                   np.array_equal(net.A_edges_s.cpu().numpy(), np.asarray(s.A_edges_s)))
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
    res["associate shape"] = (int(p0[0].numel()) > 0 and float(p0[0].abs().max()) > 0)


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
    if world > 1:                                              # conditions on the inputs, before anything is spawned
        assert cross_rank_ties_at_k("ties", world) > 0
        for S, G in SHAPES:
            _, _, _, ps, owners = sample_case(S, G, world)
            assert_case_exercises_the_exchange(ps, owners)
    ret = mp.Manager().dict()
    spawn_with_limit(_worker, (world, _free_port(), backend, ret), world, 240.0)
    assert len(ret) == world
    return [ret[r] for r in range(world)]


def _all_ranks(world):
    return _ranks(world) if world > 1 else _ranks(1, "nccl")


@pytest.mark.parametrize("world", [1, 2, 3])
def test_tables_equal_the_host_and_the_unsharded_builder_on_every_rank(world):
    """Fails without the feature: `dist.shard_time_pointers` and its two kernels do not exist."""
    for rank, r in enumerate(_all_ranks(world)):
        for name, (_, _, _, _, worlds) in CASES.items():
            if world in worlds:
                for agreed in (False, True):                    # max_t given; max_t=None = the maximum over all ranks
                    assert r[("tables", name, agreed)], (rank, name, "max_t=None" if agreed else "max_t given")


@pytest.mark.parametrize("world", [1, 2, 3])
def test_time_pointers_on_a_shard_from_the_ranks_own_rows(world):
    """Fails on the parent with NotImplementedError: "time_pointers= (the association heads' tables) is not available on a
    source-node-sharded model"."""
    for rank, r in enumerate(_all_ranks(world)):
        tag = SHAPES[0] + ((),)
        for what in ("ShardRows", "callable", "callable, flat rows", "max_t=None", "whole [P, 2] on the device", "whole [P, 2] on the host"):
            assert r[("form", tag, what)], (rank, what)
        for S, G in SHAPES:
            for kw in DEFINITIONS:
                assert r[("form", (S, G, tuple(kw)), "ShardRows")] and r[("host tables", (S, G, tuple(kw)))], (rank, S, G, kw)


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("definition", ["default", "use_updated_model_definition", "use_absolute_pos", "use_phase_types"])
def test_four_outputs_bit_equal_to_the_unsharded_model(world, definition):
    """Tables built from owned rows only, the travel time of every listed row from its owner. The two other model definitions behind the
    public guard: the sharded heads add the static terms of the unsharded `genie_assoc_fwd`, bit for bit."""
    key = () if definition == "default" else (definition,)
    for rank, r in enumerate(_all_ranks(world)):
        for S, G in SHAPES:
            tag = (S, G, key)
            assert r[("nontrivial", tag)], (rank, tag)
            assert r[("fixed", tag)], (rank, tag)
            assert r[("no picks", tag)], (rank, tag)
        if definition in ("default",):
            assert r[("forward", SHAPES[0] + (key,))], (rank, definition, "forward (22 arguments)")


@pytest.mark.parametrize("world", [1, 2, 3])
def test_callers_and_whole_graph_tables(world):
    for rank, r in enumerate(_all_ranks(world)):
        assert r["whole-graph tables"], (rank, "caller-supplied tables of the whole product graph")
        assert r["associate tables"], rank
        assert r["associate shape"], rank
        assert r["associate"], (rank, "associate_sources on a sharded leg != the unsharded leg")


def test_refusals_kept():
    for r in _ranks(2):
        got = r["refused"]
        for what, word in (("train", "training step"), ("use_subgraph", "use_subgraph"), ("window_batch", "window_batch")):
            assert word in got[what], (what, got[what])
        for what in ("train", "use_subgraph", "window_batch"):      # ... and does not speak of time_pointers=, which a shard now builds
            assert "time_pointers" not in got[what], (what, got[what])


@pytest.mark.parametrize("world", [2, 3])
def test_a_nan_on_one_rank_raises_on_every_rank(world):
    for rank, r in enumerate(_ranks(world)):
        assert "finite" in r["nan"] and "rank(s) 1" in r["nan"], (rank, r["nan"])
