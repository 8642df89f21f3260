"""GPU: the source-node-sharded path (genie_amd/dist.py) through its real schedule -- sub-range stage launches, the halo
all-to-all on the communication stream, all-gather, replicated tail -- with one process per rank.

* two processes sharing ONE GPU over gloo (host-staged transport): every kernel launch, stream dependency and buffer of the
  multi-GPU schedule runs for real; only the collective itself is not RCCL. Runs on the 1-GPU test box.
* two processes on two GPUs over RCCL ("nccl"): skipped unless the box has >= 2 GPUs.
* ONE process with a world-size-1 RCCL group: the device-collective branch of `Transport` (`all_to_all_single` with explicit
  split sizes received into a view of the workspace, `all_gather_into_tensor`) and the overlapped schedule with its
  communication / tail streams execute over RCCL itself on the 1-GPU box.
Both compare every rank's result with the unsharded HIP path bit for bit, with the overlap schedule on and off.

The `*_drop_in_*` tests run the same three process layouts THROUGH THE DROP-IN CLASS (`GCN_Detection_Network_extended(...,
process_group=True)`): the reference's `set_adjacencies(12 arguments)` once, `forward_fixed_source(Slice, Mask, ...)` with the full
`[P, 4]` tensors per window (module.py:941-961, :999-1020; called at process_continuous_days.py:634, :797), the device embedding of the
rank's own rows (`embed_window` / `node_rows`) and the whole apply loop (`apply.apply_windows_device`) -- `(y, x)` and `Out_2` bit-equal
to the unsharded class on every rank.
"""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, backend, same_gpu, ret):
    import torch.distributed as dist
    from genie_amd import dist as gdist
    from genie_amd import engine, synthetic
    from tests.util import Case
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = "cuda:0" if same_gpu else "cuda:%d" % rank
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(dev))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        S, G = 40, 900
        geom = synthetic.Geometry(S, G, L=200e3, n_query=20, seed=41)
        wins = [synthetic.make_window(geom, 400, seed=42, window=k) for k in range(3)]
        wd = {k: v.to(dev) for k, v in Case("odd_33x257").weights.items()}
        ea = torch.from_numpy(geom.edge_attr())
        pos = torch.from_numpy(geom.x_grid).float().to(dev)
        sta_csr = engine.csr_from_edges(torch.from_numpy(geom.A_sta_sta), S)
        hp = engine.HipPath(S, G, sta_csr, engine.csr_from_edges(torch.from_numpy(geom.A_src_src), G),
                            grid_order=engine.sfc_order(geom.x_grid), device=dev, sta_order=engine.sfc_order(geom.locs))
        hp.set_weights(wd)
        refs = [hp.path_fwd(torch.from_numpy(w["Slice"]).to(dev), torch.from_numpy(w["Mask"]).to(dev), ea.to(dev), pos)[0].clone()
                for w in wins]
        res = {}
        for overlap in (True, False, "p2p"):     # "p2p": the overlapped schedule with the halo bucketed by destination (one send / receive pair per peer)
            sp = gdist.ShardedPath(S, G, sta_csr, geom.A_src_src, geom.x_grid, world, rank, dev, pos_sta=geom.locs, overlap=bool(overlap),
                                   halo="p2p" if overlap == "p2p" else "a2a")
            sp.set_weights(wd)
            p = sp.plan
            ext = torch.from_numpy(p.ext_global)
            rows = (ext.view(-1, 1) * S + torch.arange(S).view(1, -1)).reshape(-1)
            own_rows = rows[: p.n_own * S]
            sp.local.ws.fill_(255)                                       # NaN-poisoned workspace
            outs = []
            for w in wins:                                               # plain: everything on the current stream
                outs.append(sp.path_fwd(torch.from_numpy(w["Slice"])[rows].to(dev), torch.from_numpy(w["Mask"])[rows].to(dev),
                                        ea[own_rows].to(dev), pos))
            torch.cuda.synchronize()
            ok_plain = all(torch.equal(o, r) for o, r in zip(outs, refs))
            outs = []
            for w in wins:                                               # pipelined: all-gather + tail on the tail stream
                outs.append(sp.path_fwd(torch.from_numpy(w["Slice"])[rows].to(dev), torch.from_numpy(w["Mask"])[rows].to(dev),
                                        ea[own_rows].to(dev), pos, pipelined=True))
            sp.wait_tail()
            torch.cuda.synchronize()
            ok_piped = all(torch.equal(o, r) for o, r in zip(outs, refs))
            res[overlap] = (ok_plain, ok_piped)
            if overlap is True:
                res["plan"] = (p.n_own, p.n_halo, p.r_send, p.r_need)
        ret[rank] = res
    finally:
        dist.destroy_process_group()


def _run(world, backend, same_gpu):
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), backend, same_gpu, ret), nprocs=world, join=True)
    assert len(ret) == world
    for rank in range(world):
        r = ret[rank]
        n_own, n_halo, r_send, r_need = r["plan"]
        assert n_halo > 0 and r_send[1] > 0 and r_need[1] > r_need[0]
        assert r_need[1] < n_own, "the test geometry must leave interior nodes for the overlapped stage-2 launch"
        assert r[True] == (True, True), (rank, "overlapped schedule", r[True])
        assert r[False] == (True, True), (rank, "sequential schedule", r[False])
        assert r["p2p"] == (True, True), (rank, "halo bucketed by destination", r["p2p"])


def test_sharded_path_two_processes_on_one_gpu_match_unsharded():
    _run(2, "gloo", True)


def test_sharded_path_three_processes_on_one_gpu_match_unsharded():
    _run(3, "gloo", True)


def test_sharded_path_world2_rccl_matches_unsharded():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL over xGMI); the 1-GPU box runs the gloo form above")
    _run(2, "nccl", False)


def _worker_world1_rccl(rank, port, ret):
    import torch.distributed as dist
    from genie_amd import dist as gdist
    from genie_amd import engine, synthetic
    from tests.util import Case
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = "cuda:0"
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(dev))
    try:
        S, G = 40, 900
        geom = synthetic.Geometry(S, G, L=200e3, n_query=20, seed=41)
        wins = [synthetic.make_window(geom, 400, seed=42, window=k) for k in range(3)]
        wd = {k: v.to(dev) for k, v in Case("odd_33x257").weights.items()}
        ea = torch.from_numpy(geom.edge_attr()).to(dev)
        pos = torch.from_numpy(geom.x_grid).float().to(dev)
        sta_csr = engine.csr_from_edges(torch.from_numpy(geom.A_sta_sta), S)
        hp = engine.HipPath(S, G, sta_csr, engine.csr_from_edges(torch.from_numpy(geom.A_src_src), G),
                            grid_order=engine.sfc_order(geom.x_grid), device=dev, sta_order=engine.sfc_order(geom.locs))
        hp.set_weights(wd)
        refs = [hp.path_fwd(torch.from_numpy(w["Slice"]).to(dev), torch.from_numpy(w["Mask"]).to(dev), ea, pos)[0].clone() for w in wins]
        res = {}
        for overlap in (True, False):
            sp = gdist.ShardedPath(S, G, sta_csr, geom.A_src_src, geom.x_grid, 1, 0, dev, pos_sta=geom.locs, overlap=overlap)
            sp.set_weights(wd)
            res["device_collectives"] = bool(sp.transport.on and sp.transport.device_collectives)
            p = sp.plan
            rows = (torch.from_numpy(p.ext_global).view(-1, 1) * S + torch.arange(S).view(1, -1)).reshape(-1)
            sp.local.ws.fill_(255)
            ok = True
            for piped in (False, True):
                outs = [sp.path_fwd(torch.from_numpy(w["Slice"])[rows].to(dev), torch.from_numpy(w["Mask"])[rows].to(dev),
                                    ea[rows.to(dev)], pos, pipelined=piped) for w in wins]
                sp.wait_tail()
                torch.cuda.synchronize()
                ok = ok and all(torch.equal(o, r) for o, r in zip(outs, refs))
            res[overlap] = ok
            # the transport itself with data: this rank's rows sent to itself with explicit split sizes, received IN PLACE into a
            # view of the workspace's wv region on the communication stream; all-gather of a padded per-node tensor
            wv = sp.wv_view()
            n = 7 * S
            send = torch.randn((7, S * sp._pitch), device=dev)
            with torch.cuda.stream(sp.comm_stream):
                recv = wv[:n].view(7, S * sp._pitch)
                sp.transport.all_to_all_rows(recv, send, [7], [7])
                buf = send.new_empty((1, 7, S * sp._pitch))
                sp.transport.all_gather_rows(buf, send)
            sp.comm_stream.synchronize()
            res["transport_%s" % overlap] = bool(torch.equal(wv[:n].reshape(7, -1), send) and torch.equal(buf[0], send))
        ret[0] = res
    finally:
        dist.destroy_process_group()


def test_sharded_path_world1_rccl_device_collectives():
    """RCCL executes the sharded path's collectives (world size 1: the only form one GPU allows; RCCL refuses two ranks on one
    device): same kernels, streams and buffers as N > 1, bitwise equal to the unsharded path."""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker_world1_rccl, args=(_free_port(), ret), nprocs=1, join=True)
    r = ret[0]
    assert r["device_collectives"], "the nccl (RCCL) process group must select the device-collective transport"
    assert r[True] and r[False], r
    assert r["transport_True"] and r["transport_False"], r


# ---- the sharded path behind the reference's interface (row e-b) -------------------------------------------------------------------------

def _drop_in_body(rank, world, dev, res):
    """Unsharded vs sharded drop-in model on this rank: the reference's call sequence, then the device embedding and the apply loop."""
    import torch.distributed as dist
    from genie_amd import apply, dist as gdist, graph, module, synthetic
    from tests.util import Case
    S, G = 40, 900
    geom = synthetic.Geometry(S, G, L=200e3, n_query=20, seed=41)
    wins = [synthetic.make_window(geom, 400, seed=42, window=k) for k in range(3)]
    c = Case("o1_20x500")            # weights with O(1) outputs
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(dev)
    A_in_sta, A_in_src, A_src_in_prod, A_src_in_sta = graph.cartesian_product_edges(geom.A_sta_sta, geom.A_src_src, S, G)
    ea = graph.GraphEdges(x=t(geom.edge_attr()), edge_index=A_src_in_prod.to(dev))
    locs, xg, xq, tq = t(geom.locs), t(geom.x_grid), t(geom.x_query), t(geom.t_query)
    adj = (A_in_sta.to(dev), A_in_src.to(dev), ea, ea, A_src_in_sta.to(dev), torch.from_numpy(geom.A_src_src).to(dev), None, None, None, None,
           locs, xg)

    def make(**kw):
        net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=dev, **kw)
        net.load_state_dict({k: v.clone() for k, v in c.weights.items()})
        return net.eval()

    ref_net = make()
    ref_net.set_adjacencies(*adj)                                                   # process_continuous_days.py:634
    with torch.no_grad():
        refs = [ref_net.forward_fixed_source(t(w["Slice"]), t(w["Mask"]), None, None, None, locs, xg, xq, tq) for w in wins]   # :797
        refs = [(y.clone(), x.clone()) for y, x in refs]
    assert float(refs[0][0].abs().max()) > 0.05
    # the apply loop's reference: the unsharded model, one tail per window
    P = synthetic.make_picks(geom, 900, seed=72)
    P[:, 0] = P[:, 0] * 0.25 + 5000.0
    P = P[np.argsort(P[:, 0], kind="stable")]
    trv = geom.travel_times().astype(np.float32)
    max_t = float(np.ceil(trv.max() + 1.0))
    Out_ref, times_ref = apply.apply_windows_device(ref_net, geom, P, trv, min_required_picks=5, max_t=max_t, tail_batch=1)
    torch.cuda.synchronize()
    for overlap, halo in ((True, "a2a"), (False, "a2a"), (True, "p2p")):
        net = make(process_group=True, shard_overlap=overlap, shard_halo=halo)
        assert net.is_sharded and net.shard_plan is None
        net.set_adjacencies(*adj)                                                   # the same 12 arguments
        p = net.shard_plan
        assert (p.rank, p.world) == (rank, world) and p.n_own == len(p.own_global) > 0
        net._shard.local.ws.fill_(255)                                              # NaN-poisoned workspace
        ok = True
        with torch.no_grad():
            for w, (y0, x0) in zip(wins, refs):                                     # full [P, 4] tensors, as the reference hands them over
                y, x = net.forward_fixed_source(t(w["Slice"]), t(w["Mask"]), None, None, None, locs, xg, xq, tq)
                ok = ok and torch.equal(y, y0) and torch.equal(x, x0)
            outs = [net.forward_fixed_source_pipelined(t(w["Slice"]), t(w["Mask"]), None, None, None, locs, xg, xq, tq) for w in wins]
            net._hip.wait_tails()
            torch.cuda.synchronize()
            ok_piped = all(torch.equal(y, y0) and torch.equal(x, x0) for (y, x, _), (y0, x0) in zip(outs, refs))
            # rows in the rank's local form (what embed_window produces): accepted as they are
            rows = net._shard.row_index()
            w = wins[1]
            y, x = net.forward_fixed_source(gdist.ShardRows(t(w["Slice"])[rows]), gdist.ShardRows(t(w["Mask"])[rows]), None, None, None,
                                            locs, xg, xq, tq)
            ok_local = torch.equal(y, refs[1][0]) and torch.equal(x, refs[1][1])
        # the apply loop: this rank embeds its owned + halo rows only
        Out, times = apply.apply_windows_device(net, geom, P, trv, min_required_picks=5, max_t=max_t)
        torch.cuda.synchronize()
        ok_apply = np.array_equal(times, times_ref) and len(times) >= 3 and torch.equal(Out, Out_ref)
        # what stays unsharded says so
        raised = 0
        for call in (lambda: net.forward_fixed(t(w["Slice"]), t(w["Mask"]), None, None, None, locs, xg, xq, xq[:2], tq, None, None),
                     lambda: net.push_window(t(w["Slice"]), t(w["Mask"]))):
            try:
                call()
            except NotImplementedError:
                raised += 1
        res[(overlap, halo)] = (ok, ok_piped, ok_local, ok_apply, raised == 2, float(Out_ref.abs().max()) > 0)
        if dist.is_initialized():
            dist.barrier()
    res["plan"] = (p.n_own, p.n_halo)
    res["device_collectives"] = bool(net._shard.transport.on and net._shard.transport.device_collectives)


def _worker_drop_in(rank, world, port, backend, same_gpu, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = "cuda:0" if same_gpu else "cuda:%d" % rank
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(dev))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = {}
        _drop_in_body(rank, world, dev, res)
        ret[rank] = res
    finally:
        dist.destroy_process_group()


def _run_drop_in(world, backend, same_gpu):
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker_drop_in, args=(world, _free_port(), backend, same_gpu, ret), nprocs=world, join=True)
    assert len(ret) == world
    for rank in range(world):
        r = ret[rank]
        if world > 1:
            assert r["plan"][1] > 0
        for k in ((True, "a2a"), (False, "a2a"), (True, "p2p")):
            assert r[k] == (True,) * 6, (rank, k, r[k], "(full inputs, pipelined, local rows, apply loop, unsharded calls raise, non-trivial)")
    return ret


def test_drop_in_class_two_processes_on_one_gpu_bit_equal_to_unsharded():
    _run_drop_in(2, "gloo", True)


def test_drop_in_class_three_processes_on_one_gpu_bit_equal_to_unsharded():
    _run_drop_in(3, "gloo", True)


def test_drop_in_class_world1_rccl_bit_equal_to_unsharded():
    ret = _run_drop_in(1, "nccl", True)
    assert ret[0]["device_collectives"], "the nccl (RCCL) process group must select the device-collective transport"


def test_drop_in_class_world2_rccl_bit_equal_to_unsharded():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL over xGMI); the 1-GPU box runs the gloo form above")
    _run_drop_in(2, "nccl", False)


def test_bench_n_ranks_control_flow_over_gloo_on_one_gpu():
    """`python bench.py --gpus 2` end to end on the 1-GPU box (`--backend gloo`: the ranks share the GPU, collectives staged through the
    host; timings meaningless and labelled so): the launcher, the drop-in class on every rank, the max-over-ranks timing, and the
    one-GPU leg rank 0 runs AFTER the sharded run under the launcher -- which, with a second rendezvous through `init_method="tcp://"`,
    made rank 0 a client of the launcher's agent store and hung for ten minutes (round 6; no N > 1 run had ever reached that line)."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "2", "--backend", "gloo", "--config", "cfg2_200x10k", "--steps", "3",
                        "--warmup", "1", "--full"], cwd=repo, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "strong" and d["unit"] == "picks/s"
    assert "FUNCTIONAL CHECK ONLY" in d["config"]["backend"] and d["config"]["rccl_ranks"] == 0
    assert d["config"]["rank0_plan"]["n_own"] == 5000 and d["config"]["rank0_plan"]["n_halo"] > 0
    assert "forward_fixed_source_pipelined" in d["config"]["entry_point"]
    one = d["one_gpu_same_config"]
    assert "error" not in one and one["ms_per_step"] > 0 and one["value"] > 0 and 0 < one["scaling_efficiency"]
