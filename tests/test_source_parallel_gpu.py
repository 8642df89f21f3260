"""GPU: the source-parallel refine and association passes (`source_parallel=` of apply.refine_sources / associate_sources /
detect_refine_associate) against the same passes on one GPU, on the small day of tests/test_day_loops_gpu.py.

* tuple form, every rank in this process (worlds 1, 2, 3, 5; 5 ranks over 4 sources leave a block empty): the ranks' rows side by side
  are the one-GPU rows bit for bit, every rank consumes the random stream of one GPU;
* group form with one process per rank: gloo on one GPU (2 and 3 ranks) and a one-rank RCCL group: every rank's dict equals the one-GPU
  dict entry by entry;
* a source-sharded model is refused."""
import datetime
import functools
import os
import socket
import time
import types

import numpy as np
import pytest
import torch

from genie_amd import apply, module
from tests.test_day_loops_gpu import _Setup

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDENT = lambda x: x                                                                        # noqa: E731
RANGES = ((0.0, 60e3), (0.0, 60e3), (-40e3, 2e3))
OFF_MIN, OFF_RNG = np.array([[-5e3, -5e3, -3e3]]), np.array([[10e3, 10e3, 6e3]])
N_QUERY = 300


@functools.lru_cache(maxsize=None)
def _setup():
    return _Setup()


class _CountedRand(object):
    def __init__(self, seed):
        self.rs, self.calls = np.random.RandomState(seed), 0

    def __call__(self, *shape):
        self.calls += 1
        return self.rs.rand(*shape)


def _candidates(s):
    """The six candidates of test_refine_pass_matches_the_oracle_chain: four near events, one in a quiet stretch (no pick: no leg
    produces a window), one at the region's corner (part of its cloud is masked)."""
    rng = np.random.default_rng(5)
    nodes = rng.choice(s.G, 4, replace=False)
    srcs = np.concatenate((s.geom_all.x_grid[nodes], rng.uniform(6995.0, 7010.0, (4, 1)), np.full((4, 1), 0.5)), axis=1)
    return np.concatenate((srcs, [[20e3, 30e3, -5e3, 30000.0, 0.5]], [[500.0, 59.6e3, 1500.0, 7002.0, 0.5]]), axis=0)


def _refine(s, srcs, rand, **kw):
    return apply.refine_sources([s.leg], s.picks, srcs, s.locs, s.tq, s.max_t, OFF_MIN, OFF_RNG, N_QUERY, IDENT, IDENT, *RANGES,
                                kernel_sig_t=s.sig, dt_embed=s.dt, rand=rand, ftrns2_device=IDENT, **kw)


@functools.lru_cache(maxsize=None)
def _one_gpu_refined(n):
    s = _setup()
    srcs = _candidates(s)[:n]
    rows, block = _refine(s, srcs, _CountedRand(77), source_parallel=(0, 1))          # world 1: all rows, as one GPU computes them
    assert block == (0, n) and rows.shape == (n, 7)
    ref, order = _refine(s, srcs, _CountedRand(77))
    return srcs, rows, ref, order


def _trv_out(s, ref):
    d = np.linalg.norm(ref[:, None, 0:3] - s.locs[None, :, :], axis=2)
    return np.stack((d / 6000.0, d / 3500.0), axis=2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _one_gpu_associated(n):
    s = _setup()
    ref = _one_gpu_refined(n)[2]
    return apply.associate_sources([s.leg], s.picks, ref, s.locs, s.tq, s.max_t, _trv_out(s, ref), IDENT, np.array([1000.0, 2000.0, 0.0]),
                                   kernel_sig_t=s.sig, dt_embed=s.dt)


@pytest.mark.parametrize("n,world", [(6, 1), (6, 2), (6, 3), (6, 5), (4, 5)])
def test_refine_rows_of_the_ranks_are_the_one_gpu_rows(n, world):
    s = _setup()
    srcs, rows_1, ref, order = _one_gpu_refined(n)
    assert rows_1[:, 3].all() and len(np.unique(rows_1[:, 0])) > 1
    blocks = apply.window_blocks(n, world)
    parts = []
    for r in range(world):
        rand = _CountedRand(77)
        rows, block = _refine(s, srcs, rand, source_parallel=(r, world))
        assert block == blocks[r] and rows.shape == (block[1] - block[0], 7) and rows.dtype == np.float64
        assert rand.calls == n                                             # the whole stream, whatever the block
        parts.append(rows)
    if world > n:
        assert any(p.shape[0] == 0 for p in parts)
    found = np.concatenate(parts)
    assert found.tobytes() == rows_1.tobytes()
    got, got_order = apply.refined_from_found(found, srcs, s.tq, IDENT)
    assert np.array_equal(got, ref) and np.array_equal(got_order, order)


@pytest.mark.parametrize("n,world", [(4, 1), (4, 2), (4, 3), (4, 5), (6, 3)])
def test_association_blocks_of_the_ranks_are_the_one_gpu_lists(n, world):
    s = _setup()
    ref = _one_gpu_refined(n)[2]
    Op, Os, Sp, Lm = _one_gpu_associated(n)
    assert len(Op) == n and sum(int(o.numel() > 0) for o in Op) >= 2
    assert n < 6 or any(o.numel() == 0 for o in Op)                      # the quiet candidate: a window without picks
    blocks = apply.window_blocks(n, world)
    got_p, got_s = [], []
    for r in range(world):
        p, q, sp, lm, block = apply.associate_sources([s.leg], s.picks, ref, s.locs, s.tq, s.max_t, _trv_out(s, ref), IDENT,
                                                      np.array([1000.0, 2000.0, 0.0]), kernel_sig_t=s.sig, dt_embed=s.dt,
                                                      source_parallel=(r, world))
        assert block == blocks[r] and len(p) == len(q) == block[1] - block[0]
        assert len(sp) == len(lm) == n                                      # the pick lists of every source, on every rank
        for i in range(n):
            assert np.array_equal(sp[i], Sp[i]) and np.array_equal(lm[i], Lm[i])
        got_p += p
        got_s += q
    assert len(got_p) == n
    for i in range(n):
        assert got_p[i].is_cuda and torch.equal(got_p[i], Op[i]) and torch.equal(got_s[i], Os[i])


def _chain(s, **kw):
    """The day of test_detection_to_association_chain_matches_its_steps through `detect_refine_associate`."""
    rng = np.random.default_rng(23)
    Q, dt_win, src_t_kernel, thresh = 150, 0.75, 5.0, 0.15
    xq = np.c_[rng.uniform(0, 60e3, (Q, 2)), rng.uniform(-30e3, 0, Q)]
    ts = 6990.0 + np.arange(400) * dt_win
    out = np.zeros((Q, len(ts)), dtype=np.float32)
    far = int(np.argmax(np.linalg.norm(xq - xq[3], axis=1)))
    for c, t0 in [(xq[3], 7001.0), (xq[3] + [2e3, 0, 0], 7002.5), (xq[far], 7011.0), (xq[90], 7100.0), (xq[91], 7190.0)]:
        d = np.linalg.norm((xq - c) * np.array([1, 1, 0.3]), axis=1)
        out += (0.7 * np.exp(-0.5 * (d / 12e3) ** 2)[:, None] * np.exp(-0.5 * ((ts - t0) / 3.0) ** 2)[None, :]).astype(np.float32)
    Out_2 = torch.from_numpy(out).to(s.leg.device)

    def trv(locs, srcs):
        d = torch.linalg.norm(locs[None, :, :] - srcs[:, None, :], dim=2)
        return torch.stack((d / 6000.0, d / 3500.0), dim=2)

    got = apply.detect_refine_associate([s.leg], s.picks, Out_2, xq, ts, s.locs, trv, s.tq, s.max_t, IDENT, IDENT, *RANGES, OFF_MIN, OFF_RNG,
                                        200, thresh, src_t_kernel, dt_win, src_t_kernel * 3.0, src_t_kernel * 1.35, 20e3,
                                        rand=np.random.RandomState(3).rand, ftrns2_device=IDENT, kernel_sig_t=s.sig, dt_embed=s.dt, **kw)
    torch.cuda.synchronize()
    return {"srcs": got["srcs"], "srcs_refined": got["srcs_refined"], "trv_out_srcs": got["trv_out_srcs"].cpu().numpy(),
            "Out_p_save": [o.cpu().numpy() for o in got["Out_p_save"]], "Out_s_save": [o.cpu().numpy() for o in got["Out_s_save"]],
            "Save_picks": got["Save_picks"], "lp_meta": got["lp_meta"]}


@functools.lru_cache(maxsize=None)
def _one_gpu_chain():
    return _chain(_setup())


def _same_dict(got, want):
    assert sorted(got) == sorted(want)
    for key, w in want.items():
        if isinstance(w, list):
            assert len(got[key]) == len(w), key
            for a, b in zip(got[key], w):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key
        else:
            assert got[key].dtype == w.dtype and got[key].shape == w.shape and got[key].tobytes() == w.tobytes(), key


def test_chain_with_a_world_of_one_equals_the_plain_chain():
    want = _one_gpu_chain()
    assert len(want["srcs"]) >= 3 and len(want["Out_p_save"]) >= 2 and sum(o.size > 0 for o in want["Out_p_save"]) >= 2
    _same_dict(_chain(_setup(), source_parallel=(0, 1)), want)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, backend, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(DEV)
    timeout = datetime.timedelta(seconds=60)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(DEV), timeout=timeout)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timeout)
    try:
        ret[rank] = (_chain(_Setup(), source_parallel=True), dist.get_backend())
    finally:
        dist.destroy_process_group()


def _run_group(world, backend, limit=240.0):
    import torch.multiprocessing as mp
    want = _one_gpu_chain()
    mgr = mp.Manager()
    ret = mgr.dict()
    ctx = mp.spawn(_worker, args=(world, _free_port(), backend, ret), nprocs=world, join=False)
    deadline = time.monotonic() + limit
    try:
        while not ctx.join(timeout=5.0):                  # returns as soon as a rank ends; raises what a rank raised
            assert time.monotonic() < deadline, "a rank of the %s group of %d is stuck" % (backend, world)
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
            p.join(10.0)
    assert len(ret) == world
    for rank in range(world):
        got, be = ret[rank]
        assert be == backend
        _same_dict(got, want)


def test_chain_two_processes_on_one_gpu_over_gloo():
    _run_group(2, "gloo")


def test_chain_three_processes_on_one_gpu_over_gloo():
    _run_group(3, "gloo")


def test_chain_world1_rccl_gathers_on_the_device():
    _run_group(1, "nccl")


def test_source_parallel_on_a_sharded_model_is_refused():
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV, shard=(0, 2))
    assert net.is_sharded
    s = _setup()
    legs = [types.SimpleNamespace(net=net, device=torch.device(DEV))]
    with pytest.raises(NotImplementedError, match="source_parallel"):
        _refine(types.SimpleNamespace(leg=legs[0], picks=s.picks, locs=s.locs, tq=s.tq, max_t=s.max_t, sig=s.sig, dt=s.dt),
                _candidates(s), np.random.RandomState(1).rand, source_parallel=(0, 2))
    ref = _one_gpu_refined(4)[2]
    with pytest.raises(NotImplementedError, match="source_parallel"):
        apply.associate_sources(legs, s.picks, ref, s.locs, s.tq, s.max_t, _trv_out(s, ref), IDENT, np.zeros(3), source_parallel=(0, 2))
