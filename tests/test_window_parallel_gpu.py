"""GPU: the fused stacking kernel (genie_stack_windows) and the window-parallel apply loop (`apply_windows_device(stack_on_device=,
window_parallel=)`).

* the fused stacking against the torch stacking it replaces (slice, scaling, `index_add_` per window): `Out_2` bit for bit, over
  step sizes, tail batches, divisors 2 / 3 / 6 / 9, a 1 s stride (many windows per column) and an output axis coarse enough that a window
  lists a column twice; two stacked runs bit-equal to each other;
* 64-bit element offsets into an `Out_2` of more than 2^31 elements;
* window-parallel, tuple form, every rank in this process: the partials summed in rank order against the one-GPU `Out_2` -- bit-equal
  in every column one rank feeds, within a derived rounding bound in the boundary columns, bit-equal everywhere on the default schedule;
* group form with one process per rank: gloo on one GPU (2 and 3 ranks), a one-rank RCCL group (the device all-reduce), two GPUs over
  RCCL when the box has them.
"""
import datetime
import functools
import os
import socket

import numpy as np
import pytest
import torch

from genie_amd import _lib, apply, engine, module, synthetic
from tests.util import Case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OFFSETS = apply.window_schedule([0.0, 100.0], 10.0)[1]          # the nine origin-time offsets of a window


def _net(case, geom, dev):
    c = Case(case)
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=dev)
    net.load_state_dict({k: v.clone() for k, v in c.weights.items()})
    net.eval()
    net.set_adjacencies_base(torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src), torch.from_numpy(geom.edge_attr()).to(dev),
                             torch.from_numpy(geom.locs).float().to(dev), torch.from_numpy(geom.x_grid).float().to(dev))
    return net


@functools.lru_cache(maxsize=None)
def _tiny(dev=DEV):
    """17 stations x 64 source nodes, windows from the default schedule (the set-up of test_device_apply_loop_matches_oracle, the picks
    spread over three times the time so that a run has more windows than one flush of 16)."""
    geom = synthetic.Geometry(17, 64, L=60e3, n_query=12, seed=71)
    P = synthetic.make_picks(geom, 300, seed=72)
    P[:, 0] = P[:, 0] * 0.75 + 5000.0
    P = P[np.argsort(P[:, 0], kind="stable")]
    trv = geom.travel_times().astype(np.float32)
    return _net("tiny_6x40", geom, dev), geom, P, trv, dict(min_required_picks=5, max_t=float(np.ceil(trv.max() + 1.0)))


@functools.lru_cache(maxsize=None)
def _stride(dev=DEV):
    """200 stations, 72 windows at 1 s stride (the set-up of test_config5_stream_200_stations_one_second_stride_matches_oracle_chain)."""
    geom = synthetic.Geometry(200, 150, L=300e3, n_query=40, seed=91)
    rng = np.random.default_rng(92)
    n = 6000
    P = np.stack([np.sort(rng.uniform(20000.0, 20200.0, n)), rng.integers(0, 200, n).astype(np.float64), np.ones(n), np.ones(n),
                  rng.integers(0, 2, n).astype(np.float64)], axis=1)
    trv = geom.travel_times().astype(np.float32)
    max_t = float(np.ceil(trv.max() + 1.0))
    tsteps, offsets, step, n_overlap, dt_win = apply.window_schedule(P[:, 0], max_t, t_win=6.0, step_size="half")
    tsteps_abs = np.arange(tsteps.min() - 3.0, tsteps.max() + 3.0 + dt_win, dt_win)
    kw = dict(tsteps_abs=tsteps_abs, step_size="half", max_t=max_t, kernel_sig_t=1.0, dt_embed=0.1, times=20010.3 + 1.0 * np.arange(72),
              tail_batch=8)
    return _net("cfg1_20x500", geom, dev), geom, P, trv, kw


def _run(setup, **kw):
    net, geom, P, trv, base = setup
    out = apply.apply_windows_device(net, geom, P, trv, **dict(base, **kw))
    torch.cuda.synchronize()
    return out


# ---- fused stacking == torch stacking ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tail_batch", [1, 3, 16])
@pytest.mark.parametrize("step_size", ["full", "partial", "half"])
def test_fused_stacking_is_bit_equal_to_torch_stacking(step_size, tail_batch):
    """n_grids = 3: the divisors are 3 (full), 9 (partial) and 6 (half), for which `x / d` and `x * (1 / d)` differ in fp32."""
    want, times = _run(_tiny(), step_size=step_size, tail_batch=tail_batch, n_grids=3.0)
    got, times_s = _run(_tiny(), step_size=step_size, tail_batch=tail_batch, n_grids=3.0, stack_on_device=True)
    again, _ = _run(_tiny(), step_size=step_size, tail_batch=tail_batch, n_grids=3.0, stack_on_device=True)
    assert len(times) >= (17 if step_size != "full" else 6) and np.array_equal(times, times_s)
    assert float(want.abs().max()) > 0 and bool(torch.isfinite(want).all())
    assert torch.equal(got, want)
    assert torch.equal(again, got)


def test_fused_stacking_default_divisor_two():
    want, _ = _run(_tiny(), tail_batch=4)
    got, _ = _run(_tiny(), tail_batch=4, stack_on_device=True)
    assert float(want.abs().max()) > 0 and torch.equal(got, want)


def test_fused_stacking_one_second_stride_batches_of_eight():
    """72 windows at 1 s stride, flushed 8 at a time: 6-7 windows feed a column, inside one flush and across flushes."""
    want, times = _run(_stride())
    got, _ = _run(_stride(), stack_on_device=True)
    again, _ = _run(_stride(), stack_on_device=True)
    table = apply.window_cols_table(_stride()[4]["tsteps_abs"], times, OFFSETS, True)
    per_col = np.bincount(table[table >= 0])
    assert len(times) == 72 and per_col.max() >= 6
    assert float(want.abs().max()) > 0.02
    assert torch.equal(got, want) and torch.equal(again, got)


@pytest.mark.parametrize("step_size,tail_batch", [("half", 3), ("full", 1), ("partial", 16)])
def test_fused_stacking_with_a_column_listed_twice_in_a_window(step_size, tail_batch):
    """An output axis of 1.5 s spacing under 0.75 s offsets: every window lists columns twice, the loop takes its `keeps` branch and the
    table drops all but the last occurrence."""
    net, geom, P, trv, base = _tiny()
    tsteps, offsets, step, n_overlap, dt_win = apply.window_schedule(P[:, 0], base["max_t"], t_win=6.0, step_size=step_size)
    coarse = np.arange(tsteps.min() - 3.0, tsteps.max() + 3.0 + dt_win, 2.0 * dt_win)
    table = apply.window_cols_table(coarse, tsteps, offsets, step_size == "half")
    assert ((table >= 0).sum(1) < len(offsets) - (1 if step_size == "half" else 0)).all()
    want, _ = _run(_tiny(), step_size=step_size, tail_batch=tail_batch, n_grids=3.0, tsteps_abs=coarse)
    got, _ = _run(_tiny(), step_size=step_size, tail_batch=tail_batch, n_grids=3.0, tsteps_abs=coarse, stack_on_device=True)
    assert float(want.abs().max()) > 0 and torch.equal(got, want)


def test_stack_windows_64_bit_offsets():
    """`Out_2` of 70 000 x 32 768 = 2.29e9 elements (rows 65 536.. lie beyond element 2^31), two overlapping windows at the far end of
    the axis; the touched columns against `index_add_` on a [Q, n_touched] reference, the columns around them untouched."""
    Q, n_cols, T = 70000, 32768, 9
    if torch.cuda.mem_get_info(torch.device(DEV))[0] < 24 * 2 ** 30:
        pytest.skip("needs 24 GB of free device memory for an Out_2 of more than 2^31 elements")
    cols = np.stack([np.arange(n_cols - 12, n_cols - 3), np.arange(n_cols - 9, n_cols)]).astype(np.int32)
    cols[0, 2] = -1                                            # a dropped offset
    cols[1, 8] = -1
    touched = np.unique(cols[cols >= 0])
    assert Q * n_cols > 2 ** 31 and touched[0] == n_cols - 12 and touched[-1] == n_cols - 2
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn((2, Q, T), device=DEV, generator=g)
    out = torch.zeros((Q, n_cols), dtype=torch.float32, device=DEV)
    scale = float(np.float32(1.0) / np.float32(6.0))
    engine.stack_windows(out, x, torch.from_numpy(cols).to(DEV), scale, int(touched[0]), int(touched[-1]))
    ref = torch.zeros((Q, len(touched)), dtype=torch.float32, device=DEV)
    for k in range(2):
        keep = np.flatnonzero(cols[k] >= 0)
        local = np.searchsorted(touched, cols[k][keep])
        ref.index_add_(1, torch.from_numpy(local).to(DEV), x[k][:, torch.from_numpy(keep).to(DEV)] / 6.0)
    torch.cuda.synchronize()
    got = out[:, torch.from_numpy(touched).to(DEV).long()]
    assert torch.equal(got, ref)
    assert float(got[65536:].abs().min()) > 0                  # written beyond element 2^31, every touched column
    assert not bool(out[:, 0].any()) and not bool(out[:, n_cols - 13].any()) and not bool(out[:, n_cols - 1].any())
    assert not bool(out[:, n_cols - 10].any())                 # inside [c_min, c_max], listed by no window (its only entry was dropped)
    assert not bool(out[Q - 1, :n_cols - 12].any()) and not bool(out[0, :n_cols - 12].any())
    del out
    torch.cuda.empty_cache()


def test_stack_windows_rejects_bad_arguments():
    lib = _lib.load()
    z = torch.zeros((4, 9), dtype=torch.float32, device=DEV)
    c = torch.zeros((1, 9), dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()
    for args in ((p(z), p(c), 17, 4, 9, 1.0, p(z), 9, 0, 8), (p(z), p(c), 1, 4, 65, 1.0, p(z), 9, 0, 8), (p(z), p(c), 1, 4, 9, 1.0, p(z), 9, 0, 9),
                 (p(z), p(c), 1, 4, 9, 1.0, p(z), 9, 5, 4), (p(z), p(c), 1, 4, 9, 1.0, p(z), 9, -1, 4), (p(z), None, 1, 4, 9, 1.0, p(z), 9, 0, 8),
                 (None, p(c), 1, 4, 9, 1.0, p(z), 9, 0, 8)):
        assert lib.genie_stack_windows(*args, None) != 0
        assert b"genie_stack_windows" in lib.genie_last_error()
    torch.cuda.synchronize()
    assert not bool(z.any())


# ---- window-parallel, tuple form: every rank in this process --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _one_gpu(which):
    out, times = _run(_stride() if which == "stride" else _tiny(), stack_on_device=True)
    return out.cpu().numpy(), times


@functools.lru_cache(maxsize=None)
def _partials(which, world):
    """([partial Out_2 (numpy) per rank], [times per rank], info of rank 0)."""
    setup = _stride() if which == "stride" else _tiny()
    outs, times, info = [], [], None
    for r in range(world):
        res = _run(setup, window_parallel=(r, world), return_info=(r == 0))
        outs.append(res[0].cpu().numpy())
        times.append(res[1])
        info = res[2] if r == 0 else info
    return outs, times, info


def _rank_ordered_sum(parts):
    tot = np.zeros_like(parts[0])
    for p in parts:
        tot = tot + p                                          # fp32, rank order
    return tot


@functools.lru_cache(maxsize=None)
def _window_contributions():
    """world = 72 on the stride case: one window per rank, so partial r IS window r's contribution (0 + v = v). Returns (the fp32 sum
    in window order, A[q, c] = sum |v| in fp64, K[c] = number of windows feeding column c)."""
    parts, times, info = _partials("stride", 72)
    A = np.zeros(parts[0].shape, dtype=np.float64)
    K = np.zeros(parts[0].shape[1], dtype=np.int64)
    for p in parts:
        A += np.abs(p.astype(np.float64))
    table = apply.window_cols_table(_stride()[4]["tsteps_abs"], np.concatenate(times), OFFSETS, True)
    for row in table:
        K[row[row >= 0]] += 1
    return _rank_ordered_sum(parts), A, K


def test_window_parallel_one_window_per_rank_sums_to_one_gpu_bits():
    ref, ref_times = _one_gpu("stride")
    parts, times, info = _partials("stride", 72)
    tot, A, K = _window_contributions()
    assert all(len(t) == 1 for t in times) and np.array_equal(np.concatenate(times), ref_times)
    assert info["windows"] == [(r, r + 1) for r in range(72)] and not info["exact_merge"] and info["rank"] == 0
    assert K.max() >= 6 and np.array_equal(K > 0, A.max(0) > 0)
    assert np.array_equal(tot, ref)                            # the host's fp32 sum in window order = the device's running sum


def test_window_parallel_empty_blocks():
    ref, ref_times = _one_gpu("stride")
    parts, times, info = _partials("stride", 80)
    assert [len(t) for t in times] == [1] * 72 + [0] * 8 and np.array_equal(np.concatenate(times), ref_times)
    assert info["columns"][72:] == [None] * 8
    assert all(not p.any() for p in parts[72:])
    assert np.array_equal(_rank_ordered_sum(parts), ref)


@pytest.mark.parametrize("world", [2, 3, 5])
def test_window_parallel_partials_sum_to_one_gpu_result(world):
    ref, ref_times = _one_gpu("stride")
    parts, times, info = _partials("stride", world)
    _, A, K = _window_contributions()
    blocks = apply.window_blocks(72, world)
    assert info["windows"] == blocks and [len(t) for t in times] == [hi - lo for lo, hi in blocks]
    assert np.array_equal(np.concatenate(times), ref_times)    # the ranks' times partition the one-GPU times, in order
    assert info["exact_merge"]
    tot = _rank_ordered_sum(parts)
    per_col = info["ranks_per_column"]
    for p, (c_lo, c_hi) in zip(parts, info["columns"]):        # a rank writes inside its reported column range only
        nz = np.flatnonzero((p != 0).any(0))
        assert c_lo <= nz.min() and nz.max() <= c_hi
    single, boundary = per_col <= 1, per_col >= 2
    assert boundary.sum() >= world - 1 and single.sum() > boundary.sum()
    assert np.array_equal(tot[:, single], ref[:, single])      # one rank's windows only: the one-GPU bits
    # a boundary column holds fl(prefix) + fl(suffix) instead of one running sum over its K windows: each ordering is within the
    # standard bound K * 2^-24 * sum|v| of the exact sum, so the two differ by at most twice that
    bound = 2.0 * K[None, :] * 2.0 ** -24 * A
    diff = np.abs(tot.astype(np.float64) - ref.astype(np.float64))
    print("world %d: %d boundary columns, max |diff| %.3g, max diff / bound %.3g" % (
        world, int(boundary.sum()), diff[:, boundary].max(), (diff[:, boundary] / np.maximum(bound[:, boundary], 1e-300)).max()))
    assert (diff[:, boundary] <= bound[:, boundary]).all()
    assert float(np.abs(ref[:, boundary]).max()) > 0


@pytest.mark.parametrize("world", [2, 3])
def test_window_parallel_default_schedule_is_bit_equal_everywhere(world):
    ref, ref_times = _one_gpu("tiny")
    parts, times, info = _partials("tiny", world)
    assert info["exact_merge"] and (info["ranks_per_column"] >= 2).any()
    assert np.array_equal(np.concatenate(times), ref_times) and len(ref_times) >= 17
    assert float(np.abs(ref).max()) > 0 and np.array_equal(_rank_ordered_sum(parts), ref)


def test_window_parallel_on_a_sharded_model_is_refused():
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV, shard=(0, 2))
    assert net.is_sharded
    net_u, geom, P, trv, base = _tiny()
    with pytest.raises(NotImplementedError, match="window_parallel"):
        apply.apply_windows_device(net, geom, P, trv, window_parallel=(0, 2), **base)


# ---- group form: one process per rank ---------------------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, backend, same_gpu, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = "cuda:0" if same_gpu else "cuda:%d" % rank
    torch.cuda.set_device(dev)
    timeout = datetime.timedelta(seconds=60)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(dev), timeout=timeout)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timeout)
    try:
        net, geom, P, trv, kw = _stride(dev)
        out, times, info = apply.apply_windows_device(net, geom, P, trv, window_parallel=True, return_info=True, **kw)
        torch.cuda.synchronize()
        ret[rank] = (out.cpu().numpy(), np.asarray(times), info["windows"], info["rank"], dist.get_backend())
    finally:
        dist.destroy_process_group()


def _run_group(world, backend, same_gpu):
    import torch.multiprocessing as mp
    ref, ref_times = _one_gpu("stride")
    parts, _, info = _partials("stride", world)
    want = _rank_ordered_sum(parts)
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), backend, same_gpu, ret), nprocs=world, join=True)
    assert len(ret) == world
    for rank in range(world):
        out, times, windows, r, be = ret[rank]
        assert r == rank and windows == info["windows"] and be == backend
        assert np.array_equal(times, ref_times)                # every rank returns the full list
        assert out.tobytes() == ret[0][0].tobytes()            # every rank holds the same bits ...
        assert np.array_equal(out, want)                       # ... those of the rank-ordered sum of the tuple-form partials
    if world == 1:
        assert np.array_equal(want, ref)


def test_window_parallel_two_processes_on_one_gpu_over_gloo():
    _run_group(2, "gloo", True)


def test_window_parallel_three_processes_on_one_gpu_over_gloo():
    _run_group(3, "gloo", True)


def test_window_parallel_world1_rccl_device_all_reduce():
    """A one-rank RCCL group (the only form one GPU allows): the in-place device all-reduce branch."""
    _run_group(1, "nccl", True)


def test_window_parallel_world2_rccl():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL over xGMI); the 1-GPU box runs the gloo form above")
    _run_group(2, "nccl", False)
