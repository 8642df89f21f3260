"""CPU: the host-side plan of the sharded time-pointer build (`dist.shard_time_pointers`) is exact without a GPU. The two kernels are
restated in numpy below (a rank's candidates with their keys, the merge of the ranks' blocks); candidates + merge, and the whole driver
with these stand-ins over `Transport(emulate=True)` and over gloo with two ranks, give `graph.time_pointers` entry for entry -- on
tie-laden travel times that are shown to hold cross-rank ties at the k-th position, on a split where a rank owns fewer than k nodes, and
with fewer than k source nodes altogether. Also here: the C ABI of the new entries, and a bad travel time on one rank raising on both."""
import ctypes
import os

import numpy as np
import pytest
import torch

from genie_amd import _lib, dist as gdist, engine, graph
from tests.test_sharded_assoc_cpu import _declared, _free_port, spawn_with_limit

EMPTY = engine.TIME_POINTERS_EMPTY_KEY
DT, WIN = 0.5, 6.0
# name -> (stations, source nodes, k, travel times rounded to multiples of, worlds)
CASES = {
    "7x45": (7, 45, 10, None, (1, 2, 3)),
    "9x53": (9, 53, 10, None, (1, 2, 3)),
    "ties": (7, 45, 10, DT / 2, (1, 2, 3)),          # equal distances across ranks: only the global id decides
    "few": (5, 12, 10, None, (3,)),                  # every rank owns 4 < k nodes
    "g<k": (4, 6, 10, DT / 2, (1, 2, 3)),            # G < k: the tables have 6 columns
}


def case(name):
    """(trv fp32 [G, S, 2], keyword arguments, source-node positions, ring graph of the source nodes) -- seeded host arithmetic."""
    S, G, k, quantum, _ = CASES[name]
    rng = np.random.default_rng([3, S, G])
    trv = rng.uniform(0, 60, (G, S, 2)).astype(np.float32)
    if quantum:
        trv = (np.round(trv / quantum) * quantum).astype(np.float32)
    pos = rng.uniform(0, 300e3, (G, 3))
    i = np.arange(G)
    A_src = np.stack((np.concatenate(((i + 1) % G, (i - 1) % G)), np.concatenate((i, i))))
    return trv, dict(max_t=60.0, dt=DT, k=k, win=WIN), pos, A_src


def plans(name, world):
    S, G = CASES[name][:2]
    _, _, pos, A_src = case(name)
    order = engine.sfc_order(pos)
    return [gdist.ShardPlan(A_src, G, world, r, order) for r in range(world)]


def own_rows(trv, plan):
    """A rank's travel-time rows: fp32 [n_own * S, 2] in its local node order."""
    return torch.from_numpy(np.ascontiguousarray(trv[plan.own_global].reshape(-1, 2)))


def candidates_np(tl_own, n_sta, node_global, dtp, k):
    """genie_time_pointers_candidates restated: per (phase, station, step) the rank's min(k, n_own) smallest keys (float64 distance,
    global product-node id) by a full lexicographic sort, padded with the empty key."""
    ng, t = node_global.numpy().astype(np.int64), dtp.numpy()
    tl = tl_own.numpy().reshape(len(ng), n_sta, 2)
    out = np.empty((2, n_sta, len(t), k, 2), dtype=np.int64)
    out[..., 0], out[..., 1] = EMPTY
    m = min(k, len(ng))
    for ph in range(2):
        for i in range(n_sta):
            d = np.abs(tl[:, i, ph].astype(np.float64)[None, :] - t[:, None])              # [n_t, n_own]
            ids = np.broadcast_to(ng * n_sta + i, d.shape)
            o = np.lexsort((ids, d), axis=-1)[:, :m]
            out[ph, i, :, :m, 0] = np.take_along_axis(d, o, 1).view(np.int64)
            out[ph, i, :, :m, 1] = np.take_along_axis(ids, o, 1)
    return torch.from_numpy(out.reshape(-1, 2))


def merge_np(cand_all, n_sta, n_t, k, k_out):
    """genie_time_pointers_merge restated: the k_out smallest of the world * k keys per entry."""
    c = cand_all.numpy().reshape(-1, 2, n_sta, n_t, k, 2)
    c = np.moveaxis(c, 0, 3).reshape(2, n_sta, n_t, -1, 2)                                  # [2, S, n_t, world * k, 2]
    d, ids = np.ascontiguousarray(c[..., 0]).view(np.float64), c[..., 1]
    o = np.lexsort((ids, d), axis=-1)[..., :k_out]
    got = np.take_along_axis(ids, o, -1)
    if (got == EMPTY[1]).any():
        raise ValueError("the ranks' candidates do not fill every station")
    got = got.astype(np.int32)
    return torch.from_numpy(got[0].reshape(-1)), torch.from_numpy(got[1].reshape(-1))


def _dtp(kw):
    return torch.from_numpy(np.arange(-kw["win"], kw["win"] + kw["max_t"] + kw["dt"], kw["dt"]))


def _equal(got, want):
    return (np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1]) and np.array_equal(got[2], want[2])
            and got[0].dtype == torch.int32)


@pytest.mark.parametrize("name", list(CASES))
def test_candidates_plus_merge_equal_the_host_builder(name):
    S, G, k, _, worlds = CASES[name]
    trv, kw, _, _ = case(name)
    want = graph.time_pointers(trv, **kw)
    assert want[0].size == S * len(want[2]) * min(k, G)
    dtp, kt = _dtp(kw), min(k, G)
    for world in worlds:
        ps = plans(name, world)
        if name == "few":
            assert all(0 < p.n_own < k for p in ps)
        blocks = [candidates_np(own_rows(trv, p), S, torch.from_numpy(p.own_global.astype(np.int32)), dtp, kt) for p in ps]
        for b, p in zip(blocks, ps):                      # a rank emits min(k, n_own) keys per entry, empty keys behind them: no cycling
            ids = b[:, 1].reshape(-1, kt).numpy()
            m = min(kt, p.n_own)
            assert (ids[:, :m] != EMPTY[1]).all() and (ids[:, m:] == EMPTY[1]).all()
            assert np.isin(ids[:, :m] // S, p.own_global).all()
        for perm in (list(range(world)), list(range(world))[::-1]):          # the merge does not depend on the order of the blocks
            ep, es = merge_np(torch.stack([blocks[r] for r in perm]), S, len(dtp), kt, kt)
            assert _equal((ep, es, want[2]), want), (name, world)


def cross_rank_ties_at_k(name, world):
    """Entries (phase, station, step) whose k-th and (k + 1)-th nearest source nodes are equally far and owned by different ranks: the
    table is right there only if the merge breaks the tie by the global id."""
    S, G, k, _, _ = CASES[name]
    trv, kw, _, _ = case(name)
    owner = plans(name, world)[0].owner
    t = _dtp(kw).numpy()
    n = 0
    for ph in range(2):
        for i in range(S):
            d = np.abs(trv[:, i, ph].astype(np.float64)[None, :] - t[:, None])
            o = np.lexsort((np.broadcast_to(np.arange(G), d.shape), d), axis=-1)
            a, b = o[:, k - 1], o[:, k]
            rows = np.arange(len(t))
            n += int(((d[rows, a] == d[rows, b]) & (owner[a] != owner[b])).sum())
    return n


@pytest.mark.parametrize("world", [2, 3])
def test_the_tie_case_holds_cross_rank_ties_at_the_kth_position(world):
    assert cross_rank_ties_at_k("ties", world) > 0
    assert cross_rank_ties_at_k("7x45", world) == 0           # (the plain case has none: it cannot stand in for the tie case)


@pytest.mark.parametrize("name", ["7x45", "ties", "g<k"])
def test_driver_over_an_emulated_transport(name):
    """One rank of a one-rank plan, every collective a copy: the driver's own arithmetic (agreed constants, dt_partition, k clipped)."""
    S, G, k, _, _ = CASES[name]
    trv, kw, _, _ = case(name)
    p = plans(name, 1)[0]
    tr = gdist.Transport(None, 1, emulate=True)
    for max_t in (kw["max_t"], None):
        kw2 = dict(kw, max_t=max_t)
        got = gdist.shard_time_pointers(own_rows(trv, p), p.own_global, S, G, tr, candidates=candidates_np, merge=merge_np, **kw2)
        assert _equal(got, graph.time_pointers(trv, **kw2)), (name, max_t)


def test_argument_errors_of_the_driver():
    trv, kw, _, _ = case("g<k")
    p = plans("g<k", 1)[0]
    tr = gdist.Transport(None, 1, emulate=True)
    rows = own_rows(trv, p)
    for bad in (dict(k=0), dict(k=33), dict(dt=0.0), dict(max_t=-20.0, win=0.1, dt=30.0)):
        with pytest.raises(ValueError):
            gdist.shard_time_pointers(rows, p.own_global, 4, 6, tr, candidates=candidates_np, merge=merge_np, **dict(kw, **bad))
    with pytest.raises(ValueError, match="owned rows"):
        gdist.shard_time_pointers(rows[:-1], p.own_global, 4, 6, tr, candidates=candidates_np, merge=merge_np, **kw)


def _gloo_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = {}
        tr = gdist.Transport(None, world)
        for name in ("7x45", "ties", "g<k"):
            S, G = CASES[name][:2]
            trv, kw, _, _ = case(name)
            p = plans(name, world)[rank]
            for max_t in (kw["max_t"], None):
                kw2 = dict(kw, max_t=max_t)
                got = gdist.shard_time_pointers(own_rows(trv, p), p.own_global, S, G, tr, candidates=candidates_np, merge=merge_np, **kw2)
                res[(name, max_t)] = _equal(got, graph.time_pointers(trv, **kw2))
        # a NaN in the rows of rank 1 only: both ranks raise, after the first collective, and neither waits in the second
        trv, kw, _, _ = case("7x45")
        p = plans("7x45", world)[rank]
        rows = own_rows(trv, p)
        if rank == 1:
            rows[3, 1] = float("nan")
        try:
            gdist.shard_time_pointers(rows, p.own_global, 7, 45, tr, candidates=candidates_np, merge=merge_np, **dict(kw, max_t=None))
            res["nan"] = "no error"
        except ValueError as e:
            res["nan"] = str(e)
        ret[rank] = res
    finally:
        dist.destroy_process_group()


def test_driver_over_gloo_with_two_ranks():
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    spawn_with_limit(_gloo_worker, (2, _free_port(), ret), 2, 60.0)
    assert len(ret) == 2
    for rank in range(2):
        for name in ("7x45", "ties", "g<k"):
            for max_t in (60.0, None):
                assert ret[rank][(name, max_t)], (rank, name, max_t)
        assert "finite" in ret[rank]["nan"] and "rank(s) 1" in ret[rank]["nan"], (rank, ret[rank]["nan"])


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(_lib.INCLUDE, "genie_hip.h")).read()
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    want = {
        "genie_time_pointers_candidates": [P, L, I, P, P, I, I, P, P, P, P],
        "genie_time_pointers_merge": [P, I, I, I, I, I, P, P, P, P],
        "genie_lslc_rows_own": [P, P, P, I, P, P, L, I, F, F, P, P, I, P, P, I, P, P, P],
    }
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    lib = _lib.load()
    for name, args in want.items():
        decl = _declared(header, "int", name)
        assert len(decl) == len(args), name
        for d, a in zip(decl, args):
            kind = P if "*" in d else (L if d.startswith("int64_t") else (F if d.startswith("float") else I))
            assert kind is a, (name, d)
        assert bound.get(name) == (I, args), name
        assert hasattr(lib, name), name
    one = ctypes.c_void_p(256)                                # (never dereferenced: every call below is refused before any launch)
    assert lib.genie_time_pointers_candidates(one, 40, 4, one, one, 10, 33, one, one, one, None) != 0            # k > 32
    assert lib.genie_time_pointers_candidates(one, 40, 4, None, one, 10, 10, one, one, one, None) != 0           # no node_global
    assert lib.genie_time_pointers_candidates(one, 42, 4, one, one, 10, 10, one, one, one, None) != 0            # rows not a multiple of n_sta
    assert lib.genie_time_pointers_merge(one, 2, 4, 10, 10, 11, one, one, one, None) != 0                        # k_out > k
    assert lib.genie_time_pointers_merge(one, 0, 4, 10, 10, 10, one, one, one, None) != 0                        # no rank
    assert lib.genie_time_pointers_merge(one, 2, 4, 1, 10, 10, one, one, one, None) != 0                         # n_t < 2
    assert lib.genie_lslc_rows_own(None, None, None, 0, None, None, 0, 0, 0.0, 0.0, None, None, 0, None, None, 0, None, None, None) != 0
    assert lib.genie_last_error()
