"""CPU: the host side of the 4-output `forward_fixed` on a source-node-sharded model -- which rank owns which of the rows a pick's
time-pointer entry lists (from a `ShardPlan`), the bookkeeping of the ragged all-gather of the ranks' compact row lists (counts of 0
included) and the placement of the rows, and the C ABI of the new entry points (declared in the header, bound in `_lib.SYMBOLS`,
exported by the built library)."""
import ctypes
import os
import re
import socket
import time

import numpy as np
import torch

from genie_amd import _lib, dist as gdist, engine, synthetic

K = 10


def sample_case(S, G, world, seed=5, n_picks=120):
    """(geom, training sample, the picks' table entry numbers, every rank's ShardPlan, owners [2][n, K] of the listed rows for the P / S
    tables) of the bit-equality test's inputs: all of it host arithmetic."""
    geom = synthetic.Geometry(S, G, n_query=20, seed=11)
    smp = synthetic.training_sample(geom, n_picks, n_src=3, seed=seed)
    dtp = smp["dt_partition"]
    ti = np.floor((smp["tpick"] - dtp[0]) / (dtp[1] - dtp[0])).astype(np.int64)
    base = smp["ipick"].astype(np.int64) * len(dtp) + ti
    order = engine.sfc_order(geom.x_grid)
    plans = [gdist.ShardPlan(geom.A_src_src, G, world, r, order) for r in range(world)]
    owners = [gdist.pointer_row_owners(smp[k], base, plans[0], S, K) for k in ("A_edges_p", "A_edges_s")]
    return geom, smp, base, plans, owners


def assert_case_exercises_the_exchange(plans, owners):
    """The three conditions on the inputs under which bit-equality says something about the exchanges."""
    world = len(plans)
    own = np.concatenate(owners)
    assert all(p.n_halo >= 1 for p in plans), "every rank needs a halo node"
    assert any(len(set(r)) >= 2 for r in own.tolist()), "some pick's ten rows must be owned by two or more ranks"
    assert any((~(own == r).any(axis=1)).any() for r in range(world)), "some rank must own none of the rows of some pick"


def test_ownership_split_of_pointer_rows():
    for S, G in ((7, 45), (9, 53)):
        for world in (2, 3):
            geom, smp, base, plans, owners = sample_case(S, G, world)
            assert_case_exercises_the_exchange(plans, owners)
            for tab, own in zip(("A_edges_p", "A_edges_s"), owners):
                assert own.shape == (len(base), K)
                e = smp[tab].reshape(-1, K)[base]                           # the ten global product nodes of every pick
                for r, p in enumerate(plans):                               # rank r's share = the nodes whose source node it owns
                    mine = np.isin(e // S, p.own_global)
                    assert np.array_equal(mine, own == r)
                    loc = p.global_to_local[e[mine] // S]
                    assert (loc >= 0).all() and (loc < p.n_own).all()       # ... found among its OWNED local nodes, not its halo
            assert sum(int((owners[0] == r).sum()) for r in range(world)) == owners[0].size      # every row has exactly one owner


def test_rows_are_placed_not_added():
    n = 6
    rows = torch.randn(n, 32)
    rows[2, 4] = -0.0
    keys = torch.tensor([5, 0, 3, 4, 1, 2], dtype=torch.int32)
    rows[:, 31] = keys.view(torch.float32)
    table = gdist.place_pick_rows(rows, n)
    assert torch.equal(table[keys.long()].view(torch.int32), rows.view(torch.int32))
    assert bool(torch.signbit(table[3, 4]))                                # -0.0 stays -0.0 (a sum with the zero table would lose it)
    assert gdist.place_pick_rows(rows[:0], 4).abs().sum() == 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


COUNTS = ((0, 3, 1), (2, 0, 0), (0, 0, 0))


def _ragged_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        tr = gdist.Transport(None, world)
        out = []
        for counts in COUNTS:
            rows = torch.full((5, 32), float("nan"))                        # beyond `count`: never part of the result
            rows[: counts[rank]] = torch.arange(counts[rank]).view(-1, 1) + 100.0 * rank
            out.append(tr.all_gather_ragged(rows, torch.tensor([counts[rank]], dtype=torch.int32), timeout=30.0).clone())
        ret[rank] = out
    finally:
        dist.destroy_process_group()


def spawn_with_limit(fn, args, world, limit):
    """`mp.spawn` with a deadline: children still alive when it passes, or when one of them failed, are killed."""
    import torch.multiprocessing as mp
    ctx = mp.spawn(fn, args=args, nprocs=world, join=False)
    end = time.monotonic() + limit
    try:
        while not ctx.join(timeout=max(0.1, end - time.monotonic())):
            assert time.monotonic() < end, "spawned ranks did not finish within %.0f s" % limit
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()


def test_ragged_gather_with_empty_ranks():
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    spawn_with_limit(_ragged_worker, (3, _free_port(), ret), 3, 60.0)
    for rank in range(3):
        for counts, got in zip(COUNTS, ret[rank]):
            want = [torch.arange(c).view(-1, 1) + 100.0 * r for r, c in enumerate(counts)]
            want = torch.cat(want).expand(-1, 32) if sum(counts) else torch.zeros(0, 32)
            assert got.shape == (sum(counts), 32) and torch.equal(got, want.float()), (rank, counts)


def _declared(header, ret, name):
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), header)
    assert m, "%s is not declared in genie_hip.h" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(_lib.INCLUDE, "genie_hip.h")).read()
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    want = {
        "genie_assoc_halo_offset": ("size_t", ctypes.c_size_t, [P]),
        "genie_assoc_fwd_part": ("int", I, [P, I, P, P, P, P, P, P, P, P, P]),
        "genie_lslc_rows": ("int", I, [P, P, P, I, P, P, L, I, F, F, P, P, I, P, P, I, P, P, P]),
        "genie_lslc_fwd_rows": ("int", I, [P, I, P, F, P, P, I, P, P]),
    }
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    lib = _lib.load()
    for name, (c_ret, res, args) in want.items():
        decl = _declared(header, c_ret, name)
        assert len(decl) == len(args), name
        for d, a in zip(decl, args):                                        # pointer / int / int64 / float, argument by argument
            kind = P if "*" in d else (L if d.startswith("int64_t") else (F if d.startswith("float") else I))
            assert kind is a, (name, d)
        assert bound.get(name) == (res, args), name
        assert hasattr(lib, name), name
    assert lib.genie_assoc_fwd_part(None, 3, None, None, None, None, None, None, None, None, None) != 0       # refused before any launch
    assert lib.genie_lslc_rows(None, None, None, 0, None, None, 0, 0, 0.0, 0.0, None, None, 0, None, None, 0, None, None, None) != 0
    assert lib.genie_lslc_fwd_rows(None, 0, None, 1.0, None, None, 0, None, None) != 0
