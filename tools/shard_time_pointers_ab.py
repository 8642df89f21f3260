"""`python tools/shard_time_pointers_ab.py [out.json]` -- config-4 shape (2000 stations x 50 000 source nodes, k = 10): wall time of the sharded time-pointer set-up (world 1 over RCCL) against what
the parent needs for the same model (graph.time_pointers on the host + upload of the whole tables). Both in this process, one warm-up each."""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genie_amd import dist as gdist, engine, graph          # noqa: E402

S, G, K, N_HOST = 2000, 50000, 10, 16
DEV = "cuda:0"
kw = dict(max_t=60.0, dt=0.6, k=K, win=6.0)
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
if "MASTER_PORT" not in os.environ:                          # a free port, as the tests take one
    import socket
    with socket.socket() as _s:
        _s.bind(("127.0.0.1", 0))
        os.environ["MASTER_PORT"] = str(_s.getsockname()[1])
torch.cuda.set_device(DEV)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
out = {"S": S, "G": G, "k": K, "kw": kw}
try:
    g = torch.Generator(device=DEV).manual_seed(1)
    trv_dev = torch.rand((G, S, 2), device=DEV, generator=g) * 60.0
    trv = trv_dev.cpu().numpy()                              # the host table [G, S, 2] fp32 (800 MB)
    del trv_dev
    order = engine.sfc_order(np.random.default_rng(2).uniform(0, 300e3, (G, 3)))
    own = np.asarray(order, dtype=np.int64)                  # world 1: every node, in space-filling-curve order
    tr = gdist.Transport(None, 1)
    assert tr.device_collectives

    def new_setup():
        t0 = time.perf_counter()
        idx = torch.from_numpy(own)
        rows = torch.from_numpy(trv)[idx].reshape(-1, 2).to(DEV)          # the rank's own rows: cut out on the host, uploaded
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        res = gdist.shard_time_pointers(rows, own, S, G, tr, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, time.perf_counter() - t1, res

    new_setup()                                              # warm-up
    runs = [new_setup() for _ in range(3)]
    out["new_total_s"] = [r[0] for r in runs]
    out["new_build_only_s"] = [r[1] for r in runs]
    ep, es, dtp = runs[-1][2]
    out["n_t"] = int(len(dtp))

    def host_part(n):
        t0 = time.perf_counter()
        res = graph.time_pointers(trv[:, :n], **kw)
        return time.perf_counter() - t0, res

    host_part(2)                                             # warm-up
    th, (hp, hs, hd) = host_part(N_HOST)
    out["host_build_s_%d_stations" % N_HOST] = th
    out["host_build_s_extrapolated_%d_stations" % S] = th * S / N_HOST
    # exactness at this size, on the stations the host built: entry (i, j, :) of station i < N_HOST
    n_t = len(hd)
    a = ep.view(S, n_t, K)[:N_HOST].cpu().numpy()
    b = np.asarray(hp).reshape(N_HOST, n_t, K)
    out["subset_equal_source_nodes"] = bool(np.array_equal(a // S, b // N_HOST) and np.array_equal(a % S, b % N_HOST))
    t0 = time.perf_counter()                                 # the parent's upload: the whole travel-time table and both tables
    up = [torch.from_numpy(trv.reshape(-1, 2)).to(DEV), torch.zeros(S * n_t * K, dtype=torch.int64).to(DEV), torch.zeros(S * n_t * K, dtype=torch.int64).to(DEV)]
    torch.cuda.synchronize()
    out["parent_upload_s"] = time.perf_counter() - t0
finally:
    dist.destroy_process_group()
if len(sys.argv) > 1:                                        # optional: a file for the result line
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out))
