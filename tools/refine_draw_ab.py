"""What the refine pass's draw costs per source: `apply.refine_sources(ftrns2_device=...)` on the config-2 shape (200 stations x 10 000
grid nodes) at the default cloud of 112 000 queries, with the host draw `rand=np.random.rand` (the default: drawn on the host, staged
through pinned memory, copied to the device) against the keyed device draw `rand=apply.PhiloxCloud(key)` (one kernel per source, nothing
from the host), alternating in ONE process on the same model, picks and library, so that the arms share clocks and box.

  timeout -k 10 400 python tools/refine_draw_ab.py [--out DIR] [--sources 32] [--reps 7]

One warm-up run per arm, then `reps` alternating runs per arm with one and with three grid legs; a run is a host clock around a pass
over `sources` candidates that ends in a device synchronise. The two arms draw DIFFERENT clouds, so only times are compared (that the
keyed arm refines what the staged path refines from the same numbers is tests/test_refine_cloud_gpu.py's business). Beside them: the
host time of one `np.random.rand(112000, 3)` and of one `PhiloxCloud.host` on this box, and the device time of one cloud kernel
(HIP events around 50 launches). Prints one JSON line and writes it to DIR/refine_draw_ab.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from genie_amd import apply, module, postproc, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--sources", type=int, default=32)
ap.add_argument("--reps", type=int, default=7)
a = ap.parse_args()

dev = "cuda:0"
n_sources, n_rand_query, reps = a.sources, 112000, a.reps
S, G, _, L, nq = synthetic.CONFIGS["cfg2_200x10k"]
geom = synthetic.Geometry(S, G, L=L, n_query=nq, seed=1)
torch.manual_seed(0)
net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=dev).eval()
net.set_adjacencies_base(torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src), torch.from_numpy(geom.edge_attr()).to(dev),
                         torch.from_numpy(geom.locs).float().to(dev), torch.from_numpy(geom.x_grid).float().to(dev))
rng = np.random.default_rng(11)
n_bg = int(250 * S / 24)
P = np.stack([rng.uniform(0.0, 3600.0, n_bg), rng.integers(0, S, n_bg).astype(np.float64), np.ones(n_bg), np.ones(n_bg),
              rng.integers(0, 2, n_bg).astype(np.float64)], axis=1)
trv = geom.travel_times().astype(np.float32)
max_t = float(np.ceil(trv.max() + 1.0))
nodes = rng.choice(G, n_sources, replace=False)
t_org = np.sort(rng.uniform(300.0, 3300.0, n_sources))
ev = []
for g, t0 in zip(nodes, t_org):
    for ph in (0, 1):
        keep = rng.random(S) < 0.8
        tt = t0 + trv[g, keep, ph] + rng.normal(0.0, 0.1, int(keep.sum()))
        ev.append(np.stack([tt, np.nonzero(keep)[0].astype(np.float64), np.ones_like(tt), np.ones_like(tt), np.full_like(tt, ph)], axis=1))
P = np.concatenate([P] + ev, axis=0)
P = P[rng.permutation(P.shape[0])]
sig = synthetic.KERNEL_SIG_T
srcs = np.concatenate((geom.x_grid[nodes] + rng.normal(0.0, 2000.0, (n_sources, 3)), (t_org + rng.normal(0.0, 0.5, n_sources)).reshape(-1, 1),
                       np.full((n_sources, 1), 0.5)), axis=1)
ident = lambda x: x                                                                        # noqa: E731
off_min, off_rng = np.array([[-15e3, -15e3, -7.5e3]]), np.array([[30e3, 30e3, 15e3]])
picks = apply.ResidentPicks(P, np.arange(S), S, dev)
leg = apply.GridLeg(net, geom.x_grid, trv)
draws = {"host_rand": lambda: np.random.rand, "philox": lambda: apply.PhiloxCloud((2024, 7))}
out = {}
for n_legs in (1, 3):
    legs = [leg] * n_legs

    def run(name):
        rand = draws[name]()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = apply.refine_sources(legs, picks, srcs, geom.locs, geom.t_query, max_t, off_min, off_rng, n_rand_query, ident, ident, (0.0, L),
                                 (0.0, L), (-40e3, 2e3), rand=rand, ftrns2_device=ident, kernel_sig_t=sig, dt_embed=0.3)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n_sources * 1e3, r

    warm = {name: run(name)[1] for name in ("host_rand", "philox")}      # warm-up of both
    ts = {"host_rand": [], "philox": []}
    for _ in range(reps):
        for name in ("host_rand", "philox"):
            ts[name].append(round(run(name)[0], 4))
    out["legs_%d" % n_legs] = {"ms_per_source": ts, "median": {k: float(np.median(v)) for k, v in ts.items()},
                               "min": {k: min(v) for k, v in ts.items()}, "max": {k: max(v) for k, v in ts.items()},
                               "philox_median_below_host_rand_max": bool(np.median(ts["philox"]) < max(ts["host_rand"])),
                               "max_value": {k: float(v[0][:, 4].max()) for k, v in warm.items()}}


def host_ms(fn, n=9):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


cloud = apply.PhiloxCloud((2024, 7))
out["host_draw_ms"] = {"np_random_rand": host_ms(lambda: np.random.rand(n_rand_query, 3)),
                       "philox_cloud_host": host_ms(lambda: cloud.host(3, n_rand_query))}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for k in range(60):
    if k == 10:
        e0.record()
    postproc.refine_cloud_device(cloud.key, k, n_rand_query, srcs[0, 0:3], off_rng, off_min, dev)
e1.record()
torch.cuda.synchronize()
out["cloud_kernel_call_ms"] = round(e0.elapsed_time(e1) / 50.0, 5)       # 50 back-to-back calls: launch + two allocations + kernel
out.update(n_sources=n_sources, n_rand_query=n_rand_query, reps=reps, n_t=int(np.asarray(geom.t_query).size))
print(json.dumps(out))
if a.out:
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "refine_draw_ab.json"), "w") as f:
        f.write(json.dumps(out, indent=1))
