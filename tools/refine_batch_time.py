"""What a source costs in the refine pass when the sources run in batches: `apply.refine_sources(ftrns2_device=..., source_batch=B)` on the
config-2 shape (200 stations x 10 000 grid nodes) at the default cloud of 112 000 queries, one grid leg, the keyed draw
(`rand=apply.PhiloxCloud(key)`), for B = 1, 4, 8 and 16, alternating in ONE process on the same model, picks and library, so that the arms
share clocks and box. B = 1 is the pass one source after the other: the yardstick of the same run.

  timeout -k 10 500 python tools/refine_batch_time.py [--out DIR] [--sources 32] [--reps 7]

One warm-up run per arm (its rows are compared: every arm must return the rows of B = 1, bit for bit), then `reps` rounds over the arms; a
run is a host clock around a pass over `sources` candidates that ends in a device synchronise. Prints one JSON line (ms per source per
run, median / min / max per arm, the spread of the yardstick) and writes it to DIR/refine_batch_time.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from genie_amd import apply, module, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--sources", type=int, default=32)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--queries", type=int, default=112000)
ap.add_argument("--config", default="cfg2_200x10k")
a = ap.parse_args()

dev = "cuda:0"
BATCHES = (1, 4, 8, 16)
n_sources, n_rand_query, reps = a.sources, a.queries, a.reps
S, G, _, L, nq = synthetic.CONFIGS[a.config]
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
srcs = np.concatenate((geom.x_grid[nodes] + rng.normal(0.0, 2000.0, (n_sources, 3)), (t_org + rng.normal(0.0, 0.5, n_sources)).reshape(-1, 1),
                       np.full((n_sources, 1), 0.5)), axis=1)
ident = lambda x: x                                                                        # noqa: E731
off_min, off_rng = np.array([[-15e3, -15e3, -7.5e3]]), np.array([[30e3, 30e3, 15e3]])
picks = apply.ResidentPicks(P, np.arange(S), S, dev)
legs = [apply.GridLeg(net, geom.x_grid, trv)]


def run(batch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = apply.refine_sources(legs, picks, srcs, geom.locs, geom.t_query, max_t, off_min, off_rng, n_rand_query, ident, ident, (0.0, L),
                             (0.0, L), (-40e3, 2e3), rand=apply.PhiloxCloud((2024, 7)), ftrns2_device=ident,
                             kernel_sig_t=synthetic.KERNEL_SIG_T, dt_embed=0.3, source_batch=batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n_sources * 1e3, r


warm = {b: run(b)[1] for b in BATCHES}
same = {str(b): bool(np.array_equal(warm[b][0], warm[1][0]) and np.array_equal(warm[b][1], warm[1][1])) for b in BATCHES}
ts = {b: [] for b in BATCHES}
for _ in range(reps):
    for b in BATCHES:
        ts[b].append(round(run(b)[0], 4))
out = {"ms_per_source": {str(b): v for b, v in ts.items()}, "median": {str(b): float(np.median(v)) for b, v in ts.items()},
       "min": {str(b): min(v) for b, v in ts.items()}, "max": {str(b): max(v) for b, v in ts.items()},
       "yardstick_spread_ms": round(max(ts[1]) - min(ts[1]), 4), "rows_equal_to_batch_1": same,
       "max_value": float(warm[1][0][:, 4].max()), "n_sources": n_sources, "n_rand_query": n_rand_query, "reps": reps, "config": a.config,
       "n_t": int(np.asarray(geom.t_query).size)}
print(json.dumps(out))
if a.out:
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "refine_batch_time.json"), "w") as f:
        f.write(json.dumps(out, indent=1))
if not all(same.values()):
    sys.exit("an arm's rows differ from source_batch=1")
