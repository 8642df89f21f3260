"""What the end of the refine pass costs per source: `apply.refine_sources(ftrns2_device=...)` on the config-2 shape (200 stations x
10 000 grid nodes) at the default cloud of 112 000 queries, this tree's `apply.py` against ANOTHER REVISION's, alternating in ONE process
on the same model, picks and library, so that the arms share clocks and box.

  git show REV:genie_amd/apply.py > /tmp/parent_apply.py
  timeout -k 10 400 python tools/refine_ab.py --parent-apply /tmp/parent_apply.py [--out DIR] [--sources 32] [--reps 7]

The other revision's file is loaded as a sibling module of the package (it must work with this tree's library, which is the case while
the C ABI only grows). One warm-up run per arm, whose results are compared (`results_bit_equal`), then `reps` alternating runs per arm
with one and with three grid legs; a run is a host clock around a pass over `sources` candidates that ends in a device synchronise.
Prints one JSON line (ms per source: every run, median, min, max) and writes it to DIR/refine_ab.json."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from genie_amd import apply as new_apply, module, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-apply", required=True, help="apply.py of the revision to compare against")
ap.add_argument("--out", default=None)
ap.add_argument("--sources", type=int, default=32)
ap.add_argument("--reps", type=int, default=7)
a = ap.parse_args()
spec = importlib.util.spec_from_file_location("genie_amd._apply_parent", a.parent_apply)
old_apply = importlib.util.module_from_spec(spec)
sys.modules["genie_amd._apply_parent"] = old_apply
spec.loader.exec_module(old_apply)

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
ident = lambda x: x
out = {}
for n_legs in (1, 3):
    arms = {}
    for name, mod in (("parent", old_apply), ("new", new_apply)):
        picks = mod.ResidentPicks(P, np.arange(S), S, dev)
        leg = mod.GridLeg(net, geom.x_grid, trv)
        arms[name] = (mod, picks, [leg] * n_legs)

    def run(name):
        mod, picks, legs = arms[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = mod.refine_sources(legs, picks, srcs, geom.locs, geom.t_query, max_t, np.array([[-15e3, -15e3, -7.5e3]]),
                               np.array([[30e3, 30e3, 15e3]]), n_rand_query, ident, ident, (0.0, L), (0.0, L), (-40e3, 2e3),
                               rand=np.random.RandomState(3).rand, ftrns2_device=ident, kernel_sig_t=sig, dt_embed=0.3)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n_sources * 1e3, r

    ra, rb = run("parent")[1], run("new")[1]      # warm-up of both, and the results compared
    same = bool(np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]))
    ts = {"parent": [], "new": []}
    for _ in range(reps):
        for name in ("parent", "new"):
            ts[name].append(round(run(name)[0], 4))
    out["legs_%d" % n_legs] = {"ms_per_source": ts, "median": {k: float(np.median(v)) for k, v in ts.items()},
                               "min": {k: min(v) for k, v in ts.items()}, "max": {k: max(v) for k, v in ts.items()},
                               "results_bit_equal": same, "max_value": float(rb[0][:, 4].max())}
out.update(n_sources=n_sources, n_rand_query=n_rand_query, reps=reps, n_t=int(np.asarray(geom.t_query).size))
print(json.dumps(out))
if a.out:
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "refine_ab.json"), "w") as f:
        f.write(json.dumps(out, indent=1))
