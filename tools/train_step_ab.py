"""What the flat training step costs against the plain one, on one GPU: `train.train_step` + `train.make_optimizer` (torch's multi-tensor
Adam over ~151 gradient tensors, `loss.item()` per sample) against `train.train_step_parallel` + `train.FlatAdam` at world 1 (one flat
gradient buffer, `genie_adam_step`, one host read per step), at the config-3 shape (200 stations x 10 000 source nodes, the reference's
4-output step `mz(*input_tensors)`, two samples per batch that share their graph tensors), alternating in ONE process on two identically
initialised models and the same library, so that the arms share clocks and box.

  timeout -k 10 600 python tools/train_step_ab.py [--out DIR] [--grid 10000] [--picks 4000] [--reps 9] [--steps 5]

One warm-up run of `steps` steps per arm, then `reps` alternating runs per arm; a run is a host clock around `steps` steps that ends in a
device synchronise. Separately the optimizer part alone, 50 calls per run: `optimizer.step()` + `HipPath.sync_weights` (the re-upload of
the weight mirror) of the torch arm against `FlatAdam.step()` + the same re-upload, on the gradients the last step left. The spread of
an arm is (max - min) of its runs; `flat_not_slower` = the flat median is below the plain median plus the plain arm's spread. The first
step's losses of the two arms are compared (they start from the same weights). Prints one JSON line and writes it to
DIR/train_step_ab.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from genie_amd import graph, module, synthetic, train  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--grid", type=int, default=10000)
ap.add_argument("--queries", type=int, default=10000)
ap.add_argument("--picks", type=int, default=4000)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--steps", type=int, default=5)
a = ap.parse_args()

dev = "cuda:0"
S, G = 200, a.grid
geom = synthetic.Geometry(S, G, L=300e3, n_query=a.queries, seed=1)
t = lambda arr, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(arr)).to(dt).to(dev)           # noqa: E731
A1, A2, A3, A4 = graph.cartesian_product_edges(geom.A_sta_sta, geom.A_src_src, S, G, device=dev)
ea = graph.GraphEdges(x=t(geom.edge_attr()), edge_index=A3)
eaf = graph.GraphEdges(x=ea.x, edge_index=A3.flip(0).contiguous())
shared = (t(geom.A_src_src, torch.long), t(geom.locs), t(geom.x_grid), t(geom.x_query), t(geom.t_query))
batch = []
for k in range(2):
    smp = synthetic.training_sample(geom, a.picks, n_src=4, seed=3, window=k)
    inputs = [t(smp["Slice"]), t(smp["Mask"]), A1, A2, ea, eaf, A4, shared[0], t(smp["A_edges_p"], torch.long), t(smp["A_edges_s"], torch.long),
              t(smp["dt_partition"]), t(smp["tlatent"]), t(smp["tpick"]), t(smp["ipick"], torch.long), t(smp["phase_label"]), shared[1],
              shared[2], shared[3], t(smp["x_query_src"]), shared[4], t(smp["tq_sample"]), t(smp["trv_out_q"])]
    batch.append((inputs, (t(smp["Lbls"]), t(smp["Lbls_query"]), t(smp["pick_lbls"]))))


def model():
    torch.manual_seed(0)
    return module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=dev).train()


net_p = model()
opt_p = train.make_optimizer(net_p)
net_f = model()
opt_f = train.FlatAdam(train.FlatParams(net_f))
arms = {"plain": lambda: train.train_step(net_p, opt_p, batch), "flat": lambda: train.train_step_parallel(net_f, opt_f, batch)}
first = {name: fn() for name, fn in arms.items()}                            # the first step of both: same weights, same batch


def run(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def ab(fns, n, reps):
    for fn in fns.values():
        run(fn, n)                                                           # warm-up of every arm
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ts[name].append(round(run(fn, n), 4))
    return {"ms": ts, "median": {k: float(np.median(v)) for k, v in ts.items()}, "min": {k: min(v) for k, v in ts.items()},
            "max": {k: max(v) for k, v in ts.items()}, "spread": {k: round(max(v) - min(v), 4) for k, v in ts.items()}}


out = {"step": ab(arms, a.steps, a.reps)}
out["step"]["flat_not_slower"] = bool(out["step"]["median"]["flat"] <= out["step"]["median"]["plain"] + out["step"]["spread"]["plain"])


def upload(net):
    net._hip.sync_weights(net._path_params, net._weight_split())


def plain_opt():
    opt_p.step()                                                             # in-place writes: sync_weights sees the new versions
    upload(net_p)


def flat_opt():
    opt_f.step()                                                             # marks the weights changed itself
    upload(net_f)


out["optimizer_and_upload"] = ab({"plain": plain_opt, "flat": flat_opt}, 50, a.reps)
out.update(first_step_loss=first, first_step_loss_rel_diff=abs(first["plain"] - first["flat"]) / abs(first["plain"]), n_sta=S, n_grid=G,
           n_picks=int(batch[0][0][12].numel()), samples_per_batch=len(batch), steps_per_run=a.steps, reps=a.reps,
           n_param_floats=int(opt_f.params.n), device=torch.cuda.get_device_name(0))
print(json.dumps(out))
if a.out:
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "train_step_ab.json"), "w") as f:
        f.write(json.dumps(out, indent=1))
