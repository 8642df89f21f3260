"""What the cell index buys the kNN of a large query set: `genie_knn` (brute force, `engine.knn_device(index=None)`) against
`genie_knn_indexed` (`engine.KnnIndex`), alternating in ONE process on the same tensors and library, so that the arms share clocks and box.

  timeout -k 10 500 python tools/knn_index_ab.py [--out DIR] [--reps 7] [--sources 16] [--skip-refine]

1. The call alone, HIP events around `--inner` back-to-back calls: 112 000 queries, k = 10, against 10 000 and 50 000 grid nodes (drawn
   as `synthetic.Geometry` draws a grid: uniform over L x L x 42 km), for a refine-style cloud (the config-2 offset box around a node)
   and for queries uniform over the grid's box. Two warm-up runs per arm, then `reps` alternating runs; every run is printed. The two
   tables are compared (`torch.equal`) before anything is timed. Beside them: the build time of the index (host clock around
   `KnnIndex(x)` ending in a synchronise: two passes, one read-back, three allocations) and the time of both calls over a ladder of
   query counts, from which the break-even count of one build plus one indexed call against one brute-force call is read.
2. The refine pass per source, config-2 shape, one leg and three legs, `rand=PhiloxCloud`: the model's `knn_index` off (the reference
   arm) and on, rows compared bit for bit.
Prints one JSON line and writes it to DIR/knn_index_ab.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from genie_amd import apply, engine, module, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--sources", type=int, default=16)
ap.add_argument("--skip-refine", action="store_true")
a = ap.parse_args()

dev = "cuda:0"
N_QUERY, K = 112000, 10
OFF_MIN, OFF_RNG = np.array([[-15e3, -15e3, -7.5e3]]), np.array([[30e3, 30e3, 15e3]])      # the config-2 offset box
out = {"n_query": N_QUERY, "k": K, "reps": a.reps, "inner": a.inner}


def to_dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)


def event_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def ab(arms, reps, inner):
    """{name: [ms per call of every run]}: two warm-up runs per arm, then the arms alternate."""
    for _ in range(2):
        for fn in arms.values():
            event_ms(fn, inner)
    ts = {name: [] for name in arms}
    for _ in range(reps):
        for name, fn in arms.items():
            ts[name].append(round(event_ms(fn, inner), 5))
    return ts


def summary(ts, ref, new):
    return {"runs_ms": ts, "median": {k: float(np.median(v)) for k, v in ts.items()}, "min": {k: min(v) for k, v in ts.items()},
            "max": {k: max(v) for k, v in ts.items()}, "every_%s_run_below_every_%s_run" % (new, ref): bool(max(ts[new]) < min(ts[ref]))}


calls = {}
for G, L in ((10000, 300e3), (50000, 1000e3)):
    rng = np.random.default_rng(G)
    grid = np.stack([rng.uniform(0, L, G), rng.uniform(0, L, G), rng.uniform(-40000.0, 2000.0, G)], axis=1)
    xc = to_dev(grid)
    t_build = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index = engine.KnnIndex(xc)
        torch.cuda.synchronize()
        t_build.append(round((time.perf_counter() - t0) * 1e3, 4))
    node = grid[rng.integers(0, G)]
    sets = {"cloud": to_dev(node[None, :] + rng.random((N_QUERY, 3)) * OFF_RNG + OFF_MIN),
            "uniform": to_dev(np.stack([rng.uniform(0, L, N_QUERY), rng.uniform(0, L, N_QUERY), rng.uniform(-40000.0, 2000.0, N_QUERY)], axis=1))}
    res = {"cells": index.cells, "cell_m": index.cell, "build_ms": t_build}
    for name, xq in sets.items():
        want, got = engine.knn_device(xc, xq, K), engine.knn_device(xc, xq, K, index=index)
        if not torch.equal(want, got):
            raise SystemExit("knn_index_ab: the indexed table differs from the brute-force one (%d nodes, %s)" % (G, name))
        ts = ab({"brute": lambda: engine.knn_device(xc, xq, K), "indexed": lambda: engine.knn_device(xc, xq, K, index=index)}, a.reps, a.inner)
        res[name] = summary(ts, "brute", "indexed")
        print("call %d nodes, %s: %s" % (G, name, json.dumps(res[name])), flush=True)
    ladder, even = {}, None
    for n in (256, 1024, 4096, 8192, 16384, 32768, N_QUERY):       # (below 16 384 rows genie_knn is its wave-per-query kernel)
        xq = sets["cloud"][:n].contiguous()
        ts = ab({"brute": lambda: engine.knn_device(xc, xq, K), "indexed": lambda: engine.knn_device(xc, xq, K, index=index)}, 3, a.inner)
        ladder[n] = {k: float(np.median(v)) for k, v in ts.items()}
        if even is None and float(np.median(t_build)) + ladder[n]["indexed"] < ladder[n]["brute"]:
            even = n
    res["ladder_cloud_ms"] = ladder
    res["first_ladder_count_where_build_plus_indexed_is_below_brute"] = even
    print("ladder %d nodes: %s (build median %.4f ms, break-even at %s)" % (G, json.dumps(ladder), float(np.median(t_build)), even), flush=True)
    calls["nodes_%d" % G] = res
    del index, xc, sets
out["call"] = calls

if not a.skip_refine:
    n_sources = a.sources
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
    srcs = np.concatenate((geom.x_grid[nodes] + rng.normal(0.0, 2000.0, (n_sources, 3)), (t_org + rng.normal(0.0, 0.5, n_sources)).reshape(-1, 1),
                           np.full((n_sources, 1), 0.5)), axis=1)
    ident = lambda x: x                                                                        # noqa: E731
    picks = apply.ResidentPicks(P, np.arange(S), S, dev)
    leg = apply.GridLeg(net, geom.x_grid, trv)
    refine = {}
    for n_legs in (1, 3):
        legs = [leg] * n_legs

        def run(on):
            net.knn_index = on
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = apply.refine_sources(legs, picks, srcs, geom.locs, geom.t_query, max_t, OFF_MIN, OFF_RNG, N_QUERY, ident, ident, (0.0, L),
                                     (0.0, L), (-40e3, 2e3), rand=apply.PhiloxCloud((2024, 7)), ftrns2_device=ident,
                                     kernel_sig_t=synthetic.KERNEL_SIG_T, dt_embed=0.3, source_parallel=(0, 1))
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n_sources * 1e3, r[0]

        rows = {name: run(on)[1] for name, on in (("brute", False), ("indexed", True))}          # warm-up of both
        if not np.array_equal(rows["brute"], rows["indexed"]):
            raise SystemExit("knn_index_ab: the refine pass's rows differ between the arms (%d legs)" % n_legs)
        ts = {"brute": [], "indexed": []}
        for _ in range(a.reps):
            for name, on in (("brute", False), ("indexed", True)):
                ts[name].append(round(run(on)[0], 4))
        r = summary(ts, "brute", "indexed")
        r["indexed_median_below_brute_min"] = bool(np.median(ts["indexed"]) < min(ts["brute"]))
        r["rows_bit_equal"] = True
        refine["legs_%d" % n_legs] = r
        print("refine pass, %d leg(s), ms per source: %s" % (n_legs, json.dumps(r)), flush=True)
    net.knn_index = False
    out["refine"] = dict(refine, n_sources=n_sources, index_searches=net.SpatialAttention._context_index.calls)

print(json.dumps(out))
if a.out:
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "knn_index_ab.json"), "w") as f:
        f.write(json.dumps(out, indent=1))
