"""The online day loop against the offline one on the same synthetic hour, in ONE process on one GPU: the config-5 stream shape of
`tools/stack_ab.py` (200 stations x 10 000 grid nodes, 10 000 queries, ~250 picks per station and day, windows at 1 s stride).

  timeout -k 10 900 python tools/online_feed_ab.py [--out FILE.json] [--seconds 3600] [--chunk 1.0] [--tail-batch 16] [--rounds 3] [--legs 1]

Online arm: `apply.OnlineDay` fed the hour's picks in chunks of `--chunk` seconds (`feed(picks of [t, t + chunk), t + chunk)`, then
`finish()`); every `feed` is timed on the host around its own synchronisation: median, 90th percentile and maximum in ms, the number of
calls, the windows the busiest call ran, the ring's size and the peak device memory of the arm. Offline arm: one
`apply_windows_device(stack_on_device=True)` over the same `tsteps_abs` / `times`, wall time of the whole loop. After one warm-up each
the arms alternate `--rounds` times; every run is printed. The two `Out_2` are asserted bit-equal. No threshold: the figures are for
`profiles/EXPERIMENTS.md`.

`--legs N` (1..32): N models with weights of their own on N source grids over the one station set (leg l: 10 000 - 16 l nodes of the
same seed, which leaves the stations where they are); the online arm is `OnlineDay(legs, ...)`, the offline arm
`apply_windows_legs(legs, ...)` on the same resident picks. With N = 1 the arms are the ones above."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genie_amd import apply, module, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--chunk", type=float, default=1.0)
    ap.add_argument("--tail-batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    S, G, _, L_box, nq = synthetic.CONFIGS["cfg2_200x10k"]
    geom = synthetic.Geometry(S, G, L=L_box, n_query=nq, seed=1)
    torch.manual_seed(0)
    trv = geom.travel_times().astype(np.float32)

    def model_on(g):
        net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=dev).eval()
        net.set_adjacencies_base(torch.from_numpy(g.A_sta_sta), torch.from_numpy(g.A_src_src), torch.from_numpy(g.edge_attr()).to(dev),
                                 torch.from_numpy(g.locs).float().to(dev), torch.from_numpy(g.x_grid).float().to(dev))
        return net

    net = model_on(geom)
    legs = [apply.GridLeg(net, geom.x_grid, trv)]
    for l in range(1, a.legs):                       # (in leg order: the models draw their weights from the one seeded stream)
        g = synthetic.Geometry(S, G - 16 * l, L=L_box, n_query=nq, seed=1)
        assert np.array_equal(g.locs, geom.locs)
        trv_l = g.travel_times().astype(np.float32)
        assert trv_l.max() + 1.0 <= np.ceil(trv.max() + 1.0)
        legs.append(apply.GridLeg(model_on(g), g.x_grid, trv_l))
    rng = np.random.default_rng(5)
    t_lo = 1000.0
    n = int(250 * S * a.seconds / 86400.0)
    P = np.stack([np.sort(rng.uniform(t_lo, t_lo + a.seconds, n)), rng.integers(0, S, n).astype(np.float64), np.ones(n), np.ones(n),
                  rng.integers(0, 2, n).astype(np.float64)], axis=1)
    max_t = float(np.ceil(trv.max() + 1.0))
    tsteps_abs = np.arange(t_lo - max_t - 6.0, t_lo + a.seconds + 6.0, 0.75)
    times = t_lo - max_t + 0.3 + 1.0 * np.arange(int(a.seconds + max_t))
    kw = dict(times=times, max_t=max_t, dt_embed=0.3, tail_batch=a.tail_batch)
    cuts = t_lo + a.chunk * np.arange(1, int(np.ceil((a.seconds + max_t + 12.0) / a.chunk)) + 1)
    edges = np.searchsorted(P[:, 0], cuts, side="left")
    resident = apply.ResidentPicks(P, np.arange(S), S, dev) if a.legs > 1 else None

    def online():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        day = apply.OnlineDay(net if a.legs == 1 else legs, geom, trv, tsteps_abs, **kw)
        blocks, ms, ran, lo = [], [], [], 0
        for t_now, hi in zip(cuts, edges):
            before = day.n_run
            t0 = time.perf_counter()
            blocks.append(day.feed(P[lo:hi], t_now)[1])
            ms.append((time.perf_counter() - t0) * 1e3)
            ran.append(day.n_run - before)
            lo = hi
        blocks.append(day.finish()[1])
        out = torch.cat(blocks, dim=1)
        ms = np.asarray(ms)
        return out, {"feeds": len(ms), "feed_ms_median": round(float(np.median(ms)), 3), "feed_ms_p90": round(float(np.percentile(ms, 90)), 3),
                     "feed_ms_max": round(float(ms.max()), 3), "feed_ms_total": round(float(ms.sum()), 1), "windows_run": len(day.times_used),
                     "windows_in_busiest_feed": int(max(ran)), "ring_cols": day.ring_cols, "pick_store_capacity": day.picks.capacity,
                     "peak_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)}

    def offline():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        if a.legs == 1:
            out, used = apply.apply_windows_device(net, geom, P, trv, tsteps_abs=tsteps_abs, stack_on_device=True, **kw)
        else:
            out, used = apply.apply_windows_legs(legs, resident, geom.x_query, geom.locs, max_t, tsteps_abs=tsteps_abs, times=times,
                                                 dt_embed=0.3, tail_batch=a.tail_batch)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        return out, {"wall_s": round(wall, 4), "windows_run": len(used), "ms_per_window": round(wall / max(len(used), 1) * 1e3, 4),
                     "peak_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)}

    online()
    offline()
    runs = []
    for r in range(a.rounds):
        out_on, res_on = online()
        out_off, res_off = offline()
        equal = bool(torch.equal(out_on, out_off))
        runs.append({"round": r, "online": res_on, "offline": res_off, "out_2_bit_equal": equal})
        del out_on, out_off
    line = {"tool": "online_feed_ab", "legs": a.legs, "shape": "config 5 stream: %d stations x %d grid nodes, %d queries, 1 s stride, tail_batch %d" % (
        S, G, nq, a.tail_batch), "seconds": a.seconds, "chunk_s": a.chunk, "picks": n, "columns": len(tsteps_abs), "runs": runs,
        "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
    if not all(r["out_2_bit_equal"] for r in runs):
        sys.exit("online_feed_ab: the online blocks are not the offline Out_2")


if __name__ == "__main__":
    main()
