"""What the per-window stacking launches of the apply loop cost: the config-5 stream shape of `bench.py --mode stream` (200 stations x
10 000 grid nodes, 10 000 queries, ~250 picks per station and day, windows at 1 s stride, tail_batch = 16) through
`apply.apply_windows_device`, with `stack_on_device` off / on / off in ONE process, so that the three figures share clocks and box.

  timeout -k 10 600 python tools/stack_ab.py --out DIR [--windows 1200] [--base 200]

Each arm runs the loop twice, over `base` and over `windows` consecutive windows, and reports (t_long - t_short) / (windows - base):
the per-call set-up (pick upload, travel-time table, a zeroed day-sized Out_2) drops out. One warm-up loop first. Prints one JSON line
and appends it to DIR/stack_ab.jsonl; the `Out_2` of the fused arm is checked bit-equal to the torch arms'."""
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
    ap.add_argument("--windows", type=int, default=1200)
    ap.add_argument("--base", type=int, default=200)
    ap.add_argument("--tail-batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    S, G, _, L, nq = synthetic.CONFIGS["cfg2_200x10k"]
    geom = synthetic.Geometry(S, G, L=L, n_query=nq, seed=1)
    torch.manual_seed(0)
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=dev).eval()
    net.set_adjacencies_base(torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src), torch.from_numpy(geom.edge_attr()).to(dev),
                             torch.from_numpy(geom.locs).float().to(dev), torch.from_numpy(geom.x_grid).float().to(dev))
    rng = np.random.default_rng(5)
    n_day = 250 * S
    P = np.stack([np.sort(rng.uniform(0.0, 86400.0, n_day)), rng.integers(0, S, n_day).astype(np.float64), np.ones(n_day), np.ones(n_day),
                  rng.integers(0, 2, n_day).astype(np.float64)], axis=1)
    trv = geom.travel_times().astype(np.float32)
    max_t = float(np.ceil(trv.max() + 1.0))
    tsteps_abs = np.arange(0.0, 86400.0, 0.75)
    times = 1000.3 + 1.0 * np.arange(a.windows)

    def loop(n, fused):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, used = apply.apply_windows_device(net, geom, P, trv, tsteps_abs=tsteps_abs, max_t=max_t, dt_embed=0.3, times=times[:n],
                                               tail_batch=a.tail_batch, stack_on_device=fused)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out, len(used)

    loop(a.base, False)
    loop(a.base, True)
    arms, keep = [], {}
    for name, fused in (("torch_1", False), ("fused", True), ("torch_2", False)):
        t_s, _, n_s = loop(a.base, fused)
        t_l, out, n_l = loop(a.windows, fused)
        c0, c1 = int(1000 / 0.75) - 8, int((1000 + a.windows) / 0.75) + 16
        keep[name] = out[:, c0:c1].clone()
        del out
        arms.append({"arm": name, "stack_on_device": fused, "ms_per_window": round((t_l - t_s) / (n_l - n_s) * 1e3, 4),
                     "windows": [n_s, n_l], "wall_s": [round(t_s, 4), round(t_l, 4)]})
    equal = bool(torch.equal(keep["fused"], keep["torch_1"]) and torch.equal(keep["torch_2"], keep["torch_1"]))
    line = {"tool": "stack_ab", "shape": "config 5 stream: %d stations x %d grid nodes, %d queries, 1 s stride, tail_batch %d" % (S, G, nq, a.tail_batch),
            "arms": arms, "out_2_bit_equal": equal, "max_abs_out_2": float(keep["torch_1"].abs().max()),
            "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "stack_ab.jsonl"), "a") as f:
            f.write(json.dumps(line) + "\n")
    if not equal:
        sys.exit("stack_ab: the fused Out_2 differs from the torch Out_2")


if __name__ == "__main__":
    main()
