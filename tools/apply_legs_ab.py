"""A day's apply loop over L source grids, two ways, in ONE process on one GPU: the config-5 stream shape of `tools/stack_ab.py` (200
stations x 10 000 grid nodes, 10 000 queries, ~250 picks per station and day, windows at 1 s stride, tail_batch = 16), L = 1 and L = 3
(three models on the same grid: the cost of a leg does not depend on where its nodes lie).

  timeout -k 10 900 python tools/apply_legs_ab.py --out DIR [--legs 1 3] [--rounds 5] [--windows 1200] [--base 200]

Arm A, what a caller had to do before: L calls of `apply_windows_device(n_grids=L, stack_on_device=True)`, each with a dense `Out_2` of
its own, added in place as they arrive (L - 1 adds; the sum is leg-major). Arm B: one `apply_windows_legs`. After one warm-up each the
arms alternate `rounds` times. A run is the loop over `base` and over `windows` consecutive windows; its figure is ms per window and
leg, (t_long - t_short) / (windows - base) / L, so that the per-call set-up drops out. Peak device memory (`max_memory_allocated`) is
taken per arm over its long loop. Prints one JSON line with EVERY run and appends it to DIR/apply_legs_ab.jsonl; with L = 1 the two
`Out_2` must be bit-equal, with L = 3 they must agree to rounding and (1 s stride: 6-8 windows per column) differ in bits."""
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
    ap.add_argument("--legs", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--windows", type=int, default=1200)
    ap.add_argument("--base", type=int, default=200)
    ap.add_argument("--tail-batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    S, G, _, L_box, nq = synthetic.CONFIGS["cfg2_200x10k"]
    geom = synthetic.Geometry(S, G, L=L_box, n_query=nq, seed=1)
    torch.manual_seed(0)
    trv = geom.travel_times().astype(np.float32)
    nets, legs = [], []
    for _ in range(max(a.legs)):
        net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=dev).eval()
        if nets:
            net.load_state_dict(nets[0].state_dict())
        net.set_adjacencies_base(torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src),
                                 torch.from_numpy(geom.edge_attr()).to(dev), torch.from_numpy(geom.locs).float().to(dev),
                                 torch.from_numpy(geom.x_grid).float().to(dev))
        nets.append(net)
        legs.append(apply.GridLeg(net, geom.x_grid, trv))
    rng = np.random.default_rng(5)
    n_day = 250 * S
    P = np.stack([np.sort(rng.uniform(0.0, 86400.0, n_day)), rng.integers(0, S, n_day).astype(np.float64), np.ones(n_day), np.ones(n_day),
                  rng.integers(0, 2, n_day).astype(np.float64)], axis=1)
    picks = apply.ResidentPicks(P, np.arange(S), S, dev)
    max_t = float(np.ceil(trv.max() + 1.0))
    tsteps_abs = np.arange(0.0, 86400.0, 0.75)
    times = 1000.3 + 1.0 * np.arange(a.windows)
    kw = dict(tsteps_abs=tsteps_abs, dt_embed=0.3, tail_batch=a.tail_batch)
    c0, c1 = int(1000 / 0.75) - 8, int((1000 + a.windows) / 0.75) + 16

    def arm_a(n, L):
        total = None
        for l in range(L):
            out, used = apply.apply_windows_device(nets[l], geom, P, trv, max_t=max_t, times=times[:n], n_grids=float(L), stack_on_device=True, **kw)
            if total is None:
                total = out
            else:
                total += out
            del out
        return total, len(used)

    def arm_b(n, L):
        out, used = apply.apply_windows_legs(legs[:L], picks, geom.x_query, geom.locs, max_t, times=times[:n], **kw)
        return out, len(used)

    def run(arm, L):
        res = {}
        for key, n in (("short", a.base), ("long", a.windows)):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            out, n_used = arm(n, L)
            torch.cuda.synchronize()
            res[key] = (time.perf_counter() - t0, n_used)
            part = out[:, c0:c1].clone()
            del out
        (t_s, n_s), (t_l, n_l) = res["short"], res["long"]
        return {"ms_per_window_and_leg": round((t_l - t_s) / (n_l - n_s) / L * 1e3, 4), "windows": [n_s, n_l],
                "wall_s": [round(t_s, 4), round(t_l, 4)], "peak_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)}, part

    results, ok = [], True
    for L in a.legs:
        run(arm_a, L)
        run(arm_b, L)
        runs = []
        for r in range(a.rounds):
            ra, out_a = run(arm_a, L)
            rb, out_b = run(arm_b, L)
            runs.append({"round": r, "A": ra, "B": rb})
        equal = bool(torch.equal(out_a, out_b))
        # K <= 8 L terms feed an element (8 windows per column at this stride); each order is within K * 2^-24 * sum|v| of the exact sum
        close = bool(torch.allclose(out_a, out_b, rtol=0.0, atol=2 * 8 * L * 2.0 ** -24 * float(out_a.abs().max())))
        ok = ok and close and (equal == (L == 1))
        results.append({"legs": L, "runs": runs, "out_2_bit_equal": equal, "out_2_equal_to_rounding": close,
                        "max_abs_out_2": float(out_b.abs().max())})
        del out_a, out_b
    line = {"tool": "apply_legs_ab", "shape": "config 5 stream: %d stations x %d grid nodes, %d queries, 1 s stride, tail_batch %d" % (
        S, G, nq, a.tail_batch), "results": results, "dense_out_2_gb": round(nq * len(tsteps_abs) * 4 / 2 ** 30, 3),
        "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "apply_legs_ab.jsonl"), "a") as f:
            f.write(json.dumps(line) + "\n")
    if not ok:
        sys.exit("apply_legs_ab: the two arms' Out_2 do not relate as they must (bit-equal for one leg, equal to rounding otherwise)")


if __name__ == "__main__":
    main()
