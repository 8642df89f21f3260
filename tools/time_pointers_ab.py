"""Host against device builder of the association heads' time-pointer tables: `graph.time_pointers` (the Python loop over stations and
phases) against `engine.time_pointers_device` (genie_time_pointers), on straight-ray travel times of the synthetic geometry
(`synthetic.CONFIGS`: box side, depth range, VP / VS), dt = 0.6 s, k = 10, win = 6 s.

  config 2 (200 x 10 000)    both arms, alternated `--reps` times after a warm-up; the tables asserted equal (np.array_equal)
  config 4 (2000 x 50 000)   the device arm; the host arm only with --host-big (it takes minutes)

The device time is a host clock around the call and a device synchronise: it includes the upload of `dt_partition`, the scratch
allocation and every kernel, and excludes loading the library (done by the warm-up). The host arm gets the travel times as the
[G, S, 2] fp32 numpy array it takes. One JSON line per size on stdout, and in `--out DIR/time_pointers_ab.json` when given.

    python tools/time_pointers_ab.py [--out DIR] [--reps 5] [--host-big] [--sizes 200x10000,2000x50000]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genie_amd import engine, graph, synthetic  # noqa: E402

DT, K, WIN = 0.6, 10, 6.0


def travel_times(n_sta, n_grid, L, dev, seed=1):
    """fp32 [G * S, 2] straight-ray P / S travel times on the device (positions drawn as `synthetic.Geometry` draws them)."""
    rng = np.random.default_rng(seed)
    locs = np.stack([rng.uniform(0, L, n_sta), rng.uniform(0, L, n_sta), rng.uniform(0.0, 2000.0, n_sta)], axis=1)
    grid = np.stack([rng.uniform(0, L, n_grid), rng.uniform(0, L, n_grid), rng.uniform(-40000.0, 2000.0, n_grid)], axis=1)
    locs, grid = torch.from_numpy(locs).to(dev), torch.from_numpy(grid).to(dev)
    out = torch.empty((n_grid, n_sta, 2), dtype=torch.float32, device=dev)
    for g0 in range(0, n_grid, 4096):
        d = torch.cdist(grid[g0:g0 + 4096], locs)
        out[g0:g0 + 4096, :, 0] = (d / synthetic.VP).float()
        out[g0:g0 + 4096, :, 1] = (d / synthetic.VS).float()
    return out.reshape(-1, 2)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def run(n_sta, n_grid, reps, with_host, dev):
    L = next((c[3] for c in synthetic.CONFIGS.values() if c[0] == n_sta and c[1] == n_grid), 300e3)
    tl = travel_times(n_sta, n_grid, L, dev)
    max_t = float(np.ceil(tl.max().item()))
    kw = dict(max_t=max_t, dt=DT, k=K, win=WIN)
    device_arm = lambda: engine.time_pointers_device(tl, n_sta, **kw)
    _, got = timed(device_arm)                                  # warm-up: library load, code objects, allocator
    res = {"n_sta": n_sta, "n_grid": n_grid, "n_t": int(got[2].size), "k": K, "dt": DT, "max_t": max_t,
           "scratch_MB": round(engine._lib.load().genie_time_pointers_scratch_bytes(n_sta * n_grid, n_sta, int(got[2].size)) / 2 ** 20, 1)}
    host_s, dev_s = [], []
    trv = tl.cpu().numpy().reshape(n_grid, n_sta, 2) if with_host else None
    for r in range(reps):
        if with_host:
            t0 = time.perf_counter()
            want = graph.time_pointers(trv, **kw)
            host_s.append(time.perf_counter() - t0)
        t, got = timed(device_arm)
        dev_s.append(t)
        if with_host and r == 0:
            same = (np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
                    and np.array_equal(got[2], want[2]))
            assert same, "device and host tables differ at %d x %d" % (n_sta, n_grid)
            res["tables_equal"] = True
    res["device_ms"] = {"median": round(1e3 * statistics.median(dev_s), 3), "min": round(1e3 * min(dev_s), 3), "max": round(1e3 * max(dev_s), 3),
                        "runs": len(dev_s)}
    if with_host:
        res["host_ms"] = {"median": round(1e3 * statistics.median(host_s), 1), "min": round(1e3 * min(host_s), 1),
                          "max": round(1e3 * max(host_s), 1), "runs": len(host_s)}
        res["host_over_device"] = round(statistics.median(host_s) / statistics.median(dev_s), 1)
    else:
        res["host_ms"] = "not timed"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-big", action="store_true", help="time the host builder at sizes above 200 x 10 000 as well (minutes)")
    ap.add_argument("--sizes", default="200x10000,2000x50000")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for size in a.sizes.split(","):
        S, G = (int(v) for v in size.split("x"))
        big = S * G > 200 * 10000
        res = run(S, G, a.reps, with_host=(not big) or a.host_big, dev=dev)
        print(json.dumps(res), flush=True)
        lines.append(res)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "time_pointers_ab.json"), "w") as f:
            for res in lines:
                f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
