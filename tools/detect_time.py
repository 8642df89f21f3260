"""Source detection after the peaks, host against device, on day-sized synthetic candidates: 10 000 queries in a 300 km box, 0.75 s
steps over 86 400 s, every event lighting up the queries within a 25 km Gaussian above thresh = 0.15 (peak time jittered by a step or
so), tc_win = 6.75 s, sp_win = 27 km, break_win = 15 s. The peak triplets are built directly (a dense Out_2 of that day is 4.6 GB).

  python tools/detect_time.py --host   --events 200 1000 3000 --out DIR     # no GPU: distance rule + grouping + LocalMarching of
                                                                            # genie_amd/postproc.py, one pass; survivors saved
  python tools/detect_time.py --device --events 200 1000 3000 --out DIR     # the same triplets through the HIP kernels: one warm-up
                                                                            # call, median of 5, wall time including the copy of the
                                                                            # survivors; equal to the saved host survivors if present
Each prints one JSON line per size and appends it to DIR/detect_time.jsonl."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genie_amd import postproc  # noqa: E402

Q, DT_WIN, SRC_T_KERNEL, THRESH, DAY = 10000, 0.75, 5.0, 0.15, 86400.0
TC_WIN, SP_WIN, BREAK_WIN, SCALE_DEPTH = SRC_T_KERNEL * 1.35, 20e3 * 1.35, 15.0, 0.2
DISTANCE = int(1.5 * SRC_T_KERNEL / DT_WIN)


def candidates(n_ev, seed=3):
    """Row-major peak triplets (row, col, height) of a day with n_ev events, the query positions and the time axis."""
    rng = np.random.default_rng(seed + n_ev)
    xq = np.c_[rng.uniform(0, 300e3, (Q, 2)), rng.uniform(-40e3, 0, Q)]
    ts = np.arange(int(DAY / DT_WIN)) * DT_WIN
    R, C, V = [], [], []
    for _ in range(n_ev):
        c, t0, a = xq[rng.integers(0, Q)], rng.uniform(50, DAY - 50), rng.uniform(0.3, 1.0)
        d = np.linalg.norm((xq - c) * np.array([1, 1, 0.3]), axis=1)
        amp = a * np.exp(-0.5 * (d / 25e3) ** 2)
        idx = np.flatnonzero(amp > THRESH)
        R.append(idx)
        C.append(np.round((t0 + rng.normal(0, 0.5, idx.size)) / DT_WIN).astype(np.int64))
        V.append(amp[idx].astype(np.float32))
    r, c, v = np.concatenate(R), np.concatenate(C), np.concatenate(V)
    _, first = np.unique(r * len(ts) + c, return_index=True)                     # one peak per (row, column), row-major
    return r[first], c[first], v[first], xq, ts


def _key(a):
    return a[np.lexsort(a.T[::-1])]


def host(r, c, v, xq, ts):
    t0 = time.time()
    keep = np.ones(r.size, bool)
    starts = np.flatnonzero(np.r_[True, r[1:] != r[:-1]])
    for a, b in zip(starts, np.r_[starts[1:], r.size]):
        if b - a > 1:
            keep[a:b] = postproc.select_by_peak_distance(c[a:b], v[a:b], DISTANCE)
    t_dist = time.time() - t0
    r, c, v = r[keep], c[keep], v[keep]
    srcs = np.concatenate((xq[r], ts[c].reshape(-1, 1), v.astype(np.float64).reshape(-1, 1)), axis=1)
    srcs = srcs[np.argsort(srcs[:, 3])]
    t0 = time.time()
    groups = postproc.group_sources(srcs, BREAK_WIN)
    out = [g if len(g) == 1 else postproc.local_marching(g, lambda x: x, tc_win=TC_WIN, sp_win=SP_WIN, scale_depth=SCALE_DEPTH,
                                                         n_steps_max=2, use_directed=False) for g in groups]
    t_march = time.time() - t0
    out = np.vstack(out)
    return out[np.argsort(out[:, 3])], dict(after_distance=int(r.size), groups=len(groups), largest_group=max(len(g) for g in groups),
                                            host_distance_s=round(t_dist, 3), host_marching_s=round(t_march, 3))


def device(r, c, v, xq, ts, repeats=5):
    import torch
    dev = "cuda:0"
    counts = np.bincount(r, minlength=Q)
    offsets = torch.from_numpy(np.cumsum(counts) - counts).to(dev)
    rd, cd, vd = (torch.from_numpy(a).to(dev) for a in (r.astype(np.int32), c.astype(np.int32), v))

    def once():
        keep = postproc._peak_distance_keep(offsets, cd, vd, DISTANCE)
        return postproc._sources_from_peaks(rd[keep], cd[keep], vd[keep], xq, ts, lambda x: x, BREAK_WIN, TC_WIN, SP_WIN, SCALE_DEPTH)

    out = once()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.time()
        again = once()                                                            # ends in the copy of the survivors: synchronous
        times.append(time.time() - t0)
        assert np.array_equal(again, out)
    return out, dict(device_s_median=round(float(np.median(times)), 5), device_s_all=[round(x, 5) for x in times],
                     gpu=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--events", type=int, nargs="+", default=[200, 1000, 3000])
    ap.add_argument("--out", default="build/detect_time")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for n_ev in a.events:
        r, c, v, xq, ts = candidates(n_ev)
        line = dict(events=n_ev, candidates=int(r.size), machine=os.uname().nodename)
        saved = os.path.join(a.out, "host_survivors_%d.npy" % n_ev)
        if a.host:
            srcs, info = host(r, c, v, xq, ts)
            np.save(saved, srcs)
            line.update(info, survivors=len(srcs))
        if a.device:
            srcs_d, info = device(r, c, v, xq, ts)
            line.update(info, survivors=len(srcs_d), equals_host=None)
            if os.path.exists(saved):
                want = np.load(saved)
                line["equals_host"] = bool(want.shape == srcs_d.shape and np.array_equal(_key(want), _key(srcs_d)))
                assert line["equals_host"], "device survivors differ from the host's at %d events" % n_ev
        print(json.dumps(line), flush=True)
        with open(os.path.join(a.out, "detect_time.jsonl"), "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
