"""Online detection behind the online day loop, on the synthetic hour of `tools/online_feed_ab.py` (config-5 stream shape: 200 stations
x 10 000 grid nodes, 10 000 queries, ~250 picks per station and day, windows at 1 s stride), in ONE process on one GPU.

  timeout -k 10 900 python tools/online_detect_ab.py [--out FILE.json] [--seconds 3600] [--chunk 1.0] [--tail-batch 16] [--rounds 3]
                                                     [--events 60]

Two arms over the same picks, alternated `--rounds` times after one warm-up each:
  feed:         `first, block = day.feed(picks of [t, t + chunk), t + chunk)`; `block + field[:, first:...]`
  feed+detect:  the same, then `det.push(first, that sum)` (`postproc.OnlineDetector`)
Every call is timed on the host around its own synchronisation (`feed` waits once; the sum is waited for in both arms): median, 90th
percentile, maximum and total in ms per arm and round. `field` plants `--events` smooth blobs over the hour (the random-weight model's
own output holds no sources), so that candidates arrive, are held and are released; the arm reports the candidates, the sources, the
releases and the largest `held`. After each feed+detect round the sources are compared with `detect_sources_device` on the
concatenated blocks (not timed; asserted equal).

Then the candidate step alone at 10 000 rows: `StreamPeaks.push` of one block of width 8, 28 and 4096 (host clock around the call and a
synchronise: COUNT, the scan, the host read of count and bound, FILL; noise below the threshold and a peak on one row in 97) and the COUNT launch alone (HIP events), medians of 50 calls after 10, three
repeats each. No threshold: the figures are for `profiles/EXPERIMENTS.md`.

  timeout -k 10 600 python tools/online_detect_ab.py --active-cols 3000 [--max-unit-cols 300] [--active-rows 10000] [--active-width 2]
                                                     [--active-per-col 40] [--out FILE.json]

runs, instead of all of the above, the detector alone over a continuously ACTIVE stretch (`active_stretch`): per-push wall time and
`held` per quarter of the stretch, with and without a unit limit. The question it answers: does the cost of a push grow with `held`?"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genie_amd import _lib, apply, module, postproc, synthetic  # noqa: E402

DETECT = dict(thresh=0.15, src_t_kernel=5.0, dt_win=0.75, break_win=15.0, tc_win=6.75, sp_win=20e3)


def blob_field(xq, n_cols, events, dev, seed=23):
    """fp32 [Q, n_cols] on the device: `events` space-time blobs (0.7 high, 12 km and 4 columns wide) at random columns and queries."""
    rng = np.random.default_rng(seed)
    xq_d = torch.from_numpy(np.asarray(xq, dtype=np.float64)[:, :3]).to(dev)
    col = torch.arange(n_cols, dtype=torch.float64, device=dev)
    out = torch.zeros((len(xq), n_cols), dtype=torch.float32, device=dev)
    scale = torch.tensor([1.0, 1.0, 0.3], dtype=torch.float64, device=dev)
    for _ in range(int(events)):
        c, at = xq_d[int(rng.integers(len(xq)))], float(rng.uniform(10, n_cols - 10))
        lo, hi = max(int(at) - 24, 0), min(int(at) + 25, n_cols)
        d = torch.linalg.norm((xq_d - c) * scale, dim=1)
        out[:, lo:hi] += (0.7 * torch.exp(-0.5 * (d / 12e3) ** 2)[:, None] * torch.exp(-0.5 * ((col[lo:hi] - at) / 4.0) ** 2)[None, :]).float()
    return out


def stats(ms):
    ms = np.asarray(ms)
    return {"calls": len(ms), "ms_median": round(float(np.median(ms)), 3), "ms_p90": round(float(np.percentile(ms, 90)), 3),
            "ms_max": round(float(ms.max()), 3), "ms_total": round(float(ms.sum()), 1)}


def stream_peaks_times(rows, widths, dev, repeats=3, calls=50, warm=10):
    """Per width: medians (ms) of `StreamPeaks.push` on the host clock and of the COUNT launch alone on HIP events."""
    lib = _lib.load()
    rng = np.random.default_rng(3)
    out = []
    for width in widths:
        n_cols = width * (calls + warm) * repeats + 1
        block = torch.from_numpy((rng.random((rows, width)) * 0.1).astype(np.float32)).to(dev)    # noise below the threshold, as a day is
        block[::97, width // 2] = 0.5                                                              # ... with a peak on one row in 97
        sp = postproc.StreamPeaks(rows, n_cols, DETECT["thresh"], dev)
        push_ms, count_ms, found = [], [], 0
        for _ in range(repeats):
            t = []
            for k in range(calls + warm):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = sp.push(sp.seen, block)[0]
                torch.cuda.synchronize()                  # (FILL is launched after the push's host read)
                t.append((time.perf_counter() - t0) * 1e3)
                found = int(r.numel())
            push_ms.append(round(float(np.median(t[warm:])), 4))
        cin, cout = (torch.zeros(2 * rows, dtype=torch.int64, device=dev) for _ in range(2))
        counts = torch.empty(rows, dtype=torch.int32, device=dev)
        bound = torch.zeros(1, dtype=torch.int64, device=dev)
        p = lambda x: ctypes.c_void_p(x.data_ptr())
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for _ in range(repeats):
            t = []
            for k in range(calls + warm):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(lib.genie_stream_peaks_count(p(block), rows, width, width, width * (k + 1), n_cols, ctypes.c_float(DETECT["thresh"]),
                                                        p(cin), p(cout), p(counts), p(bound), st), "genie_stream_peaks_count")
                e1.record()
                e1.synchronize()
                t.append(e0.elapsed_time(e1))
            count_ms.append(round(float(np.median(t[warm:])), 4))
        out.append({"rows": rows, "width": width, "candidates_per_call": found, "push_ms_medians": push_ms, "count_launch_ms_medians": count_ms})
    return out


def active_stretch(dev, rows, n_cols, width, per_col, max_unit_cols, seed=7):
    """The detector alone on a field whose columns [200, n_cols - 200) are continuously active: `3 * per_col` of the `rows` rows carry a
    one-column spike every third column (about `per_col` candidates in every column, no gap of d columns anywhere), so that nothing
    but a forced cut releases the stretch. Blocks of `width` columns; each `det.push` is timed on the host around its own
    synchronisation. Reported per quarter of the stretch, over the pushes that released nothing: the median ms and the median `held`;
    the pushes that released, apart. `max_unit_cols` None: the argument is not passed (the tool then runs on a tree without it)."""
    rng = np.random.default_rng(seed)
    xq = np.c_[rng.uniform(0, 100e3, (rows, 2)), rng.uniform(-30e3, 0, rows)]
    ts = np.arange(n_cols) * DETECT["dt_win"] + 1000.0
    x = torch.zeros((rows, n_cols), dtype=torch.float32, device=dev)
    lo, hi = 200, n_cols - 200
    busy = torch.from_numpy(np.sort(rng.choice(rows, 3 * per_col, replace=False))).to(dev)
    col = torch.arange(lo, hi, device=dev)
    spike = ((col[None, :] + busy[:, None]) % 3 == 0).float() * (0.3 + 0.5 * torch.rand((len(busy), hi - lo), device=dev))
    x[busy, lo:hi] = spike
    args = (xq, ts, lambda p: p, DETECT["thresh"], DETECT["src_t_kernel"], DETECT["dt_win"], DETECT["break_win"], DETECT["tc_win"], DETECT["sp_win"])
    kw = {} if max_unit_cols is None else {"max_unit_cols": int(max_unit_cols)}
    out = {"rows": rows, "columns": n_cols, "block_width": width, "candidates_per_column": per_col, "max_unit_cols": max_unit_cols}
    for rep in range(2):                                  # the first pass warms up (allocator, first launches)
        det = postproc.OnlineDetector(*args, device=dev, **kw)
        ms, held, released, at = [], [], [], []
        torch.cuda.synchronize()
        for a in range(0, hi, width):                     # (the quiet end and `finish` are not part of the figures)
            t0 = time.perf_counter()
            s = det.push(a, x[:, a:a + width])
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            held.append(det.held)
            released.append(len(s) > 0)
            at.append(a)
    ms, held, released, at = np.asarray(ms), np.asarray(held), np.asarray(released), np.asarray(at)
    quarters = []
    for q in range(4):
        m = (at >= lo + q * (hi - lo) // 4) & (at < lo + (q + 1) * (hi - lo) // 4) & ~released
        quarters.append({"pushes": int(m.sum()), "ms_median": round(float(np.median(ms[m])), 3), "ms_p90": round(float(np.percentile(ms[m], 90)), 3),
                         "held_median": int(np.median(held[m]))})
    out.update({"quarters_of_the_stretch": quarters, "held_max": int(held.max()), "releasing_pushes": int(released.sum()),
                "releasing_ms_median": round(float(np.median(ms[released])), 3) if released.any() else None})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--active-cols", type=int, default=0, help="run ONLY the active-stretch measurement, on an axis of this many columns")
    ap.add_argument("--active-rows", type=int, default=10000)
    ap.add_argument("--active-width", type=int, default=2)
    ap.add_argument("--active-per-col", type=int, default=40)
    ap.add_argument("--max-unit-cols", type=int, default=0, help="the detector's limit in the active-stretch measurement (0: none)")
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--chunk", type=float, default=1.0)
    ap.add_argument("--tail-batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--events", type=int, default=60)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    if a.active_cols:
        line = {"tool": "online_detect_ab", "active_stretch": active_stretch(dev, a.active_rows, a.active_cols, a.active_width, a.active_per_col,
                                                                             a.max_unit_cols or None), "detect": DETECT,
                "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(line, indent=1) + "\n")
        return
    S, G, _, L_box, nq = synthetic.CONFIGS["cfg2_200x10k"]
    geom = synthetic.Geometry(S, G, L=L_box, n_query=nq, seed=1)
    torch.manual_seed(0)
    trv = geom.travel_times().astype(np.float32)
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=dev).eval()
    net.set_adjacencies_base(torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src), torch.from_numpy(geom.edge_attr()).to(dev),
                             torch.from_numpy(geom.locs).float().to(dev), torch.from_numpy(geom.x_grid).float().to(dev))
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
    xq = np.asarray(geom.x_query, dtype=np.float64)
    field = blob_field(xq, len(tsteps_abs), a.events, dev)
    args = (xq, tsteps_abs, lambda x: x, DETECT["thresh"], DETECT["src_t_kernel"], DETECT["dt_win"], DETECT["break_win"], DETECT["tc_win"],
            DETECT["sp_win"])

    def arm(detect):
        torch.cuda.synchronize()
        day = apply.OnlineDay(net, geom, trv, tsteps_abs, **kw)
        det = postproc.OnlineDetector(*args, device=dev) if detect else None
        blocks, srcs, ms, widths, held_max, releases = [], [], [], [], 0, 0
        feeds = [(P[l:h], t) for l, h, t in zip(np.r_[0, edges[:-1]], edges, cuts)] + [(None, np.inf)]
        for chunk, t_now in feeds:
            t0 = time.perf_counter()
            first, block = day.feed(chunk, t_now)
            block = block + field[:, first:first + block.shape[1]]
            if detect:
                s = det.push(first, block)
                if len(s):
                    releases += 1
                    srcs.append(s)
                held_max = max(held_max, det.held)
            else:
                torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            widths.append(int(block.shape[1]))
            blocks.append(block)
        res = stats(ms[:-1])                              # (the last call is `finish`: the rest of the axis in one block)
        res["finish_ms"] = round(ms[-1], 3)
        res["block_width_median"], res["block_width_max"] = int(np.median(widths[:-1])), int(max(widths[:-1]))
        if detect:
            srcs.append(det.finish())
            got = np.concatenate(srcs)
            full = torch.cat(blocks, dim=1)
            want = postproc.detect_sources_device(full, *args)
            order = lambda s: s[np.lexsort((s[:, 4], s[:, 2], s[:, 1], s[:, 0], s[:, 3]))]
            res.update({"candidates": int(postproc.row_select(full, DETECT["thresh"], 1)[0].numel()), "sources": int(len(got)), "releases": releases, "held_max": held_max,
                        "equal_to_offline_detection": bool(got.shape == want.shape and np.array_equal(order(got), order(want)))})
        return res

    arm(False)
    arm(True)
    runs = []
    for r in range(a.rounds):
        runs.append({"round": r, "feed": arm(False), "feed_detect": arm(True)})
    line = {"tool": "online_detect_ab", "shape": "config 5 stream: %d stations x %d grid nodes, %d queries, 1 s stride, tail_batch %d" % (
        S, G, nq, a.tail_batch), "seconds": a.seconds, "chunk_s": a.chunk, "picks": n, "columns": len(tsteps_abs), "events": a.events,
        "detect": DETECT, "runs": runs, "stream_peaks": stream_peaks_times(nq, (8, 28, 4096), dev), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
    if not all(r["feed_detect"]["equal_to_offline_detection"] for r in runs):
        sys.exit("online_detect_ab: the online sources are not those of the offline detection")


if __name__ == "__main__":
    main()
