"""One GPU: what source detection from a column band costs against the dense detection it replaces, on a day-sized `Out_2` resident on
the device. 10 000 queries in a 300 km box, 0.75 s steps over 86 400 s (4.6 GB of fp32); every event is a 25 km Gaussian in space
around a query (height 0.3..1) times a 3 s Gaussian in time whose centre is jittered per query by half a second, zero elsewhere;
thresh 0.15, distance rule 10 columns, `break_win` 15 s, `tc_win` 6.75 s, `sp_win` 27 km (the day of tools/detect_time.py, as a matrix).
The band is the whole axis (`apply.window_band_plan` of one rank): no strip to wait for, no gather.

  python tools/band_detect_time.py --events 1000 --repeats 7 --out FILE.json

Timed, each after one warm-up call, `repeats` calls alternating between the two of a pair, wall time around a call that ends in a
device-to-host copy (so the device has finished):
  * `postproc.detect_sources_device(Out_2, ...)` against `postproc.detect_sources_banded(BandedOut2, ...)`: the whole detection;
  * `postproc.row_select(Out_2, thresh, 1)` against `postproc.band_peaks(...)`: the candidate step alone (count pass, offsets, fill pass;
    `bytes_read` = two passes over the matrix, `gb_per_s` = that over the median call time, not a kernel time).
The sources of the two must be equal row for row and the candidates triplet for triplet, or the tool fails. Prints one JSON object and
writes it to FILE.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genie_amd import apply, postproc  # noqa: E402

Q, DT_WIN, SRC_T_KERNEL, THRESH, DAY = 10000, 0.75, 5.0, 0.15, 86400.0
TC_WIN, SP_WIN, BREAK_WIN, SCALE_DEPTH = SRC_T_KERNEL * 1.35, 20e3 * 1.35, 15.0, 0.2
SIG_T, HALF = 3.0, 32                                   # the events' width in time; columns written on either side of an event's centre


def day(n_ev, q, n_cols, dev, seed=3):
    """(Out_2 [q, n_cols] fp32 on `dev`, query positions, time axis) of a day with n_ev events."""
    rng = np.random.default_rng(seed + n_ev)
    xq = np.c_[rng.uniform(0, 300e3, (q, 2)), rng.uniform(-40e3, 0, q)]
    ts = np.arange(n_cols) * DT_WIN
    out = torch.zeros((q, n_cols), dtype=torch.float32, device=dev)
    for _ in range(n_ev):
        c, t0, a = xq[rng.integers(0, q)], rng.uniform(50, ts[-1] - 50), rng.uniform(0.3, 1.0)
        d = np.linalg.norm((xq - c) * np.array([1, 1, 0.3]), axis=1)
        amp = a * np.exp(-0.5 * (d / 25e3) ** 2)
        idx = np.flatnonzero(amp > 0.01)
        t_row = t0 + rng.normal(0, 0.5, idx.size)
        c0 = int(round(t0 / DT_WIN))
        cols = np.arange(max(c0 - HALF, 0), min(c0 + HALF + 1, n_cols))
        blob = amp[idx, None] * np.exp(-0.5 * ((ts[cols][None, :] - t_row[:, None]) / SIG_T) ** 2)
        out[torch.from_numpy(idx).to(dev)[:, None], torch.from_numpy(cols).to(dev)[None, :]] += torch.from_numpy(blob.astype(np.float32)).to(dev)
    return out, xq, ts


def alternate(f, g, repeats):
    """Wall times of `repeats` calls of f and of g, alternating, after one warm-up call of each (whose results are returned)."""
    first = f(), g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(repeats):
        for fn, acc in ((f, tf), (g, tg)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                         # ends in a copy to the host
            acc.append(time.perf_counter() - t0)
    return first, tf, tg


def _ms(ts):
    return dict(median_ms=round(1e3 * float(np.median(ts)), 3), all_ms=[round(1e3 * t, 3) for t in ts])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=Q)
    ap.add_argument("--cols", type=int, default=int(DAY / DT_WIN))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="build/band_detect_time.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("band_detect_time: needs a GPU")
    dev = "cuda:0"
    Out_2, xq, ts = day(a.events, a.queries, a.cols, dev)
    plan = apply.window_band_plan(np.arange(a.cols).reshape(1, -1), a.cols, 1, n_rows=a.queries)
    banded = apply.BandedOut2(Out_2, 0, plan, complete=True)
    assert (banded.b_lo, banded.b_hi, banded.o_lo, banded.o_hi) == (0, a.cols, 0, a.cols)
    args = (xq, ts, lambda x: x, THRESH, SRC_T_KERNEL, DT_WIN, BREAK_WIN, TC_WIN, SP_WIN, SCALE_DEPTH)
    line = dict(gpu=torch.cuda.get_device_name(0), queries=a.queries, cols=a.cols, events=a.events, repeats=a.repeats,
                out2_bytes=4 * a.queries * a.cols, band_bytes=plan["band_bytes"][0])
    print("day built", flush=True)

    infos = []
    dense = lambda: postproc.detect_sources_device(Out_2, *args)

    def bands():
        srcs, info = postproc.detect_sources_banded(banded, *args)
        infos.append(info)
        return srcs

    (want, got), t_dense, t_band = alternate(dense, bands, a.repeats)
    assert all(i["fallback"] is None for i in infos), infos[0]
    assert len(want) > 0 and want.dtype == got.dtype and np.array_equal(want, got), "the banded sources differ from the dense ones"
    line.update(candidates=infos[0]["candidates"][0], sources=len(want), sources_equal=True,
                detect_sources_device=_ms(t_dense), detect_sources_banded=_ms(t_band))
    print("detection timed", flush=True)

    host3 = lambda r, c, v: (r.cpu().numpy(), c.cpu().numpy(), v.cpu().numpy())
    select = lambda: host3(*postproc.row_select(Out_2, THRESH, 1))
    peaks = lambda: host3(*postproc.band_peaks(Out_2, 0, 0, a.cols, a.cols, THRESH)[:3])
    (want3, got3), t_sel, t_peaks = alternate(select, peaks, a.repeats)
    assert all(np.array_equal(x, y) for x, y in zip(want3, got3)), "the band candidates differ from row_select's"
    two_passes = 2 * 4 * a.queries * a.cols
    for name, t in (("row_select", t_sel), ("band_peaks", t_peaks)):
        line[name] = dict(_ms(t), bytes_read=two_passes, gb_per_s=round(two_passes / float(np.median(t)) / 1e9, 1))
    line["candidates_equal"] = True
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
