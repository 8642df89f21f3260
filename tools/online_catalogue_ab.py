"""The online catalogue behind the online day loop, on the synthetic hour of `tools/online_detect_ab.py` (config-5 stream shape: 200
stations x 10 000 grid nodes, 10 000 queries, windows at 1 s stride), in ONE process on one GPU.

  timeout -k 10 900 python tools/online_catalogue_ab.py [--out FILE.json] [--seconds 3600] [--chunk 1.0] [--rounds 3] [--events 60]
                                                        [--n-rand-query 2048] [--skip-day]

Two arms over the same picks, alternated `--rounds` times after one warm-up each, every call timed on the host around its own wait:
  feed+detect:  `det.push(*day.feed(chunk, t))` with the planted field of online_detect_ab added to the block
  catalogue:    `apply.OnlineCatalogue.push(chunk, t)` on the same day and field (refine, association, second LocalMarching)
median, 90th percentile, maximum and total in ms per arm and round, and what the catalogue arm produced (sources released, retained,
the largest `pending`, `undecided` and live pick count).

Then one source's pick lists through `ResidentPicks.pick_inputs` (torch: slice, sort, gathers) and through `pick_inputs_device`
(genie_pick_lists) at 64, 1 024 and 8 192 picks of 200 stations: host clock around the call and a synchronise, medians of 50 calls
after 10, three repeats each. No threshold: the figures are for `profiles/EXPERIMENTS.md`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from genie_amd import apply, graph, module, postproc, synthetic  # noqa: E402
from online_detect_ab import DETECT, blob_field, stats  # noqa: E402


def pick_lists_times(sizes, n_sta, dev, repeats=3, calls=50, warm=10):
    rng = np.random.default_rng(3)
    out = []
    for n in sizes:
        P = np.stack([np.sort(rng.uniform(1000.0, 1030.0, n)), rng.integers(0, n_sta, n).astype(np.float64), np.ones(n), np.ones(n),
                      rng.integers(0, 2, n).astype(np.float64)], axis=1)
        picks = apply.ResidentPicks(P, np.arange(n_sta), n_sta, dev)
        row = {"picks": n, "stations": n_sta}
        for name, fn in (("torch_ms_medians", picks.pick_inputs), ("kernel_ms_medians", picks.pick_inputs_device)):
            med = []
            for _ in range(repeats):
                t = []
                for _ in range(calls + warm):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(1000.0, 24.0, 3.0, 10.0)
                    torch.cuda.synchronize()
                    t.append((time.perf_counter() - t0) * 1e3)
                med.append(round(float(np.median(t[warm:])), 4))
            row[name] = med
        a, b = picks.pick_inputs(1000.0, 24.0, 3.0, 10.0), picks.pick_inputs_device(1000.0, 24.0, 3.0, 10.0)
        row["equal"] = bool(all(torch.equal(x, y) for x, y in zip(a, b)) and a[0].shape[0] == n)
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--chunk", type=float, default=1.0)
    ap.add_argument("--tail-batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--events", type=int, default=60)
    ap.add_argument("--n-rand-query", type=int, default=2048)
    ap.add_argument("--skip-day", action="store_true", help="only the pick-list timings")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    S, G, _, L_box, nq = synthetic.CONFIGS["cfg2_200x10k"]
    line = {"tool": "online_catalogue_ab", "pick_lists": pick_lists_times((64, 1024, 8192), S, dev), "device": torch.cuda.get_device_name(0)}
    if not a.skip_day:
        geom = synthetic.Geometry(S, G, L=L_box, n_query=nq, seed=1)
        torch.manual_seed(0)
        trv_t = geom.travel_times().astype(np.float32)
        max_t = float(np.ceil(trv_t.max() + 1.0))
        sig = synthetic.KERNEL_SIG_T
        edges_p, edges_s, dt_part = graph.time_pointers(trv_t, max_t=max_t, dt=sig / 5.0, k=10, win=2.0 * sig)
        f = lambda x: torch.from_numpy(np.ascontiguousarray(x)).float().to(dev)
        net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=dev).eval()
        net.set_adjacencies_base(torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src), torch.from_numpy(geom.edge_attr()).to(dev),
                                 f(geom.locs), f(geom.x_grid), torch.from_numpy(edges_p).to(dev), torch.from_numpy(edges_s).to(dev), f(dt_part),
                                 f(trv_t.reshape(-1, 2)))
        rng = np.random.default_rng(5)
        t_lo = 1000.0
        n = int(250 * S * a.seconds / 86400.0)
        P = np.stack([np.sort(rng.uniform(t_lo, t_lo + a.seconds, n)), rng.integers(0, S, n).astype(np.float64), np.ones(n), np.ones(n),
                      rng.integers(0, 2, n).astype(np.float64)], axis=1)
        tsteps_abs = np.arange(t_lo - max_t - 6.0, t_lo + a.seconds + 6.0, 0.75)
        times = t_lo - max_t + 0.3 + 1.0 * np.arange(int(a.seconds + max_t))
        kw = dict(times=times, max_t=max_t, dt_embed=0.3, tail_batch=a.tail_batch)
        cuts = t_lo + a.chunk * np.arange(1, int(np.ceil((a.seconds + max_t + 12.0) / a.chunk)) + 1)
        edges = np.searchsorted(P[:, 0], cuts, side="left")
        xq = np.asarray(geom.x_query, dtype=np.float64)
        field = blob_field(xq, len(tsteps_abs), a.events, dev)
        ident = lambda x: x
        args = (xq, tsteps_abs, ident, DETECT["thresh"], DETECT["src_t_kernel"], DETECT["dt_win"], DETECT["break_win"], DETECT["tc_win"],
                DETECT["sp_win"])
        ranges = ((0.0, L_box), (0.0, L_box), (-40e3, 2e3))

        def trv(locs, srcs):
            d = torch.linalg.norm(locs[None, :, :] - srcs[:, None, :], dim=2)
            return torch.stack((d / synthetic.VP, d / synthetic.VS), dim=2)

        def arm(catalogue):
            torch.cuda.synchronize()
            day = apply.OnlineDay(net, geom, trv_t, tsteps_abs, **kw)
            feed = day.feed
            day.feed = lambda c, t: (lambda first, block: (first, block + field[:, first:first + block.shape[1]]))(*feed(c, t))
            det = postproc.OnlineDetector(*args, device=dev)
            cat = apply.OnlineCatalogue(day, det, geom.locs, trv, geom.t_query, ident, ident, *ranges, np.array([[-5e3, -5e3, -3e3]]),
                                        np.array([[10e3, 10e3, 6e3]]), a.n_rand_query, DETECT["tc_win"], DETECT["sp_win"],
                                        rand=apply.PhiloxCloud(11), ftrns2_device=ident) if catalogue else None
            ms, seen = [], {"released": 0, "retained": 0, "pending_max": 0, "undecided_max": 0, "live_picks_max": 0}
            feeds = [(P[l:h], t) for l, h, t in zip(np.r_[0, edges[:-1]], edges, cuts)]
            for chunk, t_now in feeds:
                t0 = time.perf_counter()
                if catalogue:
                    out = cat.push(chunk, t_now)
                    seen["released"] += len(out["srcs"])
                    seen["retained"] += len(out["srcs_refined"])
                    seen["pending_max"], seen["undecided_max"] = max(seen["pending_max"], cat.pending), max(seen["undecided_max"], cat.undecided)
                    seen["live_picks_max"] = max(seen["live_picks_max"], len(day.picks))
                else:
                    det.push(*day.feed(chunk, t_now))
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            last = cat.finish() if catalogue else (det.push(*day.feed(None, np.inf)), det.finish())
            torch.cuda.synchronize()
            res = stats(ms)
            res["finish_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            if catalogue:
                seen["released"] += len(last["srcs"])
                seen["retained"] += len(last["srcs_refined"])
                res.update(seen)
            return res

        arm(False)
        arm(True)
        line.update({"shape": "config 5 stream: %d stations x %d grid nodes, %d queries, 1 s stride, tail_batch %d" % (S, G, nq, a.tail_batch),
                     "seconds": a.seconds, "chunk_s": a.chunk, "picks": n, "events": a.events, "n_rand_query": a.n_rand_query,
                     "runs": [{"round": r, "feed_detect": arm(False), "catalogue": arm(True)} for r in range(a.rounds)]})
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
