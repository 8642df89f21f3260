#!/usr/bin/env python
"""L2 fills of k_stage2_h2u for a synthetic config, modelled on the CPU: the real block plan (genie_amd/csrc/s2u_plan.hpp) swept in
the kernel's item order, the 128-byte-line requests of c, the wu station gathers, the wv union staging, the edge fragments and the
mask replayed through one LRU L2 per XCD (tests/s2u_traffic_model.cpp, compiled here). Prints the fill bytes per buffer and per
cause (first touch / re-fetch inside an XCD after eviction / the same line fetched by another XCD) and, for comparison with a
counter run, the figure FETCH_SIZE would show if it tallied every fill at 64 B (its documented behaviour for wide streams).
Usage: python tools/s2u_traffic.py [config] [--L 1 4] [--bpc 2] [--l2-mib 4] [--order group|tile] [--jitter 0.25] [--stream-kib 256]   (no GPU needed)"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from genie_amd import engine, graph, synthetic  # noqa: E402
from tools.s2u_gate import neighbour_table  # noqa: E402

SRC = os.path.join(REPO, "tests", "s2u_traffic_model.cpp")
BUFFERS = ("c", "wu", "wv", "frag", "mask")


def station_table(geom):
    """int32 [S][8]: the station neighbours in processing order (genie_set_station_order: same neighbours, same edge order, new labels)."""
    S = geom.locs.shape[0]
    nbr = np.asarray(graph.neighbour_table(geom.A_sta_sta, S))
    assert nbr.shape == (S, 8)
    perm = np.asarray(engine.sfc_order(geom.locs))
    inv = np.empty(S, np.int32)
    inv[perm] = np.arange(S, dtype=np.int32)
    return np.ascontiguousarray(inv[nbr[perm]].astype(np.int32))


def compile_model(exe, flags=("-O2",)):
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", *flags, "-o", exe, SRC], check=True)


def parse(text):
    """The model's output -> {"plan": {...}, "fills": {buffer: {cause: lines}}, "requests": {buffer: n}, "fill_bytes": n, ...}."""
    out = {"fills": {}, "requests": {}}
    for line in text.splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "plan":
            out["plan"] = {w[i]: float(w[i + 1]) if "." in w[i + 1] else int(w[i + 1]) for i in range(1, len(w), 2)}
        elif w[0] == "fills":
            out["fills"][w[1]] = {"first": int(w[3]), "refetch": int(w[5]), "cross": int(w[7])}
            out["requests"][w[1]] = int(w[9])
        elif w[0] == "fill_bytes":
            out["fill_bytes"] = int(w[1])
        elif w[0] == "boundary_union_rows":
            out["boundary_union_rows"], out["union_rows"] = int(w[1]), int(w[3])
    return out


def run_model(exe, tab, n_nodes, sta, S, L=4, bpc=2, cus=256, l2_mib=4.0, order="group", jitter=0.0, stream_kib=0.0, workdir=None):
    """Run the compiled model on a neighbour table (int32 [n_pos][16]) and a station table (int32 [S][8])."""
    with tempfile.TemporaryDirectory(dir=workdir) as d:
        ft, fs = os.path.join(d, "tab.i32"), os.path.join(d, "sta.i32")
        np.ascontiguousarray(tab, dtype=np.int32).tofile(ft)
        np.ascontiguousarray(sta, dtype=np.int32).tofile(fs)
        r = subprocess.run([exe, ft, str(len(tab)), str(n_nodes), fs, str(S), "--L", str(L), "--bpc", str(bpc), "--cus", str(cus),
                            "--l2-mib", str(l2_mib), "--order", order, "--jitter", str(jitter), "--stream-kib", str(stream_kib)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("s2u_traffic_model failed:\n" + r.stdout)
    return parse(r.stdout)


def table(res):
    mb = lambda lines: lines * 128 / 1e6
    rows = ["%-5s %10s %10s %10s %10s   %12s" % ("MB", "first", "refetch", "cross", "fills", "requests")]
    for b in BUFFERS + ("all",):
        f = res["fills"][b]
        rows.append("%-5s %10.1f %10.1f %10.1f %10.1f   %12d" % (b, mb(f["first"]), mb(f["refetch"]), mb(f["cross"]), mb(sum(f.values())),
                                                               res["requests"][b]))
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="cfg2_200x10k")
    ap.add_argument("--L", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--bpc", type=int, default=2)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--l2-mib", type=float, default=4.0)
    ap.add_argument("--order", choices=("group", "tile"), default="group")
    ap.add_argument("--jitter", type=float, default=0.0)
    ap.add_argument("--stream-kib", type=float, default=0.0, help="c / frag / mask through a cache of their own of this size (0: through the L2)")
    a = ap.parse_args()
    S, G, n_picks, Lbox, nq = synthetic.CONFIGS[a.config]
    geom = synthetic.Geometry(S, G, L=Lbox, n_query=nq, seed=1)
    tab, sta = neighbour_table(geom), station_table(geom)
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "s2u_traffic_model")
        compile_model(exe)
        for L in a.L:
            res = run_model(exe, tab, G, sta, S, L=L, bpc=a.bpc, cus=a.cus, l2_mib=a.l2_mib, order=a.order, jitter=a.jitter, stream_kib=a.stream_kib, workdir=d)
            p = res["plan"]
            print("%s L %d bpc %d L2 %.1f MiB order %s jitter %.2f streams %s: %d blocks, %d items, %d workgroups per XCD, carried %.3f"
                  % (a.config, L, a.bpc, a.l2_mib, a.order, a.jitter, "in L2" if a.stream_kib <= 0 else "aside (%g KiB)" % a.stream_kib, p["blocks"], p["items"], p["nbx"], p["carried"]))
            print(table(res))
            print("fills %.1f MB; FETCH_SIZE if every fill tallies 64 B: %.1f MB; union rows of the chunks' boundary groups: %d of %d (%.1f %%)\n"
                  % (res["fill_bytes"] / 1e6, res["fill_bytes"] / 2e6, res["boundary_union_rows"], res["union_rows"],
                     100.0 * res["boundary_union_rows"] / max(1, res["union_rows"])))


if __name__ == "__main__":
    main()
