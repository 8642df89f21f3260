#!/usr/bin/env python
"""The read-out span of the literal call in a rocprofv3 --kernel-trace run (rocpd sqlite database or *kernel_trace.csv): per window,
the time from the end of the third k_sa_layer_m to the end of the last read-out kernel, the start offsets of the read-out kernels
after that point and their durations, set against the ideal span dur(k_ro_pre_m) + max(dur of the two heads); medians over the
windows of the second half of the trace (clocks settled).
Usage: python tools/readout_span.py <results.db | kernel_trace.csv>"""
import csv
import re
import sqlite3
import statistics
import sys


def dispatches(path):
    if path.endswith(".csv"):
        rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(path))]
    else:
        rows = sqlite3.connect(path).execute("select name, start, end from kernels").fetchall()
    return sorted(rows, key=lambda r: r[1])


def kind(name):
    if "k_readouts_m" in name:
        return "both"
    m = re.search(r"k_readout_m<\s*(\d)", name)
    if m:
        return "grid" if m.group(1) == "0" else "query"
    if "k_ro_pre_m" in name:
        return "pre"
    if "k_sa_layer_m" in name:
        return "sa"
    return None


def windows(rows):
    """One dict per literal call: sa_end and (start, end) of every read-out kernel that follows it."""
    out, cur, sa_end = [], None, None
    for name, s, e in rows:
        k = kind(name)
        if k == "sa":
            if cur:
                out.append(cur)
                cur = None
            sa_end = e
        elif k and sa_end is not None:
            cur = cur or {"sa_end": sa_end}
            cur[k] = (s, e)
    if cur:
        out.append(cur)
    return [w for w in out if "pre" in w and ("both" in w or ("grid" in w and "query" in w))]


def main():
    ws = windows(dispatches(sys.argv[1]))
    ws = ws[len(ws) // 2:]
    med = lambda v: statistics.median(v) / 1e3
    dur = lambda k: med([w[k][1] - w[k][0] for w in ws])
    off = lambda k: med([w[k][0] - w["sa_end"] for w in ws])
    heads = ["both"] if "both" in ws[0] else ["grid", "query"]
    span = med([max(w[k][1] for k in heads) - w["sa_end"] for w in ws])
    print("windows %d (second half of the trace), medians in us" % len(ws))
    for k in ["pre"] + heads:
        print("  %-5s start +%6.2f  duration %6.2f" % (k, off(k), dur(k)))
    print("  span (end of SpatialAggregation3 -> end of the last read-out) %.2f" % span)
    if heads != ["both"]:
        ideal = med([(w["pre"][1] - w["pre"][0]) + max(w["grid"][1] - w["grid"][0], w["query"][1] - w["query"][0]) for w in ws])
        serial = med([sum(w[k][1] - w[k][0] for k in ("pre", "grid", "query")) for w in ws])
        print("  ideal span dur(pre) + max(dur(grid), dur(query)) %.2f, excess %.2f; durations summed %.2f" % (ideal, span - ideal, serial))


if __name__ == "__main__":
    main()
