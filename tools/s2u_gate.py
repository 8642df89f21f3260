#!/usr/bin/env python
"""Carried fraction of k_stage2_h2u's block plan (genie_amd/csrc/s2u_plan.hpp) for a synthetic config, on the CPU: writes the
neighbour table of the processing order (int32 [G][16]: source node, its 15 neighbours; the Z-curve order of `engine.sfc_order`, the
kNN columns of `synthetic.Geometry`, as genie_ctx_create builds it), compiles tests/s2u_plan_check.cpp and runs it on the table.
Usage: python tools/s2u_gate.py [config] [L ...]      (default: cfg2_200x10k 1 2 3 4 8 16; no GPU needed)"""
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from genie_amd import engine, synthetic  # noqa: E402


def neighbour_table(geom):
    G = geom.n_grid
    order = engine.morton_order(geom.x_grid)
    nbr = geom.A_src_src[0].reshape(G, geom.k_spc)
    assert geom.k_spc == 15 and (geom.A_src_src[1].reshape(G, 15) == np.arange(G)[:, None]).all()
    tab = np.empty((G, 16), np.int32)
    tab[:, 0] = order
    tab[:, 1:] = nbr[order]
    return tab


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2_200x10k"
    Ls = sys.argv[2:] or ["1", "2", "3", "4", "8", "16"]
    S, G, n_picks, L, nq = synthetic.CONFIGS[cfg]
    geom = synthetic.Geometry(S, G, L=L, n_query=nq, seed=1)
    with tempfile.TemporaryDirectory() as d:
        tab, exe = os.path.join(d, "tab.i32"), os.path.join(d, "s2u_plan_check")
        neighbour_table(geom).tofile(tab)
        subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-o", exe, os.path.join(REPO, "tests", "s2u_plan_check.cpp")], check=True)
        subprocess.run([exe, tab, str(G)] + Ls, check=True)


if __name__ == "__main__":
    main()
