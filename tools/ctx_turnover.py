#!/usr/bin/env python
"""Cost of replacing a context, as the reference's training loop does per sample: mean wall time of HipPath create + set_weights +
commit + destroy cycles after a warm-up that fills the library's device-memory pool; prints the pool's accounting beside it
(genie_pool_stats). A/B of two libraries: run it once per GENIE_LIB_PATH; `_lib.load()` binds every declared symbol, so a library built
from a commit that has no genie_pool_stats needs that one function added to its source for the comparison. Usage: python tools/ctx_turnover.py [config] [cycles]"""
import ctypes
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from genie_amd import _lib, engine, synthetic  # noqa: E402
from tests.util import Case  # noqa: E402


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2_200x10k"
    cycles = int(sys.argv[2]) if len(sys.argv) > 2 else 300
    S, G, _, L, _ = synthetic.CONFIGS[cfg]
    geom = synthetic.Geometry(S, G, L=L, n_query=10, seed=1)
    dev = "cuda:0"
    sta = tuple(t.to(dev) for t in engine.csr_from_edges(torch.from_numpy(geom.A_sta_sta), S))
    src = tuple(t.to(dev) for t in engine.csr_from_edges(torch.from_numpy(geom.A_src_src), G))
    go, so = engine.sfc_order(geom.x_grid), engine.sfc_order(geom.locs)
    wd = {k: v.to(dev) for k, v in Case("cfg1_20x500").weights.items()}

    def cycle():
        hp = engine.HipPath(S, G, sta, src, grid_order=go, device=dev, sta_order=so)
        hp.set_weights(wd)
        hp.stage_precision()          # commits the weights: the packing kernels and the range guard's read-back
        hp.__del__()

    for _ in range(30):
        cycle()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(cycles):
        cycle()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / cycles
    b, n, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.load().genie_pool_stats(0, ctypes.byref(b), ctypes.byref(n), ctypes.byref(c)), "genie_pool_stats")
    print("context turnover %s [%s]: %.4f ms per create + set_weights + destroy over %d cycles; pool: %d live blocks, %d live bytes, "
          "%d cached bytes" % (cfg, os.path.basename(os.path.dirname(_lib.LIB_PATH)), ms, cycles, b.value, n.value, c.value))


if __name__ == "__main__":
    main()
