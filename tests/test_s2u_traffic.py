"""CPU: the host model of k_stage2_h2u's L2 fills (tests/s2u_traffic_model.cpp through tools/s2u_traffic.py), built with the address
and undefined-behaviour sanitizers: a hand-made plan of three one-node blocks whose fills are counted by hand below, and config 1
(20 stations x 500 grid nodes), where the first-touch lines of every buffer are the buffer's size and the other causes obey the
cache size."""
import os
import shutil
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools import s2u_traffic  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if (shutil.which(os.environ.get("CXX", "g++"))) is None:
        pytest.fail("no C++ compiler on PATH")
    path = str(tmp_path_factory.mktemp("s2u_traffic") / "s2u_traffic_model")
    s2u_traffic.compile_model(path, flags=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    return path


def test_three_block_plan_counted_by_hand(exe):
    """S = 16 (one station tile, every plane of a node is 256 B = 2 lines), three positions holding nodes 1, 2, 3 of 20: the plan
    cuts [0, 3) into 8 chunks, of which 2, 5 and 7 hold one node each, so there are three one-node blocks A, B, C on three XCDs,
    one workgroup each, run in that order. A and B list rows 4..18, C lists rows 5..19. Station s lists stations s+1..s+8 (mod 16),
    so a tile reads all 16 wu rows of a node. The seven empty node slots of a block read node 0, as the kernel does.
      wv    15 rows x 4 planes x 2 lines = 120 lines a block. A: 120 first. B: 120 cross. C: rows 5..18 cross (112), row 19 first (8).
      c     16 lines a node. A: node 1 and node 0 first (32). B: node 2 first (16), node 0 cross (16). C: node 3 likewise.
      frag  4 lines a node. A: 8 first. B, C: 4 first, 4 cross each.
      wu    16 rows x 64 B = 8 lines a node. A: 16 first. B, C: 8 first, 8 cross each.
      mask  64 B a node, two nodes to a line. A: nodes 1 and 0 share line 0 (1 first). B: node 2 opens line 1 (first), node 0 is
            line 0 (cross). C: node 3 is line 1 (cross), node 0 line 0 (cross).
    Nothing is fetched twice by one XCD. Requests: 8 slots x (16 c + 4 frag + 1 mask + 128 wu) and 120 wv lines a block."""
    tab = np.zeros((3, 16), np.int32)
    tab[:, 0] = [1, 2, 3]
    tab[0, 1:] = tab[1, 1:] = np.arange(4, 19)
    tab[2, 1:] = np.arange(5, 20)
    sta = (np.arange(16)[:, None] + 1 + np.arange(8)[None, :]) % 16
    res = s2u_traffic.run_model(exe, tab, 20, sta, 16, L=1)
    assert res["plan"]["blocks"] == 3 and res["plan"]["nbx"] == 1 and res["plan"]["block_tiles"] == 3
    want = {"wv": (128, 0, 232), "c": (64, 0, 32), "frag": (16, 0, 8), "wu": (32, 0, 16), "mask": (2, 0, 3)}
    for b, (first, refetch, cross) in want.items():
        assert res["fills"][b] == {"first": first, "refetch": refetch, "cross": cross}, b
    assert res["requests"] == {"wv": 360, "c": 384, "frag": 96, "mask": 24, "wu": 3072, "all": 360 + 384 + 96 + 24 + 3072}
    assert res["fill_bytes"] == 128 * sum(sum(v) for v in want.values())
    # groups of 4 change nothing where every chunk holds one block
    res4 = s2u_traffic.run_model(exe, tab, 20, sta, 16, L=4)
    assert res4["fills"] == res["fills"]
    # a cache of two lines per XCD: node 0's rows do not survive from one empty slot to the next and are fetched again
    tiny = s2u_traffic.run_model(exe, tab, 20, sta, 16, L=1, l2_mib=256.0 / 1048576.0)
    assert tiny["fills"]["c"]["refetch"] == 3 * 6 * 16 and tiny["fills"]["c"]["first"] == 64 and tiny["fills"]["c"]["cross"] == 32


def test_config_1(exe):
    from genie_amd import synthetic
    S, G, n_picks, L, nq = synthetic.CONFIGS["cfg1_20x500"]
    geom = synthetic.Geometry(S, G, L=L, n_query=nq, seed=1)
    tab, sta = s2u_traffic.neighbour_table(geom), s2u_traffic.station_table(geom)
    lines = lambda nbytes: (nbytes + 127) // 128
    runs = {}
    for key, kw in {"L1": dict(L=1), "L4": dict(L=4), "L4_big": dict(L=4, l2_mib=64.0), "L4_small": dict(L=4, l2_mib=0.125)}.items():
        res = runs[key] = s2u_traffic.run_model(exe, tab, G, sta, S, **kw)
        f = res["fills"]
        # every line of a buffer is fetched for the first time exactly once (every grid node is some node's neighbour, every station some station's)
        assert f["c"]["first"] == lines(G * S * 128) and f["wv"]["first"] == lines(G * S * 64) and f["wu"]["first"] == lines(G * S * 64)
        assert f["frag"]["first"] == lines(G * S * 32) and f["mask"]["first"] == lines(G * S * 4)
        assert res["plan"]["block_tiles"] == res["plan"]["blocks"] * 2 and res["plan"]["tiles"] == 2
        assert res["fill_bytes"] == 128 * sum(f["all"].values())
    assert runs["L1"]["plan"]["carried"] == 0 and runs["L4"]["plan"]["carried"] > 0
    assert runs["L4"]["requests"]["wv"] < runs["L1"]["requests"]["wv"]            # carried rows are not requested again
    for b in ("c", "wu", "frag", "mask"):
        assert runs["L4"]["requests"][b] == runs["L1"]["requests"][b]
    assert runs["L4_big"]["fills"]["all"]["refetch"] == 0                         # the whole problem (3.7 MB) fits
    assert runs["L4_big"]["fills"]["all"]["cross"] > 0                            # chunk boundaries share rows
    assert runs["L4_small"]["fills"]["all"]["refetch"] > runs["L4"]["fills"]["all"]["refetch"]
    assert runs["L4_small"]["fills"]["all"]["cross"] == runs["L4_big"]["fills"]["all"]["cross"] == runs["L4"]["fills"]["all"]["cross"]
