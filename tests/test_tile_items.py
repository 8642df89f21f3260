"""CPU: the item table of k_stage1_h2 with packed station tail tiles (genie_amd/csrc/tile_items.hpp, plain C++ shared by the kernel
and the host) through its stand-alone check program tests/tile_items_check.cpp, built with the address and undefined-behaviour
sanitizers: every (source node, station) of a launched range covered exactly once by the lanes the kernel gives it, partners adjacent
and inside one chunk, the item counts, S mod 16 = 0 / 1 .. 8 / 9 .. 15, node-major and tile-major sweeps, one-node chunks, and ranges
cut in two at every position (the sharded path's range launches)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_tile_items_check_program_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    exe = str(tmp_path / "tile_items_check")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(HERE, "tile_items_check.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "tile_items_check: ok" in r.stdout
    assert "S = 200, G = 10000: 125000 items (padded 130000)" in r.stdout
