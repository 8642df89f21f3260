"""CPU: the block-table plan of k_stage2_h2u (genie_amd/csrc/s2u_plan.hpp, host-only C++) through its stand-alone check program
tests/s2u_plan_check.cpp, built with the address and undefined-behaviour sanitizers: plans of random 3-D grids with 15-nearest-
neighbour graphs (G = 9, 64, 500, a shuffled order whose unions cut the blocks short, ranges starting mid-grid; groups of 1, 2, 4
and 8 blocks) replayed against an array standing in for the LDS slots; groups of one block reproduce the table of every block
staging its whole union."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_plan_check_program_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    exe = str(tmp_path / "s2u_plan_check")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(HERE, "s2u_plan_check.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "s2u_plan_check: ok" in r.stdout
    # rows are carried wherever a chunk holds several blocks, and only there
    lines = [l for l in r.stdout.splitlines() if l.startswith("G = 500 ")]
    assert any(" L 1:" in l and "fraction 0.000" in l for l in lines)
    assert any(" L 4:" in l and "fraction 0.000" not in l for l in lines)
