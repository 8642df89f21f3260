"""CPU: `python bench.py --gpus N` launches its own N ranks (the driver may also start it under torchrun); the dry-run form
exercises the launcher, the rank environment, the sharding plan and both collectives of the sharded path over gloo."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600, env=env, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout            # ONE JSON line, from rank 0
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [1, 2, 3])
def test_bench_gpus_n_launches_n_ranks(n):
    out = _run(["--gpus", str(n), "--dry-run-cpu"])
    assert out["n_gpus"] == n and out["ranks"] == n and out["ok"] is True
    assert (out["rank0_plan"]["n_halo"] > 0) == (n > 1)


def test_bench_defaults_pick_the_sharded_config_for_several_gpus():
    sys.path.insert(0, REPO)
    import importlib
    bench = importlib.import_module("bench")
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "8"]
        a = bench.parse()
    finally:
        sys.argv = argv
    assert a.mode is None and a.config is None and a.gpus == 8          # resolved in main(): sharded cfg4 when world > 1
    src = open(os.path.join(REPO, "bench.py")).read()
    assert 'a.mode = "sharded" if world > 1 else "replicas"' in src
    assert '"cfg4_2000x50k" if (a.mode == "sharded" and world > 1) else "cfg2_200x10k"' in src


def test_bench_refuses_more_ranks_than_visible_gpus_instead_of_hanging():
    """`python bench.py --gpus 8` on a node that shows fewer GPUs: a clear message and exit code 2 before anything is launched (no
    rendezvous that could hang)."""
    import torch
    if torch.cuda.device_count() >= 8:
        pytest.skip("eight GPUs visible")
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300, env=env, cwd=REPO)
    assert r.returncode == 2 and "needs 8 visible GPUs" in r.stderr and not r.stdout.strip()


def test_bench_dry_run_halo_bytes_at_the_config4_shape_with_eight_ranks():
    """What the first real 8-GPU run of config 4 (2000 stations / 50 000 source nodes sharded over source nodes) should see on the wire,
    from the sharding plan alone: the halo of `wv` rows per window is ~55-110 MB inbound per rank (64 B per halo product node), from
    2-6 peers, the largest single pair ~45 MB = 0.3 ms on one 153-GB/s xGMI link -- against ~4 ms of compute per rank. (DESIGN.md
    section 6 had guessed 240 MB from a 30 % halo fraction; the space-filling-curve partition needs 7-13 %.) Both exchange forms (one
    all_to_all_single; one send / receive pair per peer) move the right rows over gloo."""
    out = _run(["--gpus", "8", "--dry-run-cpu", "--config", "cfg4_2000x50k"])
    h = out["halo"]
    assert out["ok"] is True and out["ranks"] == 8 and h["send_recv_consistent"] is True
    assert h["bytes_per_halo_source_node"] == 2000 * 64.0 and out["rank0_plan"]["n_own"] == 6250
    assert len(h["MB_in_per_rank"]) == 8 and 30.0 < min(h["MB_in_per_rank"]) and h["MB_in_max"] < 160.0
    assert 20.0 < h["largest_pair_MB"] < 80.0 and h["largest_pair_ms_at_153_GBs"] < 0.55
    assert all(1 <= n <= 7 for n in h["peers_per_rank"])


def test_dump_outputs_writes_float32_and_samples_rows_past_the_budget(tmp_path, monkeypatch):
    """`--dump-outputs`: one float32 .npy per array (float64 kept), and an array past the byte budget becomes the same seeded sample of
    its rows on every call, so that two builds given the same arguments can be compared element for element."""
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    import importlib
    bench = importlib.import_module("bench")
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    big = torch.arange(1000 * 8, dtype=torch.float64).view(1000, 8).float()          # 32 000 B > 4096 - 40
    small = torch.tensor([1.5, 2.5], dtype=torch.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"loss": small, "x": big, "n": torch.tensor(3)})
    s, x = np.load(tmp_path / "a" / "loss.npy"), np.load(tmp_path / "a" / "x.npy")
    assert s.dtype == np.float64 and s.tolist() == [1.5, 2.5]
    assert x.dtype == np.float32 and x.shape[1] == 8 and 0 < x.shape[0] < 1000 and x.nbytes <= 4096 - s.nbytes
    rows = x[:, 0] / 8
    assert np.array_equal(rows, np.round(rows)) and np.all(np.diff(rows) > 0)        # whole rows, ascending
    assert np.array_equal(x, np.load(tmp_path / "b" / "x.npy"))
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) < 4096 + 3 * 128                # + the .npy headers
    assert np.load(tmp_path / "a" / "n.npy").dtype == np.float32
