"""bench.py --gpus N: the rank launcher (VERDICT r5 "Next" 1).  CPU only:
the refusal when fewer than N GPUs are visible, the world-size checks, and
the launcher's plumbing (N children, RANK / LOCAL_RANK / WORLD_SIZE, a gloo
rendezvous on 127.0.0.1, rank 0's line passed through, a failing rank ends
the job non-zero) with a stand-in rank script instead of the GPU bench."""

from __future__ import annotations

import json
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_gpus_2_without_devices_fails_loudly():
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0
    assert "needs 2 visible GPUs" in r.stderr
    assert '"n_gpus"' not in r.stdout


def test_check_world_rules():
    assert bench.check_world(None, env={}, devices=1) == 1
    assert bench.check_world(4, env={}, devices=8) == 4
    assert bench.check_world(None, env={"WORLD_SIZE": "2"}, devices=2) == 2
    with pytest.raises(bench.RankLaunchError, match="WORLD_SIZE=2"):
        bench.check_world(8, env={"WORLD_SIZE": "2"}, devices=8)
    with pytest.raises(bench.RankLaunchError, match="found 1"):
        bench.check_world(2, env={}, devices=1)
    with pytest.raises(bench.RankLaunchError):
        bench.check_world(0, env={}, devices=8)


def test_dump_outputs_sample_is_fixed_and_files_exact(tmp_path):
    import numpy as np

    V, n = 50, 300
    words = lambda i: 1 + (i % 3)  # noqa: E731
    pick = bench.dump_sample(0, n, V, words)
    assert len(pick) == bench.DUMP_SOURCES == len(set(pick.tolist()))
    assert (pick == bench.dump_sample(0, n, V, words)).all() and (np.diff(pick) > 0).all()
    assert (bench.dump_sample(100, n, V, words) == pick + 100).all()
    # a sample too large for the size limit is cut, never the limit raised
    big = bench.dump_sample(0, n, 100_000, lambda i: 2)
    assert 1 <= len(big) < bench.DUMP_SOURCES
    assert len(big) * 100_000 * 8 * 5 <= bench.DUMP_MAX_BYTES
    assert (big == pick[: len(big)]).all()
    rng = np.random.default_rng(1)
    rows = [rng.integers(0, 2**32, V, dtype=np.uint64) for _ in pick]
    rows[0][3] = np.uint64(2**64 - 1)
    masks = [rng.integers(0, 2**64, (V, words(int(i))), dtype=np.uint64) for i in pick]
    bench.dump_outputs(str(tmp_path / "d"), np.arange(n, dtype=np.uint32), pick, rows, masks)
    src = np.load(tmp_path / "d" / "sources.npy")
    d = np.load(tmp_path / "d" / "dist.npy")
    nh = np.load(tmp_path / "d" / "nexthop_masks.npy")
    assert src.dtype == d.dtype == nh.dtype == np.float64
    assert (src == pick).all() and d.shape == (len(pick), V) and nh.shape == (len(pick), V, 6)
    assert (d[1] == rows[1].astype(np.float64)).all() and d[0][3] == float(2**64)
    for k, m in enumerate(masks):
        W = m.shape[1]
        back = nh[k, :, 0:2 * W:2].astype(np.uint64) | (nh[k, :, 1:2 * W:2].astype(np.uint64) << np.uint64(32))
        assert (back == m).all() and not nh[k, :, 2 * W:].any()


def test_plain_run_options():
    argv, sys.argv = sys.argv, ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
    try:
        a = bench.parse()
        assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
        sys.argv += ["--full", "--dump-outputs", "x"]
        a = bench.parse()
        assert a.full and a.dump_outputs == "x"
    finally:
        sys.argv = argv


RANK_SCRIPT = textwrap.dedent("""
    import json, os, sys
    import torch, torch.distributed as dist
    world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
    assert int(os.environ["LOCAL_RANK"]) == rank
    assert os.environ["MASTER_ADDR"] == "127.0.0.1"
    dist.init_process_group("gloo")
    t = torch.tensor([rank + 1.0])
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    if rank == 0:
        n = world if "--lie" not in sys.argv else 1
        print(json.dumps({"n_gpus": n, "max_rank": float(t[0]), "argv": sys.argv[1:]}))
    if "--fail-rank1" in sys.argv and rank == 1:
        sys.exit(5)
    dist.destroy_process_group()
""")


@pytest.mark.parametrize("n", [2, 3])
def test_launcher_runs_n_ranks(tmp_path, capfd, n):
    script = tmp_path / "rank.py"
    script.write_text(RANK_SCRIPT)
    rc = bench.launch_ranks(n, ["--steps", "1"], script=str(script))
    out = capfd.readouterr().out.strip().splitlines()
    assert rc == 0
    rec = json.loads(out[-1])
    assert rec["n_gpus"] == n and rec["max_rank"] == float(n) and rec["argv"] == ["--steps", "1"]


def test_launcher_failing_rank_is_nonzero(tmp_path, capfd):
    script = tmp_path / "rank.py"
    script.write_text(RANK_SCRIPT)
    assert bench.launch_ranks(2, ["--fail-rank1"], script=str(script)) != 0


def test_launcher_refuses_wrong_n_gpus(tmp_path, capfd):
    script = tmp_path / "rank.py"
    script.write_text(RANK_SCRIPT)
    assert bench.launch_ranks(2, ["--lie"], script=str(script)) != 0
    assert '"n_gpus"' not in capfd.readouterr().out
