"""bench.py's launch contract (CPU only; nothing here touches a GPU).

  * `bench.py --gpus N` (N > 1) outside torchrun starts torchrun with N ranks as a CHILD process
    (the plan is printed by --dry-run): the driver's 8-GPU run cannot silently measure one GPU.
  * Under torchrun a WORLD_SIZE that differs from --gpus exits non-zero before any work.
  * No flags: one GPU, in process.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, world=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    if world is not None:
        env["WORLD_SIZE"] = str(world)
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=env, timeout=120)


def test_gpus_n_launches_torchrun_child():
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run"])
    assert r.returncode == 0, r.stderr
    plan = json.loads(r.stdout.strip().splitlines()[-1])
    assert plan["plan"] == "launch"
    cmd = plan["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=2" in cmd and "--master-addr=127.0.0.1" in cmd
    i = cmd.index(BENCH)
    assert cmd[i + 1:] == ["--gpus", "2", "--steps", "3", "--warmup", "1"]  # --dry-run not forwarded


def test_world_size_mismatch_fails():
    r = _run(["--gpus", "2", "--dry-run"], world=4)
    assert r.returncode != 0 and json.loads(r.stdout.strip())["plan"] == "error"
    r = _run(["--gpus", "2", "--steps", "1"], world=4)  # the real run: refused before any work
    assert r.returncode != 0 and "WORLD_SIZE=4" in r.stderr


def test_full_and_dump_outputs_are_options_of_the_plain_command():
    r = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--dump-outputs", "out", "--dry-run"])
    assert r.returncode == 0 and json.loads(r.stdout.strip())["plan"] == "run", r.stderr
    r = _run(["--gpus", "2", "--full", "--dump-outputs", "out", "--dry-run"])  # forwarded to the ranks
    cmd = json.loads(r.stdout.strip())["cmd"]
    assert cmd[cmd.index(BENCH) + 1:] == ["--gpus", "2", "--full", "--dump-outputs", "out"]
    assert _run(["--steps", "0", "--dry-run"]).returncode != 0  # a line needs at least one timed step


def test_dump_outputs_files(tmp_path):
    """--dump-outputs writes float64 .npy files of at most 64 MB in all; an xy above 48 MB is cut to
    the same seeded sample of its entries on every call."""
    import numpy as np
    import bench
    small, hist = np.arange(1000.0), np.array([3.0, 2.0, 1.0])
    bench.dump_outputs(str(tmp_path / "a"), small, hist, 2)
    assert sorted(os.listdir(tmp_path / "a")) == ["niters.npy", "resid_history.npy", "xy.npy"]
    assert np.array_equal(np.load(tmp_path / "a" / "xy.npy"), small)
    assert np.array_equal(np.load(tmp_path / "a" / "resid_history.npy"), hist)
    assert np.array_equal(np.load(tmp_path / "a" / "niters.npy"), [2.0])
    big = np.arange(7_000_000, dtype=np.float64)  # 56 MB
    bench.dump_outputs(str(tmp_path / "b"), big, hist, 2)
    bench.dump_outputs(str(tmp_path / "c"), big + 0.5, hist, 2)
    b, c = np.load(tmp_path / "b" / "xy.npy"), np.load(tmp_path / "c" / "xy.npy")
    assert b.dtype == np.float64 and b.shape == (4 * 2**20,) and np.array_equal(c, b + 0.5)
    assert np.all(np.diff(b) > 0)  # distinct entries, in index order
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= 64 * 2**20


def test_default_is_one_gpu_in_process():
    for args, world in (([], None), (["--gpus", "1"], None), ([], 2), (["--gpus", "2"], 2)):
        r = _run(args + ["--dry-run"], world=world)
        assert r.returncode == 0 and json.loads(r.stdout.strip())["plan"] == "run", (args, world, r.stdout)
