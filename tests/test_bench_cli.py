"""CPU: bench.py's launch contract. `--gpus N` must either run N ranks
(re-launching itself under torch.distributed.run before any GPU call) or
fail -- never silently run one process and report n_gpus = 1."""
import os
import subprocess
import sys

from conftest import ROOT


def test_gpus_mismatch_with_torchrun_env_fails():
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "WORLD_SIZE=3" in r.stderr


def test_plain_run_is_the_default(monkeypatch):
    """--full (secondary record, CPU baseline) is off unless asked for."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3 and a.warmup == 1
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_is_capped_and_repeatable(tmp_path):
    """Small arrays are written whole; beyond 64 MB in all the large ones
    keep a seeded, ordered sample of their permutation axis."""
    import numpy as np
    import bench
    cube = np.arange(50 * 7 * 30000, dtype=np.float64).reshape(50, 7, 30000)   # 84 MB
    obs = np.arange(350, dtype=np.float64).reshape(50, 7)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"nulls": cube, "observed": obs}, 7)
    a, b = np.load(tmp_path / "a" / "nulls.npy"), np.load(tmp_path / "b" / "nulls.npy")
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "observed.npy"), obs)
    assert a.dtype == np.float64 and a.shape[:2] == (50, 7) and 1 < a.shape[2] < 30000
    assert a.nbytes + obs.nbytes <= 64 * 2**20
    cols = a[0, 0].astype(np.int64)                       # cube[0, 0, j] == j
    assert (np.diff(cols) > 0).all()
    np.testing.assert_array_equal(a, cube[:, :, cols])
    bench.dump_outputs(str(tmp_path / "c"), {"nulls": cube[:, :, :5120]}, 7)
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "nulls.npy"), cube[:, :, :5120])


def test_relaunch_command_is_torchrun(monkeypatch):
    import bench
    calls = {}

    def fake_call(cmd):
        calls["cmd"] = cmd
        return 0

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    monkeypatch.setattr(subprocess, "call", fake_call)
    args = bench.parse()
    try:
        bench.relaunch_if_needed(args)
    except SystemExit as e:
        assert e.code == 0
    cmd = calls["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--master-addr=127.0.0.1" in cmd
    assert cmd[-4:] == ["--gpus", "4", "--steps", "3"]
