"""``bench.py``'s launch contract: ``--gpus N`` from a bare shell starts its own N ranks as a child
process (before anything touches the GPU) and relays the one JSON line and the exit code."""

import json
import os
import subprocess
import sys

from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _bare_env():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def test_gpus_n_without_a_launcher_starts_torch_distributed_run_as_a_child(monkeypatch, capsys):
    import bench

    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env

        class R:
            returncode = 7
            stdout = "[Gloo] Rank 0 is connected to 1 peer ranks.\n{\"metric\": \"m\"}\n"
        return R()

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("RANK", "5")          # a stale variable of some outer launcher must not leak in
    with pytest.raises(SystemExit) as exc:
        bench.main()
    assert exc.value.code == 7               # the child's exit code is the bench's
    out = capsys.readouterr()
    assert out.out == '{"metric": "m"}\n' and "[Gloo]" in out.err     # stdout carries the JSON line only
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    i = cmd.index(str(ROOT / "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    assert "RANK" not in seen["env"]


def test_ranks_that_do_not_match_gpus_are_refused(monkeypatch):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--no-cpu-baseline"])
    monkeypatch.setenv("WORLD_SIZE", "3")
    with pytest.raises(SystemExit) as exc:
        bench.main()
    assert "WORLD_SIZE=3" in str(exc.value.code)


@pytest.mark.gpu
def test_bench_gpus_2_from_a_bare_shell_on_one_card():
    """The rehearsal: two ranks share the one card (gloo carries the barrier), started by bench.py itself."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--workload", "small"], cwd=ROOT, env=_bare_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["value"] > 0
    assert "cpu_baseline" not in line


def test_config1_runs_on_the_cpu_through_the_product_path():
    """BASELINE configs[0] as a bench line: deskew only, no GPU, the host twin on a CPU tensor, equal to the
    oracle bit for bit (the oracle is the timed baseline beside it, never the thing measured)."""
    r = subprocess.run([sys.executable, "bench.py", "--device", "cpu", "--workload", "config1", "--steps", "1", "--warmup", "0"],
                       cwd=ROOT, env=_bare_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 0 and line["dtype"] == "f32" and line["value"] > 0
    assert line["config"]["equals_oracle_bit_for_bit"] is True and line["config"]["raw_shape"] == [256, 64, 256]
    assert line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["cores"] == 1


def test_a_plain_run_leaves_the_cpu_baseline_to_full(monkeypatch, capsys):
    """``--gpus 1 --steps N --warmup W`` measures the headline only; ``--full`` adds the CPU baseline."""
    import bench

    calls = []
    monkeypatch.setattr(bench, "cpu_baseline", lambda **kw: calls.append(kw) or {"kind": "port"})
    monkeypatch.setattr(bench, "dist_setup", lambda args: (0, 1, "cuda:0", False, None))
    monkeypatch.setattr(bench, "run_resident", lambda args, rank, world, device, shared, backend, cpu:
                        {"metric": "m", "steps": args.steps, **({"cpu_baseline": cpu} if cpu is not None else {})})
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for argv, want in ((["--gpus", "1", "--steps", "3", "--warmup", "1"], False),
                       (["--gpus", "1", "--steps", "3", "--warmup", "1", "--full"], True),
                       (["--gpus", "1", "--full", "--no-cpu-baseline"], False)):
        calls.clear()
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        bench.main()
        line = json.loads(capsys.readouterr().out)
        assert bool(calls) is want and ("cpu_baseline" in line) is want, argv


def test_dump_outputs_writes_float32_and_samples_large_arrays_at_fixed_positions(tmp_path):
    import numpy as np
    import torch

    import bench

    small = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    big = torch.randn(40, 300, 310, generator=torch.Generator().manual_seed(1))[:, 5:295, 7:300]   # a strided window
    bench.dump_outputs(tmp_path / "a", {"small": small, "big": big})
    bench.dump_outputs(tmp_path / "b", {"big": big * 2})
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (2, 3, 4) and np.array_equal(s, small.numpy())
    vals, idx = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "a" / "big_index.npy")
    assert vals.dtype == np.float32 and vals.shape == (bench.DUMP_SAMPLE,) and idx.dtype == np.float64
    i = idx.astype(np.int64)
    assert np.all(np.diff(i) > 0) and i[-1] < big.numel()
    assert np.array_equal(vals, big.contiguous().numpy().ravel()[i])
    assert np.array_equal(np.load(tmp_path / "b" / "big_index.npy"), idx)     # same shape: same positions
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= bench.DUMP_BUDGET_BYTES


@pytest.mark.gpu
def test_dump_outputs_are_the_same_from_run_to_run(tmp_path):
    """Seeded inputs: two runs with the same arguments write the same outputs, bit for bit."""
    import numpy as np

    for run in ("a", "b"):
        r = subprocess.run([sys.executable, "bench.py", "--workload", "small", "--steps", "2", "--warmup", "1",
                            "--dump-outputs", str(tmp_path / run)], cwd=ROOT, env=_bare_env(), capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and "cpu_baseline" not in line
    names = sorted(f.name for f in (tmp_path / "a").iterdir())
    assert names == ["deskewed.npy", "deskewed_index.npy", "estimate.npy", "estimate_index.npy"]
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name
    assert np.isfinite(np.load(tmp_path / "a" / "estimate.npy")).all()
