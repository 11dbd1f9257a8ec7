"""bench.py's multi-rank launch on CPU (verdict r3 item 1): ``python bench.py --gpus N`` started as ONE
plain process must start N ranks itself (the driver runs exactly that command on an 8-GPU node), the
torchrun launch must keep working, and a world size that disagrees with --gpus must be refused.
``--dry-run`` runs the launch + gloo process group + barrier-bracketed, max-over-ranks timed region
with an empty step, so no GPU is needed."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE")}
    env.update(kw)
    return env


def _run(args, env=None, timeout=120):
    if "--dry-run" in args and "--cpu-budget" not in args:
        args = args + ["--no-cpu-baseline"]
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout,
                          env=env if env is not None else _env(), cwd=REPO)


def _one_json(out):
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_gpus2_spawns_two_ranks():
    p = _run(["--gpus", "2", "--dry-run", "--steps", "3", "--warmup", "1"])
    assert p.returncode == 0, p.stderr[-3000:]
    res = _one_json(p.stdout)
    assert res["n_gpus"] == 2
    assert res["config"]["global_batch"] == 256 and res["config"]["per_rank_batch"] == 128
    assert res["process_group_world_size"] == 2
    ranks = res["ranks"]
    assert sorted(r["rank"] for r in ranks) == [0, 1]
    assert len({r["pid"] for r in ranks}) == 2 and os.getpid() not in {r["pid"] for r in ranks}
    assert all(r["pg_world_size"] == 2 for r in ranks)
    assert res["launch"]["ranks"] == 2


def test_gpus1_runs_in_process():
    p = _run(["--gpus", "1", "--dry-run", "--steps", "2"])
    assert p.returncode == 0, p.stderr[-3000:]
    res = _one_json(p.stdout)
    assert res["n_gpus"] == 1 and "launch" not in res and res["config"]["global_batch"] == 128


def test_torchrun_env_is_honoured():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), BENCH, "--gpus", "2", "--dry-run",
                        "--steps", "2", "--no-cpu-baseline"], capture_output=True, text=True, timeout=120, env=_env(),
                       cwd=REPO)
    assert p.returncode == 0, p.stderr[-3000:]
    res = _one_json(p.stdout)
    assert res["n_gpus"] == 2 and "launch" not in res


def test_world_size_mismatch_refused():
    p = _run(["--gpus", "4", "--dry-run"], env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"))
    assert p.returncode != 0 and "WORLD_SIZE=2" in p.stderr


def test_failing_rank_fails_the_launch():
    # rank 1 cannot start (the mismatch check fires in the child only for a bad env): simulate with an
    # unknown flag passed through to both children -> argparse exits 2 in each, the parent must fail
    p = _run(["--gpus", "2", "--dry-run", "--no-such-flag"])
    assert p.returncode != 0


def test_gpus2_line_carries_roofline_cpu_baseline_and_exchange():
    """the N > 1 line has the same post-timed-region keys as N = 1 — roofline (rank 0
    profiles its local step), cpu_baseline (rank 0 while the other ranks sleep in a gloo barrier) and the
    exchange block (per-phase host wait, exposed tail, local step time, RCCL world size).  These legs run
    with ``--full``."""
    p = _run(["--gpus", "2", "--dry-run", "--full", "--steps", "2", "--cpu-budget", "1", "--exchange-steps", "3"],
             timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = _one_json(p.stdout)
    assert res["n_gpus"] == 2
    assert "roofline" in res and {"frac", "r34_3x3"} <= set(res["roofline"])
    cb = res["cpu_baseline"]
    assert cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] == "port"
    ex = res["exchange"]
    assert ex["rccl_world_size"] == 2 and ex["phases"] == 3 and ex["steps_probed"] == 3
    assert {"exposed_tail_ms_per_step", "host_wait_ms_per_step", "local_step_ms",
            "exchange_exposed_ms_per_step", "late_phase_window_ms_per_step"} <= set(ex)


def test_plain_run_skips_the_secondary_legs():
    """Without ``--full`` the line carries the headline only: no CPU baseline is timed even when a budget
    is given, and the per-kernel table (it needs the roofline replays) is refused."""
    p = _run(["--gpus", "1", "--dry-run", "--steps", "2", "--cpu-budget", "1"])
    assert p.returncode == 0, p.stderr[-3000:]
    res = _one_json(p.stdout)
    assert res["steps"] == 2 and "cpu_baseline" not in res and res["exchange"] is None
    p = _run(["--gpus", "1", "--dry-run", "--kernel-table", os.devnull])
    assert p.returncode != 0 and "--full" in p.stderr


def test_dump_outputs_writes_float_arrays(tmp_path, monkeypatch):
    """``--dump-outputs``: every tensor lands as <name>.npy in float32 / float64 (integers widened), and
    the parameters as the same seeded sample on every call."""
    import numpy as np
    import torch
    import bench  # the repository root is on sys.path (tests/conftest.py)
    torch.manual_seed(0)
    model = torch.nn.Linear(7, 5)
    logits = torch.randn(4, 5)
    preds = torch.arange(4)
    bench.dump_outputs(str(tmp_path / "a"), model, loss=torch.tensor([0.5]), logits=logits, preds=preds)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["logits", "loss", "params_sample", "preds"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["logits"], logits.numpy()) and np.array_equal(got["preds"], np.arange(4.0))
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy()
    assert np.array_equal(got["params_sample"], flat)  # smaller than the sample: all of it
    monkeypatch.setattr(bench, "DUMP_PARAM_SAMPLE", 8)
    bench.dump_outputs(str(tmp_path / "b"), model)
    bench.dump_outputs(str(tmp_path / "c"), model)
    b, c = np.load(tmp_path / "b" / "params_sample.npy"), np.load(tmp_path / "c" / "params_sample.npy")
    assert b.shape == (8,) and np.array_equal(b, c) and np.isin(b, flat).all()
