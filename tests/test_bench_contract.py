"""bench.py contract (the driver's launch form) on CPU: N=2 ranks under
torch.distributed.run over gloo, a tiny Llama, one JSON line from rank 0 with
the fields the driver reads.  The GPU run of the same file is the round-end bench."""
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _plain(tmp_path, tag, steps):
    env = dict(os.environ, OMP_NUM_THREADS="2", EDL_RUN_DIR=str(tmp_path / f"run{tag}"))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--model", "llama-tiny",
           "--seq", "64", "--mbs", "1", "--accum", "2", "--dump-outputs", str(tmp_path / f"dump{tag}")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_the_last_steps_outputs(tmp_path):
    """A plain run times its steps and nothing else (the drill needs --full), and --dump-outputs
    writes the last timed step's loss, weights, gradients and clip statistics as float32 .npy:
    the same arguments give the same inputs, so on the CPU two runs agree bit for bit; one more
    timed step changes them."""
    import numpy as np
    a, b, c = _plain(tmp_path, "a", 2), _plain(tmp_path, "b", 2), _plain(tmp_path, "c", 3)
    for d, steps in ((a, 2), (b, 2), (c, 3)):
        assert d["steps"] == steps and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
        assert abs(d["value"] - 64 * 2 / (d["ms_per_step"] / 1e3)) / d["value"] < 0.01
        assert d["time_to_recover_s"] is None and "--full" in d["ttr"]["skipped"]
    names = sorted(os.listdir(tmp_path / "dumpa"))
    assert names == ["grads.npy", "loss.npy", "update_stats.npy", "weights.npy"]
    total = 0
    for n in names:
        x, y, z = (np.load(tmp_path / f"dump{t}" / n) for t in "abc")
        assert x.dtype == np.float32 and np.isfinite(x).all() and x.size == a["outputs"][n[:-4]][0]
        assert np.array_equal(x, y), n
        assert n == "update_stats.npy" or not np.array_equal(x, z), n
        total += x.nbytes
    assert abs(np.load(tmp_path / "dumpa" / "loss.npy")[0] - a["loss"]) < 1e-4   # the line rounds to 4 places
    assert np.count_nonzero(np.load(tmp_path / "dumpa" / "grads.npy")) > 0
    assert total <= 64 << 20


def test_bench_two_ranks_prints_one_json_line(tmp_path):
    env = dict(os.environ, OMP_NUM_THREADS="2", EDL_RUN_DIR=str(tmp_path / "run"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", "2", "--steps", "2",
           "--warmup", "1", "--model", "llama-tiny", "--seq", "64", "--mbs", "1", "--accum", "2"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0
    assert d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 4
    # value is the whole-job aggregate: 2 ranks x 1 seq x 64 tokens x 2 micro-batches per step
    assert abs(d["value"] - 2 * 64 * 2 * 2 / (d["ms_per_step"] * 2 / 1e3)) / d["value"] < 0.01
