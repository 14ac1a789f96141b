"""bench.py's multi-rank launch path: `python bench.py --gpus 2` must start its own ranks when no
launcher is around it, and must also run under torch.distributed.run exactly as the driver starts it.  `--dry` keeps the
GPU out of it (gloo on the host), so this runs in the CPU suite.  The plain run on the GPU and its `--dump-outputs` files are
checked by the test marked gpu."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one_json_line(stdout):
    lines = [l for l in stdout.splitlines() if l.strip()]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    return env


def test_bare_invocation_spawns_its_own_ranks():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--dry",
                          "--scaling", "weak"], capture_output=True, text=True, timeout=300, env=_env())
    assert res.returncode == 0, res.stderr[-2000:]
    out = _one_json_line(res.stdout)
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1 and out["dry"] is True
    # opt-in: every rank keeps 8 images (BASELINE config 3 = 4 x 8) -> weak scaling, whole-job value
    assert out["config"]["per_gpu_batch"] == 8 and out["config"]["global_batch"] == 16 and out["scaling"] == "weak"


def test_under_the_drivers_launcher():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--dry"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=_env())
    assert res.returncode == 0, res.stderr[-2000:]
    out = _one_json_line(res.stdout)
    # default since round 3: north_star's partition -- the metric's GLOBAL batch of 8 split over the ranks
    # (DGDE/data/build.py:63-67) -> strong scaling
    assert out["n_gpus"] == 2 and out["scaling"] == "strong"
    assert out["config"]["per_gpu_batch"] == 4 and out["config"]["global_batch"] == 8


def test_single_rank_dry():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry", "--steps", "2", "--warmup", "0"],
                         capture_output=True, text=True, timeout=300, env=_env())
    assert res.returncode == 0, res.stderr[-2000:]
    assert _one_json_line(res.stdout)["n_gpus"] == 1


def test_full_and_dump_outputs_options(tmp_path):
    bench = os.path.join(ROOT, "bench.py")
    res = subprocess.run([sys.executable, bench, "--dry", "--full", "--steps", "2", "--warmup", "0"],
                         capture_output=True, text=True, timeout=300, env=_env())
    assert res.returncode == 0, res.stderr[-2000:]
    assert _one_json_line(res.stdout)["steps"] == 2
    # the dump is the dgde train step's: refused (usage error, nothing run) where there is none
    for extra in (["--dry"], ["--workload", "gmw"]):
        res = subprocess.run([sys.executable, bench, "--dump-outputs", str(tmp_path)] + extra, capture_output=True, text=True,
                             timeout=300, env=_env())
        assert res.returncode == 2 and "--dump-outputs" in res.stderr, res.stderr[-2000:]
    assert not os.listdir(tmp_path)


def _bench_dump(dump, batch):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                          "--batch", str(batch), "--input", "320x96", "--dump-outputs", str(dump)],
                         capture_output=True, text=True, timeout=600, env=_env())
    assert res.returncode == 0, res.stderr[-2000:]
    return _one_json_line(res.stdout)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [8, 2])          # 8: the eager step (the headline's path); 2: the whole-step graph replay
def test_plain_run_and_its_dump_are_reproducible(tmp_path, batch):
    """A plain run prints the headline keys only, --steps sets the timed steps, ms_per_step is the time of one of them, and
    --dump-outputs leaves the losses, log and parameter / gradient samples of the timed path's step from the seeded inputs as
    float32 .npy files -- the same in two runs up to summation order (the last TIMED step is not: several AdamW steps amplify
    the backward's atomic-order differences to 0.1-1 of the gradients' norm)."""
    import numpy as np
    out = _bench_dump(tmp_path / "a", batch)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out
    assert out["steps"] == 3 and out["warmup"] == 2 and out["dtype"] == "f32"
    assert abs(out["value"] * out["ms_per_step"] - 1000.0 * batch) <= 1e-6 * 1000.0 * batch
    for key in ("roofline", "roofline_hbm", "roofline_op_2px", "split_bf16x3", "mixed_bf16", "step_2px", "cpu_baseline"):
        assert key not in out, key
    names = sorted(os.listdir(tmp_path / "a"))
    assert "params.npy" in names and "grads.npy" in names
    assert len([n for n in names if n.startswith("loss_")]) == 13, names
    total = 0
    for n in names:
        a = np.load(tmp_path / "a" / n)
        assert n.endswith(".npy") and a.dtype == np.float32, (n, a.dtype)
        total += a.nbytes
        if not n.startswith("log_"):                   # log entries may be a mean over an empty set (NaN, as the reference)
            assert np.isfinite(a).all(), n
    assert total <= 64 << 20
    p, g = np.load(tmp_path / "a" / "params.npy"), np.load(tmp_path / "a" / "grads.npy")
    assert p.shape == g.shape and p.ndim == 1 and p.size > 1000 and np.abs(g).max() > 0
    # a second run: the same outputs up to summation order (at 96x320 the stock solver's small layers add ~1e-3 of the
    # gradients' scale)
    _bench_dump(tmp_path / "b", batch)
    assert sorted(os.listdir(tmp_path / "b")) == names
    for n in names:
        a, b = np.load(tmp_path / "a" / n).astype(np.float64), np.load(tmp_path / "b" / n).astype(np.float64)
        fin = np.isfinite(b)
        assert (np.isfinite(a) == fin).all(), n
        rel = np.linalg.norm(a[fin] - b[fin]) / max(np.linalg.norm(b[fin]), 1e-30)
        assert rel <= (1e-2 if n == "grads.npy" else 1e-3), (n, rel)
