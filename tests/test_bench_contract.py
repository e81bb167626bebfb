"""bench.py driver-contract tests: single JSON line, correct fields,
works under torch.distributed.run exactly as the driver launches it."""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).parent.parent


def _check_line(line: str, n_gpus: int):
    rec = json.loads(line)
    # every field the driver's contract names must be present
    required = {"metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"}
    assert required <= rec.keys(), required - rec.keys()
    assert rec["metric"] == "sd21_256px_finetune_imgs_per_sec"
    assert rec["n_gpus"] == n_gpus
    assert rec["higher_is_better"] is True
    assert rec["scaling"] == "weak"
    assert rec["data"] == "synthetic"
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    assert rec["config"]["global_batch"] == 2 * n_gpus
    assert rec["config"]["parallelism"] == f"dp{n_gpus}"
    assert {"model", "global_batch", "seq_len"} <= rec["config"].keys()
    return rec


def test_bench_single_process(tmp_path):
    r = subprocess.run(
        [sys.executable, str(ROOT / "bench.py"), "--steps", "2", "--warmup",
         "1", "--model", "tiny", "--resolution", "64", "--batch-size", "2"],
        capture_output=True, text=True, cwd=str(ROOT), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout  # exactly ONE JSON line
    _check_line(lines[0], 1)


def _run_tiny(*extra):
    r = subprocess.run(
        [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--warmup",
         "1", "--model", "tiny", "--resolution", "64", "--batch-size", "2",
         *extra],
        capture_output=True, text=True, cwd=str(ROOT), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return _check_line(lines[0], 1)


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last timed step's arrays as float32 .npy,
    the same arguments give the same inputs (so the same outputs, up to
    the GPU's reduction order), --steps is honoured, --full is accepted
    and leaves the result line's meaning alone."""
    import numpy as np

    recs = [_run_tiny("--steps", "3", "--dump-outputs", str(tmp_path / "a")),
            _run_tiny("--steps", "3", "--dump-outputs", str(tmp_path / "b"),
                      "--full")]
    for rec in recs:
        assert rec["steps"] == 3 and rec["warmup"] == 1
        assert rec["unit"] == "imgs/sec"
        # value and ms_per_step describe the same timed window
        assert abs(rec["value"] * rec["ms_per_step"] / 1000.0 - 2) < 0.01
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["grad_sample.npy", "loss.npy", "param_sample.npy"]
    assert names == sorted(p.name for p in (tmp_path / "b").iterdir())
    total = 0
    arr = {}
    for n in names:
        a = np.load(tmp_path / "a" / n)
        b = np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and a.shape == b.shape and a.size > 0
        total += a.nbytes
        assert np.isfinite(a).all() and np.isfinite(b).all(), n
        if recs[0]["dtype"] == "fp32":  # CPU run: bit-reproducible
            assert np.array_equal(a, b), n
        arr[n] = (a, b)
    assert total <= 64 * 2**20
    # the tiny UNet has more than 2^20 weights, so this run takes the
    # seeded-sample branch: exactly 2^20 positions, the same in both runs
    assert arr["grad_sample.npy"][0].shape == (2**20,)
    assert arr["param_sample.npy"][0].shape == (2**20,)
    la, lb = arr["loss.npy"]
    assert la.shape == (1,)
    # Identical inputs and seeds; on the GPU only the order of fp32
    # atomics/reductions differs between runs, which flips bf16 roundings
    # (1 ulp = 2^-8) along the way. Loss: a mean over 2*4*8*8 squared fp32
    # errors, well inside 1e-2. Gradient: each element passes on the order
    # of 150 bf16 roundings through the backward chain; as a random walk
    # that is 2^-8 * sqrt(150) ~ 5% relative L2. Weights: fp32 master,
    # 4 AdamW updates of at most lr = 5e-6 each, so two runs cannot
    # differ by more than 4e-5 however the gradients differ.
    assert np.allclose(la, lb, rtol=1e-2)
    ga, gb = arr["grad_sample.npy"]
    assert np.linalg.norm(ga - gb) <= 0.05 * np.linalg.norm(ga)
    assert np.linalg.norm(ga) > 0
    pa, pb = arr["param_sample.npy"]
    assert np.abs(pa - pb).max() <= 4e-5


_COUNT_STEPS = """
import sys
import bench
from dcr_amd.train import Trainer
calls = []
orig = Trainer.train_step
def counted(self, *a, **k):
    calls.append(1)
    return orig(self, *a, **k)
Trainer.train_step = counted
sys.argv = ["bench.py"] + sys.argv[1:]
bench.main()
print("train_step calls:", len(calls), file=sys.stderr)
"""


def test_bench_steps_sets_the_timed_steps():
    """--steps N --warmup W runs exactly W + N train steps (counted at the
    trainer, not read back from the result line), and ms_per_step is the
    timed window divided by N."""
    for steps, warmup in ((1, 0), (4, 2)):
        r = subprocess.run(
            [sys.executable, "-c", _COUNT_STEPS, "--gpus", "1", "--steps",
             str(steps), "--warmup", str(warmup), "--model", "tiny",
             "--resolution", "64", "--batch-size", "2"],
            capture_output=True, text=True, cwd=str(ROOT), timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert f"train_step calls: {steps + warmup}\n" in r.stderr, \
            r.stderr[-500:]
        lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
        rec = _check_line(lines[0], 1)
        assert rec["steps"] == steps and rec["warmup"] == warmup


def test_bench_rejects_zero_steps():
    r = subprocess.run(
        [sys.executable, str(ROOT / "bench.py"), "--steps", "0"],
        capture_output=True, text=True, cwd=str(ROOT), timeout=600)
    assert r.returncode != 0 and "--steps" in r.stderr


def test_bench_torchrun_world2(tmp_path):
    """the driver's launch shape: torch.distributed.run, one rank/'GPU'."""
    env = {**os.environ, "MASTER_ADDR": "127.0.0.1"}
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29533", str(ROOT / "bench.py"), "--gpus", "2",
         "--steps", "2", "--warmup", "1", "--model", "tiny", "--resolution",
         "64", "--batch-size", "2"],
        capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout  # only rank 0 prints
    _check_line(lines[0], 2)
