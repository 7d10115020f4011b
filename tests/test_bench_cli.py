"""bench.py's command line: a plain run times its steps and prints the headline line only; --dump-outputs writes what the last
timed step computed (float32 .npy, bounded in size, sampled with a fixed seed)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_dump_sample_is_bounded_and_fixed():
    b = _bench_module()
    cap = b.DUMP_MAX_ELEMENTS["parameters"]
    small = torch.arange(1000, dtype=torch.float32)
    assert b._dump_sample("parameters", small) is small
    big = torch.arange(cap + 12345, dtype=torch.float32)
    s1, s2 = b._dump_sample("parameters", big), b._dump_sample("parameters", big)
    assert s1.numel() == cap and torch.equal(s1, s2)
    assert bool((s1[1:] > s1[:-1]).all())                       # distinct entries, in arena order
    assert 4 * sum(b.DUMP_MAX_ELEMENTS.values()) + 64 <= 64 << 20


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path):
    out_dir = tmp_path / "out"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0 and out["dtype"] == "bf16"
    assert abs(out["value"] - 2 * 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]
    assert not {"cpu_baseline", "roofline", "step"} & set(out) and "comm_plan" not in out["config"]   # --full only
    files = {f: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}
    assert set(files) == {"loss.npy", "ce.npy", "dice.npy", "logits.npy", "parameters.npy"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert files["logits.npy"].shape == (2, 9, 224, 224) and files["parameters.npy"].size == 4 << 20
    assert abs(float(files["loss.npy"].reshape(-1)[0]) - out["config"]["final_loss"]) < 1e-6
