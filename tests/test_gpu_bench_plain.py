"""`bench.py --gpus 1` as every later change is measured with it: a plain run times its steps and
prints the line and nothing else (no roofline report, no CPU baseline), `--dump-outputs` writes the
last timed step's outputs, `--full` brings the roofline report back. Config 2 (3.8 GB of tables) and
a handful of steps keep each run to a few seconds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--workload", "config2", "--steps", "5", "--warmup", "3", "--batches", "8"]


def run_bench(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "bench.py", *SMALL, *extra], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=150)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_its_steps_and_dumps_its_outputs(tmp_path):
    d = run_bench(["--dump-outputs", str(tmp_path)])
    assert d["steps"] == 5 and d["warmup"] == 3 and d["n_gpus"] == 1
    assert d["unit"] == "pairs/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["roofline"] is None and d["cpu_baseline"] is None
    B = d["config"]["per_gpu_batch"]
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(B / d["ms_per_step"] * 1e3, rel=1e-3)  # both rounded from one interval
    got = {p.name[:-4]: np.load(p) for p in tmp_path.iterdir()}
    assert {"loss", "logits", "params", "table0_batch0_rows", "table0_batch0_state", "table1_seeded_rows"} <= set(got)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    assert got["logits"].shape == (B,) and got["table1_batch0_rows"].shape[1] == d["config"]["emb_dim"]
    assert float(got["loss"][0]) == d["loss"]
    # the rows of the first resident batch have been trained: their Adagrad state has left zero
    assert (got["table0_batch0_state"] > 0).any() and (got["table1_batch0_state"] > 0).any()


def test_full_run_reports_the_roofline_beside_the_same_line():
    d = run_bench(["--full", "--no-cpu-baseline"])
    assert d["steps"] == 5 and d["ms_per_step"] > 0 and d["cpu_baseline"] is None
    k = d["roofline"]["kernels"]
    assert k["t1"]["ms"] > 0 and d["roofline"]["embedding_path"]["bytes_per_step"] > 0
