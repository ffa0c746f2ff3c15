"""bench.py as every change runs it: a plain run (set-up, warm-up, the timed steps, the line) with --dump-outputs, and the same
command with --full, whose timed steps must leave the same outputs behind and whose line adds the checks a plain run leaves out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 32768
ARGS = ["--gpus", "1", "--workload", "config1", "--batch-reads", str(B), "--steps", "3", "--warmup", "1"]


def _run(extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "bench.py"] + ARGS + extra, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _dump(d):
    files = sorted(os.listdir(d))
    assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64e6
    out = {f[:-len(".npy")]: np.load(os.path.join(d, f)) for f in files}
    assert out and all(a.dtype in (np.float32, np.float64) for a in out.values())
    return out


def test_plain_run_dumps_outputs_and_full_run_adds_the_checks(tmp_path):
    a = _run(["--dump-outputs", str(tmp_path / "plain")])
    assert a["steps"] == 3 and a["warmup"] == 1 and a["n_gpus"] == 1 and a["higher_is_better"] is True
    assert a["unit"] == "reads/s" and a["metric"] and a["dtype"]
    assert a["value"] == pytest.approx(B * 1e3 / a["ms_per_step"], rel=1e-4)
    for k in ("sanity_batch", "planted_recall", "cpu_baseline", "secondary", "value_host_to_host"):
        assert k not in a, k  # --full's
    assert a["roofline"]["achieved"] is None and a["roofline"]["kernel_ms"] <= a["ms_per_step"]
    da = _dump(tmp_path / "plain")
    assert np.array_equal(da["query_index"], np.arange(B)) and np.all(da["query_len"] == 150)
    assert np.all(da["query_kmers"] <= 130) and da["query_kmers"].mean() > 129
    n_m = len(da["match_col"])
    assert n_m > 0.5 * B and all(len(da[k]) == n_m for k in da if k.startswith("match_"))
    assert np.all(np.diff(da["match_query"]) >= 0) and np.all(da["match_qcov"] >= 0.55 - 1e-12)
    assert 0 <= da["match_col"].min() and da["match_col"].max() < a["config"]["columns"]

    f = _run(["--dump-outputs", str(tmp_path / "full"), "--full", "--no-cpu-baseline", "--no-extras"])
    assert f["sanity_batch"]["hits"] > 0.5 * B and f["planted_recall"] > 0.99 and f["roofline"]["achieved"] > 0
    assert f["hits_per_step"] == a["hits_per_step"] and f["matches_per_step"] == a["matches_per_step"]
    df = _dump(tmp_path / "full")
    assert sorted(df) == sorted(da) and all(np.array_equal(da[k], df[k]) for k in da)
