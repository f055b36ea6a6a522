"""bench.py end to end on a small shape: a plain run prints the line without the CPU baseline and the parity gate, --full adds
both and passes the gate."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--height", "128", "--width", "160", "--outer", "2", "--inner", "2"]


def _run(extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_leaves_out_the_cpu_baseline_and_parity():
    res = _run([])
    assert res["value"] > 0 and res["ms_per_step"] > 0 and res["steps"] == 2 and res["warmup"] == 1
    assert res["cpu_baseline"] is None and res["parity"] is None and "speedup_vs_cpu" not in res
    assert res["kernels"] and res["f16x3_range_events"] == 0


@pytest.mark.gpu
def test_full_run_adds_the_cpu_baseline_and_passes_the_parity_gate():
    res = _run(["--full", "--cpu-runs", "1"])
    assert res["value"] > 0 and res["cpu_baseline"]["value"] > 0 and res["speedup_vs_cpu"] > 0
    assert res["parity"]["ok"] and res["parity"]["exact_identity_start"]["ok"]
