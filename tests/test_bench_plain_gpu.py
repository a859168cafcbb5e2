"""A plain bench.py run does only what its headline needs: one JSON line right after the timed steps, none of --full's legs, and
the same workload as a --full run of the same arguments (same checksum)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--log2-entities", "10", "--height", "16", "--steps", "2", "--warmup", "1"] + list(extra)
    run = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, DAPOL_TABLE_GB="3"), capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-2000:]
    return [json.loads(l) for l in run.stdout.splitlines() if l.startswith("{")], run.stderr


@pytest.mark.gpu
def test_plain_run_is_lean_and_full_runs_the_legs(hip_lib):
    lines, err = _run()
    assert len(lines) == 1
    plain = lines[0]
    assert plain["complete"] and not plain["full"] and plain["steps"] == 2 and plain["warmup"] == 1 and plain["ms_per_step"] > 0
    assert plain["value"] > 0 and plain["higher_is_better"] and plain["unit"] == "entities/s"
    assert plain["cpu_baseline"] is None and plain["parity"] is None and plain["secondary"] is None
    assert "CPU baseline" not in err and "secondary legs" not in err
    lines, _ = _run("--full", "--no-secondary", "--cpu-budget-s", "2")
    assert len(lines) == 2 and not lines[0]["complete"] and lines[1]["complete"] and lines[1]["full"]
    full = lines[1]
    assert full["cpu_baseline"]["value"] > 0 and full["parity"]["bit_exact"]
    assert full["parity"]["inclusion_proofs_verified_on_gpu"] == full["parity"]["inclusion_proofs_checked"] > 0
    assert full["checksum"] == plain["checksum"] and full["config"] == {**plain["config"], "device_memory_in_use_gb": full["config"]["device_memory_in_use_gb"]}
