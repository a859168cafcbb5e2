"""The range prover's decisions (dapol_amd/csrc/prove_plan.inc: regime, chunking, lanes per list, splits, slices and tiles) against
tests/golden/prove_plan.json, which was recorded on the GPU from the code as it stood before the planning moved into that file.
Every regime gives the same proof bytes, so nothing else notices a threshold that moved; this does, field for field.
tests/cpp/prove_plan_host.cpp is a host-only build of the planning; see its header."""
import json
import os
import subprocess

from conftest import ROOT


def _build():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "prove_plan_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "dapol_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "prove_plan_host.cpp"), "-o", exe], check=True)
    return exe


def test_every_recorded_plan_is_reproduced():
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "prove_plan.json")))["rows"]
    assert len(rows) == 48
    lines = [" ".join(["%s=%s" % kv for kv in row["env"].items()] + ["%s=%d" % kv for kv in row["in"].items()]) for row in rows]
    env = {k: v for k, v in os.environ.items() if not k.startswith("DAPOL_")}      # a row's knobs are the only ones
    r = subprocess.run([_build()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stderr
    got = [{t.split("=")[0]: int(t.split("=")[1]) for t in line.split()} for line in r.stdout.splitlines()]
    assert len(got) == len(rows)
    bad = []
    for row, plan in zip(rows, got):
        assert plan.keys() == row["plan"].keys()
        diff = {k: (row["plan"][k], plan[k]) for k in plan if plan[k] != row["plan"][k]}
        if diff:
            bad.append(((row["in"]["n"], row["in"]["m"], row["in"]["B"]), row["env"], diff))
    assert not bad, "plans differ (field: (recorded, computed)): %r" % (bad,)
