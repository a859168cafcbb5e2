"""The range verifier's decisions (dapol_amd/csrc/verify_plan.inc: batched or proof by proof, the generator MSM's shape, chunking, bucket
method or per-point tables, transcript shapes, forks, the carve-up of the scratch) against tests/golden/verify_plan.json, which was
recorded on the GPU from the code as it stood before the planning moved into that file.  Every regime gives the same verdicts, so
nothing else notices a threshold that moved; this does, field for field.  tests/cpp/verify_plan_host.cpp is a host-only build of the
planning (see its header); it runs over the rows twice, the second time built with AddressSanitizer and UBSan."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

ROWS = json.load(open(os.path.join(ROOT, "tests", "golden", "verify_plan.json")))["rows"]


def _build(name, flags):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", *flags, "-I", os.path.join(ROOT, "dapol_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "verify_plan_host.cpp"), "-o", exe], check=True)
    return exe


def _replay(exe):
    """-> per row {"call": {...}, "rlc": {...}, "rlc_chunks": [...], "rv": {...} or None, "rv_chunks": [...]} in the golden's layout"""
    lines = [" ".join(["%s=%s" % kv for kv in row["env"].items()] + ["%s=%d" % kv for kv in row["in"].items()]) for row in ROWS]
    env = {k: v for k, v in os.environ.items() if not k.startswith("DAPOL_")}      # a row's knobs are the only ones
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and not r.stderr, r.stderr
    fresh = lambda: {"call": None, "rlc": None, "rlc_chunks": [], "rv": None, "rv_chunks": []}
    got, cur = [], fresh()
    for line in r.stdout.splitlines():
        kind, *tokens = line.split()
        fields = {t.split("=")[0]: int(t.split("=")[1]) for t in tokens}
        if kind == "end":
            got.append(cur)
            cur = fresh()
        elif kind in ("call", "rlc", "rv"):
            assert cur[kind] is None
            cur[kind] = fields
        else:
            cur[kind + "s"].append(fields)
    return got


@pytest.mark.parametrize("name,flags", [("verify_plan_host", []),
                                        ("verify_plan_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_every_recorded_plan_is_reproduced(name, flags):
    assert len(ROWS) == 68
    got = _replay(_build(name, flags))
    assert len(got) == len(ROWS)
    bad = []
    for row, plan in zip(ROWS, got):
        # (the rows came through dapol_range_verify_batch: a VArrival was attached where verify_pipe_arrival says so)
        if plan["call"] != {"pipe": 1 if row["in"]["va_K"] else 0}:
            bad.append((row["ctx"], (row["in"]["n"], row["in"]["m"], row["in"]["b"]), row["env"], "pipe", "recorded va_K", row["in"]["va_K"], "computed", plan["call"]))
        for part in ("rlc", "rlc_chunks", "rv", "rv_chunks"):
            if plan[part] != row[part]:
                bad.append((row["ctx"], (row["in"]["n"], row["in"]["m"], row["in"]["b"]), row["env"], part, "recorded", row[part], "computed", plan[part]))
    assert not bad, "plans differ: %r" % (bad,)


def test_the_rows_cover_both_sides_of_every_hand_over():
    """The golden pins a threshold only if rows sit on both sides of it."""
    rlc = [r for r in ROWS if r["rlc"]["use_rlc"]]
    rv = [r for r in ROWS if r["rv"]]
    assert len(rlc) + len(rv) == len(ROWS)
    assert {(r["in"]["b"], r["in"]["va_K"]) for r in ROWS if r["in"]["m"] == 1024 and not r["env"]} >= {(255, 0), (256, 4)}     # the 8 MB of commitments
    for field in ("small_call", "use_hi", "quad", "tree_sum", "wave_transcript", "wave_replay", "side_var"):
        assert {r["rv"][field] for r in rv} == {0, 1}, field
    assert {c["quad_var"] for r in rv for c in r["rv_chunks"]} == {0, 1}
    assert any(r["rv"]["var_waves"] <= 16 for r in rv) and any(r["rv"]["var_waves"] > 16 for r in rv)
    assert any(r["rv"]["chunk"] < r["in"]["b"] for r in rv)
    assert {r["rv"]["N"] for r in rv} >= {128, 256}
    assert {r["in"]["b"] for r in rv} >= {128, 129}
    for field in ("pipelined", "quad_gen", "gen_sweep", "use_hi", "fork_points", "wave_transcript"):
        assert {r["rlc"][field] for r in rlc} == {0, 1}, field
    for field in ("pippenger", "lazy", "wave_replay", "fork"):
        assert {c[field] for r in rlc for c in r["rlc_chunks"]} == {0, 1}, field
    assert {c["cb"] for r in rlc for c in r["rlc_chunks"]} >= {4096, 4097}
    assert {c["npts"] for r in rlc for c in r["rlc_chunks"]} >= {32712, 32770, 32759, 32776}       # 564 / 565 x 58, 1,927 / 1,928 x 17
    assert {r["rlc"]["N"] for r in rlc if not r["in"]["hi_split"]} >= {2048, 4096}
    assert any(r["rlc"]["nch"] == 1 for r in rlc) and any(len(r["rlc_chunks"]) == 2 for r in rlc)
    assert {r["rlc"]["pip_min"] for r in rlc} >= {32768, 12288, 2 ** 64 - 1}
    for r in ROWS:                                      # rlc_min - 1 and rlc_min, by default, by option and by knob
        assert r["rlc"]["use_rlc"] == (r["in"]["b"] >= r["rlc"]["rlc_min"] and "DAPOL_VERIFY_NO_RLC" not in r["env"])
    assert {(r["rlc"]["rlc_min"], r["in"]["b"]) for r in ROWS} >= {(112, 111), (112, 112), (200, 199), (200, 200), (150, 149), (150, 150)}
