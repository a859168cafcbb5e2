"""What the DAPOL_PREP=v2 digit producers rest on, on the CPU: tests/cpp/prep_scalars_host.cpp (sc.h compiled for the host, a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer) -- the unrolled recode against sc_recode_w on edge and
random scalars, and the shared fold scalars against the plain coefficients -- and the plan's side of the knob through
tests/cpp/prep_plan_host.cpp: which calls take which producers, and that the knob moves no byte of the scratch layout."""
import os
import subprocess

from conftest import ROOT

MI355X = {"opt_tail_length": 0, "opt_small_call_max": 0, "opt_generator_stationary": 0, "opt_streams": 0, "opt_chunk_proofs": 0, "opt_gs_tile_rows": 0,
          "opt_gs_slices": 0, "wbits": 17, "nwin": 15, "hi_split": 8, "n_cu": 256, "resident_waves": 4096, "budget_bytes": 139586437120, "timed": 0}
LAYOUT = ("N", "tail_n", "gs", "gs_mat", "small_call", "stab_main", "stab_tail", "chunk", "nlanes", "dig_elems", "stab_bytes", "acc_bytes", "acc_slots",
          "per_proof", "lane_bytes", "lpl", "tail_gs")


def _build(name, flags):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags + ["-I", os.path.join(ROOT, "dapol_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe], check=True)
    return exe


def test_recode_and_shared_scalars_under_sanitizers():
    exe = _build("prep_scalars_host", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 80000, r.stdout


def _plans(rows):
    exe = _build("prep_plan_host", [])
    lines = [" ".join(["%s=%s" % kv for kv in env.items()] + ["%s=%d" % kv for kv in dict(MI355X, n=n, m=m, B=b).items()]) for n, m, b, env in rows]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("DAPOL_")}
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60, env=clean)
    assert r.returncode == 0, r.stderr
    got = [{t.split("=")[0]: int(t.split("=")[1]) for t in line.split()} for line in r.stdout.splitlines()]
    assert len(got) == len(rows)
    return got


def test_the_knob_chooses_the_producers_and_moves_no_byte():
    v1, v2 = {"DAPOL_PREP": "v1"}, {"DAPOL_PREP": "v2"}
    shapes = [(64, 32, 1 << 20), (64, 32, 5000), (64, 32, 40), (64, 8, 65536), (64, 1, 4096), (32, 32, 1 << 16)]
    for n, m, b in shapes:
        dflt, new, old, junk = _plans([(n, m, b, {}), (n, m, b, v2), (n, m, b, v1), (n, m, b, {"DAPOL_PREP": "v1x"})])
        assert dflt == new == junk                                             # v2 is the default; an unknown value is no value
        assert old["prep_recode"] == old["prep_share"] == 0
        assert new["prep_recode"] == new["gs"]                                 # every swept call recodes through write_digits_gs
        assert new["prep_share"] == (new["gs_mat"] & new["stab_main"])         # the shared scalars need the swept materialisation and the tables
        for k in LAYOUT:
            assert new[k] == old[k], (n, m, b, k)
    head = _plans([(64, 32, 1 << 20, {})])[0]
    assert (head["gs"], head["gs_mat"], head["stab_main"], head["prep_recode"], head["prep_share"], head["chunk"]) == (1, 1, 1, 1, 1, 131072)
    # vector mode (no coefficient tables) and the proof-stationary materialisation keep the scalars per generator
    no_stab, no_mat, ps = _plans([(64, 32, 1 << 20, {"DAPOL_NO_STAB": "1"}), (64, 32, 1 << 20, {"DAPOL_NO_GS_MAT": "1"}), (64, 32, 1 << 20, {"DAPOL_GS": "0"})])
    assert (no_stab["prep_recode"], no_stab["prep_share"]) == (1, 0) and no_stab["stab_main"] == 0
    assert (no_mat["prep_recode"], no_mat["prep_share"]) == (1, 0) and no_mat["gs_mat"] == 0
    assert (ps["prep_recode"], ps["prep_share"], ps["gs"]) == (0, 0, 0)
