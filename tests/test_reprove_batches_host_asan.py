"""The index arithmetic of dapol_reprove_batches_plan / dapol_reprove_batches (dapol_amd/csrc/reprove_batches_plan.inc) replayed through
tests/cpp/reprove_batches_plan_host.cpp: a host-only build with its own main, run as a child process under ASan + UBSan (every array in
a heap buffer of exactly its size).  The shapes are tests/test_reprove_batches_plan_cpu.py's, with heights 63 and 64 and indexes at
2^64 - 1 for the shifts; what comes back is compared with that file's brute-force model and with the layouts restated here."""
import functools
import json
import os
import subprocess

from conftest import ROOT

from test_reprove_batches_plan_cpu import SHAPES, TOP, model, policy_plan

SHAPES_HOST = dict(SHAPES)
SHAPES_HOST[63] = ([[0], [(1 << 63) - 1], [0, (1 << 63) - 1], [(1 << 62) - 1, 1 << 62], [4, 5, 6, 7]],
                   [[], [0], [(1 << 63) - 1], [1, 1 << 62, (1 << 63) - 2]])


@functools.lru_cache(maxsize=None)
def _exe():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "reprove_batches_plan_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I", os.path.join(ROOT, "dapol_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "reprove_batches_plan_host.cpp"), "-o", exe], check=True)
    return exe


def _replay(lines):
    r = subprocess.run([_exe()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def _plan_line(hip_lib, height, batches, edited, policy, agg, has_old):
    words = ["plan", height, policy, agg, len(batches)]
    for j, b in enumerate(batches):
        level, index = hip_lib.batch_siblings(height, b)
        words += [1 if has_old is None else int(bool(has_old[j])), len(level)] + [int(x) for x in level] + [int(x) for x in index]
    return " ".join(str(w) for w in words + [len(edited)] + list(edited))


def test_planner_replayed_under_asan_matches_the_brute_force(hip_lib):
    lines, wants = [], []
    for leaf_first in (0, 1):
        old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
        try:
            for height, (batches, edits) in sorted(SHAPES_HOST.items()):
                min_S = min(len(hip_lib.batch_siblings(height, b)[0]) for b in batches)
                some_old = [(j * 7 + 1) % 3 != 0 for j in range(len(batches))]
                for policy in (0, 1):
                    for agg in sorted({0, min_S}):
                        for edited in edits:
                            for has_old in (None, some_old):
                                lines.append(_plan_line(hip_lib, height, batches, edited, policy, agg, has_old))
                                wants.append(model(hip_lib, height, batches, edited, policy, agg, has_old))
        finally:
            hip_lib.wire_config_restore(old)
    assert any(" %d" % TOP in ln for ln in lines)
    for ln, g, (n_proved, tot, sm, sm_all) in zip(lines, _replay(lines), wants):
        assert g["ok"] == 1 and g["n_proved"] == n_proved and (g["total"], g["sum_m"], g["sum_m_all"]) == (tot, sm, sm_all), ln
    bad = _replay(["plan 5 0 0 1 1 0 2 3 3", "plan 5 0 0 1 1 0 2 4 3", "plan 5 0 0 1 1 0 1 32", "plan 5 2 0 1 1 0 0", "plan 5 0 1 1 1 0 0",
                   "plan 64 0 0 1 1 0 1 %d" % TOP])
    assert [b["ok"] for b in bad] == [-1, -1, -1, 0, 0, 1]


def test_entries_and_layout_under_asan(hip_lib):
    cases = [(0, 6, 0, 8, [1]), (0, 6, 4, 8, [1, 4]), (1, 6, 3, 64, [1, 2]), (0, 4, 4, 8, [1, 4, 8]), (1, 7, 7, 16, [4, 2, 1]), (0, 0, 0, 8, [1]),
             (1, 0, 0, 8, [1]), (0, 62, 16, 64, [1, 16])]
    lines = ["entries %d %d %d %d %d %s" % (p, S, agg, n, len(cm), " ".join(map(str, cm))) for p, S, agg, n, cm in cases]
    for (p, S, agg, n, cm), g in zip(cases, _replay(lines)):
        plan = policy_plan(p, S, agg)
        assert list(zip(g["start"], g["count"], g["m"])) == plan
        assert g["cls"] == [cm.index(m) for _, _, m in plan]
        pieces = [hip_lib.lib().dapol_range_proof_size(n, m) // 16 for _, _, m in plan]
        assert g["pieces"] == pieces and g["piece0"] == [sum(pieces[:i]) for i in range(len(plan))]
        assert sum(pieces) * 16 == hip_lib.lib().dapol_entity_proof_size(S, p, agg, n)
        assert g["slot"] == [sum(m * (2 * n + 4) for _, _, m in plan[:i]) for i in range(len(plan))]      # the running sum of the draws
    lay = _replay(["layout 100 3 1 4 16 17 21 25 0 40 40 43", "layout 0 1 1 17 0 0", "layout 4294967295 2 1 2 42 46 0 7 4294967295"])
    assert lay[0] == {"party_off": [0, 40, 40], "piece_off": [0, 680, 680], "base_at": [0, 100, 200], "flag_at": [99, 199, 299], "parties": 88,
                      "proof_pieces": 755}
    assert lay[1] == {"party_off": [0], "piece_off": [0], "base_at": [0], "flag_at": [0], "parties": 0, "proof_pieces": 0}
    assert lay[2]["party_off"] == [0, 7] and lay[2]["parties"] == 7 + 2 * (4294967295 - 7) and lay[2]["flag_at"] == [4294967294, 2 * 4294967295 - 1]
