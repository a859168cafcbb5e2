"""ProvePlan::tail_gs (dapol_amd/csrc/prove_plan.inc): which calls run their tail rounds with a lane per (proof, list, window), what
DAPOL_TAIL_ORDER forces, and that the decision moves no byte of the scratch layout unless it is forced onto a call without
accumulators -- on the CPU, through tests/cpp/tail_order_plan_host.cpp.  (tests/test_prove_plan_cpu.py keeps every older field.)"""
import os
import subprocess

from conftest import ROOT

MI355X = {"opt_tail_length": 0, "opt_small_call_max": 0, "opt_generator_stationary": 0, "opt_streams": 0, "opt_chunk_proofs": 0, "opt_gs_tile_rows": 0,
          "opt_gs_slices": 0, "wbits": 17, "nwin": 15, "hi_split": 8, "n_cu": 256, "resident_waves": 4096, "budget_bytes": 139586437120, "timed": 0}
REC_NEED = 2 * 51 * 36 * 4          # two lists x 51 windows x (X | Y | Z | T of 9 limbs)


def _plans(rows):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "tail_order_plan_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "dapol_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "tail_order_plan_host.cpp"), "-o", exe], check=True)
    lines = [" ".join(["%s=%s" % kv for kv in env.items()] + ["%s=%d" % kv for kv in dict(MI355X, n=n, m=m, B=b).items()]) for n, m, b, env in rows]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("DAPOL_")}
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60, env=clean)
    assert r.returncode == 0, r.stderr
    got = [{t.split("=")[0]: int(t.split("=")[1]) for t in line.split()} for line in r.stdout.splitlines()]
    assert len(got) == len(rows)
    return got


def test_the_knob_forces_either_order_for_any_call_with_a_tail():
    gs, ps = {"DAPOL_TAIL_ORDER": "gs"}, {"DAPOL_TAIL_ORDER": "ps"}
    rows = [(64, 32, 40, gs), (64, 32, 40, ps), (64, 32, 5000, gs), (64, 32, 5000, ps), (64, 32, 1 << 20, gs), (64, 32, 1 << 20, ps),
            (64, 8, 65536, gs), (64, 32, 8, gs), (64, 1, 4096, gs), (64, 32, 40, {"DAPOL_TAIL_ORDER": "gsx"})]
    small_gs, small_ps, mid_gs, mid_ps, big_gs, big_ps, short_gs, no_tail, no_tail_1, junk = _plans(rows)
    for p in (small_gs, mid_gs, big_gs, short_gs):
        assert p["tail_n"] > 0 and p["tail_gs"] == 1 and p["tail_order"] == 1
        assert p["acc_bytes"] + p["tail_rec_bytes"] >= REC_NEED == p["tail_rec_need"]
    for p in (small_ps, mid_ps, big_ps):
        assert p["tail_n"] > 0 and p["tail_gs"] == 0 and p["tail_order"] == -1 and p["tail_rec_bytes"] == 0
    # a call without a tail has no order to force, and an unknown value is no value
    assert no_tail["tail_n"] == 0 and no_tail["tail_gs"] == 0 and no_tail["tail_rec_bytes"] == 0
    assert no_tail_1["tail_n"] == 0 and no_tail_1["tail_gs"] == 0 and no_tail_1["tail_rec_bytes"] == 0
    assert junk["tail_order"] == 0 and junk["tail_gs"] == 0
    # the record area grows only where the order is forced onto a call without (enough) accumulators: a latency-shaped call
    assert small_gs["acc_bytes"] == 0 and small_gs["tail_rec_bytes"] == REC_NEED and small_gs["per_proof"] == small_ps["per_proof"] + REC_NEED
    for a, b in ((mid_gs, mid_ps), (big_gs, big_ps)):
        assert a["tail_rec_bytes"] == 0 and a["per_proof"] == b["per_proof"] and a["lane_bytes"] == b["lane_bytes"] and a["chunk"] == b["chunk"]


def test_the_plans_own_choice_and_the_headline_chunk():
    """Without the knob the new order is taken, if at all, only by swept calls of long lists in full chunks, out of accumulators that are there; the
    headline's chunk (131,072 proofs of 64 bits x 32 parties in 102 GB) is the same size whichever order runs."""
    rows = [(64, 32, 1 << 20, {}), (64, 32, 65536, {}), (64, 32, 65535, {}), (64, 32, 5000, {}), (64, 32, 40, {}), (64, 8, 65536, {}),
            (64, 32, 1 << 20, {"DAPOL_GS": "0"}), (64, 32, 1 << 20, {"DAPOL_TAIL_ORDER": "gs"}), (64, 32, 1 << 20, {"DAPOL_TAIL_ORDER": "ps"})]
    head, full, below, mid, small, short, ps_form, head_gs, head_ps = _plans(rows)
    assert head["chunk"] == 131072 and head["tail_n"] == 64 and head["gs"] == 1
    assert head["lane_bytes"] == head_gs["lane_bytes"] == head_ps["lane_bytes"] == (131072 * 873952 + 8192 + 4095) // 4096 * 4096
    assert head["acc_bytes"] == 69120 >= REC_NEED
    for p in (head, full, below, mid, small, short, ps_form):
        assert p["tail_rec_bytes"] == 0
    assert head["tail_gs"] == full["tail_gs"]                                   # full chunks: one decision
    for p in (below, mid, small, short, ps_form):                              # below a full chunk, short lists, or not swept: proof-stationary
        assert p["tail_gs"] == 0


def test_rows_per_lane_of_the_tail_table():
    """DAPOL_TAIL_ROWS_PER_LANE = 1 / 4 forces k_rp_tail_table's rows per lane for any call with a tail; anything else is no value; a
    call without a tail builds no table; the plan's own choice is one row wherever a lane's chain is the launch's latency."""
    four, one = {"DAPOL_TAIL_ROWS_PER_LANE": "4"}, {"DAPOL_TAIL_ROWS_PER_LANE": "1"}
    rows = [(64, 32, 40, four), (64, 32, 40, one), (64, 32, 1 << 20, four), (64, 32, 1 << 20, one), (64, 8, 40, dict(four, DAPOL_TAIL_N="32")),
            (64, 32, 8, four), (64, 32, 40, {"DAPOL_TAIL_ROWS_PER_LANE": "3"}), (64, 32, 40, {}), (64, 32, 5000, {}), (64, 32, 1 << 20, {})]
    s4, s1, h4, h1, t32, no_tail, junk, small, mid, head = _plans(rows)
    assert (s4["tail_rpl"], s1["tail_rpl"], h4["tail_rpl"], h1["tail_rpl"]) == (4, 1, 4, 1)
    assert t32["tail_n"] == 32 and t32["tail_rpl"] == 4
    assert no_tail["tail_n"] == 0 and no_tail["tail_rpl"] == 1
    assert junk["tail_rpl"] == small["tail_rpl"] == mid["tail_rpl"] == 1
    assert head["tail_rpl"] in (1, 4)
    for a, b in ((s4, s1), (h4, h1)):                                       # the rows per lane move nothing in the scratch layout
        assert a["per_proof"] == b["per_proof"] and a["lane_bytes"] == b["lane_bytes"] and a["chunk"] == b["chunk"]
