#!/usr/bin/env python3
"""dapol_reprove_batches against dapol_prove_batches on the same edited tree, in the same process: what a caller who serves batch
proofs and holds the previous state's runs after e liabilities were replaced (dapol_tree_update), against what it must run without the
re-prove call.  The shape is bench_batches.py's: 2^16 leaves at stride 2^(height - 16) of a tree of the given height (default 32),
64-bit proofs, `--batches` (default 4,096) batches of k = 2 and of k = 4 random leaves, at padding / 16, splitting / 24 and padding / 0,
edited by 1, 64 and 4,096 replaced liabilities.  Per row: the old proofs are the previous state's, e random leaves get new values and
blindings, then two warm-ups and `--runs` (7) alternating timed runs of each call -- the host clock around the whole call (old arrays in
for the re-prove call, new arrays out for both) with a device synchronise.  Siblings and blobs of the two calls are compared byte for
byte on every run.  Beside each time ratio stands dapol_reprove_batches_plan's sum_m_all / sum_m_proved: what the ratio is compared with.
AHEAD: the re-prove median lies below dapol_prove_batches' median by more than that call's own max - min.  A row whose plan leaves at
least half of the sum of m unproved and that is not AHEAD is a MISS.  The last rows are the worst case -- padding with the factor at
the smallest sibling count of the call, on a context of as many parties, k = 2 only: the one aggregated proof of a batch holds (nearly)
all its siblings, so (nearly) nothing is kept, and the row states what the call costs over dapol_prove_batches.
Prints one JSON document.
Usage: python tools/bench_reprove_batches.py [--height 32] [--batches 4096] [--k 2,4] [--shapes padding/16,splitting/24,padding/0]
                                             [--edits 1,64,4096] [--no-worst] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dapol_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--height", type=int, default=32)
ap.add_argument("--batches", type=int, default=4096)
ap.add_argument("--k", default="2,4")
ap.add_argument("--shapes", default="padding/16,splitting/24,padding/0")
ap.add_argument("--edits", default="1,64,4096")
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--no-worst", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert a.runs >= 7
H, N, NBITS, seed, nb = a.height, 1 << 16, 64, bytes(range(32)), a.batches
rng = np.random.default_rng(1)
idx = (np.arange(N, dtype=np.uint64) << np.uint64(H - 16)).astype(np.uint64)
v = rng.integers(0, 2**32, size=N, dtype=np.uint64)
r = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
r[:, 31] &= 0x0F
lib, P = capi.lib(), (lambda x: x.ctypes.data_as(ctypes.c_void_p))
hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
sd = np.frombuffer(seed, np.uint8).copy()


def timed(fn):
    t0 = time.perf_counter()
    fn()
    assert hip.hipDeviceSynchronize() == 0
    return time.perf_counter() - t0


def stats(ts):
    med = statistics.median(ts)
    return {"median_s": med, "min_s": min(ts), "max_s": max(ts), "spread": (max(ts) - min(ts)) / med, "runs_s": ts}


def chk(rc):
    assert rc == 0, (rc, lib.dapol_last_error())


def pick_batches(k):
    pick = np.sort(rng.integers(0, N, size=(nb, k)), axis=1)
    while True:                                               # k DISTINCT leaves per batch: redraw the rows that repeat one
        dup = (np.diff(pick, axis=1) == 0).any(axis=1)
        if not dup.any():
            return idx[pick]                                  # [nb][k], rows strictly increasing
        pick[dup] = np.sort(rng.integers(0, N, size=(int(dup.sum()), k)), axis=1)


def run_rows(ctx, tree, k, batches, shape, policy, agg, edits, rows, worst=False):
    _, off, flat = capi._pack_batches(list(batches))
    ns, so, ro, ng = capi.batches_plan(H, list(batches), policy, agg, NBITS)
    T, R = int(so[-1]), int(ro[-1])
    old_C, old_R = np.zeros((T, 32), np.uint8), np.zeros(R, np.uint8)
    new_C, new_H, new_R = np.zeros((T, 32), np.uint8), np.zeros((T, 32), np.uint8), np.zeros(R, np.uint8)
    ref_C, ref_H, ref_R = np.zeros((T, 32), np.uint8), np.zeros((T, 32), np.uint8), np.zeros(R, np.uint8)
    proved, kept, calls = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)

    def fresh():
        chk(lib.dapol_prove_batches(ctx.h, tree.h, nb, P(off), P(flat), policy, agg, NBITS, P(sd), P(ref_C), P(ref_H), P(ref_R), None))

    def reprove():
        chk(lib.dapol_reprove_batches(ctx.h, tree.h, nb, P(off), P(flat), policy, agg, NBITS, P(sd), None, P(old_C), P(old_R), P(new_C), P(new_H), P(new_R),
                                      ctypes.byref(proved), ctypes.byref(kept), ctypes.byref(calls)))

    timed(fresh)                                              # the old proofs of the first edit
    for e in edits:
        old_C[:], old_R[:] = ref_C, ref_R                     # what the last state's call returned is what the caller holds now
        at = np.sort(rng.choice(N, size=e, replace=False))
        nv, nr = rng.integers(0, 2**32, size=e, dtype=np.uint64), rng.integers(0, 256, size=(e, 32), dtype=np.uint8)
        nr[:, 31] &= 0x0F
        tree.update(idx[at], nv, nr)
        for _ in range(2):
            timed(fresh), timed(reprove)
        tf, tn, equal = [], [], True
        for _ in range(a.runs):                               # alternating: drift of the machine hits both alike
            tf.append(timed(fresh))
            tn.append(timed(reprove))
            equal = equal and new_C.tobytes() == ref_C.tobytes() and new_H.tobytes() == ref_H.tobytes() and new_R.tobytes() == ref_R.tobytes()
        _, plan_total, sum_m, sum_m_all = capi.reprove_batches_plan(H, list(batches), idx[at], policy, agg, NBITS)
        F, Nw = stats(tf), stats(tn)
        ahead = F["median_s"] - Nw["median_s"] > F["max_s"] - F["min_s"]
        half = 2 * sum_m <= sum_m_all
        if worst:
            verdict = "worst case: %+.1f %% of dapol_prove_batches (its spread %.1f %%)" % (100.0 * (Nw["median_s"] / F["median_s"] - 1), 100.0 * F["spread"])
        else:
            verdict = "AHEAD" if ahead else ("MISS" if half else "not ahead; the plan keeps less than half of the sum of m")
        row = {"shape": shape, "k": k, "batches": nb, "edited": e, "leaves": N, "height": H, "n_bits": NBITS, "s_groups": ng,
               "siblings_min_max": [int(ns.min()), int(ns.max())], "sibling_records": T, "range_bytes": R, "reprove": Nw, "prove_batches": F,
               "time_ratio_prove_batches_over_reprove": F["median_s"] / Nw["median_s"], "sum_m_ratio_all_over_proved": sum_m_all / max(sum_m, 1),
               "sum_m_proved": sum_m, "sum_m_all": sum_m_all, "proved": int(proved.value), "kept": int(kept.value), "range_prover_calls": int(calls.value),
               "planner_total": plan_total, "bytes_equal_on_every_run": bool(equal), "verdict": verdict}
        assert equal and proved.value == plan_total, row
        rows.append(row)
        print("[bench_reprove_batches] %s k=%d e=%d: prove_batches %.3f s, re-prove %.3f s, x%.2f (sum m x%.2f), %d of %d sub-proofs in %d calls: %s"
              % (shape, k, e, F["median_s"], Nw["median_s"], row["time_ratio_prove_batches_over_reprove"], row["sum_m_ratio_all_over_proved"],
                 proved.value, proved.value + kept.value, calls.value, verdict), file=sys.stderr, flush=True)


rows = []
ks = [int(x) for x in a.k.split(",")]
edits = [int(x) for x in a.edits.split(",")]
batches_of = {k: pick_batches(k) for k in ks}
ctx = capi.Context(0, 32)
tree = capi.Tree(ctx, H, idx, v, r, seed)
for name in a.shapes.split(","):
    pol_name, agg = name.split("/")
    for k in ks:
        run_rows(ctx, tree, k, batches_of[k], name, capi.POLICY_PADDING if pol_name == "padding" else capi.POLICY_SPLITTING, int(agg), edits, rows)
tree.close()
ctx.close()
if not a.no_worst and 2 in batches_of:
    min_S = int(capi.batches_plan(H, list(batches_of[2]), capi.POLICY_PADDING, 0, NBITS)[0].min())
    parties = 1 << max(min_S - 1, 0).bit_length()
    ctx = capi.Context(0, parties)
    tree = capi.Tree(ctx, H, idx, v, r, seed)
    run_rows(ctx, tree, 2, batches_of[2], "padding/%d" % min_S, capi.POLICY_PADDING, min_S, [64], rows, worst=True)
    tree.close()
    ctx.close()
doc = {"config": "2^16 leaves at stride 2^%d, height %d, %d-bit proofs, context of 32 parties (the worst-case rows: as many as the factor needs); %d batches of "
                 "k random leaves (numpy default_rng(1)); e liabilities replaced by dapol_tree_update; host clock around each call with a device synchronise "
                 "(old siblings and blobs in, siblings and blobs back); 2 warm-ups + %d alternating runs each; outputs compared byte for byte on every run"
                 % (H - 16, H, NBITS, nb, a.runs),
       "rows": rows}
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
