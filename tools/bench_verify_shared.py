#!/usr/bin/env python3
"""dapol_verify_entities_shared against dapol_verify_entities on the blobs and paths of dapol_prove_entities_shared: the leaves,
context and 64-bit proofs of tools/bench_shared.py, both calls in the same process -- per shape one warm-up of each, then `--runs`
alternating timed runs of each (host clock around the whole call: upload of the nine host arrays, Merkle re-merge, range checks,
verdicts back).  Shapes: padding/16 and splitting/24 (sharing), padding/min(32, height) (nothing to share: the overhead of compare +
scan + gather).  Per shape it also times the bare copy of the same host arrays into one device buffer of the same size (hipMemcpy,
nothing else): the part of a call that no verification scheme can remove.  Asserts that the two verdict vectors are equal and all
ones, that dapol_diag_verify_fallbacks did not move and that `unique` is dapol_shared_plan's total.  Prints one JSON document.
Usage: python tools/bench_verify_shared.py [--log2-entities 18] [--height 30] [--runs 5] [--out FILE]"""
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
ap.add_argument("--log2-entities", type=int, default=18)
ap.add_argument("--height", type=int, default=30)          # the headline density: N = 2^(H - 12)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert a.runs >= 5, "a median of at least 5 runs"
n, H, seed = 1 << a.log2_entities, a.height, bytes(range(32))
rng = np.random.default_rng(1)
cand = np.unique(rng.integers(0, 1 << H, size=n + n // 4, dtype=np.uint64))
idx = np.sort(rng.choice(cand, size=n, replace=False)).astype(np.uint64)
v = rng.integers(0, 2**32, size=n, dtype=np.uint64)
r = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
r[:, 31] &= 0x0F
ctx = capi.Context(0, 32)
tree = capi.Tree(ctx, H, idx, v, r, seed)
lib, P = capi.lib(), (lambda x: x.ctypes.data_as(ctypes.c_void_p))
hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
sd = np.frombuffer(seed, np.uint8).copy()
lC, lH = ctx.commit_hash_batch(v, r)
root = tree.root()
rC, rH = np.frombuffer(root[0], np.uint8).copy(), np.frombuffer(root[1], np.uint8).copy()


def plan_m(policy, agg):
    """parties of every sub-proof of the plan, in blob order (policy_plan.inc)"""
    np2 = lambda x: 1 if x <= 1 else 1 << (x - 1).bit_length()
    if policy == capi.POLICY_PADDING:
        ms = [np2(agg)]
    else:
        ms, base, pos = [], np2(agg), 0
        while pos < agg:
            if agg & base:
                ms.append(base)
                pos += base
            base >>= 1
    return ms + [1] * (H - agg)


def timed(fn):
    t0 = time.perf_counter()
    rc = fn()
    dt = time.perf_counter() - t0
    assert rc == 0, (rc, lib.dapol_last_error())
    return dt


def stats(ts):
    med = statistics.median(ts)
    return {"median_s": med, "min_s": min(ts), "max_s": max(ts), "spread": (max(ts) - min(ts)) / med, "runs_s": ts}


def fallbacks():
    c = ctypes.c_uint64()
    assert lib.dapol_diag_verify_fallbacks(ctypes.byref(c)) == 0
    return c.value


def upload_only(arrays):
    """Wall time of hipMemcpy of the host arrays into one device buffer of their total size, back to back, nothing else."""
    total = sum(x.nbytes for x in arrays)
    dev = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dev), ctypes.c_size_t(total)) == 0
    try:
        ts = []
        for _ in range(a.runs + 1):
            t0, off = time.perf_counter(), 0
            for x in arrays:
                assert hip.hipMemcpy(ctypes.c_void_p(dev.value + off), P(x), ctypes.c_size_t(x.nbytes), 1) == 0      # hipMemcpyHostToDevice
                off += x.nbytes
            assert hip.hipDeviceSynchronize() == 0
            ts.append(time.perf_counter() - t0)
        return stats(ts[1:])                                # (the first pass faults the pages in)
    finally:
        hip.hipFree(dev)


shapes = [("padding/16", capi.POLICY_PADDING, 16), ("splitting/24", capi.POLICY_SPLITTING, 24), ("padding/%d" % min(32, H), capi.POLICY_PADDING, min(32, H))]
rows = []
for name, policy, agg in shapes:
    es = lib.dapol_entity_proof_size(H, policy, agg, 64)
    pC, pH, blobs, proved = tree.prove_entities_shared(idx, policy, agg, 64, seed)
    ok_e, ok_s = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    uniq = ctypes.c_uint64(0)
    per_entity = lambda: lib.dapol_verify_entities(ctx.h, H, n, P(idx), P(lC), P(lH), P(pC), P(pH), P(rC), P(rH), policy, agg, 64, P(blobs), P(sd), P(ok_e))
    shared = lambda: lib.dapol_verify_entities_shared(ctx.h, H, n, P(idx), P(lC), P(lH), n * H, P(pC), P(pH), P(rC), P(rH), policy, agg, 64, P(blobs),
                                                      blobs.nbytes, P(sd), P(ok_s), ctypes.byref(uniq))
    fb = fallbacks()
    timed(per_entity), timed(shared)                       # warm-up of both (code objects, scratch)
    te, ts = [], []
    for _ in range(a.runs):                                # alternating: drift of the box hits both alike
        te.append(timed(per_entity))
        ts.append(timed(shared))
    assert ok_e.all() and ok_s.all() and ok_e.tobytes() == ok_s.tobytes()
    assert fallbacks() == fb
    n_sub, tot, per = capi.shared_plan(H, idx, policy, agg)
    assert uniq.value == tot == proved
    ms = plan_m(policy, agg)
    work_shared = int(sum(int(u) * m for u, m in zip(n_sub, ms)))
    work_entity = n * sum(ms)
    arrays = [idx, lC, lH, pC, pH, blobs]
    up = upload_only(arrays)
    E, S = stats(te), stats(ts)
    row = {"shape": name, "entities": n, "height": H, "blob_bytes": es, "bytes_uploaded": int(sum(x.nbytes for x in arrays)) + 96,
           "per_entity": E, "shared": S, "upload_only": up,
           "unique_subproofs": int(uniq.value), "per_entity_subproofs": per,
           "distinct_over_total_subproofs": uniq.value / per,
           "sum_m_shared_over_per_entity": work_shared / work_entity,
           "time_shared_over_per_entity": S["median_s"] / E["median_s"],
           "time_ratio_per_entity_over_shared": E["median_s"] / S["median_s"],
           "upload_share_of_per_entity": up["median_s"] / E["median_s"],
           "upload_share_of_shared": up["median_s"] / S["median_s"],
           "shared_faster_by_more_than_baseline_spread": (E["median_s"] - S["median_s"]) / E["median_s"] > E["spread"],
           "overhead_pct_of_per_entity": 100.0 * (S["median_s"] - E["median_s"]) / E["median_s"],
           "overhead_inside_per_entity_spread": abs(S["median_s"] - E["median_s"]) / E["median_s"] <= E["spread"]}
    rows.append(row)
    print("[bench_verify_shared] %s: per-entity %.3f s (spread %.1f %%), shared %.3f s, x%.2f; distinct %.3f of the sub-proofs, sum m %.3f; upload alone %.3f s"
          % (name, E["median_s"], 100 * E["spread"], S["median_s"], row["time_ratio_per_entity_over_shared"], row["distinct_over_total_subproofs"],
             row["sum_m_shared_over_per_entity"], up["median_s"]), file=sys.stderr, flush=True)
    del pC, pH, blobs
doc = {"config": "2^%d random strictly increasing leaves (numpy default_rng(1)), height %d, 64-bit proofs, context of 32 parties, blobs and paths of "
                 "dapol_prove_entities_shared; host clock around each call (pageable host arrays in, verdicts out); 1 warm-up + %d alternating runs each; "
                 "upload_only: hipMemcpy of the same arrays into one device buffer, %d passes after one untimed" % (a.log2_entities, H, a.runs, a.runs),
       "rows": rows}
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
