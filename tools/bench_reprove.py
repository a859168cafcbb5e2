#!/usr/bin/env python3
"""dapol_reprove_entities_shared against dapol_prove_entities_shared on the same edited tree, in the same process: what a caller who
holds yesterday's proofs runs after k liabilities were replaced (dapol_tree_update), against what it must run without the re-prove call.
The tree is bench_shared.py's (random strictly increasing leaves, numpy default_rng(1)), 64-bit proofs, seed nonces.  Per shape and k:
the old proofs are the previous state's (a shared call for the first k of a shape -- which is also the shared call's warm-up -- and
the previous k's output afterwards), k random leaves get new values and blindings, then one warm-up of the re-prove call and `--runs`
alternating timed runs of each call: the host clock around the whole call, old paths and blobs going in, paths and blobs coming back
for both.  Sample rows of the two outputs are compared byte for byte.  Beside each time ratio stands dapol_reprove_plan's sum-of-m
ratio, and the time of hipMemcpy of the old arrays alone (host to device): the part no re-proving scheme removes.
Acceptance per row is against the shared call measured here: the re-prove median must lie below the shared median by more than the
shared spread ((max - min) / median); a row that does not is written as a MISS.  padding / H keeps nothing: its row states the overhead.
Prints one JSON document.
Usage: python tools/bench_reprove.py [--log2-entities 20] [--height 32] [--runs 5] [--shapes padding/16,splitting/24,padding/0,padding/32]
                                     [--ks 1,64,4096] [--out FILE]"""
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
ap.add_argument("--log2-entities", type=int, default=20)
ap.add_argument("--height", type=int, default=32)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--shapes", default="padding/16,splitting/24,padding/0,padding/32")
ap.add_argument("--ks", default="1,64,4096")
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
sd = np.frombuffer(seed, np.uint8).copy()
hip = ctypes.CDLL("libamdhip64.so")
hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t], [ctypes.c_void_p, ctypes.c_void_p,
                                                                                                                         ctypes.c_size_t, ctypes.c_int], [ctypes.c_void_p]


def upload_alone(arrays):
    """seconds of hipMemcpy host -> device of the arrays, into memory allocated before the clock starts"""
    bufs = []
    for x in arrays:
        d = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(d), x.nbytes) == 0
        bufs.append(d)
    t0 = time.perf_counter()
    for x, d in zip(arrays, bufs):
        assert hip.hipMemcpy(d, P(x), x.nbytes, 1) == 0                # hipMemcpyHostToDevice
    dt = time.perf_counter() - t0
    for d in bufs:
        hip.hipFree(d)
    return dt


def timed(fn):
    t0 = time.perf_counter()
    rc = fn()
    dt = time.perf_counter() - t0
    assert rc == 0, (rc, lib.dapol_last_error())
    return dt


def stats(ts):
    med = statistics.median(ts)
    return {"median_s": med, "min_s": min(ts), "max_s": max(ts), "spread": (max(ts) - min(ts)) / med, "runs_s": ts}


rows = []
for name in a.shapes.split(","):
    pol_name, agg = name.split("/")
    policy, agg = (capi.POLICY_PADDING if pol_name == "padding" else capi.POLICY_SPLITTING), int(agg)
    es = lib.dapol_entity_proof_size(H, policy, agg, 64)
    assert es, name
    need = 2 * n * es + 3 * n * H * 32                       # two blob buffers and three path buffers in host memory
    avail = next((int(line.split()[1]) * 1024 for line in open("/proc/meminfo") if line.startswith("MemAvailable")), None)
    assert avail is None or need < 0.6 * avail, "%s needs %.1f GB of host memory, %.1f GB are available" % (name, need / 1e9, avail / 1e9)
    old_C, old_R = np.zeros((n, H, 32), np.uint8), np.zeros((n, es), np.uint8)
    out_C, out_H, out_R = np.zeros((n, H, 32), np.uint8), np.zeros((n, H, 32), np.uint8), np.zeros((n, es), np.uint8)
    uniq, proved, kept = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    shared = lambda: lib.dapol_prove_entities_shared(ctx.h, tree.h, n, P(idx), policy, agg, 64, P(sd), 0, None, None, None, None, P(out_C), P(out_H), P(out_R),
                                                     ctypes.byref(uniq))
    reprove = lambda: lib.dapol_reprove_entities_shared(ctx.h, tree.h, n, P(idx), policy, agg, 64, P(sd), None, P(old_C), P(old_R), P(out_C), P(out_H), P(out_R),
                                                        ctypes.byref(proved), ctypes.byref(kept))
    timed(shared)                                          # the old proofs of the first k; the shared call's warm-up
    sample = np.unique(np.concatenate([np.arange(min(512, n)), np.arange(max(n - 512, 0), n), rng.integers(0, n, size=512)]))
    for k in [int(x) for x in a.ks.split(",")]:
        old_C, out_C = out_C, old_C                        # what the last call returned is what the caller holds now
        old_R, out_R = out_R, old_R
        at = np.sort(rng.choice(n, size=k, replace=False))
        nv, nr = rng.integers(0, 2**32, size=k, dtype=np.uint64), rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
        nr[:, 31] &= 0x0F
        t_edit = timed(lambda: lib.dapol_tree_update(tree.h, k, P(idx[at]), P(nv), P(nr)))
        timed(reprove)                                     # warm-up
        tr, ts = [], []
        for _ in range(a.runs):                            # alternating: drift of the box hits both alike
            tr.append(timed(reprove))
            got = (out_C[sample].copy(), out_R[sample].copy())
            ts.append(timed(shared))
        equal = bool(got[0].tobytes() == out_C[sample].tobytes() and got[1].tobytes() == out_R[sample].tobytes())
        t_up = upload_alone([old_C, old_R])
        _, plan_total, sum_m, sum_m_shared = capi.reprove_plan(H, idx, idx[at], policy, agg)
        R, S = stats(tr), stats(ts)
        gain = (S["median_s"] - R["median_s"]) / S["median_s"]
        keeps = sum_m * 1000 < sum_m_shared * 999          # (padding / H keeps one pair per replaced leaf: nothing, for this purpose)
        row = {"shape": name, "k": k, "entities": n, "height": H, "blob_bytes": es, "tree_update_s": t_edit, "reprove": R, "shared": S,
               "time_ratio_shared_over_reprove": S["median_s"] / R["median_s"], "sum_m_ratio_shared_over_reprove": sum_m_shared / max(sum_m, 1),
               "sum_m_proved": sum_m, "sum_m_shared": sum_m_shared, "proved": int(proved.value), "kept": int(kept.value), "planner_total": plan_total,
               "shared_unique": int(uniq.value), "upload_old_arrays_alone_s": t_up, "sample_rows_equal": equal,
               "verdict": ("PASS" if gain > S["spread"] else "MISS") if keeps else "nothing kept: overhead %+.2f %% of the shared call (spread %.2f %%)"
                          % (-100.0 * gain, 100.0 * S["spread"])}
        assert equal and proved.value == plan_total, row
        rows.append(row)
        print("[bench_reprove] %s k=%d: shared %.3f s, re-prove %.3f s, x%.2f (sum m x%.2f), upload alone %.3f s: %s" %
              (name, k, S["median_s"], R["median_s"], row["time_ratio_shared_over_reprove"], row["sum_m_ratio_shared_over_reprove"], t_up, row["verdict"]),
              file=sys.stderr, flush=True)
    del old_C, old_R, out_C, out_H, out_R
doc = {"config": "2^%d random strictly increasing leaves (numpy default_rng(1)), height %d, 64-bit proofs, seed nonces, context of 32 parties; k liabilities "
                 "replaced by dapol_tree_update; host clock around each call (old paths and blobs in, paths and blobs back); 1 warm-up + %d alternating runs each"
                 % (a.log2_entities, H, a.runs), "rows": rows}
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
