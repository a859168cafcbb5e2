#!/usr/bin/env python3
"""dapol_prove_entities_shared against dapol_prove_entities: the same random strictly increasing leaves, one context, the seed nonce
mode, 64-bit proofs, both calls in the same process -- per shape one warm-up of each, then `--runs` alternating timed runs of each
(host clock around the whole call: H2D of the indexes, gather, proving, D2H of the blobs; the path outputs are not requested).
Shapes: padding/16 and splitting/24 (sharing), padding/min(32, height) (no sharing: the overhead of heads + scan + scatter; the bytes
of the two calls are compared there).  Prints one JSON document.
Usage: python tools/bench_shared.py [--log2-entities 18] [--height 30] [--runs 5] [--out FILE]"""
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
sd = np.frombuffer(seed, np.uint8).copy()


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


shapes = [("padding/16", capi.POLICY_PADDING, 16), ("splitting/24", capi.POLICY_SPLITTING, 24), ("padding/%d" % min(32, H), capi.POLICY_PADDING, min(32, H))]
rows = []
for name, policy, agg in shapes:
    es = lib.dapol_entity_proof_size(H, policy, agg, 64)
    out_e, out_s = np.zeros((n, es), np.uint8), np.zeros((n, es), np.uint8)
    uniq = ctypes.c_uint64(0)
    per_entity = lambda: lib.dapol_prove_entities(ctx.h, tree.h, n, P(idx), policy, agg, 64, P(sd), None, None, P(out_e))
    shared = lambda: lib.dapol_prove_entities_shared(ctx.h, tree.h, n, P(idx), policy, agg, 64, P(sd), 0, None, None, None, None, None, None, P(out_s),
                                                     ctypes.byref(uniq))
    timed(per_entity), timed(shared)                       # warm-up of both (code objects, scratch, the lanes' first use)
    te, ts = [], []
    for _ in range(a.runs):                                # alternating: drift of the box hits both alike
        te.append(timed(per_entity))
        ts.append(timed(shared))
    n_sub, tot, per = capi.shared_plan(H, idx, policy, agg)
    ms = plan_m(policy, agg)
    work_shared = int(sum(int(u) * m for u, m in zip(n_sub, ms)))
    work_entity = n * sum(ms)
    E, S = stats(te), stats(ts)
    sC, sH, sblob, _ = tree.prove_entities_shared(idx[:256], policy, agg, 64, seed)      # (a statement's bytes do not depend on the call)
    assert sblob.tobytes() == out_s[:256].tobytes()
    lC, lH = ctx.commit_hash_batch(v[:256], r[:256])
    rC, rH = tree.root()[:2]
    ok = ctx.verify_entities(H, idx[:256], lC, lH, sC, sH, rC, rH, policy, agg, 64, sblob, verify_seed=seed)
    row = {"shape": name, "entities": n, "height": H, "blob_bytes": es, "per_entity": E, "shared": S,
           "time_ratio_per_entity_over_shared": E["median_s"] / S["median_s"],
           "sum_m_ratio_per_entity_over_shared": work_entity / work_shared,
           "unique_subproofs": int(uniq.value), "per_entity_subproofs": per, "shared_plan_total": tot,
           "shared_faster_by_more_than_baseline_spread": (E["median_s"] - S["median_s"]) / E["median_s"] > E["spread"],
           "overhead_pct_of_per_entity": 100.0 * (S["median_s"] - E["median_s"]) / E["median_s"],
           "bytes_equal_per_entity": bool(out_e.tobytes() == out_s.tobytes()) if work_entity == work_shared else None,
           "first_256_shared_verified": bool(ok.all())}
    assert uniq.value == tot
    rows.append(row)
    print("[bench_shared] %s: per-entity %.3f s, shared %.3f s, x%.2f (sum m x%.2f)" % (name, E["median_s"], S["median_s"],
          row["time_ratio_per_entity_over_shared"], row["sum_m_ratio_per_entity_over_shared"]), file=sys.stderr, flush=True)
    del out_e, out_s
doc = {"config": "2^%d random strictly increasing leaves (numpy default_rng(1)), height %d, 64-bit proofs, seed nonces, context of 32 parties; "
                 "host clock around each call (blobs copied back, paths not requested); 1 warm-up + %d alternating runs each" % (a.log2_entities, H, a.runs),
       "rows": rows}
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
