#!/usr/bin/env python3
"""dapol_prove_batches / dapol_verify_batches against the parent route -- a loop of dapol_prove_batch / dapol_verify_batch_checked over
the same batches -- in one process.  Tree: 2^16 leaves at stride 2^(height - 16) of a tree of the given height (default 32).  Shapes:
256 / 4,096 / 32,768 batches of k = 2 and of k = 4 random leaves, padding at aggregation 16, 64-bit proofs.  Protocol: host clock around
the whole route (host arrays in, host arrays out) with a device synchronise; two warm-ups; median of 7; spread = (max - min) / median.
The parent loop is timed on the first `--parent-batches` (default 256, never fewer) batches of a shape and scaled by nb / that number;
the row says so.  The proofs of those batches are compared byte for byte with the new call's, and every verdict must be 1.
AHEAD: the new median lies below the parent's (scaled) median by more than the parent's own (scaled) max - min; otherwise MISS.
Prints one JSON document.  Usage: python tools/bench_batches.py [--height 32] [--batches 256,4096,32768] [--k 2,4] [--out FILE]"""
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
ap.add_argument("--batches", default="256,4096,32768")
ap.add_argument("--k", default="2,4")
ap.add_argument("--parent-batches", type=int, default=256)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert a.runs >= 7 and a.parent_batches >= 256
H, N, AGG, NBITS, POLICY, seed = a.height, 1 << 16, 16, 64, capi.POLICY_PADDING, bytes(range(32))
rng = np.random.default_rng(1)
idx = (np.arange(N, dtype=np.uint64) << np.uint64(H - 16)).astype(np.uint64)
v = rng.integers(0, 2**32, size=N, dtype=np.uint64)
r = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
r[:, 31] &= 0x0F
ctx = capi.Context(0, 32)
tree = capi.Tree(ctx, H, idx, v, r, seed)
lib, P = capi.lib(), (lambda x: x.ctypes.data_as(ctypes.c_void_p))
hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
sd = np.frombuffer(seed, np.uint8).copy()
lC_all, lH_all = ctx.commit_hash_batch(v, r)
root = tree.root()
rC, rH = np.frombuffer(root[0], np.uint8).copy(), np.frombuffer(root[1], np.uint8).copy()
at = lambda arr, off: ctypes.c_void_p(arr.ctypes.data + int(off))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    assert hip.hipDeviceSynchronize() == 0
    return time.perf_counter() - t0


def stats(ts, scale=1.0):
    ts = [t * scale for t in ts]
    med = statistics.median(ts)
    return {"median_s": med, "min_s": min(ts), "max_s": max(ts), "spread": (max(ts) - min(ts)) / med, "runs_s": ts}


def measure(new, parent, scale):
    for _ in range(2):
        timed(parent), timed(new)
    tp, tn = [], []
    for _ in range(a.runs):                                # alternating: drift of the machine hits both alike
        tp.append(timed(parent))
        tn.append(timed(new))
    Pn, Nw = stats(tp, scale), stats(tn)
    ahead = Pn["median_s"] - Nw["median_s"] > Pn["max_s"] - Pn["min_s"]
    return {"new": Nw, "parent": Pn, "parent_over_new": Pn["median_s"] / Nw["median_s"], "verdict": "AHEAD" if ahead else "MISS"}


def chk(rc):
    assert rc == 0, (rc, lib.dapol_last_error())


rows = []
for nb in [int(x) for x in a.batches.split(",")]:
    for k in [int(x) for x in a.k.split(",")]:
        pick = np.sort(rng.integers(0, N, size=(nb, k)), axis=1)
        while True:                                           # k DISTINCT leaves per batch: redraw the rows that repeat one
            dup = (np.diff(pick, axis=1) == 0).any(axis=1)
            if not dup.any():
                break
            pick[dup] = np.sort(rng.integers(0, N, size=(int(dup.sum()), k)), axis=1)
        batches = idx[pick]                                   # [nb][k], rows strictly increasing
        _, off, flat = capi._pack_batches(list(batches))
        ns, so, ro, ng = capi.batches_plan(H, list(batches), POLICY, AGG, NBITS)
        T, R, sub = int(so[-1]), int(ro[-1]), min(nb, a.parent_batches)
        lC, lH = lC_all[pick.reshape(-1)].copy(), lH_all[pick.reshape(-1)].copy()
        sC, sH, blob = np.zeros((T, 32), np.uint8), np.zeros((T, 32), np.uint8), np.zeros(R, np.uint8)
        pC, pH, pblob = np.zeros((T, 32), np.uint8), np.zeros((T, 32), np.uint8), np.zeros(R, np.uint8)
        ok, pok = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8)
        groups = ctypes.c_uint64(0)

        def prove_new():
            chk(lib.dapol_prove_batches(ctx.h, tree.h, nb, P(off), P(flat), POLICY, AGG, NBITS, P(sd), P(sC), P(sH), P(blob), ctypes.byref(groups)))

        def prove_parent():
            for j in range(sub):
                chk(lib.dapol_prove_batch(ctx.h, tree.h, k, at(flat, 8 * int(off[j])), POLICY, AGG, NBITS, P(sd), at(pC, 32 * int(so[j])), at(pH, 32 * int(so[j])),
                                          at(pblob, int(ro[j]))))

        def verify_new():
            chk(lib.dapol_verify_batches(ctx.h, H, nb, P(off), P(flat), P(lC), P(lH), P(so), P(sC), P(sH), P(rC), P(rH), POLICY, AGG, NBITS, P(ro), P(blob), P(sd),
                                         P(ok)))

        def verify_parent():
            for j in range(sub):
                chk(lib.dapol_verify_batch_checked(ctx.h, H, k, at(flat, 8 * int(off[j])), at(lC, 32 * int(off[j])), at(lH, 32 * int(off[j])), int(ns[j]),
                                                   at(sC, 32 * int(so[j])), at(sH, 32 * int(so[j])), P(rC), P(rH), POLICY, AGG, NBITS, at(blob, int(ro[j])),
                                                   int(ro[j + 1] - ro[j]), P(sd), at(pok, j)))

        prove = measure(prove_new, prove_parent, nb / sub)
        s_end, r_end = int(so[sub]), int(ro[sub])
        assert groups.value == ng
        assert sC[:s_end].tobytes() == pC[:s_end].tobytes() and sH[:s_end].tobytes() == pH[:s_end].tobytes() and blob[:r_end].tobytes() == pblob[:r_end].tobytes()
        verify = measure(verify_new, verify_parent, nb / sub)
        assert ok.all() and pok[:sub].all()
        row = {"batches": nb, "k": k, "leaves": N, "height": H, "policy": "padding", "aggregation_factor": AGG, "n_bits": NBITS, "s_groups": ng,
               "siblings_min_max": [int(ns.min()), int(ns.max())], "sibling_records": T, "range_bytes": R,
               "parent_timed_on_batches": sub, "parent_scaled_by": nb / sub, "prove": prove, "verify": verify,
               "prove_ms_per_s_group": 1e3 * prove["new"]["median_s"] / ng, "verify_ms_per_s_group": 1e3 * verify["new"]["median_s"] / ng,
               "rows_compared_byte_for_byte": sub}
        rows.append(row)
        print("[bench_batches] nb=%d k=%d: %d S-groups; prove %.3f s vs parent %.3f s (x%.1f, %s); verify %.3f s vs %.3f s (x%.1f, %s)"
              % (nb, k, ng, prove["new"]["median_s"], prove["parent"]["median_s"], prove["parent_over_new"], prove["verdict"], verify["new"]["median_s"],
                 verify["parent"]["median_s"], verify["parent_over_new"], verify["verdict"]), file=sys.stderr, flush=True)
doc = {"config": "2^16 leaves at stride 2^%d, height %d, padding at aggregation %d, %d-bit proofs, context of 32 parties; k random leaves per batch "
                 "(numpy default_rng(1)); host clock around each route with a device synchronise; 2 warm-ups + %d alternating runs each; the parent loop "
                 "(dapol_prove_batch / dapol_verify_batch_checked per batch) is timed on the first min(nb, %d) batches and scaled by nb over that number"
                 % (H - 16, H, AGG, NBITS, a.runs, a.parent_batches),
       "rows": rows}
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
