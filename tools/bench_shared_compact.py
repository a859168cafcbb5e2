#!/usr/bin/env python3
"""The compact form of shared proofs against the routes it replaces, with the method of tools/bench_shared.py: the same random strictly
increasing leaves, one context, seed nonces, 64-bit proofs, all calls in the same process -- per shape one warm-up of each route, then
`--runs` alternating timed runs (host clock around the whole call, which ends with a blocking copy back), median, spread = (max - min) /
median of the parent route's runs.  The acceptance rule where dapol_shared_plan reports sharing: the new median lies below the parent
route's median by more than the parent route's own spread; otherwise the row is a MISS.
  prove   dapol_prove_entities_shared_compact against dapol_prove_entities_shared (range output copied back in both, paths not requested);
  verify  dapol_verify_entities_compact against dapol_verify_entities fed the expansion (the parent route), dapol_verify_entities_shared
          as a third column with --third; "upload alone" = hipMemcpy of the host arrays of either form into one device buffer;
  store   refresh + read_compact against refresh + read of all rows, after an update of --edits leaves before every run.
Shapes: padding/16, splitting/24, padding/0 (sharing) and padding/min(32, height) (nothing shared: the overhead is reported).
The document is rewritten after every row, so a run that is cut short leaves what it measured.
Usage: python tools/bench_shared_compact.py [--log2-entities 18] [--height 30] [--runs 5] [--parts prove,verify,store] [--third] [--out FILE]"""
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
ap.add_argument("--parts", default="prove,verify,store")
ap.add_argument("--shapes", default=None, help="comma-separated subset, e.g. padding/16,padding/0")
ap.add_argument("--third", action="store_true")
ap.add_argument("--edits", type=int, default=1024)
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
parts = set(a.parts.split(","))
shapes = [("padding/16", capi.POLICY_PADDING, 16), ("splitting/24", capi.POLICY_SPLITTING, 24), ("padding/0", capi.POLICY_PADDING, 0),
          ("padding/%d" % min(32, H), capi.POLICY_PADDING, min(32, H))]
if a.shapes:
    shapes = [s for s in shapes if s[0] in a.shapes.split(",")]
doc = {"config": "2^%d random strictly increasing leaves (numpy default_rng(1)), height %d, 64-bit proofs, seed nonces, context of 32 parties; host clock "
                 "around each call (range output / verdicts copied back; pageable host arrays); 1 warm-up + %d alternating runs of each route; spread = "
                 "(max - min) / median of the parent route" % (a.log2_entities, H, a.runs),
       "rows": []}


def emit():
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return text


def timed(fn):
    t0 = time.perf_counter()
    rc = fn()
    dt = time.perf_counter() - t0
    assert rc == 0, (rc, lib.dapol_last_error())
    return dt


def stats(ts):
    med = statistics.median(ts)
    return {"median_s": med, "min_s": min(ts), "max_s": max(ts), "spread": (max(ts) - min(ts)) / med, "runs_s": ts}


def alternate(routes):
    """One warm-up of every route, then a.runs rounds that run them one after the other; {name: stats}."""
    for fn in routes.values():
        timed(fn)
    ts = {k: [] for k in routes}
    for _ in range(a.runs):
        for k, fn in routes.items():
            ts[k].append(timed(fn))
    return {k: stats(x) for k, x in ts.items()}


def verdict(parent, new, shares):
    gain = (parent["median_s"] - new["median_s"]) / parent["median_s"]
    out = {"time_ratio_parent_over_new": parent["median_s"] / new["median_s"], "gain_fraction": gain, "parent_spread": parent["spread"]}
    out["rule"] = ("PASS" if gain > parent["spread"] else "MISS") if shares else "overhead only (nothing shared)"
    return out


def upload_only(arrays):
    """Median wall time of hipMemcpy of the host arrays into one device buffer of their total size, back to back, nothing else."""
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
        return {"bytes": total, "median_s": statistics.median(ts[1:])}
    finally:
        hip.hipFree(dev)


def say(msg):
    print("[bench_shared_compact] " + msg, file=sys.stderr, flush=True)


for name, policy, agg in shapes:
    es = lib.dapol_entity_proof_size(H, policy, agg, 64)
    n_sub, tot, per = capi.shared_plan(H, idx, policy, agg)
    clen = capi.shared_compact_plan(H, idx, policy, agg, 64)[2]
    shares = tot < per
    row = {"shape": name, "entities": n, "height": H, "blob_bytes_total": n * es, "compact_bytes_total": clen, "bytes_ratio": n * es / clen,
           "shared_plan_total": tot, "per_entity_subproofs": per}
    doc["rows"].append(row)
    blobs, compact = np.zeros((n, es), np.uint8), np.zeros(clen, np.uint8)
    pC, pH = np.zeros((n, H, 32), np.uint8), np.zeros((n, H, 32), np.uint8)
    uniq, length = ctypes.c_uint64(0), ctypes.c_uint64(0)
    if "prove" in parts:
        routes = {"shared": lambda: lib.dapol_prove_entities_shared(ctx.h, tree.h, n, P(idx), policy, agg, 64, P(sd), 0, None, None, None, None, None, None,
                                                                    P(blobs), ctypes.byref(uniq)),
                  "compact": lambda: lib.dapol_prove_entities_shared_compact(ctx.h, tree.h, n, P(idx), policy, agg, 64, P(sd), 0, None, None, None, None, None,
                                                                             None, P(compact), clen, ctypes.byref(length), ctypes.byref(uniq))}
        st = alternate(routes)
        assert length.value == clen and uniq.value == tot
        assert capi.shared_expand(H, idx, policy, agg, 64, compact, 0, 64).tobytes() == blobs[:64].tobytes()
        row["prove"] = dict(st, **verdict(st["shared"], st["compact"], shares))
        say("%s prove: shared %.3f s, compact %.3f s, %s" % (name, st["shared"]["median_s"], st["compact"]["median_s"], row["prove"]["rule"]))
        emit()
    if "verify" in parts:
        # the inputs of all routes: paths and blobs of the shared call, the compact buffer of the same proofs
        assert lib.dapol_prove_entities_shared(ctx.h, tree.h, n, P(idx), policy, agg, 64, P(sd), 0, None, None, None, None, P(pC), P(pH), P(blobs), None) == 0
        compact = capi.shared_compress(H, idx, policy, agg, 64, blobs)
        flat = blobs.reshape(-1)
        ok_e, ok_c, ok_s = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        head = (ctx.h, H, n, P(idx), P(lC), P(lH))
        routes = {"per_entity": lambda: lib.dapol_verify_entities(*head, P(pC), P(pH), P(rC), P(rH), policy, agg, 64, P(flat), P(sd), P(ok_e)),
                  "compact": lambda: lib.dapol_verify_entities_compact(*head, n * H, P(pC), P(pH), P(rC), P(rH), policy, agg, 64, P(compact), clen, P(sd), P(ok_c),
                                                                       ctypes.byref(uniq))}
        if a.third:
            routes["shared"] = lambda: lib.dapol_verify_entities_shared(*head, n * H, P(pC), P(pH), P(rC), P(rH), policy, agg, 64, P(flat), flat.shape[0], P(sd),
                                                                        P(ok_s), None)
        st = alternate(routes)
        assert ok_e.all() and ok_c.all() and (ok_s.all() or not a.third)
        small = [idx, lC, lH, pC, pH]
        row["verify"] = dict(st, **verdict(st["per_entity"], st["compact"], shares))
        row["verify"]["unique_checked"] = int(uniq.value)
        row["verify"]["upload_alone"] = {"expanded": upload_only(small + [flat]), "compact": upload_only(small + [compact])}
        say("%s verify: per-entity %.3f s, compact %.3f s, %s" % (name, st["per_entity"]["median_s"], st["compact"]["median_s"], row["verify"]["rule"]))
        emit()
    if "store" in parts:
        store = capi.ProofStore(tree, policy, agg, 64, seed)
        try:
            store.refresh()
            sidx = np.zeros(n, np.uint64)
            k = min(a.edits, n)
            eidx = np.ascontiguousarray(idx[:: n // k][:k])
            flip = [0]

            def edit():
                flip[0] ^= 1
                tree.update(eidx, np.full(k, 1 + flip[0], np.uint64), np.ascontiguousarray(r[:k]))

            def refresh_read():
                edit()
                t0 = time.perf_counter()
                rc = lib.dapol_proof_store_refresh(store.h, 0, None, None, None, None)
                rc = rc or lib.dapol_proof_store_read(store.h, 0, n, P(sidx), P(pC), P(pH), P(blobs))
                refresh_read.t = time.perf_counter() - t0
                return rc

            def refresh_read_compact():
                edit()
                t0 = time.perf_counter()
                rc = lib.dapol_proof_store_refresh(store.h, 0, None, None, None, None)
                rc = rc or lib.dapol_proof_store_read(store.h, 0, n, P(sidx), P(pC), P(pH), None)
                rc = rc or lib.dapol_proof_store_read_compact(store.h, P(compact), clen, ctypes.byref(length))
                refresh_read_compact.t = time.perf_counter() - t0
                return rc

            ts = {"read": [], "read_compact": []}
            assert refresh_read() == 0 and refresh_read_compact() == 0                     # warm-up (the edits are not timed)
            for _ in range(a.runs):
                assert refresh_read() == 0
                ts["read"].append(refresh_read.t)
                assert refresh_read_compact() == 0
                ts["read_compact"].append(refresh_read_compact.t)
            st = {kk: stats(x) for kk, x in ts.items()}
            row["store"] = dict(st, edits=k, **verdict(st["read"], st["read_compact"], shares))
            say("%s store: refresh + read %.3f s, refresh + read_compact %.3f s, %s" % (name, st["read"]["median_s"], st["read_compact"]["median_s"],
                                                                                         row["store"]["rule"]))
        finally:
            store.close()
            tree.update(eidx, np.ascontiguousarray(v[:: n // k][:k]), np.ascontiguousarray(r[:: n // k][:k]))       # the tree as it was
        emit()
    del blobs, compact, pC, pH
print(emit())
