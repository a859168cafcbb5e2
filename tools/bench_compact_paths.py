#!/usr/bin/env python3
"""Compact Merkle paths against the routes they replace, with the method of tools/bench_shared_compact.py: one context, seed nonces,
64-bit proofs, all calls in the same process -- per row one warm-up of each route, then `--runs` alternating timed runs (host clock
around the whole call, which ends with a blocking copy back, then a device synchronise), median, spread = (max - min) / median.  The
rule: AHEAD when the new median lies below the baseline's by more than the baseline's own max - min; anything else is a MISS.
  verify  dapol_verify_entities_compact_paths against dapol_verify_entities_compact fed the expanded paths (the baseline, which exists
          without this feature); upload bytes and "upload alone" (hipMemcpy of the host arrays of either form into one device buffer)
          for both forms; the path stage's own device time in both routes (dapol_diag_compact_paths: events around the path launches;
          the baseline's per-entity re-merge of the same call is timed by running the new entry point with DAPOL_CPATHS_FALLBACK=1,
          which expands on the device and launches the baseline's path kernel and nothing else for the paths);
  paths   dapol_tree_paths_compact against dapol_tree_paths (C and H requested), with the bytes returned.
Leaf sets: the random set of profiles/shared_compact_2e18_h30.json (numpy default_rng(1)) and 2^k consecutive leaves.
Policies: padding / H, padding / 16, padding / 0.  The document is rewritten after every row.
Usage: python tools/bench_compact_paths.py [--log2-entities 18] [--height 30] [--runs 5] [--sets random,consecutive] [--shapes ...] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

os.environ.setdefault("DAPOL_ENV_KNOBS", "1")              # (DAPOL_CPATHS_FALLBACK is a measurement knob)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dapol_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-entities", type=int, default=18)
ap.add_argument("--height", type=int, default=30)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--sets", default="random,consecutive")
ap.add_argument("--shapes", default=None, help="comma-separated subset, e.g. padding/30,padding/0")
ap.add_argument("--parts", default="verify,paths")
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert a.runs >= 5, "a median of at least 5 runs"
n, H, seed = 1 << a.log2_entities, a.height, bytes(range(32))
lib, P = capi.lib(), (lambda x: x.ctypes.data_as(ctypes.c_void_p))
hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
sd = np.frombuffer(seed, np.uint8).copy()
ctx = capi.Context(0, 32)
shapes = [("padding/%d" % min(32, H), capi.POLICY_PADDING, min(32, H)), ("padding/16", capi.POLICY_PADDING, 16), ("padding/0", capi.POLICY_PADDING, 0)]
if a.shapes:
    shapes = [s for s in shapes if s[0] in a.shapes.split(",")]
parts = set(a.parts.split(","))
doc = {"config": "2^%d strictly increasing leaves, height %d, 64-bit proofs, seed nonces, context of 32 parties; host clock around each call plus a device "
                 "synchronise (pageable host arrays); 1 warm-up + %d alternating runs of each route; spread = (max - min) / median; AHEAD = the new median "
                 "lies below the baseline's by more than the baseline's max - min" % (a.log2_entities, H, a.runs),
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
    assert hip.hipDeviceSynchronize() == 0
    dt = time.perf_counter() - t0
    assert rc == 0, (rc, lib.dapol_last_error())
    return dt


def stats(ts):
    med = statistics.median(ts)
    return {"median_s": med, "min_s": min(ts), "max_s": max(ts), "spread": (max(ts) - min(ts)) / med, "runs_s": ts}


def alternate(routes, after=None):
    """One warm-up of every route, then a.runs rounds that run them one after the other; {name: stats}.  after[name]() is called after
    every timed run of that route and its results are kept."""
    for fn in routes.values():
        timed(fn)
    ts, extra = {k: [] for k in routes}, {k: [] for k in routes}
    for _ in range(a.runs):
        for k, fn in routes.items():
            ts[k].append(timed(fn))
            if after and k in after:
                extra[k].append(after[k]())
    return {k: stats(x) for k, x in ts.items()}, extra


def verdict(base, new):
    out = {"time_ratio_baseline_over_new": base["median_s"] / new["median_s"], "baseline_max_minus_min_s": base["max_s"] - base["min_s"]}
    out["rule"] = "AHEAD" if base["median_s"] - new["median_s"] > base["max_s"] - base["min_s"] else "MISS"
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
    print("[bench_compact_paths] " + msg, file=sys.stderr, flush=True)


def leaf_set(name):
    if name == "random":                                     # the set of profiles/shared_compact_2e18_h30.json
        rng = np.random.default_rng(1)
        cand = np.unique(rng.integers(0, 1 << H, size=n + n // 4, dtype=np.uint64))
        return np.sort(rng.choice(cand, size=n, replace=False)).astype(np.uint64)
    assert name == "consecutive"
    return np.arange(n, dtype=np.uint64) + np.uint64((1 << (H - 1)) - n // 2 if H < 64 else 0)       # a dense book across the middle of the tree


for set_name in a.sets.split(","):
    idx = leaf_set(set_name)
    rng = np.random.default_rng(2)
    v = rng.integers(0, 2**32, size=n, dtype=np.uint64)
    r = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    r[:, 31] &= 0x0F
    tree = capi.Tree(ctx, H, idx, v, r, seed)
    lC, lH = ctx.commit_hash_batch(v, r)
    root = tree.root()
    rC, rH = np.frombuffer(root[0], np.uint8).copy(), np.frombuffer(root[1], np.uint8).copy()
    n_rec = capi.compact_paths_plan(H, idx, want_ref=False)[2]
    pC, pH = np.zeros((n, H, 32), np.uint8), np.zeros((n, H, 32), np.uint8)
    cC, cH = np.zeros((n_rec, 32), np.uint8), np.zeros((n_rec, 32), np.uint8)
    cnt = ctypes.c_uint64(0)
    if "paths" in parts:
        routes = {"per_entity": lambda: lib.dapol_tree_paths(tree.h, n, P(idx), P(pC), P(pH), None, None),
                  "compact": lambda: lib.dapol_tree_paths_compact(tree.h, n, P(idx), P(cC), P(cH), n_rec, ctypes.byref(cnt))}
        st, _ = alternate(routes)
        eC, eH = capi.compact_paths_expand(H, idx, cC, cH, 0, 64)
        assert cnt.value == n_rec and eC.tobytes() == pC[:64].tobytes() and eH.tobytes() == pH[:64].tobytes()
        row = {"part": "paths", "leaf_set": set_name, "entities": n, "height": H, "per_entity_records": n * H, "distinct_records": n_rec,
               "record_ratio": n * H / n_rec, "bytes_returned": {"per_entity": n * H * 64, "compact": n_rec * 64}}
        row.update(st, **verdict(st["per_entity"], st["compact"]))
        doc["rows"].append(row)
        say("%s paths: per-entity %.4f s, compact %.4f s, %s" % (set_name, st["per_entity"]["median_s"], st["compact"]["median_s"], row["rule"]))
        emit()
    if "verify" not in parts:
        continue
    assert lib.dapol_tree_paths(tree.h, n, P(idx), P(pC), P(pH), None, None) == 0
    assert lib.dapol_tree_paths_compact(tree.h, n, P(idx), P(cC), P(cH), n_rec, ctypes.byref(cnt)) == 0
    for name, policy, agg in shapes:
        clen = capi.shared_compact_plan(H, idx, policy, agg, 64)[2]
        compact, length, uniq, merges = np.zeros(clen, np.uint8), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        assert lib.dapol_prove_entities_shared_compact(ctx.h, tree.h, n, P(idx), policy, agg, 64, P(sd), 0, None, None, None, None, None, None, P(compact), clen,
                                                       ctypes.byref(length), ctypes.byref(uniq)) == 0
        ok_b, ok_n = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        head = (ctx.h, H, n, P(idx), P(lC), P(lH))
        tail = (P(rC), P(rH), policy, agg, 64, P(compact), clen, P(sd))
        routes = {"baseline": lambda: lib.dapol_verify_entities_compact(*head, n * H, P(pC), P(pH), *tail, P(ok_b), ctypes.byref(uniq)),
                  "compact_paths": lambda: lib.dapol_verify_entities_compact_paths(*head, n_rec, P(cC), P(cH), *tail, P(ok_n), ctypes.byref(uniq),
                                                                                   ctypes.byref(merges))}
        st, extra = alternate(routes, after={"compact_paths": capi.diag_compact_paths})
        assert ok_b.all() and ok_n.all() and merges.value == n_rec and all(route == 1 for _, route in extra["compact_paths"])
        row = {"part": "verify", "leaf_set": set_name, "shape": name, "entities": n, "height": H, "per_entity_records": n * H, "distinct_records": n_rec,
               "record_ratio": n * H / n_rec, "range_proofs_checked": int(uniq.value)}
        row.update(st, **verdict(st["baseline"], st["compact_paths"]))
        row["path_stage_device_ms"] = {"compact_paths": statistics.median(ms for ms, _ in extra["compact_paths"])}
        # the baseline's path stage: the per-entity re-merge of the same call, alone (it includes the device expansion, a copy kernel)
        os.environ["DAPOL_CPATHS_FALLBACK"] = "1"
        try:
            ms = []
            for _ in range(a.runs + 1):
                timed(routes["compact_paths"])
                got, route = capi.diag_compact_paths()
                assert route == 3 and ok_n.all() and merges.value == n * H
                ms.append(got)
            row["path_stage_device_ms"]["per_entity_remerge"] = statistics.median(ms[1:])
        finally:
            del os.environ["DAPOL_CPATHS_FALLBACK"]
        link = np.zeros(n_rec, np.uint32)                      # (the verifier uploads one index word per record beside them)
        row["upload_alone"] = {"expanded": upload_only([idx, lC, lH, pC, pH, compact]), "compact_paths": upload_only([lC, lH, cC, cH, link, compact])}
        doc["rows"].append(row)
        say("%s %s verify: baseline %.4f s, compact paths %.4f s, %s; path stage %.2f ms shared, %.2f ms per entity" % (
            set_name, name, st["baseline"]["median_s"], st["compact_paths"]["median_s"], row["rule"], row["path_stage_device_ms"]["compact_paths"],
            row["path_stage_device_ms"]["per_entity_remerge"]))
        emit()
        del compact
    del tree, pC, pH, cC, cH
print(emit())
