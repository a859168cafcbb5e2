"""dapol_tree_insert_liabilities on the headline tree: python tools/bench_insert_liabilities.py [log2_entities=20] [repeats=7]
2^20 ids `id-%08d` at height 32 under BLAKE3 (the set-up of tests/test_gpu_parity.py::test_leaf_derivation_at_2e20) are the tree; k = 1 /
64 / 4,096 / 65,536 further ids join it, two ways, each on a tree of its own that keeps growing from call to call:
  new     dapol_tree_insert_liabilities (packed ids, as the other route's derivation takes them);
  parent  what a caller had before it: dapol_build_leaf_nodes over ALL ids, old and new, the new rows picked out of its output,
          Tree.insert of those rows.
Timed with a host clock around the whole route and a device synchronise: two warm-up calls (reported, not counted), then `repeats`
timed ones.  Every call checks that both routes gave the same indexes and the same root.  Prints one JSON line per (k, route) with the
median and spread = (max - min) / median, and one line per k with the verdict: the new median lies below the parent's by more than the
parent's spread (max - min, in ms)."""
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dapol_amd import capi  # noqa: E402
import bench  # noqa: E402

lg = int(sys.argv[1]) if len(sys.argv) > 1 else 20
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
KS = (1, 64, 4096, 65536)
n, height, seed = 1 << lg, 32, b"bench-audit-seed"
total = n + (2 + reps) * max(KS)
ids = np.char.add("id-", np.char.zfill(np.arange(total).astype("U8"), 8)).astype("S11")
vals = np.random.default_rng(4).integers(0, 1 << 32, size=total, dtype=np.uint64)
sd = np.frombuffer(seed, np.uint8)
hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
ctx = capi.Context(0, 1)
L = capi.lib()
P = capi._ptr


def packed(a, b):
    """ids a .. b - 1 as the C ABI takes them (internal id = external id, as in the headline leaf test)."""
    return np.frombuffer(ids[a:b].tobytes(), np.uint8), (np.arange(b - a + 1, dtype=np.uint64) * 11).astype(np.uint32)


def sync():
    assert hip.hipDeviceSynchronize() == 0


def route_new(tr, a, b):
    ib, off = packed(a, b)
    v = np.ascontiguousarray(vals[a:b])
    by_e = np.zeros(b - a, np.uint64)
    sync()
    t0 = time.perf_counter()
    capi._chk(L.dapol_tree_insert_liabilities(tr.h, capi.DIGEST_BLAKE3, P(sd), len(seed), b - a, P(ib), P(off), P(ib), P(off), P(v), P(by_e)))
    sync()
    return (time.perf_counter() - t0) * 1e3, by_e


def route_parent(tr, a, b):
    """The tree holds ids 0 .. a - 1 (the 2^20, then what earlier calls added); ids a .. b - 1 join."""
    ib, off = packed(0, b)
    v = np.ascontiguousarray(vals[:b])
    sync()
    t0 = time.perf_counter()
    out = ctx.build_leaf_nodes_packed(ib, off, ib, off, v, seed, height)
    by_e = out["idx_by_entity"][a:]
    pos = np.searchsorted(out["leaf_idx"], by_e)
    tr.insert(by_e, out["v"][pos], out["r"][pos])
    sync()
    return (time.perf_counter() - t0) * 1e3, by_e


ib, off = packed(0, n)
base = ctx.build_leaf_nodes_packed(ib, off, ib, off, vals[:n], seed, height)
rows = {}
for k in KS:
    trees = {way: capi.Tree(ctx, height, base["leaf_idx"], base["v"], base["r"], bench.PAD_SEED) for way in ("new", "parent")}
    runs = {"new": [], "parent": []}
    a = n                                                          # every k starts from the 2^20 tree; its calls add ids n, n + 1, ...
    for _ in range(2 + reps):
        b = a + k
        t_new, idx_new = route_new(trees["new"], a, b)
        t_par, idx_par = route_parent(trees["parent"], a, b)
        assert np.array_equal(idx_new, idx_par), "the two routes disagree on the indexes"
        assert trees["new"].root() == trees["parent"].root(), "the two routes disagree on the root"
        runs["new"].append((t_new, trees["new"].last_update_path()))
        runs["parent"].append((t_par, trees["parent"].last_update_path()))
        a = b
    for way in ("new", "parent"):
        trees[way].close()
        cold, hot = runs[way][:2], runs[way][2:]
        ms = sorted(t for t, _ in hot)
        med = float(np.median(ms))
        rows[(k, way)] = dict(median_ms=med, min_ms=ms[0], max_ms=ms[-1])
        print(json.dumps({"leaves": n, "height": height, "k": k, "route": way, "last_update_path": sorted({p for _, p in hot}),
                          "median_ms": round(med, 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3), "spread": round((ms[-1] - ms[0]) / med, 3),
                          "ms": [round(t, 3) for t, _ in hot], "warmup_ms": [round(c, 3) for c, _ in cold], "repeats": reps, "same_indexes_and_root": True}), flush=True)
    new, par = rows[(k, "new")], rows[(k, "parent")]
    print(json.dumps({"leaves": n, "height": height, "k": k, "verdict": "new median below the parent's by more than the parent's max - min",
                      "holds": bool(par["median_ms"] - new["median_ms"] > par["max_ms"] - par["min_ms"]),
                      "parent_minus_new_ms": round(par["median_ms"] - new["median_ms"], 3), "parent_max_minus_min_ms": round(par["max_ms"] - par["min_ms"], 3)}),
          flush=True)
