"""dapol_tree_insert on the headline tree: python tools/bench_tree_insert.py [log2_entities=20] [repeats=7]
For k = 1 / 64 / 1,024 / 4,096 / 16,384 / 65,536 uniformly random free indexes, and for one directed shape -- every free index of one
aligned block between two leaves of the strided layout, a whole new subtree (4,095 leaves at 2^20) -- three ways, each on a tree built
for it: Tree.insert (the path it took is reported), Tree.update of the same kind of batch (what a caller had before dapol_tree_insert;
that code is unchanged), and the forced rebuild (update_incremental_max = -1).  Timed with a host clock around the call and a device
synchronise: two warm-up calls (reported, not counted), then `repeats` timed ones, every call with new indexes into the same growing
tree, as an exchange that keeps its tree between rounds would.  Prints one JSON line per (shape, way) with the median and
spread = (max - min) / median."""
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
n, height = 1 << lg, 32
stride = (1 << height) // n
idx, v, r = bench.synth_inputs(n, height, 0, n)
hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
ctx = capi.Context(0, 1)


def random_free(rng, used, k):
    """k distinct indexes that are neither leaves of the strided layout nor in `used` (which they join)."""
    out = np.zeros(0, np.uint64)
    while len(out) < k:
        x = rng.integers(0, 1 << height, size=k - len(out) + 16, dtype=np.uint64)
        x = np.setdiff1d(np.unique(x[x % np.uint64(stride) != 0]), used)
        out = np.union1d(out, x)[:k] if len(out) else x[:k]
    return rng.permutation(out)


def block_free(rng, used, k):
    """Every free index of one aligned block of `stride` indexes (its first index is the block's leaf)."""
    while True:
        b = np.uint64(int(rng.integers(0, n)) * stride)
        if b not in used:
            return rng.permutation(np.arange(1, stride, dtype=np.uint64) + b), b


def timed(tr, call, new):
    nv = np.arange(len(new), dtype=np.uint64) + np.uint64(1)
    nr = np.zeros((len(new), 32), np.uint8)
    nr[:, :8] = new.view(np.uint8).reshape(-1, 8)
    assert hip.hipDeviceSynchronize() == 0
    t0 = time.perf_counter()
    getattr(tr, call)(new, nv, nr)
    assert hip.hipDeviceSynchronize() == 0
    return (time.perf_counter() - t0) * 1e3, tr.last_update_path()


shapes = [("random", k) for k in (1, 64, 1024, 4096, 16384, 65536)] + [("block", stride - 1)]
for shape, k in shapes:
    for way in ("insert", "update", "rebuild"):
        o = capi.Options()
        o.update_incremental_max = -1 if way == "rebuild" else 0
        ctx.set_options(o)
        tr = capi.Tree(ctx, height, idx, v, r, bench.PAD_SEED)
        rng = np.random.default_rng(11)                          # the three ways see the same batches
        used = np.zeros(0, np.uint64)
        runs = []
        for _ in range(2 + reps):                                # the first two calls allocate the scratch and both level buffers
            if shape == "random":
                new = random_free(rng, used, k)
                used = np.union1d(used, new)
            else:
                new, b = block_free(rng, used, k)
                used = np.union1d(used, [b])
            runs.append(timed(tr, "insert" if way != "update" else "update", new))
        tr.close()
        cold, runs = runs[:2], runs[2:]
        ms = sorted(t for t, _ in runs)
        med = float(np.median(ms))
        print(json.dumps({"leaves": n, "height": height, "shape": shape, "k": k, "way": way, "last_update_path": sorted({p for _, p in runs}),
                          "median_ms": round(med, 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3), "spread": round((ms[-1] - ms[0]) / med, 3),
                          "warmup_ms": [round(c, 3) for c, _ in cold], "repeats": reps}), flush=True)
