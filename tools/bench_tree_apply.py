"""dapol_tree_apply on the headline tree: python tools/bench_tree_apply.py [log2_entities=20] [repeats=7] [out.json]
Rows: r removals + r new leaves + r replacements at uniformly random positions for r = 1 / 64 / 1,024 / 4,096 / 16,384 and 21,845 (65,535
edits: the largest batch the in-place gate admits), and one directed
shape -- an aligned group of 64 leaves removed beside a dense block of 1,024 new leaves.  Every row is timed on three routes, on ONE
tree in one process, the routes alternating within every repetition:
  apply    Tree.apply of the whole change set (the path it took is reported)
  three    what a caller had before dapol_tree_apply: Tree.remove, then Tree.insert, then Tree.update
  rebuild  Tree.apply with update_incremental_max = -1 (the forced rebuild)
After every timed call the tree is put back by the inverse apply (not timed) and its root is checked against the original, so every
call of every route starts from the same tree.  Timed with a host clock around the call(s) and a device synchronise: two warm-up
repetitions (reported, not counted), then `repeats` timed ones.  Prints one JSON line per (row, route) with the median and
spread = (max - min) / median, then one verdict line per row by the rule of the insert tables: apply is AHEAD of a route when its
median lies below that route's median by more than that route's own max - min, otherwise MISS.  With out.json, all lines go there too."""
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
out_path = sys.argv[3] if len(sys.argv) > 3 else None
n, height = 1 << lg, 32
stride = (1 << height) // n
idx, v, r = bench.synth_inputs(n, height, 0, n)
hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
ctx = capi.Context(0, 1)
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


def liabilities(new_idx, salt):
    nv = np.arange(len(new_idx), dtype=np.uint64) + np.uint64(salt)
    nr = np.zeros((len(new_idx), 32), np.uint8)
    nr[:, :8] = np.ascontiguousarray(new_idx).view(np.uint8).reshape(-1, 8)
    nr[:, 8] = salt
    return nv, nr


def random_row(rng, k):
    """k leaves to remove, k free indexes to add, k other leaves to replace."""
    at = rng.choice(n, size=2 * k, replace=False)
    new = np.zeros(0, np.uint64)
    while len(new) < k:
        x = rng.integers(0, 1 << height, size=k - len(new) + 16, dtype=np.uint64)
        new = np.union1d(new, x[x % np.uint64(stride) != 0])[:k]
    return np.sort(at[:k]), rng.permutation(new), np.sort(at[k:])


def block_row(rng):
    """An aligned group of 64 leaves goes; 1,024 new leaves fill the indexes after the first leaf of the group beside it."""
    g = int(rng.integers(0, n // 64)) & ~1
    return np.arange(g * 64, g * 64 + 64), np.arange(1, 1025, dtype=np.uint64) + np.uint64((g + 1) * 64 * stride), np.zeros(0, np.int64)


def sync():
    assert hip.hipDeviceSynchronize() == 0


def set_max(value):
    o = capi.Options()
    o.update_incremental_max = value
    ctx.set_options(o)


tr = capi.Tree(ctx, height, idx, v, r, bench.PAD_SEED)
root0 = tr.root()
rows = [("random", k) for k in (1, 64, 1024, 4096, 16384, 21845) if 3 * k <= n // 8] + [("block", 64)]
for shape, k in rows:
    rng = np.random.default_rng(17 + k)
    gone, new, repl = random_row(rng, k) if shape == "random" else block_row(rng)
    new_v, new_r = liabilities(new, 1)
    repl_v, repl_r = liabilities(idx[repl], 2)
    put_idx, put_v, put_r = np.concatenate([new, idx[repl]]), np.concatenate([new_v, repl_v]), np.concatenate([new_r, repl_r])
    back = np.concatenate([gone, repl]).astype(np.int64)         # the inverse: the new leaves go, the old liabilities come back
    runs = {"apply": [], "three": [], "rebuild": []}
    for _ in range(2 + reps):
        for route in ("apply", "three", "rebuild"):
            set_max(-1 if route == "rebuild" else 0)
            sync()
            t0 = time.perf_counter()
            if route == "three":
                tr.remove(idx[gone])
                paths = [tr.last_update_path()]
                tr.insert(new, new_v, new_r)
                paths.append(tr.last_update_path())
                if len(repl):
                    tr.update(idx[repl], repl_v, repl_r)
                    paths.append(tr.last_update_path())
            else:
                was_new = tr.apply(idx[gone], put_idx, put_v, put_r)
                paths = [tr.last_update_path()]
            sync()
            runs[route].append(((time.perf_counter() - t0) * 1e3, tuple(paths)))
            assert route == "three" or was_new.sum() == len(new)
            set_max(0)
            tr.apply(new, idx[back], v[back], r[back])
            assert tr.root() == root0, "the inverse apply did not restore the tree"
    stats = {}
    for route, rr in runs.items():
        cold, rr = rr[:2], rr[2:]
        ms = sorted(t for t, _ in rr)
        med = float(np.median(ms))
        stats[route] = (med, ms[-1] - ms[0])
        emit({"leaves": n, "height": height, "shape": shape, "removed": len(gone), "new": len(new), "replaced": len(repl), "route": route,
              "last_update_path": sorted({p for _, p in rr}), "median_ms": round(med, 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
              "spread": round((ms[-1] - ms[0]) / med, 3), "warmup_ms": [round(c, 3) for c, _ in cold], "repeats": reps})
    verdict = {"leaves": n, "height": height, "shape": shape, "removed": len(gone), "new": len(new), "replaced": len(repl)}
    for other in ("three", "rebuild"):
        med, width = stats[other]
        verdict["apply_vs_" + other] = "AHEAD" if med - stats["apply"][0] > width else "MISS"
        verdict[other + "_over_apply"] = round(med / stats["apply"][0], 2)
    emit(verdict)
tr.close()
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(json.dumps(x) for x in lines) + "\n")
