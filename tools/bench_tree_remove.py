"""dapol_tree_remove on the headline tree: python tools/bench_tree_remove.py [log2_entities=20] [repeats=7]
For k = 1 / 64 / 1,024 / 4,096 removed leaves: the in-place path (last_update_path 4) against the forced rebuild
(update_incremental_max = -1), each timed with a host clock around the call and a device synchronise.  Every (k, path) removes
from one tree built for it, as an exchange that keeps its tree between rounds would: two warm-up removals (reported, not counted),
then `repeats` timed ones.  Prints one JSON line per (k, path) with the median."""
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
idx, v, r = bench.synth_inputs(n, height, 0, n)
hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
ctx = capi.Context(0, 1)
rng = np.random.default_rng(5)


def timed_remove(tr, alive, k):
    sel = rng.choice(np.flatnonzero(alive), size=k, replace=False)
    alive[sel] = False
    assert hip.hipDeviceSynchronize() == 0
    t0 = time.perf_counter()
    tr.remove(idx[sel])
    assert hip.hipDeviceSynchronize() == 0
    return (time.perf_counter() - t0) * 1e3, tr.last_update_path()


for k in (1, 64, 1024, 4096):
    for rebuild in (False, True):
        o = capi.Options()
        o.update_incremental_max = -1 if rebuild else 0
        ctx.set_options(o)
        tr = capi.Tree(ctx, height, idx, v, r, bench.PAD_SEED)
        alive = np.ones(n, bool)
        cold = [timed_remove(tr, alive, k)[0] for _ in range(2)]  # warm-up: the first two removals allocate the scratch and both level buffers
        runs = [timed_remove(tr, alive, k) for _ in range(reps)]
        tr.close()
        ms = sorted(t for t, _ in runs)
        print(json.dumps({"leaves": n, "height": height, "k": k, "path": "rebuild" if rebuild else "in_place",
                          "last_update_path": sorted({p for _, p in runs}), "median_ms": round(float(np.median(ms)), 3),
                          "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3), "warmup_ms": [round(c, 3) for c in cold],
                          "repeats": reps}), flush=True)
