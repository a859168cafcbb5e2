"""The tree paths the other tree tools do not reach: python tools/bench_tree_small_paths.py
Host ms around the call with a device synchronise, two warm-ups, then the timed repeats; one JSON line per case with the median, min, max.
  phased 2^12            dapol_tree_build of 4,096 leaves, height 32, 31 times: the small-tree phases (k_tree_structure_small,
                         k_tree_padding_all, k_tree_sum_level, k_tree_compress_all, k_tree_hash_level)
  levelwise fused 2^18   the same of 2^18 leaves, 7 times, with DAPOL_TREE_LEVELWISE=1 DAPOL_TREE_SPLIT=0: k_tree_merge<0> in seed mode
  paths 4096 of 2^18     dapol_tree_paths of 4,096 leaves of that tree, 15 times: k_tree_find_leaves, k_tree_path_walk (and 12 MB to the host)
A/B of two builds: run it once per library (DAPOL_HIP_LIB), alternated."""
import ctypes
import json
import os
import sys
import time

os.environ["DAPOL_ENV_KNOBS"] = "1"
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dapol_amd import capi  # noqa: E402
import bench  # noqa: E402

hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
ctx = capi.Context(0, 1)
height = 32


def report(case, n, ms, check):
    ms = sorted(ms)
    print(json.dumps({"case": case, "leaves": n, "median_ms": round(float(np.median(ms)), 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
                      "check": check, "repeats": len(ms)}), flush=True)


def timed(f):
    assert hip.hipDeviceSynchronize() == 0
    t0 = time.perf_counter()
    out = f()
    assert hip.hipDeviceSynchronize() == 0
    return (time.perf_counter() - t0) * 1e3, out


def builds(case, lg, reps, env):
    n = 1 << lg
    idx, v, r = bench.synth_inputs(n, height, 0, n)
    os.environ.update(env)
    try:
        ms = []
        for _ in range(2 + reps):
            t, tr = timed(lambda: capi.Tree(ctx, height, idx, v, r, bench.PAD_SEED))
            root = tr.root()[0].hex()[:16]
            ms.append(t)
            tr.close()
    finally:
        for k in env:
            os.environ.pop(k, None)
    report(case, n, ms[2:], root)


builds("phased 2^12", 12, 31, {})
builds("levelwise fused (SPLIT=0) 2^18", 18, 7, {"DAPOL_TREE_LEVELWISE": "1", "DAPOL_TREE_SPLIT": "0"})
n = 1 << 18
idx, v, r = bench.synth_inputs(n, height, 0, n)
tr = capi.Tree(ctx, height, idx, v, r, bench.PAD_SEED)
pick = idx[np.sort(np.random.default_rng(3).choice(n, size=4096, replace=False))]
runs = [timed(lambda: tr.paths(pick)) for _ in range(2 + 15)]
import hashlib  # noqa: E402
report("paths 4096 of 2^18", n, [t for t, _ in runs[2:]], hashlib.sha256(b"".join(a.tobytes() for a in runs[-1][1])).hexdigest()[:16])
tr.close()
