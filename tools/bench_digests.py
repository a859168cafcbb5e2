"""What each 32-byte digest costs on the headline shapes: python tools/bench_digests.py [log2_entities=20] [repeats=7] [out.json]
For BLAKE3, Blake2s, SHA-256 and SHA3-256, on a context of that digest: the tree build over 2^20 strided leaves at height 32 (the
leaves resident in HBM: Workload.build, as bench.py --mode build times it) and dapol_build_leaf_nodes over 2^20 ids `id-%08d` under
the same digest (host-inclusive: the ids go up and the leaves come back).  Timed with a host clock around the call and a device
synchronise, in one process: two warm-up calls (reported, not counted), then `repeats` timed ones.  Prints one JSON line per
(digest, what) with the median, spread = (max - min) / median and the ratio of the median to BLAKE3's; with a third argument the
lines are also written there as one JSON list.  A digest the loaded library refuses (an older build through DAPOL_HIP_LIB) is
reported as refused and skipped."""
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
idx, v, r = bench.synth_inputs(n, height, 0, n)
ids = np.char.add("id-", np.char.zfill(np.arange(n).astype("U8"), 8)).astype("S11")
off = (np.arange(n + 1, dtype=np.uint64) * 11).astype(np.uint32)
packed = ids.tobytes()
vals = np.random.default_rng(4).integers(0, 1 << 32, size=n, dtype=np.uint64)
hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
DIGESTS = [("blake3", 0), ("blake2s", 1), ("sha256", 4), ("sha3_256", 5)]


def timed(call):
    assert hip.hipDeviceSynchronize() == 0
    t0 = time.perf_counter()
    res = call()
    assert hip.hipDeviceSynchronize() == 0
    return (time.perf_counter() - t0) * 1e3, res


lines, base = [], {}
for name, dg in DIGESTS:
    try:
        ctx = capi.Context(0, 1, digest=dg)
    except capi.DapolError as e:
        lines.append({"digest": name, "refused": e.code})
        print(json.dumps(lines[-1]), flush=True)
        continue
    w = capi.Workload(ctx, height, idx, v, r)
    whats = [("tree_build", lambda: w.build(bench.PAD_SEED)[0]),
             ("leaf_derivation", lambda: ctx.build_leaf_nodes_packed(packed, off, packed, off, vals, b"bench-audit-seed", height, dg)["leaf_idx"][:4].tolist())]
    for what, call in whats:
        runs = [timed(call) for _ in range(2 + reps)]
        cold, ms = [t for t, _ in runs[:2]], sorted(t for t, _ in runs[2:])
        med = float(np.median(ms))
        base.setdefault(what, med)                               # BLAKE3 comes first
        check = runs[-1][1]
        lines.append({"digest": name, "what": what, "entities": n, "height": height, "median_ms": round(med, 3), "min_ms": round(ms[0], 3),
                      "max_ms": round(ms[-1], 3), "spread": round((ms[-1] - ms[0]) / med, 3), "ratio_to_blake3": round(med / base[what], 3),
                      "warmup_ms": [round(c, 3) for c in cold], "repeats": reps,
                      "check": check[1].hex()[:16] if what == "tree_build" else check})
        print(json.dumps(lines[-1]), flush=True)
    w.close()
    ctx.close()
if out_path:
    with open(out_path, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
