#!/usr/bin/env python3
"""dapol_batch_store against the whole dapol_reprove_batches call on the same edited tree, in the same process: what a caller who serves
batch proofs between edits runs with the store, against what it runs when it holds the old siblings and blobs on the host.  The shape is
bench_reprove_batches.py's: 2^16 leaves at stride 2^(height - 16) of a tree of the given height (default 32), 64-bit proofs, `--batches`
(default 4,096) batches of k = 2 and of k = 4 random leaves, at padding / 16, splitting / 24 and padding / 0, edited by 1, 64 and 4,096
replaced liabilities.  Two store legs are timed: "refresh + fetch of `--fetch` (256) random batches" and "refresh + read of everything",
each on a store of its own; the baseline is dapol_reprove_batches with the previous state's arrays going up and all new arrays coming
down.  A RUN replaces the same e leaves with new random values and blindings (dapol_tree_update, not timed) and then times the three
legs one after the other on that same edited tree, so every run re-proves the same sub-proofs in all three and no leg ever sees an
edit twice; the host clock stands around each leg with a device synchronise.  Two warm-up runs, then `--runs` (7) timed ones.  On every
run the store's full read is compared byte for byte with the baseline's outputs, and the fetched rows with their slices.  AHEAD: the
leg's median lies below the baseline's median by more than the baseline's own max - min; otherwise the row says that no gain beyond the
baseline's spread was seen.  The store's own earlier runs are never the yardstick.
Prints one JSON document.
Usage: python tools/bench_batch_store.py [--height 32] [--batches 4096] [--k 2,4] [--shapes padding/16,splitting/24,padding/0]
                                         [--edits 1,64,4096] [--fetch 256] [--out FILE]"""
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
ap.add_argument("--batches", type=int, default=4096)
ap.add_argument("--k", default="2,4")
ap.add_argument("--shapes", default="padding/16,splitting/24,padding/0")
ap.add_argument("--edits", default="1,64,4096")
ap.add_argument("--fetch", type=int, default=256)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert a.runs >= 7
H, N, NBITS, seed, nb = a.height, 1 << 16, 64, bytes(range(32)), a.batches
rng = np.random.default_rng(1)
idx = (np.arange(N, dtype=np.uint64) << np.uint64(H - 16)).astype(np.uint64)
v = rng.integers(0, 2**32, size=N, dtype=np.uint64)
r = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
r[:, 31] &= 0x0F
lib, P = capi.lib(), (lambda x: x.ctypes.data_as(ctypes.c_void_p))
hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
sd = np.frombuffer(seed, np.uint8).copy()


def timed(fn):
    t0 = time.perf_counter()
    fn()
    assert hip.hipDeviceSynchronize() == 0
    return time.perf_counter() - t0


def stats(ts):
    med = statistics.median(ts)
    return {"median_s": med, "min_s": min(ts), "max_s": max(ts), "spread": (max(ts) - min(ts)) / med, "runs_s": ts}


def chk(rc):
    assert rc == 0, (rc, lib.dapol_last_error())


def pick_batches(k):
    pick = np.sort(rng.integers(0, N, size=(nb, k)), axis=1)
    while True:                                               # k DISTINCT leaves per batch: redraw the rows that repeat one
        dup = (np.diff(pick, axis=1) == 0).any(axis=1)
        if not dup.any():
            return idx[pick]                                  # [nb][k], rows strictly increasing
        pick[dup] = np.sort(rng.integers(0, N, size=(int(dup.sum()), k)), axis=1)


def run_rows(ctx, tree, k, batches, shape, policy, agg, edits, rows):
    _, off, flat = capi._pack_batches(list(batches))
    ns, so, ro, ng = capi.batches_plan(H, list(batches), policy, agg, NBITS)
    T, R = int(so[-1]), int(ro[-1])
    old_C, old_R = np.zeros((T, 32), np.uint8), np.zeros(R, np.uint8)
    new_C, new_H, new_R = np.zeros((T, 32), np.uint8), np.zeros((T, 32), np.uint8), np.zeros(R, np.uint8)
    all_C, all_H, all_R = np.zeros((T, 32), np.uint8), np.zeros((T, 32), np.uint8), np.zeros(R, np.uint8)
    want = np.sort(rng.choice(nb, size=min(a.fetch, nb), replace=False)).astype(np.uint64)
    rows_i = want.astype(np.int64)
    qs = np.concatenate([[0], np.cumsum(so[rows_i + 1] - so[rows_i])]).astype(np.int64)
    qr = np.concatenate([[0], np.cumsum(ro[rows_i + 1] - ro[rows_i])]).astype(np.int64)
    got_C, got_H, got_R = np.zeros((int(qs[-1]), 32), np.uint8), np.zeros((int(qs[-1]), 32), np.uint8), np.zeros(int(qr[-1]), np.uint8)
    proved, kept, calls = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    s_proved, s_kept, s_calls, s_moved = (ctypes.c_uint64(0) for _ in range(4))
    serving, reading = capi.BatchStore(tree, policy, agg, NBITS, seed), capi.BatchStore(tree, policy, agg, NBITS, seed)

    def refresh(store):
        chk(lib.dapol_batch_store_refresh(store.h, 0, None, None, ctypes.byref(s_proved), ctypes.byref(s_kept), ctypes.byref(s_calls), ctypes.byref(s_moved)))

    def leg_fetch():
        refresh(serving)
        chk(lib.dapol_batch_store_fetch(serving.h, want.shape[0], P(want), P(got_C), P(got_H), P(got_R)))

    def leg_read():
        refresh(reading)
        chk(lib.dapol_batch_store_read(reading.h, 0, nb, P(all_C), P(all_H), P(all_R)))

    def leg_reprove():
        chk(lib.dapol_reprove_batches(ctx.h, tree.h, nb, P(off), P(flat), policy, agg, NBITS, P(sd), None, P(old_C), P(old_R), P(new_C), P(new_H), P(new_R),
                                      ctypes.byref(proved), ctypes.byref(kept), ctypes.byref(calls)))

    def fetched_equal():
        for i, j in enumerate(rows_i):
            s0, s1, r0, r1 = int(so[j]), int(so[j + 1]), int(ro[j]), int(ro[j + 1])
            if (got_C[qs[i]:qs[i + 1]].tobytes() != new_C[s0:s1].tobytes() or got_H[qs[i]:qs[i + 1]].tobytes() != new_H[s0:s1].tobytes() or
                    got_R[qr[i]:qr[i + 1]].tobytes() != new_R[r0:r1].tobytes()):
                return False
        return True

    try:
        serving.refresh(list(batches)), reading.refresh(list(batches))            # the fill, not timed
        chk(lib.dapol_batch_store_read(reading.h, 0, nb, P(old_C), None, P(old_R)))   # the previous state's arrays, as the baseline's caller holds them
        for e in edits:
            at = np.sort(rng.choice(N, size=e, replace=False))
            tf, tr, tb, equal, same_work = [], [], [], True, True
            for run in range(2 + a.runs):                     # two warm-ups, then the timed runs
                nv, nr = rng.integers(0, 2**32, size=e, dtype=np.uint64), rng.integers(0, 256, size=(e, 32), dtype=np.uint8)
                nr[:, 31] &= 0x0F
                tree.update(idx[at], nv, nr)
                t = [timed(leg_fetch)]
                fetch_counts = (s_proved.value, s_kept.value, s_calls.value, s_moved.value)
                t.append(timed(leg_read))
                read_counts = (s_proved.value, s_kept.value, s_calls.value, s_moved.value)
                t.append(timed(leg_reprove))
                base_counts = (proved.value, kept.value, calls.value, 0)
                equal = (equal and all_C.tobytes() == new_C.tobytes() and all_H.tobytes() == new_H.tobytes() and all_R.tobytes() == new_R.tobytes() and
                         fetched_equal())
                same_work = same_work and fetch_counts == read_counts == base_counts
                old_C[:], old_R[:] = new_C, new_R             # what this state's call returned is what the caller holds at the next edit
                if run >= 2:
                    tf.append(t[0]), tr.append(t[1]), tb.append(t[2])
            _, plan_total, sum_m, sum_m_all = capi.reprove_batches_plan(H, list(batches), idx[at], policy, agg, NBITS)
            F, Rd, B = stats(tf), stats(tr), stats(tb)
            band = B["max_s"] - B["min_s"]

            def verdict(leg):
                return "AHEAD" if B["median_s"] - leg["median_s"] > band else "no gain beyond the baseline's run-to-run spread"
            row = {"shape": shape, "k": k, "batches": nb, "edited": e, "leaves": N, "height": H, "n_bits": NBITS, "s_groups": ng,
                   "siblings_min_max": [int(ns.min()), int(ns.max())], "sibling_records": T, "range_bytes": R, "fetched_batches": int(want.shape[0]),
                   "fetched_bytes": int(qr[-1] + 64 * qs[-1]), "refresh_fetch": F, "refresh_read_all": Rd, "reprove_batches": B,
                   "time_ratio_reprove_over_refresh_fetch": B["median_s"] / F["median_s"], "time_ratio_reprove_over_refresh_read_all": B["median_s"] / Rd["median_s"],
                   "proved": int(proved.value), "kept": int(kept.value), "range_prover_calls": int(calls.value), "planner_total": plan_total,
                   "sum_m_proved": sum_m, "sum_m_all": sum_m_all, "bytes_equal_on_every_run": bool(equal), "counters_equal_on_every_run": bool(same_work),
                   "verdict_refresh_fetch": verdict(F), "verdict_refresh_read_all": verdict(Rd)}
            assert equal and same_work and proved.value == plan_total, row
            rows.append(row)
            print("[bench_batch_store] %s k=%d e=%d: reprove_batches %.4f s (spread %.1f %%), refresh + fetch %d %.4f s (x%.2f, %s), refresh + read all %.4f s (x%.2f, %s)"
                  % (shape, k, e, B["median_s"], 100 * B["spread"], want.shape[0], F["median_s"], row["time_ratio_reprove_over_refresh_fetch"], verdict(F),
                     Rd["median_s"], row["time_ratio_reprove_over_refresh_read_all"], verdict(Rd)), file=sys.stderr, flush=True)
    finally:
        serving.close()
        reading.close()


rows = []
ks = [int(x) for x in a.k.split(",")]
edits = [int(x) for x in a.edits.split(",")]
batches_of = {k: pick_batches(k) for k in ks}
ctx = capi.Context(0, 32)
tree = capi.Tree(ctx, H, idx, v, r, seed)
for name in a.shapes.split(","):
    pol_name, agg = name.split("/")
    for k in ks:
        run_rows(ctx, tree, k, batches_of[k], name, capi.POLICY_PADDING if pol_name == "padding" else capi.POLICY_SPLITTING, int(agg), edits, rows)
tree.close()
ctx.close()
doc = {"config": "2^16 leaves at stride 2^%d, height %d, %d-bit proofs, context of 32 parties; %d batches of k random leaves (numpy default_rng(1)); per run the "
                 "same e liabilities are replaced with new random values by dapol_tree_update (not timed), then three legs are timed on that tree: "
                 "dapol_batch_store_refresh + _fetch of %d random batches, dapol_batch_store_refresh + _read of every row (a store each), and the whole "
                 "dapol_reprove_batches call (old siblings and blobs in, siblings and blobs back) -- the baseline; host clock around each leg with a device "
                 "synchronise; 2 warm-up runs + %d timed runs; the full read is compared with the baseline's outputs byte for byte on every run"
                 % (H - 16, H, NBITS, nb, min(a.fetch, nb), a.runs),
       "rows": rows}
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
