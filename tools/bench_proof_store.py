#!/usr/bin/env python3
"""dapol_proof_store against dapol_reprove_entities_shared on the same edited tree, in the same process: what an operator who serves
inclusion proofs runs after k liabilities were replaced (dapol_tree_update).  The tree is bench_reprove.py's (random strictly increasing
leaves, numpy default_rng(1)), 64-bit proofs, seed nonces.  Per shape the store is filled once (refresh of every leaf) and the host holds
the same rows (a read of all of them).  Per k: one warm-up and `--runs` timed rounds; every round replaces k fresh random liabilities and
then runs both legs on that same tree, in alternating order, the host clock around whole calls (each ends with a device synchronise):
  OLD   dapol_reprove_entities_shared on the parent's terms: the previous round's paths and blobs in, all paths and blobs out;
  NEW   dapol_proof_store_refresh, then dapol_proof_store_fetch of 1,024 random leaves.
A read of every row (dapol_proof_store_read) is timed in every round as well: refresh + full read is the comparison for a caller who
wants everything back.  `proved` must be equal in both legs and sample rows of both are compared byte for byte.  Acceptance per row, where
the re-prover keeps anything: the NEW median must lie below the OLD median by more than the OLD spread ((max - min) / median); a row
that does not is written as a MISS.  padding / H keeps nothing: its row states the overhead or gain as it is.
After the k rounds of a shape: the row-moving path (`--runs` rounds of insert of 4,096 new leaves + refresh, remove of the same + refresh)
and dapol_proof_store_verify against dapol_verify_entities fed the same rows from the host, on a store refreshed to `--verify-rows`
evenly spaced leaves (1 warm-up + `--runs` alternating runs).  Memory figures are store_plan.inc's formulas.
Prints one JSON document; --out FILE writes it, replacing the rows of the shapes measured and keeping the others of an earlier run.
Usage: python tools/bench_proof_store.py [--log2-entities 20] [--height 32] [--runs 5] [--shapes padding/16,splitting/24,padding/0,padding/32]
                                         [--ks 1,4096] [--fetch 1024] [--moved 4096] [--verify-rows 65536] [--out FILE]"""
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
ap.add_argument("--log2-entities", type=int, default=20)
ap.add_argument("--height", type=int, default=32)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--shapes", default="padding/16,splitting/24,padding/0,padding/32")
ap.add_argument("--ks", default="1,4096")
ap.add_argument("--fetch", type=int, default=1024)
ap.add_argument("--moved", type=int, default=4096)
ap.add_argument("--verify-rows", type=int, default=65536)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert a.runs >= 5, "a median of at least 5 runs"
n, H, seed = 1 << a.log2_entities, a.height, bytes(range(32))
rng = np.random.default_rng(1)
cand = np.unique(rng.integers(0, 1 << H, size=n + n // 4, dtype=np.uint64))
idx = np.sort(rng.choice(cand, size=n, replace=False)).astype(np.uint64)
spare_leaves = np.setdiff1d(cand, idx)[:a.moved]              # indexes that are no leaves: what the row-moving rounds insert and remove
v = rng.integers(0, 2**32, size=n, dtype=np.uint64)
r = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
r[:, 31] &= 0x0F
ctx = capi.Context(0, 32)
tree = capi.Tree(ctx, H, idx, v, r, seed)
lib, P = capi.lib(), (lambda x: x.ctypes.data_as(ctypes.c_void_p))
sd = np.frombuffer(seed, np.uint8).copy()


def timed(fn):
    t0 = time.perf_counter()
    rc = fn()
    dt = time.perf_counter() - t0
    assert rc == 0, (rc, lib.dapol_last_error())
    return dt


def stats(ts):
    med = statistics.median(ts)
    return {"median_s": med, "min_s": min(ts), "max_s": max(ts), "spread": (max(ts) - min(ts)) / med, "runs_s": list(ts)}


def liabilities(k):
    nv, nr = rng.integers(0, 2**32, size=k, dtype=np.uint64), rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
    nr[:, 31] &= 0x0F
    return nv, nr


rows = []
for name in a.shapes.split(","):
    pol_name, agg = name.split("/")
    policy, agg = (capi.POLICY_PADDING if pol_name == "padding" else capi.POLICY_SPLITTING), int(agg)
    es = lib.dapol_entity_proof_size(H, policy, agg, 64)
    assert es, name
    need = 2 * n * es + 3 * n * H * 32                       # two blob buffers and three path buffers in host memory
    avail = next((int(line.split()[1]) * 1024 for line in open("/proc/meminfo") if line.startswith("MemAvailable")), None)
    assert avail is None or need < 0.6 * avail, "%s needs %.1f GB of host memory, %.1f GB are available" % (name, need / 1e9, avail / 1e9)
    store = capi.ProofStore(tree, policy, agg, 64, seed)
    t0 = time.perf_counter()
    fill_proved = store.refresh()[0]
    t_fill = time.perf_counter() - t0
    old_C, old_R = np.zeros((n, H, 32), np.uint8), np.zeros((n, es), np.uint8)
    out_C, out_H, out_R = np.zeros((n, H, 32), np.uint8), np.zeros((n, H, 32), np.uint8), np.zeros((n, es), np.uint8)
    for x in (old_C, old_R, out_C, out_H, out_R):
        x.fill(0)                                            # map the pages now: a first write inside a timed call would be charged to that leg
    got_idx = np.zeros(n, np.uint64)
    read_all = lambda: lib.dapol_proof_store_read(store.h, 0, n, P(got_idx), P(out_C), P(out_H), P(out_R))
    timed(read_all)                                          # what the host holds before the first edit (and the warm-up of the read)
    assert got_idx.tobytes() == idx.tobytes()
    kf = min(a.fetch, n)
    f_found, f_C, f_H, f_R = np.zeros(kf, np.uint8), np.zeros((kf, H, 32), np.uint8), np.zeros((kf, H, 32), np.uint8), np.zeros((kf, es), np.uint8)
    proved, kept, s_proved, s_kept, s_moved = (ctypes.c_uint64(0) for _ in range(5))
    reprove = lambda: lib.dapol_reprove_entities_shared(ctx.h, tree.h, n, P(idx), policy, agg, 64, P(sd), None, P(old_C), P(old_R), P(out_C), P(out_H), P(out_R),
                                                        ctypes.byref(proved), ctypes.byref(kept))
    refresh = lambda: lib.dapol_proof_store_refresh(store.h, 0, None, ctypes.byref(s_proved), ctypes.byref(s_kept), ctypes.byref(s_moved))
    bytes_of = {"idx": n * 8, "path_C": n * H * 32, "path_H": n * H * 32, "range": n * es}      # store_plan.inc: store_bytes(n, H, 32, es)
    memory = {"store_resident_bytes": bytes_of["idx"] + 2 * (bytes_of["path_C"] + bytes_of["path_H"]) + bytes_of["range"],
              "row_moving_transient_bytes": bytes_of["range"] + bytes_of["path_C"], "blob_bytes_per_row": es}
    for k in [int(x) for x in a.ks.split(",")]:
        t_old, t_new, t_refresh, t_fetch, t_read, t_edit = [], [], [], [], [], []
        equal, same_proved, sum_m, sum_m_shared = True, True, 0, 0
        for run in range(a.runs + 1):                        # round 0 is the warm-up of both legs
            old_C, out_C = out_C, old_C                      # what the last round returned is what the caller holds now
            old_R, out_R = out_R, old_R
            at = np.sort(rng.choice(n, size=k, replace=False))
            nv, nr = liabilities(k)
            te = timed(lambda: lib.dapol_tree_update(tree.h, k, P(idx[at]), P(nv), P(nr)))
            want = np.sort(rng.choice(n, size=kf, replace=False))
            q = idx[rng.permutation(want)]                   # any order
            fetch = lambda: lib.dapol_proof_store_fetch(store.h, kf, P(q), P(f_found), P(f_C), P(f_H), P(f_R))

            def new_leg():
                tr_ = timed(refresh)
                tf_ = timed(fetch)
                return tr_, tf_
            if run % 2:
                to = timed(reprove)
                tr_, tf_ = new_leg()
            else:
                tr_, tf_ = new_leg()
                to = timed(reprove)
            at_q = np.searchsorted(idx, q)                   # the re-prover's rows of the fetched leaves
            equal &= bool(f_found.all() and f_C.tobytes() == out_C[at_q].tobytes() and f_H.tobytes() == out_H[at_q].tobytes() and
                          f_R.tobytes() == out_R[at_q].tobytes())
            same_proved &= proved.value == s_proved.value and kept.value == s_kept.value and s_moved.value == 0
            if run == 0:
                _, plan_total, sum_m, sum_m_shared = capi.reprove_plan(H, idx, idx[at], policy, agg)
                assert plan_total == proved.value, (plan_total, proved.value)
                continue
            trd = timed(read_all)                            # (overwrites the re-prover's outputs with the same bytes)
            t_old.append(to); t_new.append(tr_ + tf_); t_refresh.append(tr_); t_fetch.append(tf_); t_read.append(trd); t_edit.append(te)
        O, N = stats(t_old), stats(t_new)
        full = stats([x + y for x, y in zip(t_refresh, t_read)])
        gain = (O["median_s"] - N["median_s"]) / O["median_s"]
        keeps = sum_m * 1000 < sum_m_shared * 999            # (padding / H keeps one pair per replaced leaf: nothing, for this purpose)
        row = {"kind": "update", "shape": name, "k": k, "entities": n, "height": H, "fetched": kf, "fill_s": t_fill, "fill_proved": fill_proved,
               "tree_update_s": statistics.median(t_edit), "old_reprove": O, "new_refresh_plus_fetch": N, "refresh": stats(t_refresh), "fetch": stats(t_fetch),
               "read_all": stats(t_read), "refresh_plus_read_all": full, "time_ratio_old_over_new": O["median_s"] / N["median_s"],
               "time_ratio_old_over_refresh_plus_read_all": O["median_s"] / full["median_s"], "proved_last_round": int(s_proved.value),
               "kept_last_round": int(s_kept.value), "sum_m_proved_first_round": sum_m, "sum_m_shared": sum_m_shared, "proved_equal_in_both_legs": same_proved,
               "sample_rows_equal": equal, "memory": memory,
               "verdict": ("PASS" if gain > O["spread"] else "MISS") if keeps else "nothing kept: %+.2f %% against the re-prover (its spread %.2f %%)"
                          % (-100.0 * gain, 100.0 * O["spread"])}
        assert equal and same_proved, row
        rows.append(row)
        print("[bench_proof_store] %s k=%d: re-prover %.3f s, refresh %.3f + fetch %.4f s, x%.2f; refresh + read all %.3f s, x%.2f: %s" %
              (name, k, O["median_s"], row["refresh"]["median_s"], row["fetch"]["median_s"], row["time_ratio_old_over_new"], full["median_s"],
               row["time_ratio_old_over_refresh_plus_read_all"], row["verdict"]), file=sys.stderr, flush=True)
    del old_C, old_R
    # ---- the row-moving path: the same `moved` new leaves go in and out
    km = len(spare_leaves)
    if km:
        t_ins, t_rem, t_tree = [], [], []
        mv, mr = liabilities(km)
        for run in range(a.runs + 1):
            t_tree.append(timed(lambda: lib.dapol_tree_insert(tree.h, km, P(spare_leaves), P(mv), P(mr))))
            ti = timed(refresh)
            assert s_moved.value == n and store.rows == n + km
            timed(lambda: lib.dapol_tree_remove(tree.h, km, P(spare_leaves)))
            trm = timed(refresh)
            assert s_moved.value == n and store.rows == n
            if run:
                t_ins.append(ti); t_rem.append(trm)
        timed(read_all)
        sample = np.unique(np.concatenate([np.arange(min(512, n)), np.arange(max(n - 512, 0), n), rng.integers(0, n, size=512)]))
        chk = tree.prove_entities_shared(idx[sample], policy, agg, 64, seed)
        # (a shared call over a subset shares less, but equal statements have equal bytes: rows are comparable sub-proof by sub-proof only
        # where the keys agree, so compare the paths, which do not depend on the call)
        moved_ok = bool(chk[0].tobytes() == out_C[sample].tobytes() and chk[1].tobytes() == out_H[sample].tobytes() and got_idx.tobytes() == idx.tobytes())
        row = {"kind": "move", "shape": name, "moved_leaves": km, "entities": n, "refresh_after_insert": stats(t_ins), "refresh_after_remove": stats(t_rem),
               "tree_insert_s": statistics.median(t_tree[1:]), "moved_rows": n, "paths_equal_after": moved_ok, "memory": memory}
        assert moved_ok, row
        rows.append(row)
        print("[bench_proof_store] %s rows move: refresh after insert of %d %.3f s, after remove %.3f s" %
              (name, km, row["refresh_after_insert"]["median_s"], row["refresh_after_remove"]["median_s"]), file=sys.stderr, flush=True)
    del out_C, out_H, out_R
    # ---- verify() against dapol_verify_entities fed the same rows from the host
    nv_rows = min(a.verify_rows, n)
    if nv_rows:
        sub_at = np.arange(0, n, n // nv_rows)[:nv_rows]
        sub = idx[sub_at]
        store.refresh(sub)
        s_idx, s_C, s_H, s_R = store.read()
        root = tree.root()
        # the leaves' own commitments and hashes, as a verifier holds them: from the tree's level 0 (not timed)
        l_idx, _, _, l_C, l_Hh, _ = tree.level_nodes(0)
        pos = np.searchsorted(l_idx[:n], sub)
        lC, lH = np.ascontiguousarray(l_C[pos]), np.ascontiguousarray(l_Hh[pos])
        del l_idx, l_C, l_Hh
        ok_s, ok_h = np.zeros(nv_rows, np.uint8), None
        t_s, t_h = [], []
        for run in range(a.runs + 1):
            t0 = time.perf_counter()
            ok_h = ctx.verify_entities(H, s_idx, lC, lH, s_C, s_H, root[0], root[1], policy, agg, 64, s_R, verify_seed=seed)
            th = time.perf_counter() - t0
            ts = timed(lambda: lib.dapol_proof_store_verify(store.h, P(sd), P(ok_s)))
            if run:
                t_s.append(ts); t_h.append(th)
        row = {"kind": "verify", "shape": name, "rows": nv_rows, "store_verify": stats(t_s), "verify_entities_from_host": stats(t_h),
               "all_valid": bool(ok_s.all() and ok_h.all()), "verdicts_equal": bool(ok_s.tobytes() == ok_h.tobytes())}
        assert row["all_valid"] and row["verdicts_equal"], row
        rows.append(row)
        print("[bench_proof_store] %s verify of %d rows: store %.3f s, dapol_verify_entities from the host %.3f s" %
              (name, nv_rows, row["store_verify"]["median_s"], row["verify_entities_from_host"]["median_s"]), file=sys.stderr, flush=True)
        del s_C, s_H, s_R
    store.close()
doc = {"config": "2^%d random strictly increasing leaves (numpy default_rng(1)), height %d, 64-bit proofs, seed nonces, context of 32 parties; per round k fresh "
                 "liabilities replaced by dapol_tree_update, then both legs on that tree in alternating order; host clock around whole calls; 1 warm-up + %d "
                 "rounds" % (a.log2_entities, H, a.runs), "rows": rows}
if a.out and os.path.exists(a.out):
    with open(a.out) as f:
        prev = json.load(f)
    if prev.get("config") == doc["config"]:
        measured = set(a.shapes.split(","))
        doc["rows"] = [x for x in prev["rows"] if x["shape"] not in measured] + rows
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
