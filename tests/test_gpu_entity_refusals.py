"""What the four per-entity proving entry points REFUSE, and in which order: dapol_prove_entities_upper, dapol_prove_entities_tape,
dapol_prove_entities_shared and dapol_reprove_entities_shared share one call frame (dapol_amd/csrc/host_entity.inc), and their argument
checks differ in small ways that callers may depend on -- which refusal wins when two arguments are bad at once, and what a call of zero
entities returns when another argument is bad.  tests/golden/entity_refusals.json holds (return code, dapol_last_error text) of every
single fault and every pair of faults below, with b = 0 and b = 2, as the entry points gave them BEFORE they were rebuilt on the shared
frame; this test replays the table and compares code and text exactly.

The trees: height 6, 8 leaves, in an 8-party context.  Two faults cannot be shown on that tree and bring one of their own in the same
context: an aggregation that needs 16 parties needs a path of 9 siblings or more (a height-12 tree, aggregation 9), and tape mode on a
shard needs a shard (the left half of a height-7 tree: 6 levels as well).  A pair of faults that set the same argument is no pair.

Regenerate (only when a change of behaviour is meant): python tests/test_gpu_entity_refusals.py <out.json> on a GPU."""
import ctypes
import itertools
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entity_refusals.json")

# fault -> (the entry points it applies to, the arguments it replaces)
ALL = ("upper", "tape", "shared", "reprove")
FAULTS = [
    ("null_nonce", ALL, {"nonce": None}),                      # (the tape in tape mode)
    ("null_leaf_idx", ALL, {"leaf_idx": None}),
    ("null_range_out", ALL, {"range_out": None}),
    ("other_ctx", ALL, {"ctx": "ctx2"}),
    ("n_upper_-1", ("upper", "shared"), {"n_upper": -1}),
    ("n_upper_17", ("upper", "shared"), {"n_upper": 17}),
    ("bad_policy", ALL, {"policy": 7}),
    ("agg_above_height", ALL, {"agg": 7}),
    ("bad_n_bits", ALL, {"n_bits": 12}),
    ("needs_16_parties", ALL, {"tree": "tall", "agg": 9}),
    ("not_increasing", ("shared", "reprove"), {"leaf_idx": "reversed"}),
    ("unknown_leaf", ALL, {"leaf_idx": "unknown"}),
    ("tape_on_shard", ("tape",), {"tree": "shard"}),
    ("has_old_without_arrays", ("reprove",), {"has_old": "set"}),
]


def case_names():
    """(entry point, faults, b) of every case, in the order of the golden file"""
    out = []
    for fn in ALL:
        mine = [f for f in FAULTS if fn in f[1]]
        sets = [(f,) for f in mine] + [p for p in itertools.combinations(mine, 2) if not set(p[0][2]) & set(p[1][2])]
        for fs in sets:
            for b in (0, 2):
                out.append((fn, [f[0] for f in fs], b))
    return out


class _World:
    def __init__(self, capi):
        self.capi, self.L = capi, capi.lib()
        rng = np.random.default_rng(11)
        self.ctx, self.ctx2 = capi.Context(0, 8), capi.Context(0, 8)

        def tree(height, shard_bits=0):
            idx = np.sort(rng.choice(1 << 6, size=8, replace=False).astype(np.uint64))
            v = rng.integers(0, 8, size=8, dtype=np.uint64)
            r = rng.integers(0, 256, size=(8, 32), dtype=np.uint8)
            r[:, 31] &= 0x0F
            return idx, capi.Tree(self.ctx, height, idx, v, r, SEED, shard_bits=shard_bits)
        self.trees = {"main": tree(6), "tall": tree(12), "shard": tree(7, 1)}
        assert self.trees["shard"][1].height == 6

    def run(self, fn, faults, b):
        a = {"ctx": "ctx", "tree": "main", "leaf_idx": "first", "policy": 0, "agg": 6, "n_bits": 8, "nonce": "given", "n_upper": 0, "range_out": "given",
             "has_old": "clear"}
        for name, _, repl in FAULTS:
            if name in faults:
                a.update(repl)
        idx, tr = self.trees[a["tree"]]
        absent = next(i for i in range(int(idx[0]) + 1, 64) if i not in set(map(int, idx)))
        leaf = {None: None, "first": idx[:2].copy(), "reversed": idx[[1, 0]].copy(), "unknown": np.array([idx[0], absent], np.uint64)}[a["leaf_idx"]]
        ctx = getattr(self, a["ctx"])
        h = tr.height + max(0, min(a["n_upper"], 16))
        C, H, out = np.zeros((2, h, 32), np.uint8), np.zeros((2, h, 32), np.uint8), np.zeros((2, 4096), np.uint8)
        P = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)
        rout = out if a["range_out"] else None
        seed = np.frombuffer(SEED, np.uint8).copy() if a["nonce"] else None
        cnt = ctypes.c_uint64(0)
        common = (ctx.h, tr.h, b, P(leaf), a["policy"], a["agg"], a["n_bits"])
        if fn == "upper":
            rc = self.L.dapol_prove_entities_upper(*common, P(seed), a["n_upper"], None, None, None, None, P(C), P(H), P(rout))
        elif fn == "shared":
            rc = self.L.dapol_prove_entities_shared(*common, P(seed), a["n_upper"], None, None, None, None, P(C), P(H), P(rout), ctypes.byref(cnt))
        elif fn == "tape":
            tape = np.zeros(2 * 64 * 4096, np.uint8) if a["nonce"] else None           # (more draws than any plan here takes)
            rc = self.L.dapol_prove_entities_tape(*common, P(tape), P(C), P(H), P(rout))
        else:
            has_old = np.full(2, 1 if a["has_old"] == "set" else 0, np.uint8)
            rc = self.L.dapol_reprove_entities_shared(*common, P(seed), P(has_old), None, None, P(C), P(H), P(rout), ctypes.byref(cnt), ctypes.byref(cnt))
        return int(rc), (self.L.dapol_last_error().decode() if rc else "")


def record(capi):
    w = _World(capi)
    rows = []
    for fn, faults, b in case_names():
        rc, text = w.run(fn, faults, b)
        assert rc != 0 or b == 0, (fn, faults, b)                # with entities to prove, every case here is a refusal
        rows.append({"fn": fn, "faults": faults, "b": b, "rc": rc, "text": text})
    return rows


def test_every_refusal_keeps_its_code_text_and_precedence(hip_lib):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert [(r["fn"], r["faults"], r["b"]) for r in want] == [(fn, fs, b) for fn, fs, b in case_names()]      # the table is the whole list
    got = record(hip_lib)
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, diff[:5]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.setdefault("DAPOL_ENV_KNOBS", "1")
    from dapol_amd import capi as _capi
    with open(sys.argv[1], "w") as f:
        json.dump(record(_capi), f, indent=0)
    print("recorded", len(case_names()), "cases")
