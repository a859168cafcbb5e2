"""The index arithmetic of the compact form of shared proofs (dapol_amd/csrc/shared_compact_plan.inc: key shifts, the layout, expand /
compress, the verifier's key and head predicates) against a brute-force restatement written here, on random index sets at heights 1, 6,
33 and 64 under both sibling orders and both policies.  tests/cpp/shared_compact_host.cpp is a host-only build of that file with its
own main, run directly under ASan + UBSan: every buffer lives on the heap with exactly its size."""
import functools
import json
import os
import random
import subprocess

from conftest import ROOT

from test_shared_plan_abi import key_depth, plan_of
from test_verify_shared_cpu import proof_bytes


@functools.lru_cache(maxsize=None)
def _exe():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "shared_compact_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I", os.path.join(ROOT, "dapol_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "shared_compact_host.cpp"), "-o", exe], check=True)
    return exe


def _replay(lines):
    r = subprocess.run([_exe()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def pattern(i):
    return (i * 131 + (i >> 8) * 7 + (i >> 16) + 3) & 0xFF


class Case:
    def __init__(self, pyref, policy, H, agg, n_bits, leaf_first, idx, coms, first, count):
        self.policy, self.H, self.agg, self.n_bits, self.leaf_first = policy, H, agg, n_bits, leaf_first
        self.idx, self.coms, self.first, self.count = idx, coms, first, count
        self.plan = plan_of(pyref, policy, H, agg)
        self.b = len(idx)

    def line(self):
        hx = b"".join(self.coms).hex() or "-"
        return "%d %d %d %d %d %d %s %s %d %d" % (self.policy, self.H, self.agg, self.n_bits, self.leaf_first, self.b, " ".join(str(x) for x in self.idx), hx,
                                                  self.first, self.count)

    def check(self, got):
        plan, b, H = self.plan, self.b, self.H
        shifts = [H - key_depth(st, cnt, H, self.leaf_first) for st, cnt, _ in plan]
        assert got["plan"] == 1 and got["n_sub"] == len(plan) and got["shift"] == shifts
        key = lambda x, sh: 0 if sh >= 64 else x >> sh
        sizes = [proof_bytes(self.n_bits, m) for _, _, m in plan]
        sub_off, ref, kflag, hflag = [0], [], [], []
        for s, (start, count, _) in enumerate(plan):
            keys = sorted({key(x, shifts[s]) for x in self.idx})
            ref += [keys.index(key(x, shifts[s])) for x in self.idx]
            sub_off.append(sub_off[-1] + len(keys) * sizes[s])
            for e in range(b):
                k = e == 0 or key(self.idx[e], shifts[s]) != key(self.idx[e - 1], shifts[s])
                cov = lambda r: self.coms[r][start * 32:(start + count) * 32]
                kflag.append(int(k))
                hflag.append(int(k or cov(e) != cov(e - 1)))
        assert got["sub_off"] == sub_off and got["len"] == sub_off[-1] and got["ref"] == ref
        assert got["kflag"] == kflag and got["hflag"] == hflag and got["hflag16"] == hflag
        assert got["group_ref_ok"] == 1 and got["round_trip"] == 1
        assert got["window_ok"] == int(self.first + self.count <= b)
        if got["window_ok"]:
            want = bytearray()
            for e in range(self.first, self.first + self.count):
                for s in range(len(plan)):
                    at = sub_off[s] + ref[s * b + e] * sizes[s]
                    want += bytes(pattern(i) for i in range(at, at + sizes[s]))
            assert got["expand"] == want.hex()


def random_indexes(rng, H, b):
    """Strictly increasing, clustered: neighbours that share long prefixes, and the ends of the range."""
    top = (1 << H) - 1
    out = set()
    while len(out) < min(b, top + 1):
        base = rng.choice((0, top, rng.randrange(top + 1)))
        out.add(min(top, max(0, base ^ rng.randrange(1 << rng.randrange(0, min(H, 8) + 1)))))
    return sorted(out)


def make_case(pyref, rng, policy, H, agg, n_bits, leaf_first, b):
    idx = random_indexes(rng, H, b)
    plan = plan_of(pyref, policy, H, agg)
    # commitments that are a function of the subtree they speak about (as an honest tree's are): equal keys, equal covered bytes
    depth = lambda i: H - i if leaf_first else i + 1
    honest = [b"".join(random.Random(hash((i, x >> (H - depth(i)) if depth(i) else 0))).randbytes(32) for i in range(H)) for x in idx]
    coms = [bytearray(c) for c in honest]
    # one-byte corruptions at the first, a middle and the last row of a run of some sub-proof
    shifts = [H - key_depth(st, cnt, H, leaf_first) for st, cnt, _ in plan]
    for _ in range(rng.choice((0, 1, 2, 3))):
        s = rng.randrange(len(plan))
        start, count, _ = plan[s]
        if not count or not idx:
            continue
        k = lambda x: 0 if shifts[s] >= 64 else x >> shifts[s]
        heads = [e for e in range(len(idx)) if e == 0 or k(idx[e]) != k(idx[e - 1])]
        h = rng.choice(heads)
        end = next((x for x in heads if x > h), len(idx))
        e = rng.choice((h, (h + end - 1) // 2, end - 1))
        at = rng.choice((start * 32, (start + count) * 32 - 1, rng.randrange(start * 32, (start + count) * 32)))
        coms[e][at] ^= 1 << rng.randrange(8)
    n = len(idx)
    first, count = rng.choice(((0, n), (n - 1 if n else 0, 1 if n else 0), (min(3, n), min(2, n - min(3, n))), (0, 0), (n, 0)))
    return Case(pyref, policy, H, agg, n_bits, leaf_first, idx, [bytes(c) for c in coms], first, count)


SHAPES = [(0, 1, 0), (0, 1, 1), (1, 1, 0), (1, 1, 1), (0, 6, 0), (0, 6, 3), (0, 6, 6), (1, 6, 3), (1, 6, 5), (1, 6, 6), (0, 33, 0), (0, 33, 16), (1, 33, 24),
          (1, 33, 33), (0, 64, 0), (0, 64, 2), (0, 64, 64), (1, 64, 63)]


def test_layout_expand_compress_and_heads_match_a_brute_force(pyref):
    rng = random.Random(47)
    cases = []
    for policy, H, agg in SHAPES:
        for leaf_first in (0, 1):
            for b in ((0, 1, 2) if H == 1 else (0, 1, 2, 9, 20) if H == 6 else (1, 5)):
                for _ in range(3 if H == 6 and b > 2 else 1):
                    cases.append(make_case(pyref, rng, policy, H, agg, 8 if H != 33 else 64, leaf_first, b))
    # directed: H = 6, padding / 3, the run of rows 0-3 of sub-proof 0 with one covered byte flipped in its first, middle and last row
    for e in (0, 1, 3):
        c = make_case(pyref, random.Random(1), 0, 6, 3, 8, 0, 0)
        c.idx, c.b = [0, 1, 2, 3, 16, 17, 40, 63], 8
        c.coms = [b"\x11" * 192] * 8
        c.coms[e] = b"\x11" * 40 + b"\x12" + b"\x11" * 151
        c.first, c.count = 0, 8
        cases.append(c)
    got = _replay([c.line() for c in cases])
    for c, g in zip(cases, got):
        c.check(g)
    # among them: corrupted commitments that make heads where the keys repeat, and windows that are refused
    assert any(g["hflag"] != g["kflag"] for g in got)
    assert sum(g["hflag"][:8] != g["kflag"][:8] for g in got[-3:]) == 3
    assert [sum(g["hflag"]) - sum(g["kflag"]) for g in got[-3:]] == [1, 2, 1]


def test_a_refused_window_and_a_bad_plan():
    got = _replay(["0 6 3 8 0 2 4 5 " + "00" * 384 + " 1 2", "0 6 3 8 0 2 4 5 " + "00" * 384 + " 3 0",
                   "2 6 1 8 0 0 - 0 0", "0 6 7 8 0 0 - 0 0", "0 6 3 12 0 0 - 0 0"])
    assert [g.get("window_ok") for g in got[:2]] == [0, 0] and [g["plan"] for g in got] == [1, 1, 0, 0, 0]
