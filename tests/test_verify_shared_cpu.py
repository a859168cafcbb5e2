"""dapol_verify_entities_shared without a device: the symbol is declared, exported and bound, a NULL context is an invalid argument,
and the index arithmetic the kernels share with the host (dapol_amd/csrc/verify_shared_plan.inc: spans, groups, the is-head predicate,
ranks, the compact layout, the gather's lanes, the verdict expansion) equals a brute-force restatement written here.
tests/cpp/verify_shared_host.cpp is a host-only build of that file with its own main, run directly under ASan + UBSan: the rows live in
heap buffers of exactly their size, so a read outside a span is an error there."""
import ctypes
import functools
import json
import os
import random
import subprocess

import numpy as np
import pytest
from conftest import ROOT

from test_abi import declared_symbols
from test_shared_plan_abi import plan_of


def test_verify_shared_symbol_is_declared_exported_and_bound(hip_lib):
    s = "dapol_verify_entities_shared"
    assert s in declared_symbols()
    assert hasattr(hip_lib.lib(), s)
    assert s in hip_lib.EXPORTED_SYMBOLS
    assert callable(getattr(hip_lib.Context, "verify_entities_shared", None))


def test_verify_shared_without_a_context_is_an_invalid_argument(hip_lib):
    lib = hip_lib.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    idx, z32, ok = np.array([5], np.uint64), np.zeros(32, np.uint8), np.full(1, 7, np.uint8)
    es = lib.dapol_entity_proof_size(6, 0, 1, 8)
    pC, rp = np.zeros((6, 32), np.uint8), np.zeros(es, np.uint8)
    uniq = ctypes.c_uint64(12345)
    assert lib.dapol_verify_entities_shared(None, 6, 1, p(idx), p(z32), p(z32), 6, p(pC), p(pC), p(z32), p(z32), 0, 1, 8, p(rp), es, p(z32), p(ok),
                                            ctypes.byref(uniq)) == 8
    assert b"null" in lib.dapol_last_error()
    assert ok[0] == 7 and uniq.value == 12345


# ------------------------------------------------------------------------------------------------ the replay
@functools.lru_cache(maxsize=None)
def _exe():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "verify_shared_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I", os.path.join(ROOT, "dapol_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "verify_shared_host.cpp"), "-o", exe], check=True)
    return exe


def _replay(lines):
    r = subprocess.run([_exe()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def proof_bytes(n_bits, m):
    lg = (n_bits * m - 1).bit_length()
    return 32 * (9 + 2 * lg)


class Case:
    """b rows for (policy, H, agg, n_bits): blobs [b][entity bytes], commitments [b][H][32], a verdict per possible head."""

    def __init__(self, pyref, policy, H, agg, n_bits, blobs, coms, verdicts):
        self.policy, self.H, self.agg, self.n_bits = policy, H, agg, n_bits
        self.plan = plan_of(pyref, policy, H, agg)
        self.sizes = [proof_bytes(n_bits, m) for _, _, m in self.plan]
        self.off = [sum(self.sizes[:s]) for s in range(len(self.plan) + 1)]
        self.blobs, self.coms, self.verdicts = blobs, coms, verdicts
        self.b = len(blobs)
        assert all(len(x) == self.off[-1] for x in blobs) and all(len(c) == H * 32 for c in coms)

    def line(self):
        hx = lambda rows: b"".join(rows).hex() or "-"
        return "%d %d %d %d %d %s %s %d %s" % (self.policy, self.H, self.agg, self.n_bits, self.b, hx(self.blobs), hx(self.coms), len(self.verdicts),
                                               " ".join(str(v) for v in self.verdicts))

    def proof(self, e, s):
        return self.blobs[e][self.off[s]:self.off[s + 1]]

    def covered(self, e, s):
        start, count, _ = self.plan[s]
        return self.coms[e][start * 32:(start + count) * 32]

    def check(self, got):
        plan, b = self.plan, self.b
        assert got["plan"] == 1 and got["n_sub"] == len(plan) and got["entity_pieces"] * 16 == self.off[-1]
        assert got["fits"] == 1 and got["forwards"] == int(b * len(plan) <= 64)
        assert [q * 16 for q in got["q0"]] == self.off[:-1] and [p * 16 for p in got["pieces"]] == self.sizes
        assert got["start"] == [st for st, _, _ in plan] and got["count"] == [c for _, c, _ in plan]
        assert got["span"] == [sz // 16 + 2 * c for sz, (_, c, _) in zip(self.sizes, plan)]
        groups = []                                            # runs of equal m: [s0, k, m]
        for s, (_, _, m) in enumerate(plan):
            if groups and groups[-1][2] == m:
                groups[-1][1] += 1
            else:
                groups.append([s, 1, m])
        assert got["g_s0"] == [g[0] for g in groups] and got["g_k"] == [g[1] for g in groups] and got["g_m"] == [g[2] for g in groups]
        assert got["g_pieces"] == [self.sizes[g[0]] // 16 for g in groups] and got["g_q0"] == [self.off[g[0]] // 16 for g in groups]
        # the definition: row e repeats row e - 1 iff the sub-proof's bytes and the commitments it covers are equal
        flag = [int(e == 0 or self.proof(e, s) != self.proof(e - 1, s) or self.covered(e, s) != self.covered(e - 1, s))
                for s in range(len(plan)) for e in range(b)] + [0]
        assert got["flag"] == flag
        rank = list(np.cumsum(flag)) if flag else []
        assert got["rank"] == [int(x) for x in rank]
        if b == 0:
            return
        heads = int(rank[-1])
        first = [int(rank[g[0] * b]) - 1 for g in groups] + [heads]
        assert got["first"] == first
        U = [first[i + 1] - first[i] for i in range(len(groups))]
        assert got["piece_off"] == [sum(U[j] * self.sizes[groups[j][0]] // 16 for j in range(i)) for i in range(len(groups))]
        assert got["party_off"] == [sum(U[j] * groups[j][2] for j in range(i)) for i in range(len(groups))]
        assert got["pieces_total"] == sum(u * self.sizes[g[0]] // 16 for u, g in zip(U, groups))
        assert got["parties_total"] == sum(u * g[2] for u, g in zip(U, groups))
        # every head is copied exactly once, piece by piece, to the row that counts the heads before it inside its group
        want = []
        for gi, (s0, k, m) in enumerate(groups):
            for e in range(b):
                for s in range(s0, s0 + k):
                    if flag[s * b + e]:
                        row = sum(flag[s0 * b:s * b + e])
                        want += [x for piece in range(self.sizes[s] // 16 + 2 * m) for x in (gi, row, piece, s, e)]
        assert got["gather"] == want
        rows = [int(rank[s * b + e]) - 1 for s in range(len(plan)) for e in range(b)]
        assert got["row"] == rows
        # a row's head is the last head at or before it
        for s in range(len(plan)):
            for e in range(b):
                h = max(x for x in range(e + 1) if flag[s * b + x])
                assert rows[s * b + e] == rows[s * b + h]
        assert len(self.verdicts) >= heads
        assert got["ok"] == [int(all(self.verdicts[rows[s * b + e]] for s in range(len(plan)))) for e in range(b)]


SHAPES = [(0, 6, 0, 8), (0, 6, 1, 8), (0, 6, 3, 8), (0, 6, 6, 8), (1, 6, 1, 8), (1, 6, 3, 8), (1, 6, 5, 8), (1, 6, 6, 8), (0, 1, 1, 8), (1, 1, 0, 8),
          (0, 64, 0, 8), (0, 64, 2, 8), (1, 64, 63, 8), (0, 32, 16, 64), (1, 32, 24, 64), (0, 0, 0, 8)]


def random_case(pyref, rng, policy, H, agg, n_bits, b):
    """Rows that mostly copy their predecessor; then single bytes are changed where the predicate has its edges: the first and the last
    byte of a sub-proof, of the commitments it covers, and the bytes just outside them (which belong to a neighbour or to nobody)."""
    proto = Case(pyref, policy, H, agg, n_bits, [], [], [])
    es = proto.off[-1]
    blobs, coms = [], []
    for e in range(b):
        if e and rng.random() < 0.8:
            blob, com = bytearray(blobs[-1]), bytearray(coms[-1])
        else:
            blob, com = bytearray(rng.randbytes(es)), bytearray(rng.randbytes(H * 32))
        for _ in range(rng.choice((0, 0, 1, 1, 2, 5))):
            s = rng.randrange(len(proto.plan))
            start, count, _ = proto.plan[s]
            kind = rng.randrange(7)
            if kind == 0:
                blob[proto.off[s]] ^= 1 << rng.randrange(8)                      # first byte of the proof
            elif kind == 1:
                blob[proto.off[s + 1] - 1] ^= 1 << rng.randrange(8)              # last byte
            elif kind == 2:
                blob[rng.randrange(proto.off[s], proto.off[s + 1])] ^= 1 << rng.randrange(8)
            elif kind == 3 and count:
                com[start * 32] ^= 1 << rng.randrange(8)                         # equal proofs, unequal commitments: first covered byte
            elif kind == 4 and count:
                com[(start + count) * 32 - 1] ^= 1 << rng.randrange(8)           # ... last covered byte
            elif kind == 5 and start + count < H:
                com[(start + count) * 32] ^= 1 << rng.randrange(8)               # the first byte after the covered commitments
            elif kind == 6 and start > 0:
                com[start * 32 - 1] ^= 1 << rng.randrange(8)                     # the last byte before them
        blobs.append(bytes(blob))
        coms.append(bytes(com))
    n_heads_max = b * len(proto.plan)
    verdicts = [int(rng.random() < 0.8) for _ in range(n_heads_max)]
    return Case(pyref, policy, H, agg, n_bits, blobs, coms, verdicts)


def test_plan_flags_ranks_and_verdicts_match_a_brute_force(pyref):
    rng = random.Random(46)
    cases = []
    for policy, H, agg, n_bits in SHAPES:
        big = H >= 32
        for b in ((0, 1, 2, 5) if big else (0, 1, 2, 3, 9, 20)):
            for _ in range(1 if big or b < 2 else 4):
                cases.append(random_case(pyref, rng, policy, H, agg, n_bits, b))
    # directed: one byte apart in the first / the last byte of a span; equal proofs with unequal commitments and the reverse
    for policy, H, agg, n_bits in ((0, 6, 3, 8), (1, 6, 5, 8), (0, 64, 2, 8), (0, 6, 0, 8)):
        proto = Case(pyref, policy, H, agg, n_bits, [], [], [])
        base_b, base_c = rng.randbytes(proto.off[-1]), rng.randbytes(H * 32)
        for s, (start, count, _) in enumerate(proto.plan):
            edits = [("b", proto.off[s]), ("b", proto.off[s + 1] - 1)]
            if count:
                edits += [("c", start * 32), ("c", (start + count) * 32 - 1)]
            if start + count < H:
                edits.append(("c", (start + count) * 32))
            if start:
                edits.append(("c", start * 32 - 1))
            for which, at in edits:
                bb, cc = bytearray(base_b), bytearray(base_c)
                (bb if which == "b" else cc)[at] ^= 0x80
                rows_b, rows_c = [base_b, base_b, bytes(bb), bytes(bb), base_b], [base_c, base_c, bytes(cc), bytes(cc), base_c]
                verdicts = [int(rng.random() < 0.7) for _ in range(5 * len(proto.plan))]
                cases.append(Case(pyref, policy, H, agg, n_bits, rows_b, rows_c, verdicts))
    got = _replay([c.line() for c in cases])
    for c, g in zip(cases, got):
        c.check(g)
    # among them: flags that differ between sub-proofs of one row pair, runs longer than two, and verdict vectors with zeros
    assert any(0 < sum(g["flag"]) < len(g["flag"]) - 1 for g in got if g.get("flag"))
    assert any(0 in g["ok"] and 1 in g["ok"] for g in got if g.get("ok"))


def test_a_bad_policy_aggregation_or_width_has_no_plan():
    got = _replay(["2 6 1 8 0 - - 0 ", "0 6 7 8 0 - - 0 ", "0 6 -1 8 0 - - 0 ", "0 6 3 12 0 - - 0 "])
    assert [g["plan"] for g in got] == [0, 0, 0, 0]


def test_call_size_limits_at_their_boundaries(pyref):
    """b x (plan size + 1) must stay below 2^32 (and b itself): the predicate flips exactly at ceil(2^32 / (n_sub + 1)).  The forwarding
    regime is b x plan size <= 64.  The gather of a group must fit one launch of 256-lane blocks: 2^31 - 1 of them."""
    shapes = [(0, 6, 3, 8), (0, 6, 0, 8), (0, 6, 6, 8), (1, 64, 63, 8), (0, 64, 0, 8), (0, 32, 16, 64)]
    cases = []
    for policy, H, agg, n_bits in shapes:
        plan = plan_of(pyref, policy, H, agg)
        n_sub = len(plan)
        edge = -(-(1 << 32) // (n_sub + 1))                      # the smallest b that no longer fits
        fwd = 64 // n_sub
        for b in (0, 1, fwd, fwd + 1, edge - 1, edge, edge + 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 64) - 1):
            cases.append((policy, H, agg, n_bits, b, plan))
    got = _replay(["limits %d %d %d %d %d" % c[:5] for c in cases])
    seen = set()
    for (policy, H, agg, n_bits, b, plan), g in zip(cases, got):
        n_sub = len(plan)
        assert g["n_sub"] == n_sub
        assert g["fits"] == int(b < (1 << 32) and b * (n_sub + 1) < (1 << 32)), (policy, H, agg, b)
        assert g["forwards"] == int(b * n_sub <= 64), (policy, H, agg, b)
        groups = {}
        for s, (_, _, m) in enumerate(plan):                    # runs of equal m are contiguous in a plan
            groups[m] = groups.get(m, 0) + 1
        lanes = max(b * k * (proof_bytes(n_bits, m) // 16 + 2 * m) for m, k in groups.items())
        if b < (1 << 40):                                        # (beyond that the C arithmetic is modulo 2^64; such calls never fit anyway)
            assert g["gather_fits"] == int(lanes // 256 < 0x7fffffff), (policy, H, agg, b)
        seen.add((g["fits"], g["forwards"]))
    assert seen == {(1, 1), (1, 0), (0, 0)}
