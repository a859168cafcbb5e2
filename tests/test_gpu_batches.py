"""dapol_prove_batches / dapol_verify_batches: many multi-leaf inclusion proofs in one call.

The definition is dapol_prove_batch / dapol_verify_batch_checked applied batch by batch, so every test compares against those: siblings
and range blobs byte for byte, verdicts one by one.  The call below mixes, interleaved in caller order, batches of 1, 2, 3 and 5 leaves,
different k with equal sibling counts S, a sibling pair, a full 4-leaf subtree, repeated batches, an S-group of one row and one of more
than 33 rows (past the quad and no-tail small-call gates of the prover)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
H = 6
LEAVES = [1, 5, 9, 12, 17, 20, 21, 22, 23, 26, 30, 33, 37, 40, 44, 47, 50, 54, 57, 60, 63]
HEAVY = 21                                              # the leaf that holds 300 in the forged tree


def _batches():
    singles = [[x] for x in LEAVES] + [[x] for x in LEAVES[:10]]                     # 31 batches of one leaf (S = 6), ten of them twice
    others = [[20, 22], [21, 23], [20, 23],                                         # k = 2 with S = 6: the same group as the single leaves
              [20, 21], [20, 21, 22], [20, 21],                                     # a sibling pair (S = 5), k = 3 with S = 5, the pair again
              [20, 21, 22, 23],                                                     # a full subtree: S = 4, a group of one row
              [1, 5], [1, 63], [1, 30, 44], [17, 23, 63], [1, 5, 9, 12, 17], [20, 21, 22, 23, 26], [33, 37, 40, 44, 47]]
    mixed = singles + others
    order = np.random.default_rng(5).permutation(len(mixed))
    return [mixed[i] for i in order]


BATCHES = _batches()


def _blindings(rng, n):
    r = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    r[:, 31] &= 0x0F
    return r


class _Tree:
    def __init__(self, hip_lib, ctx, heavy_value=None):
        rng = np.random.default_rng(17)
        self.idx = np.array(LEAVES, np.uint64)
        self.v = rng.integers(0, 4, size=len(LEAVES)).astype(np.uint64)
        if heavy_value is not None:
            self.v[LEAVES.index(HEAVY)] = heavy_value
        self.r = _blindings(rng, len(LEAVES))
        self.tree = hip_lib.Tree(ctx, H, self.idx, self.v, self.r, SEED)
        self.root = self.tree.root()
        self.lC, self.lH = ctx.commit_hash_batch(self.v, self.r)
        self.where = {x: i for i, x in enumerate(LEAVES)}

    def leaves_of(self, batches):
        sel = [self.where[x] for b in batches for x in b]
        return self.lC[sel], self.lH[sel]


@pytest.fixture(scope="module")
def honest(hip_lib, gpu_ctx):
    return _Tree(hip_lib, gpu_ctx)


_LOOP = {}


def _loop(t, policy, agg, n_bits, leaf_first=0):
    """The parent route, once per configuration: dapol_prove_batch batch by batch -> [(sib_C, sib_H, blob bytes)]."""
    key = (policy, agg, n_bits, leaf_first)
    if key not in _LOOP:
        _LOOP[key] = [t.tree.prove_batch(np.array(b, np.uint64), policy, agg, n_bits, SEED)[2:] for b in BATCHES]
    return _LOOP[key]


def _fallbacks(hip_lib):
    n = ctypes.c_uint64()
    assert hip_lib.lib().dapol_diag_verify_fallbacks(ctypes.byref(n)) == 0
    return n.value


def test_the_call_has_the_shapes_it_is_meant_to_have(hip_lib):
    ns, _, _, ng = hip_lib.batches_plan(H, BATCHES, 0, 0, 8)
    ns = [int(x) for x in ns]
    rows = {s: ns.count(s) for s in set(ns)}
    assert len(BATCHES) >= 40 and ng == len(rows) >= 3
    assert 1 in rows.values() and max(rows.values()) >= 33
    assert {len(b) for b in BATCHES} >= {1, 2, 3, 5}
    by_S = {}
    for b, s in zip(BATCHES, ns):
        by_S.setdefault(s, set()).add(len(b))
    assert any(len(ks) >= 2 for ks in by_S.values())                                 # two different k with equal S
    assert ns[BATCHES.index([20, 21])] == H - 1 and ns[BATCHES.index([20, 21, 22, 23])] == H - 2
    assert BATCHES.count([20, 21]) == 2
    k = [len(b) for b in BATCHES]
    assert any(k[i] != k[i + 1] for i in range(len(k) - 1)) and sorted(k) != k      # interleaved, not grouped by the caller


# padding at aggregation 0 and at the smallest S (4); splitting at 3 = 2 + 1, a split of two parts; both sibling orders; 64 bits once
@pytest.mark.parametrize("policy,agg,n_bits,leaf_first", [(0, 0, 8, 0), (0, 4, 8, 0), (1, 3, 8, 0), (0, 0, 8, 1), (0, 4, 8, 1), (1, 3, 8, 1), (1, 3, 64, 0)])
def test_bytes_equal_prove_batch(hip_lib, honest, policy, agg, n_bits, leaf_first):
    t = honest
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        want = _loop(t, policy, agg, n_bits, leaf_first)
        so, ro, sC, sH, blob, ng = t.tree.prove_batches(BATCHES, policy, agg, n_bits, SEED)
        plan = hip_lib.batches_plan(H, BATCHES, policy, agg, n_bits)
        assert so.tolist() == plan[1].tolist() and ro.tolist() == plan[2].tolist() and ng == plan[3]
        for j, (wC, wH, wb) in enumerate(want):
            s0, s1, r0, r1 = int(so[j]), int(so[j + 1]), int(ro[j]), int(ro[j + 1])
            assert sC[s0:s1].tobytes() == wC.tobytes() and sH[s0:s1].tobytes() == wH.tobytes(), (j, BATCHES[j], "siblings")
            assert blob[r0:r1].tobytes() == wb, (j, BATCHES[j], "range blob")
        pC, pH, eb = t.tree.prove_entities(t.idx, policy, agg, n_bits, SEED)
        for j, b in enumerate(BATCHES):
            if len(b) != 1:
                continue
            row, s0, s1, r0, r1 = t.where[b[0]], int(so[j]), int(so[j + 1]), int(ro[j]), int(ro[j + 1])
            assert sC[s0:s1].tobytes() == pC[row].tobytes() and sH[s0:s1].tobytes() == pH[row].tobytes()
            assert blob[r0:r1].tobytes() == eb[row].tobytes(), (j, "a batch of one leaf is prove_entities' proof")
    finally:
        hip_lib.wire_config_restore(old)


def test_null_sibling_outputs_and_an_empty_call(hip_lib, honest):
    t = honest
    lib = hip_lib.lib()
    nb, off, flat = hip_lib._pack_batches(BATCHES[:6])
    _, so, ro, _ = hip_lib.batches_plan(H, BATCHES[:6], 0, 4, 8)
    out = np.zeros(int(ro[-1]), np.uint8)
    seed = np.frombuffer(SEED, np.uint8).copy()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.dapol_prove_batches(t.tree.ctx.h, t.tree.h, nb, p(off), p(flat), 0, 4, 8, p(seed), None, None, p(out), None) == 0
    want = b"".join(w[2] for w in _loop(t, 0, 4, 8)[:6])
    assert out.tobytes() == want
    ng = ctypes.c_uint64(7)
    assert lib.dapol_prove_batches(t.tree.ctx.h, t.tree.h, 0, p(off), None, 0, 4, 8, p(seed), None, None, None, ctypes.byref(ng)) == 0 and ng.value == 0


def _raw_prove(hip_lib, tree, batches, policy, agg, n_bits=8):
    """The C call on sentinel-filled outputs: (status, message, True if no output byte changed)."""
    lib = hip_lib.lib()
    nb, off, flat = hip_lib._pack_batches(batches)
    C, Hh, out = (np.full(64 * 1024, 0xA5, np.uint8) for _ in range(3))
    ng = ctypes.c_uint64(0xA5A5)
    seed = np.frombuffer(SEED, np.uint8).copy()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.dapol_prove_batches(tree.ctx.h, tree.h, nb, p(off), p(flat), policy, agg, n_bits, p(seed), p(C), p(Hh), p(out), ctypes.byref(ng))
    untouched = bool((C == 0xA5).all() and (Hh == 0xA5).all() and (out == 0xA5).all() and ng.value == 0xA5A5)
    return rc, lib.dapol_last_error().decode(), untouched


def test_refusals_write_nothing(hip_lib, gpu_ctx, honest):
    t = honest
    some = BATCHES[:8]
    rc, msg, untouched = _raw_prove(hip_lib, t.tree, some + [[20, 21, 24]], 0, 0)           # 24 is no leaf of the tree: the last batch
    assert (rc, untouched) == (9, True), msg
    rc, msg, untouched = _raw_prove(hip_lib, t.tree, BATCHES, 0, 5)                          # the smallest S is 4
    assert (rc, untouched) == (8, True) and "batch %d:" % BATCHES.index([20, 21, 22, 23]) in msg and "aggregation_factor" in msg
    rc, msg, untouched = _raw_prove(hip_lib, t.tree, some, 0, 0, n_bits=12)
    assert (rc, untouched) == (8, True) and "n_bits" in msg
    low = [i for i, x in enumerate(LEAVES) if x < 32]
    shard = hip_lib.Tree(gpu_ctx, H, t.idx[low], t.v[low], t.r[low], SEED, shard_bits=1)
    try:
        rc, msg, untouched = _raw_prove(hip_lib, shard, [[1], [5, 9]], 0, 0)
        assert (rc, untouched) == (8, True) and "shard" in msg
    finally:
        shard.close()
    wide = hip_lib.Context(0, 8, digest=hip_lib.DIGEST_BLAKE2B)
    try:
        wt = hip_lib.Tree(wide, H, t.idx, t.v, t.r, SEED)
        rc, msg, untouched = _raw_prove(hip_lib, wt, [[1], [5, 9]], 0, 0)
        assert (rc, untouched) == (3, True), msg
        with pytest.raises(hip_lib.DapolError) as e:
            wide.verify_batches(H, [[1]], np.zeros((1, 32), np.uint8), np.zeros((1, 64), np.uint8), [0, 0], np.zeros((0, 32), np.uint8), np.zeros((0, 64), np.uint8),
                                bytes(32), bytes(64), 0, 0, 8, [0, 0], np.zeros(0, np.uint8), verify_seed=SEED)
        assert e.value.code == 3
        wt.close()
    finally:
        wide.close()


class _Call:
    """One proved call and what the verifier takes: flat leaves, offsets, siblings, blobs."""

    def __init__(self, t, batches, policy, agg, n_bits):
        self.t, self.batches, self.policy, self.agg, self.n_bits = t, batches, policy, agg, n_bits
        self.so, self.ro, self.sC, self.sH, self.blob, _ = t.tree.prove_batches(batches, policy, agg, n_bits, SEED)
        self.lC, self.lH = t.leaves_of(batches)
        self.loff = np.concatenate([[0], np.cumsum([len(b) for b in batches])]).astype(int)

    def verify(self, ctx, rows=None, **over):
        a = dict(so=self.so, ro=self.ro, sC=self.sC, sH=self.sH, blob=self.blob, lC=self.lC, lH=self.lH)
        a.update(over)
        if rows is not None:                                      # a call of its own over some of the batches
            cut = lambda arr, off: np.concatenate([arr[int(off[j]):int(off[j + 1])] for j in rows])
            new_off = lambda off: np.concatenate([[0], np.cumsum([int(off[j + 1]) - int(off[j]) for j in rows])]).astype(np.uint64)
            a = dict(so=new_off(a["so"]), ro=new_off(a["ro"]), sC=cut(a["sC"], a["so"]), sH=cut(a["sH"], a["so"]), blob=cut(a["blob"], a["ro"]),
                     lC=cut(a["lC"], self.loff), lH=cut(a["lH"], self.loff))
        batches = self.batches if rows is None else [self.batches[j] for j in rows]
        return ctx.verify_batches(H, batches, a["lC"], a["lH"], a["so"], a["sC"], a["sH"], self.t.root[0], self.t.root[1], self.policy, self.agg, self.n_bits,
                                  a["ro"], a["blob"], verify_seed=SEED).tolist()

    def verify_one(self, ctx, j, **over):
        """dapol_verify_batch_checked for batch j of the (possibly tampered) call"""
        a = dict(so=self.so, ro=self.ro, sC=self.sC, sH=self.sH, blob=self.blob, lC=self.lC, lH=self.lH)
        a.update(over)
        s0, s1, r0, r1, l0, l1 = int(a["so"][j]), int(a["so"][j + 1]), int(a["ro"][j]), int(a["ro"][j + 1]), self.loff[j], self.loff[j + 1]
        return int(ctx.verify_batch(H, np.array(self.batches[j], np.uint64), a["lC"][l0:l1], a["lH"][l0:l1], a["sC"][s0:s1], a["sH"][s0:s1], self.t.root[0],
                                    self.t.root[1], self.policy, self.agg, self.n_bits, a["blob"][r0:r1].tobytes(), verify_seed=SEED))


@pytest.fixture(scope="module")
def call(honest):
    return _Call(honest, BATCHES, 0, 4, 8)


def test_the_provers_output_verifies_without_a_fallback(hip_lib, gpu_ctx, call):
    before = _fallbacks(hip_lib)
    assert call.verify(gpu_ctx) == [1] * len(BATCHES)
    assert _fallbacks(hip_lib) == before
    assert [call.verify_one(gpu_ctx, j) for j in range(0, len(BATCHES), 4)] == [1] * len(range(0, len(BATCHES), 4))
    other = _Call(call.t, BATCHES, 1, 3, 8)                        # splitting: two aggregated parts and a run of individual proofs
    assert other.verify(gpu_ctx) == [1] * len(BATCHES)
    assert _fallbacks(hip_lib) == before


def test_four_tampered_batches_fail_and_nothing_else(hip_lib, gpu_ctx, call):
    c = call
    ns = [int(c.so[j + 1] - c.so[j]) for j in range(len(BATCHES))]
    k1 = [j for j, b in enumerate(BATCHES) if len(b) == 1]
    a, b, cc, d = BATCHES.index([1, 30, 44]), k1[3], k1[20], BATCHES.index([20, 21, 22])
    blob, sC, sH, lH = c.blob.copy(), c.sC.copy(), c.sH.copy(), c.lH.copy()
    blob[int(c.ro[a]) + 40] ^= 1                                   # a: one range byte flipped
    sC[int(c.so[b])] = c.sC[int(c.so[b]) + 1]                      # b: a sibling commitment replaced by another valid point
    lH[c.loff[d] + 1, 7] ^= 0x80                                   # d: a leaf hash wrong
    drop = int(c.so[cc + 1]) - 1                                   # cc: the caller holds one sibling record fewer
    sC, sH = np.delete(sC, drop, axis=0), np.delete(sH, drop, axis=0)
    so = c.so.copy()
    so[cc + 1:] -= 1
    over = dict(blob=blob, sC=sC, sH=sH, lH=lH, so=so)
    want = [int(j not in (a, b, cc, d)) for j in range(len(BATCHES))]
    assert len({a, b, cc, d}) == 4 and ns[cc] == H
    assert c.verify(gpu_ctx, **over) == want
    for j in (a, b, cc, d, 0, len(BATCHES) - 1):
        assert c.verify_one(gpu_ctx, j, **over) == want[j], j


def test_a_sibling_that_is_no_point_fails_its_batch_alone(hip_lib, gpu_ctx, call):
    """s = 1 is negative, so no Ristretto encoding: the merge kernel flags the batch whose sibling it is, and no other."""
    c = call
    j = BATCHES.index([1, 5, 9, 12, 17])
    sC = c.sC.copy()
    sC[int(c.so[j + 1]) - 1] = np.frombuffer(bytes([1]) + bytes(31), np.uint8)
    want = [int(i != j) for i in range(len(BATCHES))]
    assert c.verify(gpu_ctx, sC=sC) == want
    assert c.verify_one(gpu_ctx, j, sC=sC) == 0


def test_a_short_blob_fails_alone_though_it_shifts_every_later_offset(hip_lib, gpu_ctx, call):
    """The caller holds 5 bytes fewer of one batch's blob: an invalid proof, and the blobs behind it no longer start at multiples of 16."""
    c = call
    j = 9
    cut = int(c.ro[j + 1])
    blob = np.delete(c.blob, np.arange(cut - 5, cut))
    ro = c.ro.copy()
    ro[j + 1:] -= 5
    want = [int(i != j) for i in range(len(BATCHES))]
    assert c.verify(gpu_ctx, blob=blob, ro=ro) == want
    assert c.verify_one(gpu_ctx, j, blob=blob, ro=ro) == 0 and c.verify_one(gpu_ctx, j + 1, blob=blob, ro=ro) == 1


@pytest.mark.parametrize("policy,agg", [(0, 4), (1, 3), (0, 0)])
def test_a_sibling_out_of_range_is_rejected_by_the_algebra_alone(hip_lib, gpu_ctx, policy, agg):
    """One leaf holds 300 and the proofs are 8-bit: the prover commits to the whole value and proves its low bits, so every proof is
    consistent in its transcript and wrong in one term.  A batch is forged iff a sibling's subtree holds that leaf (the sibling's sum is
    then >= 300), that is iff the leaf is not one of the batch's own."""
    t = _Tree(hip_lib, gpu_ctx, heavy_value=300)
    c = _Call(t, BATCHES, policy, agg, 8)
    want = []
    for b in BATCHES:
        level, index = hip_lib.batch_siblings(H, np.array(b, np.uint64))
        holds = any((HEAVY >> int(l)) == int(i) for l, i in zip(level, index))
        assert holds == (HEAVY not in b)
        want.append(int(not holds))
    assert 0 < sum(want) < len(want)
    assert c.verify(gpu_ctx) == want                              # one combination of many batches
    forged, good = want.index(0), want.index(1)
    for j in (forged, good, BATCHES.index([20, 21, 22, 23]), BATCHES.index([1, 5, 9, 12, 17])):
        assert c.verify(gpu_ctx, rows=[j]) == [want[j]], j         # the batch alone in its call
        assert c.verify_one(gpu_ctx, j) == want[j], j
    rows = [forged, good, good, forged]
    assert c.verify(gpu_ctx, rows=rows) == [want[j] for j in rows]
    t.tree.close()
