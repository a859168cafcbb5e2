"""dapol_reprove_batches: after an edit of the tree only the sub-proofs of the batches whose sibling commitments moved are proved again.

The definition is dapol_prove_batches on the edited tree, so every test compares against a fresh call of it: siblings and range blobs
byte for byte.  The call mixes, interleaved in caller order, single leaves, batches of 2, 3 and 5 leaves, a sibling pair, a full
4-leaf subtree and repeated batches.  Scenario A is one dapol_tree_apply that replaces leaf 44, inserts a new leaf 2 and removes
leaf 57: the caller drops the batches that hold 57 and adds two batches around leaf 2 that have no old proof.  Scenario B replaces
leaf 21 alone: every batch without 21 then has exactly one dirty sub-proof, and the list is chosen so that [20, 22] is the only batch
whose dirty sibling lies among the four nearest the leaves -- one class of m then gets one dirty row and the other more than 33."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
OTHER_SEED = bytes(range(100, 132))
H = 6
LEAVES = [1, 5, 9, 12, 17, 20, 21, 22, 23, 26, 30, 33, 37, 40, 44, 47, 50, 54, 57, 60, 63]
# (policy, aggregation, n_bits, leaf_first): padding at 0 and at the smallest S (4); splitting at 3 = 2 + 1; both sibling orders; 64 bits once
CONFIGS = [(0, 0, 8, 0), (0, 4, 8, 0), (1, 3, 8, 0), (0, 0, 8, 1), (0, 4, 8, 1), (1, 3, 8, 1), (1, 3, 64, 0)]


def _batches():
    singles = [[x] for x in (1, 5, 9, 12, 21, 33, 37, 40, 44, 47, 50, 54, 57, 60, 63)]
    singles += singles[:10]                                                          # ten of them twice
    others = [[20, 22],                                                              # the one batch without 21 that has a leaf beside it
              [20, 21], [20, 21, 22], [20, 21], [21, 23],                            # a sibling pair (twice), k = 3 with S = 5, k = 2 with S = 5
              [20, 21, 22, 23],                                                      # a full subtree: S = 4
              [1, 5], [1, 63], [1, 33, 44], [9, 40, 63], [5, 9], [12, 33], [47, 50], [54, 60], [37, 40], [50, 57], [44, 47, 60],
              [1, 5, 9, 12, 33], [20, 21, 22, 23, 26], [33, 37, 40, 44, 47]]
    mixed = singles + others
    order = np.random.default_rng(5).permutation(len(mixed))
    return [mixed[i] for i in order]


BATCHES = _batches()


def _blindings(rng, n):
    r = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    r[:, 31] &= 0x0F
    return r


def _new_tree(hip_lib, ctx):
    rng = np.random.default_rng(17)
    idx = np.array(LEAVES, np.uint64)
    v = rng.integers(0, 4, size=len(LEAVES)).astype(np.uint64)
    return hip_lib.Tree(ctx, H, idx, v, _blindings(rng, len(LEAVES)), SEED)


def _edit(tree, scenario):
    rng = np.random.default_rng(23)
    if scenario == "A":
        was_new = tree.apply([57], [44, 2], [3, 1], _blindings(rng, 2))
        assert was_new.tolist() == [False, True]
    elif scenario == "B":
        tree.update([21], [2], _blindings(rng, 1))


EDITED = {"A": [2, 44, 57], "B": [21], "none": []}


class _Old:
    """Proofs in batches_plan's layout, and how to cut the rows of some batches out of them."""

    def __init__(self, out):
        self.so, self.ro, self.sC, self.sH, self.blob = out[:5]

    def rows(self, keep, fill=0xEE):
        """The layout of a new batch list: keep[j] = row of this call that batch j had, or None (its old rows are filled with junk)."""
        sC, blob = [], []
        for j, size in keep:
            if j is None:
                sC.append(np.full((size[0], 32), fill, np.uint8))
                blob.append(np.full(size[1], fill, np.uint8))
            else:
                sC.append(self.sC[int(self.so[j]):int(self.so[j + 1])])
                blob.append(self.blob[int(self.ro[j]):int(self.ro[j + 1])])
        return np.concatenate(sC).reshape(-1, 32), np.concatenate(blob)


class _Scenario:
    """One edit of one tree: the old proofs of every configuration (taken before the edit), the batch list after it with its old rows
    aligned, and the fresh proofs of the edited tree.  Everything is computed once and never changed."""

    def __init__(self, hip_lib, ctx, name, configs=CONFIGS, seeds=(SEED,)):
        self.name, self.hip_lib = name, hip_lib
        self.tree = _new_tree(hip_lib, ctx)
        old = {}
        for cfg in configs:
            for seed in seeds:
                old[cfg, seed] = _Old(self._fresh(BATCHES, cfg, seed))
        _edit(self.tree, name)
        self.root = self.tree.root()
        if name == "A":                                            # the batches that lost leaf 57 go, two around the new leaf 2 come
            keep = [j for j, b in enumerate(BATCHES) if 57 not in b]
            self.batches = [BATCHES[j] for j in keep]
            self.rows = list(keep)
            for at, b in ((3, [2]), (17, [1, 2, 5])):
                self.batches.insert(at, b)
                self.rows.insert(at, None)
            self.has_old = [int(j is not None) for j in self.rows]
        else:
            self.batches, self.rows, self.has_old = BATCHES, list(range(len(BATCHES))), None
        self.fresh, self.old = {}, {}
        for cfg in configs:
            self.fresh[cfg] = _Old(self._fresh(self.batches, cfg, SEED))
            f = self.fresh[cfg]
            sizes = [(int(f.so[j + 1] - f.so[j]), int(f.ro[j + 1] - f.ro[j])) for j in range(len(self.batches))]
            for seed in seeds:
                self.old[cfg, seed] = old[cfg, seed].rows(list(zip(self.rows, sizes)))

    def _fresh(self, batches, cfg, seed):
        policy, agg, n_bits, leaf_first = cfg
        saved = self.hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
        try:
            return self.tree.prove_batches(batches, policy, agg, n_bits, seed)
        finally:
            self.hip_lib.wire_config_restore(saved)

    def reprove(self, cfg, old=None, seed=SEED, has_old="scenario", **kw):
        policy, agg, n_bits, leaf_first = cfg
        oC, oR = self.old[cfg, SEED] if old is None else old
        saved = self.hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
        try:
            return self.tree.reprove_batches(self.batches, oC, oR, policy, agg, n_bits, seed, has_old=self.has_old if has_old == "scenario" else has_old, **kw)
        finally:
            self.hip_lib.wire_config_restore(saved)

    def plan(self, cfg, has_old="scenario", edited=None):
        policy, agg, n_bits, leaf_first = cfg
        saved = self.hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
        try:
            return self.hip_lib.reprove_batches_plan(H, self.batches, EDITED[self.name] if edited is None else edited, policy, agg, n_bits,
                                                     self.has_old if has_old == "scenario" else has_old)
        finally:
            self.hip_lib.wire_config_restore(saved)

    def subproofs(self, cfg, j):
        """[(first byte, last byte + 1, m, first sibling, siblings)] of the sub-proofs of batch j inside the blob of the call, in plan order."""
        policy, agg, n_bits, leaf_first = cfg
        S = int(self.fresh[cfg].so[j + 1] - self.fresh[cfg].so[j])
        if policy == 0:
            plan = [(0, agg, 1 << max(agg - 1, 0).bit_length())]
        else:
            plan, pos = [], 0
            for i in range(agg.bit_length() - 1, -1, -1):
                if agg >> i & 1:
                    plan.append((pos, 1 << i, 1 << i))
                    pos += 1 << i
        plan += [(i, 1, 1) for i in range(agg, S)]
        at, out = int(self.fresh[cfg].ro[j]), []
        for start, count, m in plan:
            size = self.hip_lib.lib().dapol_range_proof_size(n_bits, m)
            out.append((at, at + size, m, start, count))
            at += size
        assert at == int(self.fresh[cfg].ro[j + 1])
        return out

    def subproof_over(self, cfg, j, leaf):
        """the sub-proof of batch j that holds the sibling above `leaf` (which is no leaf of the batch)"""
        saved = self.hip_lib.wire_config_set(siblings_leaf_first=cfg[3])
        try:
            level, index = self.hip_lib.batch_siblings(H, np.array(self.batches[j], np.uint64))
        finally:
            self.hip_lib.wire_config_restore(saved)
        (sib,) = [i for i, (l, x) in enumerate(zip(level, index)) if (leaf >> int(l)) == int(x)]
        (sub,) = [i for i, (_, _, _, start, count) in enumerate(self.subproofs(cfg, j)) if start <= sib < start + count]
        return sub


@pytest.fixture(scope="module")
def scen(hip_lib, gpu_ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Scenario(hip_lib, gpu_ctx, name, seeds=(SEED, OTHER_SEED) if name == "B" else (SEED,))
        return made[name]
    yield get
    for s in made.values():
        s.tree.close()


def _dirty_rows_by_m(s, cfg):
    """dirty sub-proofs per m, from the plan call's totals (two classes at most in these configurations: m = 1 and one larger m)"""
    policy, agg, n_bits, _ = cfg
    n_proved, tot, sm, sm_all = s.plan(cfg)
    big = 1 << max(agg - 1, 0).bit_length()
    if big == 1:
        return {1: tot}
    assert policy == 0
    return {big: (sm - tot) // (big - 1), 1: tot - (sm - tot) // (big - 1)}


def test_the_calls_have_the_shapes_they_are_meant_to_have(hip_lib, scen):
    assert len(BATCHES) >= 40 and {len(b) for b in BATCHES} >= {1, 2, 3, 5}
    assert BATCHES.count([20, 21]) == 2 and [20, 21, 22, 23] in BATCHES and [20, 22] in BATCHES
    k = [len(b) for b in BATCHES]
    assert any(k[i] != k[i + 1] for i in range(len(k) - 1)) and sorted(k) != k      # interleaved, not grouped by the caller
    b = scen("B")
    without = sum(21 not in x for x in BATCHES)
    assert _dirty_rows_by_m(b, (0, 0, 8, 0)) == {1: without} and without > 33        # the class m = 1 past the small-call gates of the prover
    assert _dirty_rows_by_m(b, (0, 4, 8, 0)) == {4: without - 1, 1: 1}               # a class of exactly one row: [20, 22]'s last proof
    assert _dirty_rows_by_m(b, (0, 4, 8, 1)) == {4: 1, 1: without - 1}               # leaf first it is the aggregated proof
    a = scen("A")
    assert a.has_old.count(0) == 2 and len(a.batches) == len(BATCHES) - sum(57 in x for x in BATCHES) + 2 >= 40
    assert all(57 not in x for x in a.batches) and any(2 in x for x in a.batches)
    n_proved, tot, sm, sm_all = a.plan((0, 4, 8, 0))
    assert 0 < tot and sm < sm_all and all(int(n_proved[j]) == len(a.subproofs((0, 4, 8, 0), j)) for j, h in enumerate(a.has_old) if not h)


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "p%d-a%d-n%d-lf%d" % c)
def test_bytes_equal_a_fresh_prove_batches(hip_lib, scen, cfg, name):
    s = scen(name)
    f = s.fresh[cfg]
    so, ro, sC, sH, blob, proved, kept, calls = s.reprove(cfg)
    assert so.tolist() == f.so.tolist() and ro.tolist() == f.ro.tolist()
    assert sC.tobytes() == f.sC.tobytes() and sH.tobytes() == f.sH.tobytes(), "siblings"
    for j in range(len(s.batches)):
        r0, r1 = int(ro[j]), int(ro[j + 1])
        assert blob[r0:r1].tobytes() == f.blob[r0:r1].tobytes(), (j, s.batches[j], "range blob")
    n_proved, tot, sm, sm_all = s.plan(cfg)
    n_pairs = sum(len(s.subproofs(cfg, j)) for j in range(len(s.batches)))
    assert proved == tot and kept == n_pairs - tot and proved > 0 and kept > 0
    distinct_m = {sub[2] for j in range(len(s.batches)) for sub in s.subproofs(cfg, j)}
    assert 1 <= calls <= len(distinct_m)
    # three batches against the single-batch call: one of one leaf, the sibling pair, five leaves
    policy, agg, n_bits, leaf_first = cfg
    saved = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        for b in ([1], [20, 21], [1, 5, 9, 12, 33]):
            j = s.batches.index(b)
            _, _, wC, wH, wb = s.tree.prove_batch(np.array(b, np.uint64), policy, agg, n_bits, SEED)
            s0, s1, r0, r1 = int(so[j]), int(so[j + 1]), int(ro[j]), int(ro[j + 1])
            assert sC[s0:s1].tobytes() == wC.tobytes() and sH[s0:s1].tobytes() == wH.tobytes() and blob[r0:r1].tobytes() == wb, (b, "prove_batch")
    finally:
        hip_lib.wire_config_restore(saved)


def _changed(s, cfg, j, old_blob, new_blob):
    """which sub-proofs of batch j differ between two blobs of the call"""
    return [i for i, (a, z, *_) in enumerate(s.subproofs(cfg, j)) if old_blob[a:z].tobytes() != new_blob[a:z].tobytes()]


@pytest.mark.parametrize("cfg", [(0, 0, 8, 0), (0, 4, 8, 0), (0, 4, 8, 1)], ids=lambda c: "p%d-a%d-n%d-lf%d" % c)
def test_one_replaced_leaf_dirties_one_sub_proof_of_every_other_batch(hip_lib, scen, cfg):
    s = scen("B")
    oC, oR = s.old[cfg, SEED]
    so, ro, sC, sH, blob, proved, kept, calls = s.reprove(cfg)
    n_proved = s.plan(cfg)[0]
    for j, b in enumerate(BATCHES):
        changed = _changed(s, cfg, j, oR, blob)
        assert len(changed) == int(n_proved[j]) == (0 if 21 in b else 1), (j, b, changed)
    j = BATCHES.index([20, 22])
    subs = s.subproofs(cfg, j)
    assert _changed(s, cfg, j, oR, blob) == [s.subproof_over(cfg, j, 21)]
    if cfg[3] == 0:                                               # root side first: the leaf-level siblings 21 and 23 (left to right) come last, as
        assert s.subproof_over(cfg, j, 21) == len(subs) - 2 and subs[-2][2] == 1      # individual proofs with the largest slot bases
    else:                                                         # leaf first: sibling 0, inside the aggregated proof
        assert s.subproof_over(cfg, j, 21) == 0 and subs[0][2] == 4
    assert proved == sum(21 not in b for b in BATCHES)


def test_kept_bytes_come_out_as_they_went_in_and_dirty_ones_are_replaced(hip_lib, scen):
    cfg = (0, 4, 8, 0)
    s = scen("B")
    oC, oR = s.old[cfg, SEED]
    j = BATCHES.index([20, 22])
    subs = s.subproofs(cfg, j)
    assert s.subproof_over(cfg, j, 21) == len(subs) - 2
    kept_at, dirty_at = subs[-1][0] + 7, subs[-2][0] + 7           # the last individual proof stays; the one before it is over leaf 21
    tampered = oR.copy()
    tampered[kept_at] ^= 0x40
    tampered[dirty_at] ^= 0x40
    blob = s.reprove(cfg, old=(oC, tampered))[4]
    want = s.fresh[cfg].blob.copy()
    want[kept_at] ^= 0x40                                          # old bytes are not checked: the flip stays
    assert blob.tobytes() == want.tobytes()
    assert blob[dirty_at] == s.fresh[cfg].blob[dirty_at] != tampered[dirty_at]


def test_old_proofs_under_another_seed_stay_valid(hip_lib, gpu_ctx, scen):
    cfg = (0, 4, 8, 0)
    policy, agg, n_bits, _ = cfg
    s = scen("B")
    oC, oR = s.old[cfg, OTHER_SEED]
    assert oR.tobytes() != s.old[cfg, SEED][1].tobytes()
    so, ro, sC, sH, blob, proved, kept, calls = s.reprove(cfg, old=(oC, oR))
    f = s.fresh[cfg]
    for j, b in enumerate(BATCHES):
        dirty = _changed(s, cfg, j, oR, blob)
        for i, (a, z, *_) in enumerate(s.subproofs(cfg, j)):
            if i in dirty:
                assert blob[a:z].tobytes() == f.blob[a:z].tobytes(), (j, i, "a dirty piece is the fresh one under the new seed")
            else:
                assert blob[a:z].tobytes() == oR[a:z].tobytes()
        assert len(dirty) == (0 if 21 in b else 1)
    assert proved == sum(21 not in b for b in BATCHES)
    # the mixture verifies against the edited tree's root
    rng = np.random.default_rng(17)
    v = rng.integers(0, 4, size=len(LEAVES)).astype(np.uint64)
    r = _blindings(rng, len(LEAVES))
    v[LEAVES.index(21)], r[LEAVES.index(21)] = 2, _blindings(np.random.default_rng(23), 1)[0]
    lC, lH = gpu_ctx.commit_hash_batch(v, r)
    sel = [LEAVES.index(x) for b in BATCHES for x in b]
    ok = gpu_ctx.verify_batches(H, BATCHES, lC[sel], lH[sel], so, sC, sH, s.root[0], s.root[1], policy, agg, n_bits, ro, blob, verify_seed=SEED)
    assert ok.tolist() == [1] * len(BATCHES)


@pytest.mark.parametrize("cfg", [(0, 4, 8, 0), (1, 3, 8, 1)], ids=lambda c: "p%d-a%d-n%d-lf%d" % c)
def test_without_old_proofs_the_call_is_prove_batches(hip_lib, scen, cfg):
    s = scen("B")
    f = s.fresh[cfg]
    n_pairs = sum(len(s.subproofs(cfg, j)) for j in range(len(BATCHES)))
    so, ro, sC, sH, blob, proved, kept, calls = s.reprove(cfg, old=(None, None), has_old=[0] * len(BATCHES))
    assert sC.tobytes() == f.sC.tobytes() and sH.tobytes() == f.sH.tobytes() and blob.tobytes() == f.blob.tobytes()
    assert (proved, kept) == (n_pairs, 0)
    # a mix: every third batch has no old proof, and junk where its old rows would be
    flags = [int(j % 3 != 0) for j in range(len(BATCHES))]
    oC, oR = s.old[cfg, SEED]
    jC, jR = oC.copy(), oR.copy()
    for j, has in enumerate(flags):
        if not has:
            jC[int(so[j]):int(so[j + 1])] = 0xEE
            jR[int(ro[j]):int(ro[j + 1])] = 0xEE
    out = s.reprove(cfg, old=(jC, jR), has_old=flags)
    assert out[2].tobytes() == f.sC.tobytes() and out[4].tobytes() == f.blob.tobytes()
    assert out[5] == s.plan(cfg, has_old=flags)[1] and out[5] + out[6] == n_pairs


def test_no_edit_proves_nothing(hip_lib, gpu_ctx):
    cfg = (0, 4, 8, 0)
    s = _Scenario(hip_lib, gpu_ctx, "none", configs=[cfg])
    try:
        oC, oR = s.old[cfg, SEED]
        so, ro, sC, sH, blob, proved, kept, calls = s.reprove(cfg)
        assert (proved, calls) == (0, 0) and kept == sum(len(s.subproofs(cfg, j)) for j in range(len(BATCHES)))
        assert sC.tobytes() == oC.tobytes() and blob.tobytes() == oR.tobytes() and sH.tobytes() == s.fresh[cfg].sH.tobytes()
        junk = np.full_like(oR, 0x5A)                             # nothing is dirty: whatever bytes went in come out
        assert s.reprove(cfg, old=(oC, junk))[4].tobytes() == junk.tobytes()
    finally:
        s.tree.close()


def test_outputs_may_alias_the_old_arrays(hip_lib, scen):
    cfg = (1, 3, 8, 0)
    s = scen("A")
    oC, oR = s.old[cfg, SEED]
    aC, aR = oC.copy(), oR.copy()
    separate = s.reprove(cfg)
    aliased = s.reprove(cfg, old=(aC, aR), alias=True)
    assert np.shares_memory(aliased[2], aC) and np.shares_memory(aliased[4], aR)
    assert aC.tobytes() == separate[2].tobytes() == s.fresh[cfg].sC.tobytes() and aR.tobytes() == separate[4].tobytes() == s.fresh[cfg].blob.tobytes()
    assert aliased[3].tobytes() == separate[3].tobytes() and aliased[5:] == separate[5:]


def _raw(hip_lib, tree, batches, policy, agg, n_bits, has_old, oC, oR):
    """The C call on sentinel-filled outputs: (status, message, True if no output byte and no counter changed)."""
    lib = hip_lib.lib()
    nb, off, flat = hip_lib._pack_batches(batches)
    C, Hh, out = (np.full(64 * 1024, 0xA5, np.uint8) for _ in range(3))
    counters = [ctypes.c_uint64(0xA5A5) for _ in range(3)]
    seed = np.frombuffer(SEED, np.uint8).copy()
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.dapol_reprove_batches(tree.ctx.h, tree.h, nb, p(off), p(flat), policy, agg, n_bits, p(seed), p(has_old), p(oC), p(oR), p(C), p(Hh), p(out),
                                   *[ctypes.byref(c) for c in counters])
    untouched = bool((C == 0xA5).all() and (Hh == 0xA5).all() and (out == 0xA5).all() and all(c.value == 0xA5A5 for c in counters))
    return rc, lib.dapol_last_error().decode(), untouched


def test_refusals_write_nothing(hip_lib, gpu_ctx, scen):
    cfg = (0, 4, 8, 0)
    s = scen("A")
    oC, oR = s.old[cfg, SEED]
    some = s.batches[:8]
    big_C, big_R = np.zeros((1024, 32), np.uint8), np.zeros(64 * 1024, np.uint8)
    rc, msg, untouched = _raw(hip_lib, s.tree, some + [[50, 57]], 0, 4, 8, None, big_C, big_R)       # 57 was removed: the last batch
    assert (rc, untouched) == (9, True), msg
    rc, msg, untouched = _raw(hip_lib, s.tree, some, 0, 4, 8, None, None, None)                      # has_old = NULL promises old arrays
    assert (rc, untouched) == (8, True) and "old" in msg
    rc, msg, untouched = _raw(hip_lib, s.tree, some, 0, 4, 8, np.array([0] * 7 + [1], np.uint8), None, big_R)
    assert (rc, untouched) == (8, True) and "old" in msg
    # dapol_prove_batches' refusals, its messages, before the old arrays are looked at
    rc, msg, untouched = _raw(hip_lib, s.tree, s.batches, 0, 5, 8, None, None, None)                 # the smallest S is 4
    assert (rc, untouched) == (8, True) and "batch %d:" % s.batches.index([20, 21, 22, 23]) in msg and "aggregation_factor" in msg
    rc, msg, untouched = _raw(hip_lib, s.tree, some, 0, 0, 12, None, None, None)
    assert (rc, untouched) == (8, True) and "n_bits" in msg
    rc, msg, untouched = _raw(hip_lib, s.tree, [[5, 1]], 0, 0, 8, None, None, None)
    assert (rc, untouched) == (8, True) and "batch 0:" in msg and "leaf indexes" in msg
    low = [x for x in LEAVES if x < 32]
    shard = hip_lib.Tree(gpu_ctx, H, np.array(low, np.uint64), np.ones(len(low), np.uint64), _blindings(np.random.default_rng(1), len(low)), SEED, shard_bits=1)
    try:
        rc, msg, untouched = _raw(hip_lib, shard, [[1], [5, 9]], 0, 0, 8, None, big_C, big_R)
        assert (rc, untouched) == (8, True) and "shard" in msg
    finally:
        shard.close()
    wide = hip_lib.Context(0, 8, digest=hip_lib.DIGEST_BLAKE2B)
    try:
        wt = hip_lib.Tree(wide, H, np.array(low, np.uint64), np.ones(len(low), np.uint64), _blindings(np.random.default_rng(1), len(low)), SEED)
        rc, msg, untouched = _raw(hip_lib, wt, [[1], [5, 9]], 0, 0, 8, None, big_C, big_R)
        assert (rc, untouched) == (3, True), msg
        wt.close()
    finally:
        wide.close()
    # an empty call is fine and zeroes the counters
    lib = hip_lib.lib()
    counters = [ctypes.c_uint64(7) for _ in range(3)]
    off, seed = np.zeros(1, np.uint64), np.frombuffer(SEED, np.uint8).copy()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.dapol_reprove_batches(s.tree.ctx.h, s.tree.h, 0, p(off), None, 0, 4, 8, p(seed), None, None, None, None, None, None,
                                     *[ctypes.byref(c) for c in counters]) == 0
    assert [c.value for c in counters] == [0, 0, 0]


@pytest.mark.parametrize("W", [8, 16])
def test_bytes_at_pinned_window_widths(hip_lib, W):
    """RangeArgs::slot_of enters the nonce path that every table width shares: scenario B once more on contexts whose width is pinned."""
    ctx = hip_lib.Context(0, 4, options=hip_lib.Options(window_bits=W, high_half_rows=-1))
    try:
        assert ctx.get_options().window_bits == W
        cfgs = [(0, 4, 8, 0), (1, 3, 8, 1)]
        s = _Scenario(hip_lib, ctx, "B", configs=cfgs)
        try:
            for cfg in cfgs:
                so, ro, sC, sH, blob, proved, kept, calls = s.reprove(cfg)
                assert sC.tobytes() == s.fresh[cfg].sC.tobytes() and blob.tobytes() == s.fresh[cfg].blob.tobytes(), (W, cfg)
                assert proved == sum(21 not in b for b in BATCHES) and kept > 0
        finally:
            s.tree.close()
    finally:
        ctx.close()
