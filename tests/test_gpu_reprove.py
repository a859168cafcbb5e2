"""dapol_reprove_entities_shared: after an edit of the tree only the sub-proofs whose sibling commitments moved are proven again; the
others keep the caller's old bytes.  The tests pin the DEFINITION (include/dapol_hip.h): with old data from
dapol_prove_entities_shared under the same seed the outputs equal a fresh shared call on the edited tree byte for byte, `proved` is
the number of HEADS (dapol_reprove_plan's total where every edit changes its leaf's commitment) and `kept` the number of pairs that are
not dirty.  Expected heads are recomputed here from the old and the new commitments by the HEAD rule, row by row."""
import ctypes

import numpy as np
import pytest

from test_shared_plan_abi import H6_CASES, H6_LEAVES, key_depth, plan_of

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))
N_BITS = 64
ORDERS = [0, 1]                      # dapol_wire_config.siblings_leaf_first
H8_LEAVES = [0, 1, 2, 3, 9, 20, 21, 37, 40, 41, 44, 58, 64, 65, 70, 77, 90, 96, 97, 100, 111, 120, 128, 129, 131, 140, 150, 160, 161, 170, 180, 192,
             200, 210, 220, 230, 240, 250, 254, 255]                   # 40 leaves of the height-8 tree: sibling pairs, lone leaves, both ends
H8_CASES = [(0, 0), (0, 3), (0, 8), (1, 5), (1, 8)]                   # (policy, aggregation_factor): padding 0 / 3 / H, splitting 5 / H


@pytest.fixture(scope="module")
def ctx8(hip_lib):
    c = hip_lib.Context(0, 8)
    yield c
    c.close()


class Live:
    """A tree and the liabilities it holds, edited together."""

    def __init__(self, hip_lib, ctx, H, leaves, seed=1):
        self.ctx, self.H = ctx, H
        self.rng = np.random.default_rng(seed)
        self.leaves = {int(x): self._liability() for x in leaves}
        idx, v, r = self.arrays()
        self.tree = hip_lib.Tree(ctx, H, idx, v, r, SEED)

    def _liability(self):
        r = self.rng.integers(0, 256, size=32, dtype=np.uint8)
        r[31] &= 0x0F
        return int(self.rng.integers(0, 1000)), r

    def arrays(self):
        idx = np.array(sorted(self.leaves), np.uint64)
        return idx, np.array([self.leaves[int(x)][0] for x in idx], np.uint64), np.stack([self.leaves[int(x)][1] for x in idx])

    def _batch(self, xs):
        return np.array(xs, np.uint64), np.array([self.leaves[x][0] for x in xs], np.uint64), np.stack([self.leaves[x][1] for x in xs])

    def update(self, xs):                      # a new value AND a new blinding: the commitment really changes
        for x in xs:
            assert x in self.leaves
            self.leaves[x] = self._liability()
        self.tree.update(*self._batch(xs))

    def insert(self, xs):
        for x in xs:
            assert x not in self.leaves
            self.leaves[x] = self._liability()
        self.tree.insert(*self._batch(xs))

    def remove(self, xs):
        for x in xs:
            del self.leaves[x]
        self.tree.remove(np.array(xs, np.uint64))

    def fresh(self, policy, agg, idx=None):
        idx = self.arrays()[0] if idx is None else idx
        return self.tree.prove_entities_shared(idx, policy, agg, N_BITS, SEED)

    def verdicts(self, policy, agg, pC, pH, blobs):
        idx, v, r = self.arrays()
        lC, lH = self.ctx.commit_hash_batch(v, r)
        root = self.tree.root()
        return self.ctx.verify_entities(self.H, idx, lC, lH, pC, pH, root[0], root[1], policy, agg, N_BITS, blobs, verify_seed=SEED)


def heads_and_kept(pyref, H, policy, agg, leaf_first, idx, has_old, old_C, new_C):
    """The HEAD rule over the bytes: (heads, kept pairs)."""
    heads = kept = 0
    for start, count, _ in plan_of(pyref, policy, H, agg):
        D = key_depth(start, count, H, leaf_first)
        key = lambda x: (int(x) >> (H - D)) if D else 0
        prev = False
        for e, x in enumerate(idx):
            dirty = not has_old[e] or old_C[e, start:start + count].tobytes() != new_C[e, start:start + count].tobytes()
            heads += int(dirty and (e == 0 or key(x) != key(idx[e - 1]) or not prev))
            kept += int(not dirty)
            prev = dirty
    return heads, kept


def reprove_and_check(hip_lib, pyref, live, policy, agg, leaf_first, old, edited):
    """old = (leaf_idx, path_C, blobs) of the shared call before the edit.  Re-proves, compares everything with a fresh shared call on
    the edited tree and with the planner, verifies every entity; returns the new (leaf_idx, path_C, blobs) and `proved`."""
    H = live.H
    idx = live.arrays()[0]
    old_idx, old_C, old_blobs = old
    pC, pH, blobs, proved, kept = live.tree.reprove_entities_shared(idx, old_idx, old_C, old_blobs, policy, agg, N_BITS, SEED)
    fC, fH, fblobs, unique = live.fresh(policy, agg)
    assert pC.tobytes() == fC.tobytes() and pH.tobytes() == fH.tobytes()
    assert blobs.tobytes() == fblobs.tobytes(), (policy, agg, leaf_first, edited)
    has_old = np.isin(idx, old_idx).astype(np.uint8)
    at = np.minimum(np.searchsorted(old_idx, idx), len(old_idx) - 1)
    want_heads, want_kept = heads_and_kept(pyref, H, policy, agg, leaf_first, idx, has_old, old_C[at], fC)
    n_sub, plan_total, sum_m, sum_m_shared = hip_lib.reprove_plan(H, idx, sorted(edited), policy, agg, has_old)
    print("policy %d agg %d leaf_first %d edited %s: proved %d (planner %d, shared %d), kept %d of %d" %
          (policy, agg, leaf_first, sorted(edited), proved, plan_total, unique, kept, len(idx) * len(n_sub)))
    assert (proved, kept) == (want_heads, want_kept)
    assert proved == plan_total
    if agg < H and has_old.all() and len(edited) == 1:
        assert proved < hip_lib.shared_plan(H, idx, policy, agg)[1] == unique       # individual proofs on the lower levels: most are kept
    assert live.verdicts(policy, agg, pC, pH, blobs).all()
    return (idx, pC, blobs), proved


# ------------------------------------------------------------------------------------------------ (1) nothing edited
@pytest.mark.parametrize("leaf_first", ORDERS)
def test_nothing_edited_proves_nothing(hip_lib, pyref, ctx8, leaf_first):
    """Every group has U = 0 (the range prover is not entered) and row 0 of every group is NOT a head."""
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        live = Live(hip_lib, ctx8, 6, H6_LEAVES)
        idx = live.arrays()[0]
        for policy, agg in H6_CASES:
            oC, oH, oblobs, _ = live.fresh(policy, agg)
            pC, pH, blobs, proved, kept = live.tree.reprove_entities_shared(idx, idx, oC, oblobs, policy, agg, N_BITS, SEED)
            assert proved == 0 and kept == len(idx) * len(plan_of(pyref, policy, 6, agg)), (policy, agg)
            assert blobs.tobytes() == oblobs.tobytes() and pC.tobytes() == oC.tobytes() and pH.tobytes() == oH.tobytes()
    finally:
        hip_lib.wire_config_restore(old)


# ------------------------------------------------------------------------------------------------ (2) one liability replaced
@pytest.mark.parametrize("leaf_first", ORDERS)
@pytest.mark.parametrize("policy,agg", H8_CASES)
def test_one_liability_replaced(hip_lib, pyref, ctx8, policy, agg, leaf_first):
    """A leaf in the middle, then the first, then the last; each re-prove feeds the next.  40 leaves x up to 9 sub-proofs: the pairs and
    the blob pieces cross 256-lane blocks."""
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        live = Live(hip_lib, ctx8, 8, H8_LEAVES, seed=2)
        idx = live.arrays()[0]
        oC, _, oblobs, _ = live.fresh(policy, agg)
        state = (idx, oC, oblobs)
        for x in (100, 0, 255):
            live.update([x])
            state, proved = reprove_and_check(hip_lib, pyref, live, policy, agg, leaf_first, state, [x])
            if agg == 8 and policy == 0:
                assert proved == len(idx) - 1                  # one sub-proof over every sibling: only the edited leaf's own is kept
    finally:
        hip_lib.wire_config_restore(old)


# ------------------------------------------------------------------------------------------------ (3) a mixed edit in one go
@pytest.mark.parametrize("leaf_first", ORDERS)
@pytest.mark.parametrize("policy,agg", [(0, 3), (1, 5), (0, 0)])
def test_mixed_edit_in_one_go(hip_lib, pyref, ctx8, policy, agg, leaf_first):
    """insert (8: the sibling of leaf 9; 130: inside the run 128, 129, 131 that nothing else touches; 253: beside the last pair), then remove,
    then update -- and ONE re-prove over all of it.  The Python wrapper aligns the old rows."""
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        live = Live(hip_lib, ctx8, 8, H8_LEAVES, seed=3)
        oC, _, oblobs, _ = live.fresh(policy, agg)
        state = (live.arrays()[0], oC, oblobs)
        live.insert([130, 8, 253])
        live.remove([77, 192])
        live.update([41, 200])
        reprove_and_check(hip_lib, pyref, live, policy, agg, leaf_first, state, [130, 8, 253, 77, 192, 41, 200])
    finally:
        hip_lib.wire_config_restore(old)


# ------------------------------------------------------------------------------------------------ (4) no old data
def test_no_old_data_is_the_shared_call(hip_lib, ctx8):
    live = Live(hip_lib, ctx8, 8, H8_LEAVES, seed=4)
    idx = live.arrays()[0]
    for policy, agg in ((0, 3), (1, 5)):
        fC, fH, fblobs, unique = live.fresh(policy, agg)
        pC, pH, blobs, proved, kept = live.tree.reprove_entities_shared(idx, None, None, None, policy, agg, N_BITS, SEED)     # has_old all zero, old arrays NULL
        assert blobs.tobytes() == fblobs.tobytes() and pC.tobytes() == fC.tobytes() and pH.tobytes() == fH.tobytes()
        assert proved == unique and kept == 0


# ------------------------------------------------------------------------------------------------ (5), (6) old bytes that lie
@pytest.mark.parametrize("leaf_first", ORDERS)
def test_tampered_old_commitments_are_proved_again(hip_lib, pyref, ctx8, leaf_first):
    """A flipped byte of old_path_C32 inside one sub-proof's range of one row makes exactly that (sub-proof, row) dirty: the output is
    still the fresh call's, and `proved` grows by the heads the HEAD rule gives -- a row in the middle of a key run is a head of its own;
    two adjacent rows of a run are one head; the first and the last byte of a range count, the byte after it belongs to a neighbour."""
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        live = Live(hip_lib, ctx8, 8, H8_LEAVES, seed=5)
        idx = live.arrays()[0]
        policy, agg = 0, 3
        plan = plan_of(pyref, policy, 8, agg)
        fC, fH, fblobs, _ = live.fresh(policy, agg)
        for rows, sib, byte in (([1], 0, 0), ([1, 2], 2, 31), ([0], 3, 5), ([39], 7, 31), ([10, 12], 1, 17)):
            bad = fC.copy()
            for e in rows:
                bad[e, sib, byte] ^= 0x40
            has_old = np.ones(len(idx), np.uint8)
            want_heads, want_kept = heads_and_kept(pyref, 8, policy, agg, leaf_first, idx, has_old, bad, fC)
            assert 1 <= want_heads <= len(rows) and want_kept == len(idx) * len(plan) - len(rows)
            pC, pH, blobs, proved, kept = live.tree.reprove_entities_shared(idx, idx, bad, fblobs, policy, agg, N_BITS, SEED)
            assert (proved, kept) == (want_heads, want_kept), (rows, sib)
            assert blobs.tobytes() == fblobs.tobytes() and pC.tobytes() == fC.tobytes()
        # the aggregated proof of rows 0 .. 3 (one key under root-first order): rows 1 and 2 dirty together are ONE head there
        if not leaf_first:
            assert heads_and_kept(pyref, 8, policy, agg, 0, idx, np.ones(len(idx), np.uint8), _flip(fC, [1, 2], 2, 31), fC)[0] == 1
    finally:
        hip_lib.wire_config_restore(old)


def _flip(C, rows, sib, byte):
    bad = C.copy()
    for e in rows:
        bad[e, sib, byte] ^= 0x40
    return bad


def test_kept_bytes_are_kept_unchecked(hip_lib, pyref, ctx8):
    """Old bytes are not checked: a flipped byte of a kept sub-proof comes out flipped, and dapol_verify_entities rejects exactly that
    entity.  (A flipped byte of a DIRTY sub-proof is overwritten.)"""
    live = Live(hip_lib, ctx8, 8, H8_LEAVES, seed=6)
    idx = live.arrays()[0]
    policy, agg = 0, 3
    oC, _, oblobs, _ = live.fresh(policy, agg)
    live.update([100])
    fC, fH, fblobs, _ = live.fresh(policy, agg)
    ps = hip_lib.lib().dapol_range_proof_size(N_BITS, 4)
    e = int(np.nonzero(idx == 255)[0][0])
    assert oC[e, 1:].tobytes() == fC[e, 1:].tobytes() and oC[e, 0].tobytes() != fC[e, 0].tobytes()      # leaf 100 lies below leaf 255's first sibling only
    bad = oblobs.copy()
    bad[e, ps + 700] ^= 0x01              # inside the individual proof of sibling 4: kept
    bad[e, 100] ^= 0x01                   # inside the aggregated proof over siblings 0 .. 2: dirty, proved again
    pC, pH, blobs, proved, kept = live.tree.reprove_entities_shared(idx, idx, oC, bad, policy, agg, N_BITS, SEED)
    want = fblobs.copy()
    want[e, ps + 700] ^= 0x01
    assert blobs.tobytes() == want.tobytes()
    ok = live.verdicts(policy, agg, pC, pH, blobs)
    assert ok.tolist() == [int(i != e) for i in range(len(idx))]


# ------------------------------------------------------------------------------------------------ (7) aliased outputs
def test_outputs_may_alias_the_old_arrays(hip_lib, ctx8):
    live = Live(hip_lib, ctx8, 8, H8_LEAVES, seed=7)
    idx = live.arrays()[0]
    policy, agg = 1, 5
    oC, _, oblobs, _ = live.fresh(policy, agg)
    live.update([41])
    live.insert([8])
    new_idx = live.arrays()[0]
    sC, sH, sblobs, sproved, skept = live.tree.reprove_entities_shared(new_idx, idx, oC, oblobs, policy, agg, N_BITS, SEED)
    at = np.minimum(np.searchsorted(idx, new_idx), len(idx) - 1)
    has_old = (idx[at] == new_idx).astype(np.uint8)
    C, blobs = np.ascontiguousarray(oC[at]), np.ascontiguousarray(oblobs[at])          # the aligned old rows: inputs AND outputs
    seed = np.frombuffer(SEED, np.uint8).copy()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    proved, kept = ctypes.c_uint64(), ctypes.c_uint64()
    rc = hip_lib.lib().dapol_reprove_entities_shared(ctx8.h, live.tree.h, len(new_idx), p(new_idx), policy, agg, N_BITS, p(seed), p(has_old), p(C), p(blobs),
                                                     p(C), None, p(blobs), ctypes.byref(proved), ctypes.byref(kept))
    assert rc == 0 and (proved.value, kept.value) == (sproved, skept)
    assert C.tobytes() == sC.tobytes() and blobs.tobytes() == sblobs.tobytes()
    assert sblobs.tobytes() == live.fresh(policy, agg)[2].tobytes()


# ------------------------------------------------------------------------------------------------ (8) launch boundaries
@pytest.mark.parametrize("leaf_first", ORDERS)
def test_a_single_entity(hip_lib, pyref, ctx8, leaf_first):
    """b = 1: one row, every group at most one head; with an edit under one of its siblings and without."""
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        live = Live(hip_lib, ctx8, 8, H8_LEAVES, seed=8)
        one = np.array([97], np.uint64)
        for policy, agg in ((0, 3), (1, 5)):
            oC, oH, oblobs, _ = live.fresh(policy, agg, one)
            pC, pH, blobs, proved, kept = live.tree.reprove_entities_shared(one, one, oC, oblobs, policy, agg, N_BITS, SEED)
            assert proved == 0 and blobs.tobytes() == oblobs.tobytes()
            live.update([96])                                                # its sibling at the deepest level
            fC, fH, fblobs, _ = live.fresh(policy, agg, one)
            pC, pH, blobs, proved, kept = live.tree.reprove_entities_shared(one, one, oC, oblobs, policy, agg, N_BITS, SEED)
            assert blobs.tobytes() == fblobs.tobytes() and pC.tobytes() == fC.tobytes() and pH.tobytes() == fH.tobytes()
            assert (proved, kept) == heads_and_kept(pyref, 8, policy, agg, leaf_first, one, [1], oC, fC) and proved == 1
            assert proved == hip_lib.reprove_plan(8, one, [96], policy, agg)[1]
    finally:
        hip_lib.wire_config_restore(old)


def test_a_64_byte_digest_context(hip_lib, pyref):
    """Blake2b-512 node hashes: path_H32 is [b][H][64], everything else as before."""
    ctx = hip_lib.Context(0, 8, digest=hip_lib.DIGEST_BLAKE2B)
    try:
        live = Live(hip_lib, ctx, 6, H6_LEAVES, seed=9)
        idx = live.arrays()[0]
        oC, oH, oblobs, _ = live.fresh(0, 3)
        assert oH.shape == (len(idx), 6, 64)
        live.update([17])
        fC, fH, fblobs, _ = live.fresh(0, 3)
        pC, pH, blobs, proved, kept = live.tree.reprove_entities_shared(idx, idx, oC, oblobs, 0, 3, N_BITS, SEED)
        assert blobs.tobytes() == fblobs.tobytes() and pC.tobytes() == fC.tobytes() and pH.tobytes() == fH.tobytes()
        assert proved == hip_lib.reprove_plan(6, idx, [17], 0, 3)[1] < hip_lib.shared_plan(6, idx, 0, 3)[1]
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ (9) refusals
def test_refusals_leave_the_outputs_alone(hip_lib, ctx8):
    live = Live(hip_lib, ctx8, 6, H6_LEAVES, seed=10)
    idx = live.arrays()[0]
    policy, agg = 0, 3
    oC, _, oblobs, _ = live.fresh(policy, agg)
    lib, p = hip_lib.lib(), (lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p))
    seed = np.frombuffer(SEED, np.uint8).copy()
    es = lib.dapol_entity_proof_size(6, policy, agg, N_BITS)
    C, Hh, out = np.full((8, 6, 32), 0xAB, np.uint8), np.full((8, 6, 32), 0xAB, np.uint8), np.full((8, es), 0xAB, np.uint8)
    proved, kept = ctypes.c_uint64(12345), ctypes.c_uint64(54321)

    def call(ctx, ix, has_old, old_C, old_R, pol=policy, a=agg, n=None):
        ix = np.array(ix, np.uint64)
        return lib.dapol_reprove_entities_shared(ctx.h, live.tree.h, len(ix) if n is None else n, p(ix), pol, a, N_BITS, p(seed), p(has_old), p(old_C), p(old_R),
                                                 p(C), p(Hh), p(out), ctypes.byref(proved), ctypes.byref(kept))

    untouched = lambda: (C == 0xAB).all() and (Hh == 0xAB).all() and (out == 0xAB).all() and (proved.value, kept.value) == (12345, 54321)
    for bad in ([1, 0], [2, 2], [0, 16, 3]):                                             # non-increasing indexes
        assert call(ctx8, bad, None, oC, oblobs) == 8 and untouched()
    assert call(ctx8, [0, 1, 5, 16], None, oC, oblobs) == 9 and untouched()              # no liability at leaf 5
    assert call(ctx8, idx, None, None, oblobs) == 8 and untouched()                      # has_old NULL implies old data: the arrays must be there
    assert call(ctx8, idx, None, oC, None) == 8 and untouched()
    some = np.zeros(8, np.uint8)
    some[3] = 1
    assert call(ctx8, idx, some, None, None) == 8 and untouched()                        # one row claims old data
    assert call(ctx8, idx, None, oC, oblobs, a=7) == 8 and untouched()                   # aggregation_factor > H
    assert call(ctx8, idx, None, oC, oblobs, pol=2) == 8 and untouched()
    few = hip_lib.Context(0, 2)                                                          # a context with too few parties: padding / 3 needs 4
    try:
        t2 = hip_lib.Tree(few, 6, *live.arrays(), SEED)
        rc = lib.dapol_reprove_entities_shared(few.h, t2.h, 8, p(idx), policy, agg, N_BITS, p(seed), None, p(oC), p(oblobs), p(C), p(Hh), p(out),
                                               ctypes.byref(proved), ctypes.byref(kept))
        assert rc == 8 and untouched()
        assert call(few, idx, None, oC, oblobs) == 8 and untouched()                     # another context's tree
        t2.close()
    finally:
        few.close()
    assert call(ctx8, idx, None, None, None, n=0) == 0 and (proved.value, kept.value) == (0, 0)       # b = 0 is OK and writes no row
    assert (C == 0xAB).all() and (out == 0xAB).all()
    # the call after the refusals is healthy
    pC, pH, blobs, pr, kp = live.tree.reprove_entities_shared(idx, idx, oC, oblobs, policy, agg, N_BITS, SEED)
    assert pr == 0 and kp == 8 * 4 and blobs.tobytes() == oblobs.tobytes()
