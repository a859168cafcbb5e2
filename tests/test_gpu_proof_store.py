"""dapol_proof_store: the proofs of dapol_prove_entities_shared kept on the device and re-proved in place after an edit of the tree.  The
tests pin the DEFINITION (include/dapol_hip.h): after every refresh the store's rows equal a fresh shared call on the tree as it is now
byte for byte, `proved` / `kept` are what dapol_reprove_entities_shared reports when it is fed the store's previous rows, `moved_rows` is
0 while the leaf set stays and the number of surviving leaves otherwise, and verify() gives dapol_verify_entities' verdicts against the
current tree.  Trees: the height-6 and height-8 ones of the shared-proof and re-prove suites (8 and 40 leaves: every row, group and piece
boundary of the kernels is in play), both sibling orders, Context(0, 8)."""
import ctypes

import numpy as np
import pytest

from test_gpu_reprove import H8_CASES, H8_LEAVES, N_BITS, ORDERS, SEED, Live
from test_shared_plan_abi import H6_CASES, H6_LEAVES, plan_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx8(hip_lib):
    c = hip_lib.Context(0, 8)
    yield c
    c.close()


class wire_order:
    def __init__(self, hip_lib, leaf_first):
        self.lib, self.leaf_first = hip_lib, leaf_first

    def __enter__(self):
        self.old = self.lib.wire_config_set(siblings_leaf_first=self.leaf_first)

    def __exit__(self, *exc):
        self.lib.wire_config_restore(self.old)


def snapshot(store):
    return tuple(a.tobytes() for a in store.read())


def equals_fresh(live, store, policy, agg, idx=None):
    """The store's rows against a fresh shared call over idx (default: every leaf); returns the shared call's `unique`."""
    idx = live.arrays()[0] if idx is None else np.array(idx, np.uint64)
    fC, fH, fblobs, unique = live.fresh(policy, agg, idx)
    sidx, C, H, blobs = store.read()
    assert store.rows == len(idx) and sidx.tolist() == idx.tolist()
    assert C.tobytes() == fC.tobytes() and H.tobytes() == fH.tobytes()
    assert blobs.tobytes() == fblobs.tobytes(), (policy, agg)
    return unique


def stale_verdicts(live, store, policy, agg, edited):
    """verify() of a store that has not been refreshed since `edited` were replaced: dapol_verify_entities' verdicts for the rows read
    back against the tree as it is now.  The root moved, so no row whose path passes an edited leaf verifies -- every row but the edited
    leaves' own: an edit lies below none of its leaf's own siblings, so a lone edited leaf's old path still leads to the new root."""
    idx, C, H, blobs = store.read()
    ok = store.verify(SEED)
    assert ok.tolist() == live.verdicts(policy, agg, C, H, blobs).tolist()
    assert not ok[~np.isin(idx, edited)].any()
    if len(edited) == 1:
        assert ok[np.isin(idx, edited)].all()
    return ok


def refresh_like_the_reprover(live, store, policy, agg, idx=None):
    """One refresh (idx None: every leaf), checked against the re-prover fed with the store's previous rows and against a fresh shared
    call; returns (proved, kept, moved_rows)."""
    old_idx, old_C, _, old_blobs = store.read()
    new_idx = live.arrays()[0] if idx is None else np.array(idx, np.uint64)
    if len(old_idx):
        want = live.tree.reprove_entities_shared(new_idx, old_idx, old_C, old_blobs, policy, agg, N_BITS, SEED)[3:]
    else:
        want = live.tree.reprove_entities_shared(new_idx, None, None, None, policy, agg, N_BITS, SEED)[3:]
    proved, kept, moved = store.refresh(None if idx is None else new_idx)
    assert (proved, kept) == want, (policy, agg, new_idx.tolist())
    assert moved == (0 if old_idx.tolist() == new_idx.tolist() else len(set(old_idx.tolist()) & set(new_idx.tolist())))
    equals_fresh(live, store, policy, agg, new_idx)
    return proved, kept, moved


# ------------------------------------------------------------------------------------------------ (1), (2) fill, then nothing edited
@pytest.mark.parametrize("leaf_first", ORDERS)
@pytest.mark.parametrize("H,leaves,cases", [(6, H6_LEAVES, H6_CASES), (8, H8_LEAVES, H8_CASES)])
def test_fill_then_refresh_with_nothing_edited(hip_lib, pyref, ctx8, H, leaves, cases, leaf_first):
    with wire_order(hip_lib, leaf_first):
        live = Live(hip_lib, ctx8, H, leaves, seed=21)
        for policy, agg in cases:
            store = hip_lib.ProofStore(live.tree, policy, agg, N_BITS, SEED)
            try:
                assert store.rows == 0 and store.entity_bytes == hip_lib.lib().dapol_entity_proof_size(H, policy, agg, N_BITS)
                assert store.verify().shape == (0,)
                proved, kept, moved = store.refresh()
                unique = equals_fresh(live, store, policy, agg)
                assert (proved, kept, moved) == (unique, 0, 0), (policy, agg)
                assert store.verify(SEED).tolist() == [1] * len(leaves)
                before = snapshot(store)
                assert store.refresh() == (0, len(leaves) * len(plan_of(pyref, policy, H, agg)), 0)
                assert snapshot(store) == before
                assert store.refresh(live.arrays()[0]) == (0, len(leaves) * len(plan_of(pyref, policy, H, agg)), 0)     # the same set, spelled out
                assert snapshot(store) == before
            finally:
                store.close()


# ------------------------------------------------------------------------------------------------ (3) update: rows stay in place
@pytest.mark.parametrize("leaf_first", ORDERS)
@pytest.mark.parametrize("policy,agg", H8_CASES)
def test_update_is_reproved_in_place(hip_lib, pyref, ctx8, policy, agg, leaf_first):
    """A leaf in the middle, then the first, then the last, then five at once.  Before the refresh no row verifies but a lone edited
    leaf's own (stale_verdicts)."""
    with wire_order(hip_lib, leaf_first):
        live = Live(hip_lib, ctx8, 8, H8_LEAVES, seed=22)
        store = hip_lib.ProofStore(live.tree, policy, agg, N_BITS, SEED)
        try:
            store.refresh()
            idx = live.arrays()[0]
            for edited in ([100], [0], [255], [3, 40, 41, 129, 240]):
                live.update(edited)
                stale = stale_verdicts(live, store, policy, agg, edited)
                assert len(edited) == 1 or not stale.any()                  # (each of the five has another of them below a sibling)
                proved, kept, moved = refresh_like_the_reprover(live, store, policy, agg)
                assert moved == 0
                assert proved == hip_lib.reprove_plan(8, idx, sorted(edited), policy, agg)[1]
                assert store.verify(SEED).tolist() == [1] * len(idx)
        finally:
            store.close()


# ------------------------------------------------------------------------------------------------ (4) insert / remove: rows move
@pytest.mark.parametrize("leaf_first", ORDERS)
@pytest.mark.parametrize("policy,agg", [(0, 3), (1, 5), (0, 0)])
def test_insert_and_remove_move_rows(hip_lib, pyref, ctx8, policy, agg, leaf_first):
    with wire_order(hip_lib, leaf_first):
        start = [x for x in H8_LEAVES if x not in (0, 255)]
        live = Live(hip_lib, ctx8, 8, start, seed=23)
        store = hip_lib.ProofStore(live.tree, policy, agg, N_BITS, SEED)
        try:
            store.refresh()
            n = len(start)
            for new in ([0], [255], [8], [50, 51]):             # a new first leaf, a new last one, the sibling of leaf 9, a sibling pair
                live.insert(new)
                assert refresh_like_the_reprover(live, store, policy, agg)[2] == n
                n += len(new)
            for gone in ([0], [255], [20], [64, 131, 250]):     # the first, the last, one of the pair 20 / 21, several
                live.remove(gone)
                n -= len(gone)
                assert refresh_like_the_reprover(live, store, policy, agg)[2] == n
            live.remove([77, 192])                              # a mixed sequence, ONE refresh
            live.insert([130, 253])
            live.update([41, 200])
            assert refresh_like_the_reprover(live, store, policy, agg)[2] == n - 2
            assert store.verify(SEED).all() and store.rows == n
        finally:
            store.close()


# ------------------------------------------------------------------------------------------------ (5) explicit subsets
@pytest.mark.parametrize("leaf_first", ORDERS)
@pytest.mark.parametrize("policy,agg", [(0, 3), (1, 5)])
def test_explicit_subsets(hip_lib, pyref, ctx8, policy, agg, leaf_first):
    with wire_order(hip_lib, leaf_first):
        live = Live(hip_lib, ctx8, 8, H8_LEAVES, seed=24)
        store = hip_lib.ProofStore(live.tree, policy, agg, N_BITS, SEED)
        try:
            every2 = H8_LEAVES[::2]
            assert refresh_like_the_reprover(live, store, policy, agg, every2)[1:] == (0, 0)
            assert refresh_like_the_reprover(live, store, policy, agg, H8_LEAVES)[2] == len(every2)            # a superset
            assert refresh_like_the_reprover(live, store, policy, agg, H8_LEAVES[::4])[2] == len(H8_LEAVES[::4])  # a subset
            assert refresh_like_the_reprover(live, store, policy, agg, H8_LEAVES[1::4])[2] == 0                 # a disjoint set
            assert refresh_like_the_reprover(live, store, policy, agg, [97])[2] == int(97 in H8_LEAVES[1::4])    # b == 1
            assert store.refresh([]) == (0, 0, 0) and store.rows == 0                                              # b == 0 with a pointer
            assert [a.shape[0] for a in store.read()] == [0, 0, 0, 0]
            proved, kept, moved = refresh_like_the_reprover(live, store, policy, agg)                             # None again
            assert (kept, moved) == (0, 0) and store.rows == len(H8_LEAVES)
            assert store.verify(SEED).all()
        finally:
            store.close()


# ------------------------------------------------------------------------------------------------ (6) fetch
@pytest.mark.parametrize("leaf_first", ORDERS)
def test_fetch(hip_lib, ctx8, leaf_first):
    with wire_order(hip_lib, leaf_first):
        live = Live(hip_lib, ctx8, 8, H8_LEAVES, seed=25)
        store = hip_lib.ProofStore(live.tree, 0, 3, N_BITS, SEED)
        try:
            held = H8_LEAVES[::2]
            store.refresh(held)
            idx, C, H, blobs = store.read()
            before = snapshot(store)
            row = {int(x): e for e, x in enumerate(idx)}

            def check(query, found, fC, fH, fblobs):
                for i, x in enumerate(query):
                    if x in row:
                        e = row[x]
                        assert found[i] == 1 and fC[i].tobytes() == C[e].tobytes() and fH[i].tobytes() == H[e].tobytes() and fblobs[i].tobytes() == blobs[e].tobytes()
                    else:
                        assert found[i] == 0 and not fC[i].any() and not fH[i].any() and not fblobs[i].any()

            check(held[::-1], *store.fetch(held[::-1]))                              # every row, reversed
            dup = [held[3], held[0], held[3], held[-1], held[3], held[0]]
            check(dup, *store.fetch(dup))
            assert store.fetch(dup)[0].all()
            absent = [held[1], H8_LEAVES[1], held[2], H8_LEAVES[3], 5, held[0]]      # two leaves the store does not hold, one that is no leaf of the tree
            assert 5 not in H8_LEAVES
            found = store.fetch(absent)
            assert found[0].tolist() == [1, 0, 1, 0, 0, 1]
            check(absent, *found)
            assert [a.shape[0] for a in store.fetch([])] == [0, 0, 0, 0]            # k == 0
            assert hip_lib.lib().dapol_proof_store_fetch(store.h, 0, None, None, None, None, None) == 0
            assert snapshot(store) == before
        finally:
            store.close()


# ------------------------------------------------------------------------------------------------ (7) refusals
def test_refusals_leave_the_store_alone(hip_lib, ctx8):
    live = Live(hip_lib, ctx8, 6, H6_LEAVES, seed=26)
    idx = live.arrays()[0]
    policy, agg = 0, 3
    store = hip_lib.ProofStore(live.tree, policy, agg, N_BITS, SEED)
    lib, p = hip_lib.lib(), (lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p))
    seed = np.frombuffer(SEED, np.uint8).copy()
    try:
        store.refresh()
        before = snapshot(store)
        out = (ctypes.c_uint64(11), ctypes.c_uint64(22), ctypes.c_uint64(33))
        for bad in ([1, 0], [2, 2], [0, 16, 3]):                                                        # non-increasing indexes
            a = np.array(bad, np.uint64)
            assert lib.dapol_proof_store_refresh(store.h, len(a), p(a), *map(ctypes.byref, out)) == 8 and snapshot(store) == before
        a = np.array([0, 1, 5, 16], np.uint64)                                                          # no liability at leaf 5
        assert lib.dapol_proof_store_refresh(store.h, len(a), p(a), *map(ctypes.byref, out)) == 9 and snapshot(store) == before
        assert lib.dapol_proof_store_refresh(store.h, 2, None, *map(ctypes.byref, out)) == 8            # rows announced, no pointer
        assert [o.value for o in out] == [11, 22, 33]
        for first, count in ((0, 9), (8, 1), (9, 0), (3, 6)):                                           # read past the end
            with pytest.raises(hip_lib.DapolError) as e:
                store.read(first, count)
            assert e.value.code == 8
        assert lib.dapol_proof_store_read(store.h, 2**63, 2**63, None, None, None, None) == 8           # first + count wraps
        assert [x.shape[0] for x in store.read(8, 0)] == [0, 0, 0, 0]
        # the sibling order flipped after creation: every call refuses, nothing is written
        old = hip_lib.wire_config_set(siblings_leaf_first=1)
        try:
            for call in (store.refresh, store.read, store.verify, lambda: store.fetch(idx), lambda: store.refresh(idx[:3])):
                with pytest.raises(hip_lib.DapolError) as e:
                    call()
                assert e.value.code == 8 and "siblings_leaf_first" in str(e.value)
        finally:
            hip_lib.wire_config_restore(old)
        assert snapshot(store) == before and store.refresh() == (0, 8 * 4, 0)

        # creation: what the re-prover refuses, with its code and message, compared by calling both
        def both(ctx, tree, pol, a, n_bits):
            rc1 = lib.dapol_reprove_entities_shared(ctx.h, tree.h, 0, None, pol, a, n_bits, p(seed), None, None, None, None, None, None, None, None)
            m1 = lib.dapol_last_error()
            h = ctypes.c_void_p(0x1234)
            rc2 = lib.dapol_proof_store_create(ctx.h, tree.h, pol, a, n_bits, p(seed), ctypes.byref(h))
            m2 = lib.dapol_last_error()
            assert rc1 == rc2 == 8 and m1 == m2 and h.value == 0x1234, (pol, a, n_bits, rc1, rc2, m1, m2)

        both(ctx8, live.tree, 2, agg, N_BITS)                                                           # a bad policy
        both(ctx8, live.tree, policy, 7, N_BITS)                                                        # aggregation_factor > H
        both(ctx8, live.tree, policy, agg, 7)                                                           # n_bits
        few = hip_lib.Context(0, 2)                                                                     # padding / 3 needs 4 parties
        try:
            t2 = hip_lib.Tree(few, 6, *live.arrays(), SEED)
            both(few, t2, policy, agg, N_BITS)
            both(few, live.tree, policy, agg, N_BITS)                                                   # another context's tree
            both(few, live.tree, 2, agg, N_BITS)                                                        # ... comes first
            t2.close()
        finally:
            few.close()
        h = ctypes.c_void_p(0x1234)
        assert lib.dapol_proof_store_create(ctx8.h, live.tree.h, policy, agg, N_BITS, None, ctypes.byref(h)) == 8 and h.value == 0x1234
        # a workload's tree does not own its leaves
        w = hip_lib.Workload(ctx8, 6, *live.arrays())
        try:
            w.build(SEED)
            assert lib.dapol_proof_store_create(ctx8.h, w.tree_handle(), policy, agg, N_BITS, p(seed), ctypes.byref(h)) == 8 and h.value == 0x1234
            assert b"own its leaves" in lib.dapol_last_error()
        finally:
            w.close()
        # the tree cannot go while a store is open
        root = live.tree.root()
        with pytest.raises(hip_lib.DapolError) as e:
            live.tree.close()
        assert e.value.code == 8 and live.tree.h and live.tree.root() == root
        assert snapshot(store) == before and store.verify(SEED).all()
        second = hip_lib.ProofStore(live.tree, 1, 5, N_BITS, SEED)                                      # two stores: both must go first
        store.close()
        with pytest.raises(hip_lib.DapolError):
            live.tree.close()
        second.close()
        live.tree.close()
        assert not live.tree.h
    finally:
        store.close()


# ------------------------------------------------------------------------------------------------ (8) a 64-byte digest
def test_a_64_byte_digest_context(hip_lib, pyref):
    """Blake2b-512 node hashes: the hash rows are 64 bytes.  The re-prover accepts such a context (test_gpu_reprove.py), so the store does."""
    ctx = hip_lib.Context(0, 8, digest=hip_lib.DIGEST_BLAKE2B)
    try:
        live = Live(hip_lib, ctx, 6, H6_LEAVES, seed=27)
        store = hip_lib.ProofStore(live.tree, 0, 3, N_BITS, SEED)
        try:
            proved, kept, moved = store.refresh()
            assert store.read()[2].shape == (8, 6, 64)
            assert proved == equals_fresh(live, store, 0, 3) and store.verify(SEED).all()
            live.update([17])
            assert stale_verdicts(live, store, 0, 3, [17]).sum() == 1
            proved, kept, moved = refresh_like_the_reprover(live, store, 0, 3)
            assert moved == 0 and proved == hip_lib.reprove_plan(6, live.arrays()[0], [17], 0, 3)[1]
            live.insert([41])
            assert refresh_like_the_reprover(live, store, 0, 3)[2] == 8
            found, C, H, blobs = store.fetch([41, 5])
            assert found.tolist() == [1, 0] and H.shape == (2, 6, 64) and H[0].tobytes() == store.read()[2][7].tobytes() and not H[1].any()
            assert store.verify(SEED).all()
        finally:
            store.close()
    finally:
        ctx.close()
