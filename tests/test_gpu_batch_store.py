"""dapol_batch_store: the proofs of dapol_prove_batches for one batch list, kept on the GPU and re-proved in place after edits of the tree.

The definition is dapol_prove_batches on the tree as it is now, so every comparison is against a fresh call of it (bytes), of
dapol_reprove_batches with the store's previous rows as the old data (counters) or of dapol_verify_batches over the rows read back
(verdicts) -- never against the store itself.  The tree, the leaves, the interleaved batch list, the two edits and the configurations
are those of test_gpu_reprove_batches.py."""
import contextlib
import ctypes

import numpy as np
import pytest

from test_gpu_reprove_batches import BATCHES, CONFIGS, EDITED, H, LEAVES, SEED, _Old, _blindings, _edit, _new_tree

pytestmark = pytest.mark.gpu
IDS = lambda c: "p%d-a%d-n%d-lf%d" % c
UNKNOWN_LEAF, INVALID_ARGUMENT, INVALID_DIGEST_SIZE = 9, 8, 3


@contextlib.contextmanager
def _order(hip_lib, cfg):
    saved = hip_lib.wire_config_set(siblings_leaf_first=cfg[3])
    try:
        yield
    finally:
        hip_lib.wire_config_restore(saved)


def _fresh(tree, batches, cfg):
    return _Old(tree.prove_batches(batches, cfg[0], cfg[1], cfg[2], SEED))


def _pairs(hip_lib, batches, cfg, height=H):
    """(batch, sub-proof) pairs of a list: what a refresh proves when nothing is old"""
    return hip_lib.reprove_batches_plan(height, batches, [], cfg[0], cfg[1], cfg[2], has_old=[0] * len(batches))[1]


def _same(store, want):
    C, Hh, blob = store.read()
    return C.tobytes() == want.sC.tobytes() and Hh.tobytes() == want.sH.tobytes() and blob.tobytes() == want.blob.tobytes()


@pytest.fixture(scope="module")
def unedited(hip_lib, gpu_ctx):
    """The fresh proofs of BATCHES on the unedited tree, per configuration: computed once, never changed."""
    tree = _new_tree(hip_lib, gpu_ctx)
    made = {}

    def get(cfg):
        if cfg not in made:
            with _order(hip_lib, cfg):
                made[cfg] = _fresh(tree, BATCHES, cfg)
        return made[cfg]
    yield get
    tree.close()


@contextlib.contextmanager
def _filled(hip_lib, gpu_ctx, cfg, batches=BATCHES):
    """A tree of its own and a store filled with `batches`, under the configuration's sibling order."""
    with _order(hip_lib, cfg):
        tree = _new_tree(hip_lib, gpu_ctx)
        store = hip_lib.BatchStore(tree, cfg[0], cfg[1], cfg[2], SEED)
        try:
            fill = store.refresh(batches)
            yield tree, store, fill
        finally:
            store.close()
            tree.close()


def _reference_counters(hip_lib, tree, batches, old, rows, cfg):
    """dapol_reprove_batches' (proved, kept, n_calls) for `batches`, where batch j has the old row rows[j] of `old` (None: no old proof)."""
    _, so, ro, _ = hip_lib.batches_plan(H, batches, cfg[0], cfg[1], cfg[2])
    sizes = [(int(so[j + 1] - so[j]), int(ro[j + 1] - ro[j])) for j in range(len(batches))]
    oC, oR = old.rows(list(zip(rows, sizes)))
    has_old = None if all(r is not None for r in rows) else [int(r is not None) for r in rows]
    return tree.reprove_batches(batches, oC, oR, cfg[0], cfg[1], cfg[2], SEED, has_old=has_old)[5:8]


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_fill_then_a_refresh_with_nothing_edited(hip_lib, gpu_ctx, unedited, cfg):
    with _filled(hip_lib, gpu_ctx, cfg) as (tree, store, fill):
        want = unedited(cfg)
        n = _pairs(hip_lib, BATCHES, cfg)
        assert store.rows == len(BATCHES) and fill[0] == n and fill[1] == 0 and fill[2] >= 1 and fill[3] == 0
        assert _same(store, want)
        batches, so, ro = store.layout()
        assert batches == BATCHES and so.tolist() == want.so.tolist() and ro.tolist() == want.ro.tolist()
        assert store.refresh() == (0, n, 0, 0) and _same(store, want)                     # the list it holds
        assert store.refresh(BATCHES) == (0, n, 0, 0) and _same(store, want)              # the same list, row for row: in place too
        assert store.refresh() == (0, n, 0, 0) and _same(store, want)                     # (both sibling sets have been the spare by now)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_an_update_and_a_null_list_refresh(hip_lib, gpu_ctx, unedited, cfg):
    with _filled(hip_lib, gpu_ctx, cfg) as (tree, store, fill):
        _edit(tree, "B")
        ref = _reference_counters(hip_lib, tree, BATCHES, unedited(cfg), list(range(len(BATCHES))), cfg)
        proved, kept, calls, moved = store.refresh()
        assert _same(store, _fresh(tree, BATCHES, cfg))
        assert (proved, kept, calls) == ref and moved == 0
        assert proved == sum(21 not in b for b in BATCHES) and kept > 0
        assert store.refresh() == (0, proved + kept, 0, 0) and _same(store, _fresh(tree, BATCHES, cfg))


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_an_apply_that_removes_a_leaf_and_the_list_that_follows_it(hip_lib, gpu_ctx, unedited, cfg):
    with _filled(hip_lib, gpu_ctx, cfg) as (tree, store, fill):
        old = unedited(cfg)
        _edit(tree, "A")
        with pytest.raises(hip_lib.DapolError) as e:                                      # the stored list still holds batches with leaf 57
            store.refresh()
        assert e.value.code == UNKNOWN_LEAF
        assert store.rows == len(BATCHES) and _same(store, old)
        rows = [j for j, b in enumerate(BATCHES) if 57 not in b]
        batches = [BATCHES[j] for j in rows]
        for at, b in ((3, [2]), (17, [1, 2, 5])):
            batches.insert(at, b)
            rows.insert(at, None)
        lowest = [None if r is None else BATCHES.index(BATCHES[r]) for r in rows]          # the continuation: the lowest equal old row
        ref = _reference_counters(hip_lib, tree, batches, old, lowest, cfg)
        proved, kept, calls, moved = store.refresh(batches)
        assert _same(store, _fresh(tree, batches, cfg)) and store.layout()[0] == batches
        assert (proved, kept, calls) == ref and moved == len(batches) - 2 and proved > 0 and kept > 0
        assert store.verify(SEED).tolist() == [1] * len(batches)


def test_a_permutation_and_a_repeated_batch_continue_the_lowest_equal_row(hip_lib, gpu_ctx, unedited):
    cfg = (0, 4, 8, 0)
    with _filled(hip_lib, gpu_ctx, cfg) as (tree, store, fill):
        n = _pairs(hip_lib, BATCHES, cfg)
        perm = [BATCHES[i] for i in np.random.default_rng(3).permutation(len(BATCHES))]
        assert perm != BATCHES
        assert store.refresh(perm) == (0, n, 0, len(BATCHES)) and _same(store, _fresh(tree, perm, cfg))
        more = perm[:9] + [[20, 21], [1, 5, 9, 12, 33]] + perm[9:]                          # both are in the list already ([20, 21] twice)
        n_more = _pairs(hip_lib, more, cfg)
        assert store.refresh(more) == (0, n_more, 0, len(more)) and _same(store, _fresh(tree, more, cfg))
        # rows move AND an edit dirties them: the comparison runs against the commitments the move brought along
        old = _fresh(tree, more, cfg)
        _edit(tree, "B")
        back = more[::-1]
        ref = _reference_counters(hip_lib, tree, back, old, [more.index(b) for b in back], cfg)
        proved, kept, calls, moved = store.refresh(back)
        assert (proved, kept, calls) == ref and moved == len(back) and 0 < proved < n_more
        assert _same(store, _fresh(tree, back, cfg))
        assert store.refresh([]) == (0, 0, 0, 0) and store.rows == 0 and store.verify(SEED).shape == (0,)
        assert store.refresh() == (0, 0, 0, 0) and store.rows == 0
        assert store.refresh(BATCHES)[3] == 0 and _same(store, _fresh(tree, BATCHES, cfg))     # filled again from empty: nothing to continue


def test_a_batch_without_siblings(hip_lib, gpu_ctx):
    """All four leaves of a height-2 tree in one batch: S = 0, and at aggregation 0 its blob is the lone pad proof."""
    rng = np.random.default_rng(41)
    idx = np.arange(4, dtype=np.uint64)
    tree = hip_lib.Tree(gpu_ctx, 2, idx, rng.integers(0, 4, size=4).astype(np.uint64), _blindings(rng, 4), SEED)
    store = hip_lib.BatchStore(tree, 0, 0, 8, SEED)
    try:
        for batches in ([[0, 1, 2, 3]], [[1], [0, 1, 2, 3], [2, 3], [0, 1, 2, 3]]):
            n = _pairs(hip_lib, batches, (0, 0, 8), height=2)
            want = _Old(tree.prove_batches(batches, 0, 0, 8, SEED))
            at = batches.index([0, 1, 2, 3])
            assert want.so[at + 1] == want.so[at] and want.ro[at + 1] > want.ro[at]
            assert store.refresh([]) == (0, 0, 0, 0)                                      # (empty: nothing to continue)
            assert store.refresh(batches)[:2] == (n, 0) and _same(store, want)
            tree.update([1], [3], _blindings(rng, 1))
            proved, kept, calls, moved = store.refresh()
            want = _Old(tree.prove_batches(batches, 0, 0, 8, SEED))
            assert _same(store, want) and moved == 0 and proved + kept == n
            assert proved == sum(len(b) < 4 and 1 not in b for b in batches)              # the siblingless row is kept: zero siblings moved
            qs, qr, C, Hh, blob = store.fetch([at, 0, at])
            r0, r1 = int(want.ro[at]), int(want.ro[at + 1])
            assert blob[:r1 - r0].tobytes() == blob[-(r1 - r0):].tobytes() == want.blob[r0:r1].tobytes()
            assert int(qs[1]) == 0 and int(qs[-1]) == C.shape[0] == int(want.so[1] - want.so[0])
            assert store.verify(SEED).tolist() == [1] * len(batches)
    finally:
        store.close()
        tree.close()


def _raw_fetch(hip_lib, store, rows, outputs=True):
    """The C call on sentinel-filled outputs: (status, True if no output byte changed)."""
    rows = np.asarray(rows, np.uint64)
    C, Hh, out = (np.full(64 * 1024, 0xA5, np.uint8) for _ in range(3))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = hip_lib.lib().dapol_batch_store_fetch(store.h, rows.shape[0], p(rows) if rows.shape[0] else None, *([p(C), p(Hh), p(out)] if outputs else [None] * 3))
    return rc, bool((C == 0xA5).all() and (Hh == 0xA5).all() and (out == 0xA5).all())


@pytest.mark.parametrize("cfg", [(0, 4, 8, 0), (1, 3, 8, 1)], ids=IDS)
def test_fetch_gathers_rows_in_query_order(hip_lib, gpu_ctx, unedited, cfg):
    with _filled(hip_lib, gpu_ctx, cfg) as (tree, store, fill):
        want = unedited(cfg)
        rng = np.random.default_rng(9)
        query = [int(x) for x in rng.integers(0, len(BATCHES), size=70)] + [len(BATCHES) - 1, 0, 0]
        assert len(set(query)) < len(query)
        qs, qr, C, Hh, blob = store.fetch(query)
        _, pso, pro, _ = hip_lib.batches_plan(H, [BATCHES[r] for r in query], cfg[0], cfg[1], cfg[2])
        assert qs.tolist() == pso.tolist() and qr.tolist() == pro.tolist()
        for i, r in enumerate(query):
            s0, s1, r0, r1 = int(want.so[r]), int(want.so[r + 1]), int(want.ro[r]), int(want.ro[r + 1])
            assert C[int(qs[i]):int(qs[i + 1])].tobytes() == want.sC[s0:s1].tobytes(), (i, r)
            assert Hh[int(qs[i]):int(qs[i + 1])].tobytes() == want.sH[s0:s1].tobytes(), (i, r)
            assert blob[int(qr[i]):int(qr[i + 1])].tobytes() == want.blob[r0:r1].tobytes(), (i, r)
        C2, H2, blob2 = store.read(5, 7)
        assert C2.tobytes() == want.sC[int(want.so[5]):int(want.so[12])].tobytes() and H2.tobytes() == want.sH[int(want.so[5]):int(want.so[12])].tobytes()
        assert blob2.tobytes() == want.blob[int(want.ro[5]):int(want.ro[12])].tobytes()
        assert _raw_fetch(hip_lib, store, [0, len(BATCHES), 1]) == (INVALID_ARGUMENT, True)     # row == rows
        assert _raw_fetch(hip_lib, store, []) == (0, True)                                      # k == 0
        assert _raw_fetch(hip_lib, store, query, outputs=False) == (0, True)                    # NULL outputs
        assert hip_lib.lib().dapol_batch_store_read(store.h, len(BATCHES) - 1, 2, None, None, None) == INVALID_ARGUMENT
        assert _same(store, want)


@pytest.mark.parametrize("cfg", [(0, 4, 8, 0), (1, 3, 8, 1), (0, 0, 8, 0)], ids=IDS)
def test_verify_against_the_tree_as_it_is_now(hip_lib, gpu_ctx, cfg):
    policy, agg, n_bits, _ = cfg
    with _filled(hip_lib, gpu_ctx, cfg) as (tree, store, fill):
        rng = np.random.default_rng(17)                                                    # _new_tree's values and blindings
        v = rng.integers(0, 4, size=len(LEAVES)).astype(np.uint64)
        r = _blindings(rng, len(LEAVES))
        sel = [LEAVES.index(x) for b in BATCHES for x in b]

        def reference():
            lC, lH = gpu_ctx.commit_hash_batch(v, r)
            root = tree.root()
            C, Hh, blob = store.read()
            _, so, ro = store.layout()
            return gpu_ctx.verify_batches(H, BATCHES, lC[sel], lH[sel], so, C, Hh, root[0], root[1], policy, agg, n_bits, ro, blob, verify_seed=SEED).tolist()
        assert store.verify(SEED).tolist() == reference() == [1] * len(BATCHES)
        assert store.verify().tolist() == [1] * len(BATCHES)                                # a seed from the OS
        at = LEAVES.index(21)
        before = gpu_ctx.commit_hash_batch(v, r)[0][at].tobytes()
        _edit(tree, "B")
        v[at], r[at] = 2, _blindings(np.random.default_rng(23), 1)[0]
        assert gpu_ctx.commit_hash_batch(v, r)[0][at].tobytes() != before                   # the edit really changes the commitment
        n_proved = hip_lib.reprove_batches_plan(H, BATCHES, EDITED["B"], policy, agg, n_bits)[0]
        stale = store.verify(SEED).tolist()
        assert stale == [int(x == 0) for x in n_proved] == reference()
        assert all(stale[j] == int(21 in b) for j, b in enumerate(BATCHES)) and 0 < sum(stale) < len(BATCHES)
        store.refresh()
        assert store.verify(SEED).tolist() == reference() == [1] * len(BATCHES)


def _raw_refresh(hip_lib, store, batches):
    lib = hip_lib.lib()
    nb, off, flat = hip_lib._pack_batches(batches)
    counters = [ctypes.c_uint64(0xA5A5) for _ in range(4)]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.dapol_batch_store_refresh(store.h, nb, p(off), p(flat), *[ctypes.byref(c) for c in counters])
    return rc, lib.dapol_last_error().decode(), all(c.value == 0xA5A5 for c in counters)


def test_refusals_leave_the_store_as_it_was(hip_lib, gpu_ctx, unedited):
    """Every refusal here is a host-side validation: nothing reaches the device."""
    cfg = (0, 4, 8, 0)
    lib = hip_lib.lib()
    with _filled(hip_lib, gpu_ctx, cfg) as (tree, store, fill):
        want = unedited(cfg)
        some = BATCHES[:8]
        rc, msg, untouched = _raw_refresh(hip_lib, store, some + [[5, 1]])                  # a non-increasing batch
        assert (rc, untouched) == (INVALID_ARGUMENT, True) and "batch 8:" in msg and "leaf indexes" in msg and _same(store, want)
        rc, msg, untouched = _raw_refresh(hip_lib, store, some[:3] + [[]] + some[3:])       # an empty batch
        assert (rc, untouched) == (INVALID_ARGUMENT, True) and "batch 3:" in msg and "leaf indexes" in msg and _same(store, want)
        rc, msg, untouched = _raw_refresh(hip_lib, store, some + [[5, 64]])                 # not below 2^height
        assert (rc, untouched) == (INVALID_ARGUMENT, True) and "batch 8:" in msg and _same(store, want)
        assert lib.dapol_batch_store_refresh(store.h, 3, None, None, None, None, None, None) == INVALID_ARGUMENT and _same(store, want)
        assert store.rows == len(BATCHES) and store.layout()[0] == BATCHES
        saved = hip_lib.wire_config_set(siblings_leaf_first=1)                              # the other sibling order
        try:
            ok = np.full(len(BATCHES), 0xA5, np.uint8)
            assert _raw_refresh(hip_lib, store, some)[0::2] == (INVALID_ARGUMENT, True)
            assert lib.dapol_batch_store_refresh(store.h, 0, None, None, None, None, None, None) == INVALID_ARGUMENT
            assert "siblings_leaf_first" in lib.dapol_last_error().decode()
            assert lib.dapol_batch_store_verify(store.h, None, ok.ctypes.data_as(ctypes.c_void_p)) == INVALID_ARGUMENT and (ok == 0xA5).all()
            assert lib.dapol_batch_store_read(store.h, 0, 1, None, None, None) == INVALID_ARGUMENT
            assert lib.dapol_batch_store_layout(store.h, None, None, None, None) == INVALID_ARGUMENT
        finally:
            hip_lib.wire_config_restore(saved)
        assert _same(store, want)
        assert lib.dapol_tree_destroy(tree.h) == INVALID_ARGUMENT and "store" in lib.dapol_last_error().decode()      # the tree outlives its stores
        assert _same(store, want) and store.refresh() == (0, fill[0], 0, 0)
    # an aggregation factor above the smallest sibling count (the full subtree [20, 21, 22, 23] has 4)
    with _order(hip_lib, cfg):
        tree = _new_tree(hip_lib, gpu_ctx)
        store = hip_lib.BatchStore(tree, 0, 5, 8, SEED)
        try:
            small = [[1], [5], [1, 5], [20, 21], [12, 33], [1, 63], [20, 21]]
            store.refresh(small)
            want = _Old(tree.prove_batches(small, 0, 5, 8, SEED))
            rc, msg, untouched = _raw_refresh(hip_lib, store, BATCHES)
            assert (rc, untouched) == (INVALID_ARGUMENT, True) and "batch %d:" % BATCHES.index([20, 21, 22, 23]) in msg and "aggregation_factor" in msg
            assert store.rows == len(small) and _same(store, want)
        finally:
            store.close()
            tree.close()
    # what _create refuses: a shard tree, a 64-byte digest, NULL arguments
    seed = np.frombuffer(SEED, np.uint8).copy()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    low = [x for x in LEAVES if x < 32]
    shard = hip_lib.Tree(gpu_ctx, H, np.array(low, np.uint64), np.ones(len(low), np.uint64), _blindings(np.random.default_rng(1), len(low)), SEED, shard_bits=1)
    try:
        h = ctypes.c_void_p(0x5A5A)
        assert lib.dapol_batch_store_create(gpu_ctx.h, shard.h, 0, 0, 8, p(seed), ctypes.byref(h)) == INVALID_ARGUMENT and "shard" in lib.dapol_last_error().decode()
        assert h.value == 0x5A5A
        assert lib.dapol_batch_store_create(gpu_ctx.h, shard.h, 0, 0, 8, None, ctypes.byref(h)) == INVALID_ARGUMENT and h.value == 0x5A5A
    finally:
        shard.close()
    wide = hip_lib.Context(0, 8, digest=hip_lib.DIGEST_BLAKE2B)
    try:
        wt = hip_lib.Tree(wide, H, np.array(low, np.uint64), np.ones(len(low), np.uint64), _blindings(np.random.default_rng(1), len(low)), SEED)
        h = ctypes.c_void_p(0x5A5A)
        assert lib.dapol_batch_store_create(wide.h, wt.h, 0, 0, 8, p(seed), ctypes.byref(h)) == INVALID_DIGEST_SIZE and h.value == 0x5A5A
        wt.close()
    finally:
        wide.close()
