"""dapol_batches_plan, the host-only planner of dapol_prove_batches / dapol_verify_batches, without a device: declared, exported and
bound; its offsets against a model built batch by batch from capi.batch_siblings and dapol_entity_proof_size; every refusal with its
code and the batch it names, in precedence order."""
import ctypes

import numpy as np
import pytest

from test_abi import declared_symbols

TOP = (1 << 64) - 1
# height -> batches, in caller order: single leaves, a sibling pair, whole subtrees (S = H - log2 k), overlapping and repeated batches
SHAPES = {
    0: [[0], [0]],
    1: [[0], [1], [0, 1], [1]],
    3: [list(range(8)), [3], [2, 3], list(range(8)), [4, 5, 6, 7]],               # all 2^H leaves: S = 0
    5: [[7], [6, 7], [8, 9, 10, 11], [6, 7, 9], [7, 9, 30], [6, 7], [31], [0, 31], list(range(16, 32)), [7]],
    64: [[0], [1 << 63, TOP], [0, 1], [4, 5, 6, 7], [TOP - 1, TOP], [0, 1], [5, 1 << 40, TOP]],
}


def model(hip_lib, height, batches, policy, agg, n_bits):
    lib = hip_lib.lib()
    ns = [len(hip_lib.batch_siblings(height, b)[0]) for b in batches]
    es = [lib.dapol_entity_proof_size(s, policy, agg, n_bits) for s in ns]
    return ns, [0] + list(np.cumsum(ns)), [0] + list(np.cumsum(es)), len(set(ns))


def test_batches_symbols_are_declared_exported_and_bound(hip_lib):
    for s in ("dapol_batches_plan", "dapol_prove_batches", "dapol_verify_batches"):
        assert s in declared_symbols()
        assert hasattr(hip_lib.lib(), s)
        assert s in hip_lib.EXPORTED_SYMBOLS
    assert callable(getattr(hip_lib, "batches_plan", None))
    assert callable(getattr(hip_lib.Tree, "prove_batches", None))
    assert callable(getattr(hip_lib.Context, "verify_batches", None))


@pytest.mark.parametrize("leaf_first", [0, 1])
@pytest.mark.parametrize("height", sorted(SHAPES))
def test_plan_matches_the_batch_by_batch_model(hip_lib, height, leaf_first):
    batches = SHAPES[height]
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        min_S = min(len(hip_lib.batch_siblings(height, b)[0]) for b in batches)
        for policy in (0, 1):
            for agg in sorted({0, min_S}):
                for n_bits in (8, 64):
                    ns, so, ro, ng = hip_lib.batches_plan(height, batches, policy, agg, n_bits)
                    want = model(hip_lib, height, batches, policy, agg, n_bits)
                    assert ([int(x) for x in ns], [int(x) for x in so], [int(x) for x in ro], ng) == want, (height, policy, agg, n_bits)
    finally:
        hip_lib.wire_config_restore(old)


def test_the_shapes_have_the_sibling_counts_they_are_named_for(hip_lib):
    ns = lambda h: [int(x) for x in hip_lib.batches_plan(h, SHAPES[h], 0, 0, 8)[0]]
    assert ns(0) == [0, 0]
    assert ns(3)[:3] == [0, 3, 2] and ns(3)[4] == 1                   # all leaves; one leaf: its path; a pair: H - 1; a subtree of 4: H - 2
    assert ns(5)[:3] == [5, 4, 3] and ns(5)[8] == 1                   # 16 leaves of a subtree at height 5: S = 5 - 4
    assert ns(64)[:4] == [64, 63 + 62, 63, 62]
    assert hip_lib.batches_plan(5, SHAPES[5], 0, 0, 8)[3] == len(set(ns(5))) >= 4


def test_no_batches_and_null_outputs(hip_lib):
    ns, so, ro, ng = hip_lib.batches_plan(5, [], 0, 3, 8)
    assert (len(ns), [int(x) for x in so], [int(x) for x in ro], ng) == (0, [0], [0], 0)
    lib = hip_lib.lib()
    off, leaf = np.array([0, 1, 3], np.uint64), np.array([7, 6, 7], np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.dapol_batches_plan(5, 2, p(off), p(leaf), 0, 0, 8, None, None, None, None) == 0
    ng = ctypes.c_uint64(99)
    assert lib.dapol_batches_plan(5, 2, p(off), p(leaf), 0, 0, 8, None, None, None, ctypes.byref(ng)) == 0 and ng.value == 2


def refused(hip_lib, height, batches, policy=0, agg=0, n_bits=8):
    with pytest.raises(hip_lib.DapolError) as e:
        hip_lib.batches_plan(height, batches, policy, agg, n_bits)
    return e.value.code, str(e.value)


def test_refusals_name_the_first_batch_in_caller_order(hip_lib):
    for batches, j in (([[3], [2, 1], [5, 5]], 1), ([[3], [4, 9], [5, 5]], 2), ([[32]], 0), ([[7], []], 1), ([[], [7]], 0), ([[0, 1], [1, 2], [31, 32]], 2)):
        code, msg = refused(hip_lib, 5, batches)
        assert code == 8 and "batch %d:" % j in msg and "leaf indexes" in msg, (batches, msg)
    code, msg = refused(hip_lib, 0, [[0], [1]])
    assert code == 8 and "batch 1:" in msg
    # aggregation_factor outside [0, S_j]: S = 5, 4, 3 for these three batches
    three = [[7], [6, 7], [8, 9, 10, 11]]
    for policy in (0, 1):
        for agg, j in ((4, 2), (5, 1), (6, 0), (-1, 0)):
            code, msg = refused(hip_lib, 5, three, policy, agg)
            assert code == 8 and "batch %d:" % j in msg and "aggregation_factor" in msg, (policy, agg, msg)
    code, msg = refused(hip_lib, 5, three, 2, 0)                        # no such policy: dapol_prove_batch's refusal, for batch 0
    assert code == 8 and "batch 0:" in msg
    for n_bits in (0, 7, 128):
        code, msg = refused(hip_lib, 5, three, 0, 3, n_bits)
        assert code == 8 and "batch 0:" in msg and "n_bits" in msg


def test_refusals_keep_dapol_prove_batch_precedence(hip_lib):
    # within one batch: leaf indexes, then aggregation_factor, then n_bits
    assert "leaf indexes" in refused(hip_lib, 5, [[2, 1]], 0, 99, 7)[1]
    assert "aggregation_factor" in refused(hip_lib, 5, [[7]], 0, 99, 7)[1]
    assert "n_bits" in refused(hip_lib, 5, [[7]], 0, 5, 7)[1]
    # across batches: the first batch that would be refused, whatever its reason
    code, msg = refused(hip_lib, 5, [[7], [6, 7], [2, 1]], 0, 5)        # batch 1: aggregation 5 > S = 4; batch 2: bad indexes
    assert "batch 1:" in msg and "aggregation_factor" in msg
    code, msg = refused(hip_lib, 5, [[7], [2, 1]], 0, 0, 7)             # batch 0: n_bits; batch 1: bad indexes
    assert "batch 0:" in msg and "n_bits" in msg
    # the height before anything else
    code, msg = refused(hip_lib, 65, [[2, 1]], 0, 99, 7)
    assert code == 1
    assert refused(hip_lib, -1, [[0]])[0] == 1


def raw_plan(hip_lib, height, off, leaf=None, agg=0):
    off = np.array(off, np.uint64)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    lib = hip_lib.lib()
    rc = lib.dapol_batches_plan(height, off.shape[0] - 1, p(off), p(leaf), 0, agg, 8, None, None, None, None)
    return rc, lib.dapol_last_error().decode()


def test_offsets_are_checked_before_any_leaf_is_read(hip_lib):
    """batch_off alone decides these refusals: no leaf array exists behind the offsets (NULL), so reading one would fault."""
    lib = hip_lib.lib()
    assert lib.dapol_batches_plan(5, 1, None, None, 0, 0, 8, None, None, None, None) == 8
    rc, msg = raw_plan(hip_lib, 5, [1, 2])
    assert rc == 8 and "batch_off[0]" in msg
    rc, msg = raw_plan(hip_lib, 5, [0, 3, 2, 4])
    assert rc == 8 and "decrease" in msg
    assert raw_plan(hip_lib, 65, [0, 3, 2])[0] == 1                     # (the height still comes first)
    # sum of k x height >= 2^32: refused from the offsets; one leaf fewer passes this check and only then misses the leaves
    for height in (64, 32, 5, 1):
        bound = -(-(1 << 32) // height)                                  # the smallest leaf count with leaves x height >= 2^32
        rc, msg = raw_plan(hip_lib, height, [0, 1, bound])
        assert rc == 8 and "2^32" in msg, (height, msg)
        rc, msg = raw_plan(hip_lib, height, [0, 0, bound])               # (an empty batch 0 would be refused too: the bound comes first)
        assert rc == 8 and "2^32" in msg
        rc, msg = raw_plan(hip_lib, height, [0, 1, bound - 1])
        assert rc == 8 and "2^32" not in msg and "null" in msg, (height, msg)
    rc, msg = raw_plan(hip_lib, 0, [0, 1 << 40])                         # height 0: no sibling to gather, no bound
    assert rc == 8 and "2^32" not in msg and "null" in msg
