"""dapol_reprove_batches_plan, the host-only planner of dapol_reprove_batches, without a device: declared, exported and bound; its
counts against a brute-force model built from capi.batch_siblings' positions and the policies' plans restated here; the cases an edit
must not dirty; every refusal with its code and the batch it names, in precedence order."""
import ctypes

import numpy as np
import pytest

from test_abi import declared_symbols

TOP = (1 << 64) - 1
# height -> (batches in caller order, edit lists); the batches are tests/test_batches_plan_cpu.py's kind: single leaves, a sibling pair,
# whole subtrees, overlapping and repeated batches, a batch of all 2^H leaves (S = 0)
SHAPES = {
    0: ([[0], [0]], [[], [0]]),
    1: ([[0], [1], [0, 1], [1]], [[], [0], [1], [0, 1]]),
    3: ([list(range(8)), [3], [2, 3], list(range(8)), [4, 5, 6, 7]], [[], [3], [0, 7], [2, 5, 6], list(range(8))]),
    5: ([[7], [6, 7], [8, 9, 10, 11], [6, 7, 9], [7, 9, 30], [6, 7], [31], [0, 31], list(range(16, 32)), [7]],
        [[], [7], [6], [0], [12, 13], [31], [3, 8, 20, 30], list(range(0, 32, 3))]),
    64: ([[0], [1 << 63, TOP], [0, 1], [4, 5, 6, 7], [TOP - 1, TOP], [0, 1], [5, 1 << 40, TOP]],
         [[], [0], [TOP], [1, 1 << 62], [2, 6, 1 << 40, (1 << 63) - 1, 1 << 63, TOP - 1]]),
}


def policy_plan(policy, S, agg):
    """[(start, count, m)] of the policy over S siblings: padding = one proof of the first `agg` siblings padded to a power of two (one
    pad party at aggregation 0), splitting = one proof per set bit of `agg`, largest first; then one proof per remaining sibling."""
    np2 = lambda x: 1 << max(x - 1, 0).bit_length()
    plan = []
    if policy == 0:
        plan.append((0, agg, np2(agg)))
    else:
        pos, base = 0, np2(agg)
        while pos < agg:
            if agg & base:
                plan.append((pos, base, base))
                pos += base
            base >>= 1
    return plan + [(i, 1, 1) for i in range(agg, S)]


def model(hip_lib, height, batches, edited, policy, agg, has_old=None):
    n_proved, sm, sm_all = [], 0, 0
    for j, b in enumerate(batches):
        level, index = hip_lib.batch_siblings(height, b)
        below = [any((x >> int(l)) == int(i) for x in edited) for l, i in zip(level, index)]
        proved = 0
        for start, count, m in policy_plan(policy, len(level), agg):
            dirty = (has_old is not None and not has_old[j]) or any(below[start:start + count])
            proved += dirty
            sm += m * dirty
            sm_all += m
        n_proved.append(proved)
    return n_proved, sum(n_proved), sm, sm_all


def test_reprove_batches_symbols_are_declared_exported_and_bound(hip_lib):
    for s in ("dapol_reprove_batches_plan", "dapol_reprove_batches"):
        assert s in declared_symbols()
        assert hasattr(hip_lib.lib(), s)
        assert s in hip_lib.EXPORTED_SYMBOLS
    assert callable(getattr(hip_lib, "reprove_batches_plan", None))
    assert callable(getattr(hip_lib.Tree, "reprove_batches", None))


@pytest.mark.parametrize("leaf_first", [0, 1])
@pytest.mark.parametrize("height", sorted(SHAPES))
def test_plan_matches_the_brute_force_model(hip_lib, height, leaf_first):
    batches, edits = SHAPES[height]
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        min_S = min(len(hip_lib.batch_siblings(height, b)[0]) for b in batches)
        some_old = [(j * 7 + 1) % 3 != 0 for j in range(len(batches))]
        for policy in (0, 1):
            for agg in sorted({0, min_S}):
                for edited in edits:
                    for has_old in (None, some_old):
                        n_proved, tot, sm, sm_all = hip_lib.reprove_batches_plan(height, batches, edited, policy, agg, 8, has_old)
                        want = model(hip_lib, height, batches, edited, policy, agg, has_old)
                        assert ([int(x) for x in n_proved], tot, sm, sm_all) == want, (height, policy, agg, edited, has_old)
    finally:
        hip_lib.wire_config_restore(old)


def test_the_shapes_dirty_what_they_are_meant_to(hip_lib):
    batches = SHAPES[5][0]
    # an empty edit list proves nothing; without old proofs everything is proved
    n_proved, tot, sm, sm_all = hip_lib.reprove_batches_plan(5, batches, [], 0, 0, 8)
    assert tot == 0 and sm == 0 and not n_proved.any() and sm_all > 0
    n_proved, tot, sm, _ = hip_lib.reprove_batches_plan(5, batches, [], 0, 0, 8, [0] * len(batches))
    assert tot == sum(len(hip_lib.batch_siblings(5, b)[0]) + 1 for b in batches) and sm == sm_all
    # has_old rows of 0 are proved whole, the others follow the edits
    flags = [1] * len(batches)
    flags[2] = 0
    n_proved, tot, _, _ = hip_lib.reprove_batches_plan(5, batches, [], 0, 0, 8, flags)
    assert int(n_proved[2]) == len(hip_lib.batch_siblings(5, batches[2])[0]) + 1 == tot
    # an edited leaf that is a leaf of the batch dirties nothing of that batch: 7 is in batches 0, 1, 3, 4, 5 and 9, and one edit below
    # one sibling of every other batch dirties exactly one sub-proof of it at aggregation 0
    n_proved = [int(x) for x in hip_lib.reprove_batches_plan(5, batches, [7], 0, 0, 8)[0]]
    assert n_proved == [0 if 7 in b else 1 for b in batches]
    # a batch of all 2^H leaves has no sibling: only its pad proof exists, and no edit dirties it
    n_proved, tot, _, sm_all = hip_lib.reprove_batches_plan(3, [list(range(8))], [0, 5], 0, 0, 8)
    assert (int(n_proved[0]), tot, sm_all) == (0, 0, 1)
    assert hip_lib.reprove_batches_plan(3, [list(range(8))], [0, 5], 1, 0, 8)[3] == 0             # splitting at 0: no sub-proof at all
    # aggregation = S: the one proof holds every sibling, nothing can be kept
    n_proved, tot, sm, sm_all = hip_lib.reprove_batches_plan(5, [[7], [9], [30]], [8], 0, 5, 8)
    assert (tot, sm, sm_all) == (3, 24, 24)


def test_no_batches_and_null_outputs(hip_lib):
    n_proved, tot, sm, sm_all = hip_lib.reprove_batches_plan(5, [], [3], 0, 3, 8)
    assert (len(n_proved), tot, sm, sm_all) == (0, 0, 0, 0)
    lib = hip_lib.lib()
    off, leaf, ed = np.array([0, 1, 3], np.uint64), np.array([7, 6, 7], np.uint64), np.array([0], np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.dapol_reprove_batches_plan(5, 2, p(off), p(leaf), None, 1, p(ed), 0, 0, 8, None, None, None, None) == 0
    tot = ctypes.c_uint64(99)
    assert lib.dapol_reprove_batches_plan(5, 2, p(off), p(leaf), None, 1, p(ed), 0, 0, 8, None, ctypes.byref(tot), None, None) == 0 and tot.value == 2
    assert lib.dapol_reprove_batches_plan(5, 2, p(off), p(leaf), None, 0, None, 0, 0, 8, None, ctypes.byref(tot), None, None) == 0 and tot.value == 0


def refused(hip_lib, height, batches, edited=(), policy=0, agg=0, n_bits=8):
    with pytest.raises(hip_lib.DapolError) as e:
        hip_lib.reprove_batches_plan(height, batches, list(edited), policy, agg, n_bits)
    return e.value.code, str(e.value)


def test_refusals_are_dapol_batches_plan_s_then_the_edits(hip_lib):
    for batches, j in (([[3], [2, 1], [5, 5]], 1), ([[32]], 0), ([[7], []], 1), ([[0, 1], [1, 2], [31, 32]], 2)):
        code, msg = refused(hip_lib, 5, batches)
        assert code == 8 and "batch %d:" % j in msg and "leaf indexes" in msg, (batches, msg)
    three = [[7], [6, 7], [8, 9, 10, 11]]                                # S = 5, 4, 3
    for policy in (0, 1):
        for agg, j in ((4, 2), (5, 1), (6, 0), (-1, 0)):
            code, msg = refused(hip_lib, 5, three, (), policy, agg)
            assert code == 8 and "batch %d:" % j in msg and "aggregation_factor" in msg, (policy, agg, msg)
    code, msg = refused(hip_lib, 5, three, (), 0, 3, 7)
    assert code == 8 and "batch 0:" in msg and "n_bits" in msg
    # the edits: strictly increasing and below 2^height
    for edited in ([3, 3], [4, 3], [32], [0, 40]):
        code, msg = refused(hip_lib, 5, three, edited)
        assert code == 8 and "edited" in msg, (edited, msg)
    assert hip_lib.reprove_batches_plan(64, [[0]], [TOP], 0, 0, 8)[1] == 1      # (no bound at height 64)
    # precedence: the height, then the batches (leaf indexes, aggregation_factor, n_bits within one batch), then the edits
    assert refused(hip_lib, 65, [[2, 1]], [3, 3], 0, 99, 7)[0] == 1
    assert refused(hip_lib, -1, [[0]])[0] == 1
    assert "leaf indexes" in refused(hip_lib, 5, [[2, 1]], [3, 3], 0, 99, 7)[1]
    assert "aggregation_factor" in refused(hip_lib, 5, [[7]], [3, 3], 0, 99, 7)[1]
    assert "n_bits" in refused(hip_lib, 5, [[7]], [3, 3], 0, 5, 7)[1]
    code, msg = refused(hip_lib, 5, [[7], [6, 7], [2, 1]], [3, 3], 0, 5)
    assert "batch 1:" in msg and "aggregation_factor" in msg
    # null arguments
    lib = hip_lib.lib()
    assert lib.dapol_reprove_batches_plan(5, 1, None, None, None, 0, None, 0, 0, 8, None, None, None, None) == 8
    off, leaf = np.array([0, 1], np.uint64), np.array([7], np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.dapol_reprove_batches_plan(5, 1, p(off), p(leaf), None, 2, None, 0, 0, 8, None, None, None, None) == 8
    assert "null" in lib.dapol_last_error().decode()
