"""dapol_shared_plan / dapol_prove_entities_shared in the C ABI, without a device: declared, exported and bound; the plan is host-only
index arithmetic and is checked against a numpy brute force (distinct idx >> (H - D) per sub-proof) under both sibling orders."""
import ctypes

import numpy as np
import pytest

from test_abi import declared_symbols

H6_LEAVES = [0, 1, 2, 3, 16, 17, 40, 63]
H6_CASES = [(0, a) for a in (0, 1, 3, 6)] + [(1, a) for a in (1, 3, 5, 6)]         # (policy, aggregation_factor)


def plan_of(pyref, policy, H, agg):
    """[(start, count, m)] in blob order, as policy_plan.inc lays it (pyref.policy_plan + the individual proofs)."""
    plan, pos = pyref.policy_plan("padding" if policy == 0 else "splitting", H, agg)
    return list(plan) + [(i, 1, 1) for i in range(pos, H)]


def key_depth(start, count, H, leaf_first):
    if count == 0:
        return 0
    return H - start if leaf_first else start + count


def brute_force(pyref, leaves, policy, H, agg, leaf_first):
    out = []
    for start, count, _ in plan_of(pyref, policy, H, agg):
        sh = H - key_depth(start, count, H, leaf_first)
        out.append(len({(int(x) >> sh) if sh < 64 else 0 for x in leaves}))
    return out


def test_shared_symbols_are_declared_exported_and_bound(hip_lib):
    for s in ("dapol_shared_plan", "dapol_prove_entities_shared"):
        assert s in declared_symbols()
        assert hasattr(hip_lib.lib(), s)
        assert s in hip_lib.EXPORTED_SYMBOLS
    assert callable(getattr(hip_lib, "shared_plan", None))
    assert callable(getattr(hip_lib.Tree, "prove_entities_shared", None))


def test_prove_shared_without_a_context_is_an_invalid_argument(hip_lib):
    lib = hip_lib.lib()
    idx = np.array([5], np.uint64)
    seed, out = np.zeros(32, np.uint8), np.zeros(4096, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.dapol_prove_entities_shared(None, None, 1, p(idx), 0, 1, 8, p(seed), 0, None, None, None, None, None, None, p(out), None) == 8
    assert b"null" in lib.dapol_last_error()


@pytest.mark.parametrize("leaf_first", [0, 1])
def test_shared_plan_matches_brute_force(hip_lib, pyref, leaf_first):
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        cases = [(6, H6_LEAVES, pol, agg) for pol, agg in H6_CASES]
        cases += [(64, [0, 1, 1 << 63, (1 << 64) - 1], pol, agg) for pol, agg in ((0, 0), (0, 2), (0, 64), (1, 24), (1, 63))]
        cases += [(6, [37], 0, 3), (1, [0, 1], 0, 1), (1, [1], 1, 0), (0, [0], 0, 0)]       # a single leaf; the smallest trees
        for H, leaves, pol, agg in cases:
            n_sub, tot, per = hip_lib.shared_plan(H, leaves, pol, agg)
            want = brute_force(pyref, leaves, pol, H, agg, leaf_first)
            assert [int(x) for x in n_sub] == want, (H, pol, agg, leaf_first)
            assert tot == sum(want) and per == len(leaves) * len(want)
        n_sub, tot, per = hip_lib.shared_plan(6, [], 0, 3)                                  # no leaves: nothing to prove
        assert (len(n_sub), tot, per) == (0, 0, 0)
    finally:
        hip_lib.wire_config_restore(old)
    # totals alone (the array may be NULL)
    lib = hip_lib.lib()
    idx = np.array(H6_LEAVES, np.uint64)
    tot, per = ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.dapol_shared_plan(6, 8, idx.ctypes.data_as(ctypes.c_void_p), 0, 3, None, ctypes.byref(tot), ctypes.byref(per)) == 0
    assert (tot.value, per.value) == (sum(brute_force(pyref, H6_LEAVES, 0, 6, 3, 0)), 8 * 4)


def test_shared_plan_shares_where_paths_share(hip_lib):
    """The sense of the numbers: padding with aggregation 3 over the eight H = 6 leaves, root side first -- the aggregated proof speaks
    about the depth-3 subtree (keys 0, 16, 40, 56: four of them), the individual proofs about depths 4, 5, 6."""
    n_sub, tot, per = hip_lib.shared_plan(6, H6_LEAVES, 0, 3)
    assert [int(x) for x in n_sub] == [4, 4, 5, 8] and (tot, per) == (21, 32)


def test_shared_plan_refuses_bad_indexes_and_plans(hip_lib):
    for H, bad in ((6, [2, 1]), (6, [3, 3]), (6, [1, 64]), (6, [0, 5, 4, 9]), (0, [1])):
        with pytest.raises(hip_lib.DapolError) as e:
            hip_lib.shared_plan(H, bad, 0, 0)
        assert e.value.code == 8, (H, bad)
    for pol, agg in ((0, 7), (1, 7), (0, -1), (2, 1)):
        with pytest.raises(hip_lib.DapolError) as e:
            hip_lib.shared_plan(6, H6_LEAVES, pol, agg)
        assert e.value.code == 8
