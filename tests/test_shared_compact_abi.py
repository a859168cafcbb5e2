"""The compact form of shared proofs in the C ABI, without a device: the symbols are declared, exported and bound; the layout
(dapol_shared_compact_plan), dapol_shared_expand and dapol_shared_compress are host-only index arithmetic and byte moves, checked against
a numpy brute force (distinct idx >> (H - D) per sub-proof, ranks by np.unique) under both sibling orders."""
import ctypes

import numpy as np
import pytest

from test_abi import declared_symbols
from test_shared_plan_abi import H6_CASES, H6_LEAVES, key_depth, plan_of

ORDERS = [0, 1]                      # dapol_wire_config.siblings_leaf_first
N_BITS = 8
H64_LEAVES = [0, 1, 1 << 63, (1 << 64) - 1]
CASES = ([(6, H6_LEAVES, pol, agg) for pol, agg in H6_CASES] + [(64, H64_LEAVES, pol, agg) for pol, agg in ((0, 0), (0, 2), (0, 64), (1, 24), (1, 63))] +
         [(6, [37], 0, 3), (6, [37], 1, 5), (6, [], 0, 3), (6, [], 1, 6)])


def brute_force(hip_lib, pyref, leaves, policy, H, agg, n_bits, leaf_first):
    """(sub_off, ref, compact_len, n_unique) from the definition."""
    plan = plan_of(pyref, policy, H, agg)
    sub_off, ref, n_unique = [0], [], []
    for start, count, m in plan:
        sh = H - key_depth(start, count, H, leaf_first)
        keys = np.array([(int(x) >> sh) if sh < 64 else 0 for x in leaves], dtype=object)
        uniq, rank = (np.unique(keys.astype(np.uint64), return_inverse=True) if len(leaves) else (np.zeros(0), np.zeros(0, int)))
        n_unique.append(len(uniq))
        ref.append([int(x) for x in rank])
        sub_off.append(sub_off[-1] + len(uniq) * hip_lib.lib().dapol_range_proof_size(n_bits, m))
    return sub_off, ref, sub_off[-1], n_unique


def pattern_compact(hip_lib, pyref, leaves, policy, H, agg, n_bits, leaf_first):
    """A synthetic compact buffer: proof u of sub-proof s is filled with a byte pattern of (s, u, position)."""
    plan = plan_of(pyref, policy, H, agg)
    _, _, _, n_unique = brute_force(hip_lib, pyref, leaves, policy, H, agg, n_bits, leaf_first)
    parts = {}
    for s, (_, _, m) in enumerate(plan):
        ps = hip_lib.lib().dapol_range_proof_size(n_bits, m)
        for u in range(n_unique[s]):
            parts[(s, u)] = ((np.arange(ps) * 7 + 31 * s + 101 * u + 1) % 251).astype(np.uint8)
    flat = [parts[(s, u)] for s in range(len(plan)) for u in range(n_unique[s])]
    return parts, (np.concatenate(flat) if flat else np.zeros(0, np.uint8))


def test_compact_symbols_are_declared_exported_and_bound(hip_lib):
    for s in ("dapol_shared_compact_plan", "dapol_shared_expand", "dapol_shared_compress", "dapol_prove_entities_shared_compact",
              "dapol_verify_entities_compact", "dapol_proof_store_read_compact"):
        assert s in declared_symbols()
        assert hasattr(hip_lib.lib(), s)
        assert s in hip_lib.EXPORTED_SYMBOLS
    for name in ("shared_compact_plan", "shared_expand", "shared_compress"):
        assert callable(getattr(hip_lib, name, None))
    assert callable(getattr(hip_lib.Tree, "prove_entities_shared_compact", None))
    assert callable(getattr(hip_lib.Context, "verify_entities_compact", None))
    assert callable(getattr(hip_lib.ProofStore, "read_compact", None))


def test_compact_calls_without_a_context_are_invalid_arguments(hip_lib):
    lib = hip_lib.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    idx, z32, ok = np.array([5], np.uint64), np.zeros(32, np.uint8), np.full(1, 7, np.uint8)
    out, n, uniq = np.full(4096, 0xAB, np.uint8), ctypes.c_uint64(777), ctypes.c_uint64(12345)
    assert lib.dapol_prove_entities_shared_compact(None, None, 1, p(idx), 0, 1, 8, p(z32), 0, None, None, None, None, None, None, p(out), 4096,
                                                   ctypes.byref(n), ctypes.byref(uniq)) == 8
    assert b"null" in lib.dapol_last_error() and (out == 0xAB).all() and (n.value, uniq.value) == (777, 12345)
    pC = np.zeros((6, 32), np.uint8)
    assert lib.dapol_verify_entities_compact(None, 6, 1, p(idx), p(z32), p(z32), 6, p(pC), p(pC), p(z32), p(z32), 0, 1, 8, p(out), 4096, p(z32), p(ok),
                                             ctypes.byref(uniq)) == 8
    assert b"null" in lib.dapol_last_error() and ok[0] == 7 and uniq.value == 12345


@pytest.mark.parametrize("leaf_first", ORDERS)
def test_layout_matches_brute_force_and_round_trips(hip_lib, pyref, leaf_first):
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        for H, leaves, pol, agg in CASES:
            tag = (H, len(leaves), pol, agg, leaf_first)
            want_off, want_ref, want_len, want_unique = brute_force(hip_lib, pyref, leaves, pol, H, agg, N_BITS, leaf_first)
            sub_off, ref, length = hip_lib.shared_compact_plan(H, leaves, pol, agg, N_BITS)
            assert [int(x) for x in sub_off] == want_off, tag
            assert ref.shape == (len(want_ref), len(leaves)) and ref.tolist() == want_ref, tag
            assert length == want_len, tag
            if leaves:
                n_unique, tot, _ = hip_lib.shared_plan(H, leaves, pol, agg)
                sizes = [hip_lib.lib().dapol_range_proof_size(N_BITS, m) for _, _, m in plan_of(pyref, pol, H, agg)]
                assert [int(x) for x in n_unique] == want_unique and length == sum(int(u) * sz for u, sz in zip(n_unique, sizes)), tag
            # compress(expand(x)) == x over a buffer whose every proof is distinguishable
            _, x = pattern_compact(hip_lib, pyref, leaves, pol, H, agg, N_BITS, leaf_first)
            assert x.shape[0] == length
            blobs = hip_lib.shared_expand(H, leaves, pol, agg, N_BITS, x)
            assert blobs.shape[0] == len(leaves)
            assert hip_lib.shared_compress(H, leaves, pol, agg, N_BITS, blobs).tobytes() == x.tobytes(), tag
    finally:
        hip_lib.wire_config_restore(old)
    # the length alone (both arrays may be NULL)
    idx, length = np.array(H6_LEAVES, np.uint64), ctypes.c_uint64()
    assert hip_lib.lib().dapol_shared_compact_plan(6, 8, idx.ctypes.data_as(ctypes.c_void_p), 0, 3, 8, None, None, ctypes.byref(length)) == 0
    assert length.value == brute_force(hip_lib, pyref, H6_LEAVES, 0, 6, 3, 8, 0)[2]


def test_the_runs_that_the_tamper_tests_rely_on(hip_lib):
    """Padding / 3 over the eight H = 6 leaves, root side first: 21 distinct proofs of 32, sub-proof 0 in runs of 4, 2, 1, 1 rows."""
    sub_off, ref, length = hip_lib.shared_compact_plan(6, H6_LEAVES, 0, 3, 8)
    assert [int(r.max()) + 1 for r in ref] == [4, 4, 5, 8]
    assert ref[0].tolist() == [0, 0, 0, 0, 1, 1, 2, 3]
    assert length == 4 * 608 + 17 * 480 and [int(x) for x in sub_off] == [0, 4 * 608, 4 * 608 + 4 * 480, 4 * 608 + 9 * 480, length]


@pytest.mark.parametrize("leaf_first", ORDERS)
def test_expand_gives_each_blob_the_patterns_its_ref_names(hip_lib, pyref, leaf_first):
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        for pol, agg in H6_CASES:
            plan = plan_of(pyref, pol, 6, agg)
            sizes = [hip_lib.lib().dapol_range_proof_size(N_BITS, m) for _, _, m in plan]
            off = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
            parts, x = pattern_compact(hip_lib, pyref, H6_LEAVES, pol, 6, agg, N_BITS, leaf_first)
            _, ref, _ = hip_lib.shared_compact_plan(6, H6_LEAVES, pol, agg, N_BITS)
            b = len(H6_LEAVES)
            for first, count in ((0, b), (b - 1, 1), (3, 2), (0, 0), (b, 0)):
                blobs = hip_lib.shared_expand(6, H6_LEAVES, pol, agg, N_BITS, x, first, count)
                assert blobs.shape == (count, off[-1])
                for e in range(first, first + count):
                    for s in range(len(plan)):
                        assert blobs[e - first, off[s]:off[s + 1]].tobytes() == parts[(s, int(ref[s, e]))].tobytes(), (pol, agg, first, e, s)
            # expand(compress(y)) == y for y built from such patterns
            y = hip_lib.shared_expand(6, H6_LEAVES, pol, agg, N_BITS, x)
            c = hip_lib.shared_compress(6, H6_LEAVES, pol, agg, N_BITS, y)
            assert hip_lib.shared_expand(6, H6_LEAVES, pol, agg, N_BITS, c).tobytes() == y.tobytes()
    finally:
        hip_lib.wire_config_restore(old)


def test_compress_reads_the_first_row_of_every_run_only(hip_lib, pyref):
    parts, x = pattern_compact(hip_lib, pyref, H6_LEAVES, 0, 6, 3, N_BITS, 0)
    y = hip_lib.shared_expand(6, H6_LEAVES, 0, 3, N_BITS, x)
    y[1:4, :608] = 0xEE                                  # rows 1-3 repeat row 0 in sub-proof 0: not looked at
    assert hip_lib.shared_compress(6, H6_LEAVES, 0, 3, N_BITS, y).tobytes() == x.tobytes()
    y[0, 0] ^= 1                                         # the head of that run is
    assert hip_lib.shared_compress(6, H6_LEAVES, 0, 3, N_BITS, y).tobytes() != x.tobytes()


def test_refusals_leave_the_outputs_untouched(hip_lib, pyref):
    lib, p = hip_lib.lib(), (lambda a: a.ctypes.data_as(ctypes.c_void_p))
    _, x = pattern_compact(hip_lib, pyref, H6_LEAVES, 0, 6, 3, N_BITS, 0)
    es = lib.dapol_entity_proof_size(6, 0, 3, N_BITS)
    good = np.array(H6_LEAVES, np.uint64)
    blobs_in = hip_lib.shared_expand(6, H6_LEAVES, 0, 3, N_BITS, x)

    def all_three(H, idx, pol, agg, n_bits, clen=None, first=0, count=None, cap=None):
        idx = np.array(idx, np.uint64)
        b = len(idx)
        sub_off, ref, length = np.full(16, 0xAB, np.uint64), np.full(16 * max(b, 1), 0xAB, np.uint32), ctypes.c_uint64(777)
        out, cout, clen_out = np.full((max(b, 1), es), 0xAB, np.uint8), np.full(len(x) + 64, 0xAB, np.uint8), ctypes.c_uint64(777)
        rc = (lib.dapol_shared_compact_plan(H, b, p(idx), pol, agg, n_bits, p(sub_off), p(ref), ctypes.byref(length)),
              lib.dapol_shared_expand(H, b, p(idx), pol, agg, n_bits, p(x), len(x) if clen is None else clen, first, b if count is None else count, p(out)),
              lib.dapol_shared_compress(H, b, p(idx), pol, agg, n_bits, p(blobs_in), p(cout), len(x) if cap is None else cap, ctypes.byref(clen_out)))
        untouched = ((sub_off == 0xAB).all() and (ref == 0xAB).all() and length.value == 777, (out == 0xAB).all(),
                     (cout == 0xAB).all() and clen_out.value == 777)
        return rc, untouched

    for H, idx, pol, agg, n_bits in ((6, [0, 1, 3, 2, 16, 17, 40, 63], 0, 3, 8), (6, [0, 1, 2, 2, 16, 17, 40, 63], 0, 3, 8),       # not increasing
                                     (6, [0, 1, 2, 3, 16, 17, 40, 64], 0, 3, 8),                                                   # an index >= 2^H
                                     (6, H6_LEAVES, 2, 3, 8), (6, H6_LEAVES, 0, 7, 8), (6, H6_LEAVES, 1, -1, 8),                    # policy, factor
                                     (6, H6_LEAVES, 0, 3, 12), (6, H6_LEAVES, 0, 3, 0)):                                           # n_bits
        rc, untouched = all_three(H, idx, pol, agg, n_bits)
        assert rc == (8, 8, 8) and all(untouched), (H, idx, pol, agg, n_bits)
    rc, untouched = all_three(65, H6_LEAVES, 0, 3, 8)
    assert rc == (1, 1, 1) and all(untouched)
    for kw in (dict(clen=len(x) - 1), dict(clen=len(x) + 1), dict(clen=0), dict(first=1), dict(first=8, count=1), dict(first=9, count=0),
               dict(first=3, count=(1 << 64) - 2)):
        rc, untouched = all_three(6, good, 0, 3, 8, **kw)
        assert rc[1] == 8 and untouched[1], kw
    rc, untouched = all_three(6, good, 0, 3, 8, cap=len(x) - 1)                  # one byte short
    assert rc[2] == 8 and untouched[2]
    rc, untouched = all_three(6, good, 0, 3, 8)                                   # and the healthy call writes all three
    assert rc == (0, 0, 0) and not any(untouched)
