"""dapol_prove_entities_shared: every distinct sub-proof statement of a call is proven once and written into the blob of every entity
that contains it.  The tests pin the DEFINITION (include/dapol_hip.h): the bytes of a sub-proof are those of dapol_range_prove_batch
over its siblings (pads (0, 1)) with stream id S = the leaf index with the low H - D bits cleared and slot base 0, D being the largest
depth among the sub-proof's siblings under the configured sibling order."""
import ctypes

import numpy as np
import pytest

from test_shared_plan_abi import H6_CASES, H6_LEAVES, key_depth, plan_of

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))
ORDERS = [0, 1]                      # dapol_wire_config.siblings_leaf_first


@pytest.fixture(scope="module")
def ctx8(hip_lib):
    c = hip_lib.Context(0, 8)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx1(hip_lib):
    c = hip_lib.Context(0, 1)
    yield c
    c.close()


def _blindings(rng, n):
    r = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    r[:, 31] &= 0x0F
    return r


def _tree(hip_lib, ctx, H, leaves, seed=1, vmax=20, shard_bits=0):
    rng = np.random.default_rng(seed)
    idx = np.array(sorted(leaves), np.uint64)
    v = rng.integers(0, vmax + 1, size=len(idx), dtype=np.uint64)
    r = _blindings(rng, len(idx))
    return idx, v, r, hip_lib.Tree(ctx, H, idx, v, r, SEED, shard_bits=shard_bits)


def _key(leaf, H, D):
    sh = H - D
    return 0 if sh >= 64 else (int(leaf) >> sh) << sh


def _offsets(hip_lib, plan, n_bits):
    sizes = [hip_lib.lib().dapol_range_proof_size(n_bits, m) for _, _, m in plan]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(int)


def check_definition(hip_lib, pyref, ctx, idx, sib_v, sib_r, policy, agg, n_bits, leaf_first, blobs, pairs=None):
    """Every (entity, sub-proof) of `pairs` (default: all) against dapol_range_prove_batch, one call per distinct m over the distinct
    (sub-proof, S) statements: siblings from the path arrays, stream id S, slot base 0, pad parties (0, 1).  Returns the number of
    distinct statements among the pairs."""
    H = sib_v.shape[1]
    plan = plan_of(pyref, policy, H, agg)
    off = _offsets(hip_lib, plan, n_bits)
    assert blobs.shape[1] == off[-1]
    if pairs is None:
        pairs = [(e, s) for e in range(len(idx)) for s in range(len(plan))]
    one = np.zeros(32, np.uint8)
    one[0] = 1
    stmts = {}                                           # (s, S) -> first entity that has it
    for e, s in pairs:
        start, count, m = plan[s]
        stmts.setdefault((s, _key(idx[e], H, key_depth(start, count, H, leaf_first))), e)
    expect = {}
    for m in sorted({plan[s][2] for s, _ in stmts}):
        rows = [(k, e) for k, e in stmts.items() if plan[k[0]][2] == m]
        v, r = np.zeros((len(rows), m), np.uint64), np.tile(one, (len(rows), m, 1))
        for i, ((s, S), e) in enumerate(rows):
            start, count, _ = plan[s]
            v[i, :count] = sib_v[e, start:start + count]
            r[i, :count] = sib_r[e, start:start + count]
        got = ctx.range_prove_batch(n_bits, m, v, r, nonce_seed=SEED, stream_id=[k[1] for k, _ in rows], slot_base=0)
        for i, (k, _) in enumerate(rows):
            expect[k] = got[i].tobytes()
    for e, s in pairs:
        start, count, m = plan[s]
        S = _key(idx[e], H, key_depth(start, count, H, leaf_first))
        assert blobs[e, off[s]:off[s + 1]].tobytes() == expect[(s, S)], (policy, agg, leaf_first, e, s)
    return len(stmts)


def verify_all(ctx, tree_root, H, idx, v, r, pC, pH, policy, agg, n_bits, blobs):
    lC, lH = ctx.commit_hash_batch(v, r)
    rC, rH = tree_root[0], tree_root[1]
    return ctx.verify_entities(H, idx, lC, lH, pC, pH, rC, rH, policy, agg, n_bits, blobs, verify_seed=SEED)


@pytest.fixture(scope="module")
def h6(hip_lib, ctx8):
    return _tree(hip_lib, ctx8, 6, H6_LEAVES)


@pytest.mark.parametrize("leaf_first", ORDERS)
@pytest.mark.parametrize("policy,agg", H6_CASES)
def test_definition_sharing_and_verification(hip_lib, pyref, ctx8, h6, policy, agg, leaf_first):
    """(1) every sub-proof of every entity equals the range_prove_batch row of its statement; (3) entities with equal S carry identical
    bytes (they are compared with the same expected row) and `unique` is shared_plan's total, below b x plan size -- except where the
    definition leaves nothing to share: padding with aggregation = H has one sub-proof whose deepest sibling is the leaf's own (D = H in
    either order), so every key is a leaf and `unique` is exactly b x plan size; (4) all verify."""
    idx, v, r, tr = h6
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        sC, sH, sv, sr = tr.paths(idx)
        pC, pH, blobs, unique = tr.prove_entities_shared(idx, policy, agg, 8, SEED)
        assert pC.tobytes() == sC.tobytes() and pH.tobytes() == sH.tobytes()
        n_stmts = check_definition(hip_lib, pyref, ctx8, idx, sv, sr, policy, agg, 8, leaf_first, blobs)
        n_sub, tot, per = hip_lib.shared_plan(6, idx, policy, agg)
        assert unique == tot == n_stmts
        assert per == len(idx) * len(n_sub)
        every_key_is_a_leaf = all(key_depth(st, cnt, 6, leaf_first) == 6 for st, cnt, _ in plan_of(pyref, policy, 6, agg))
        assert unique == per if every_key_is_a_leaf else unique < per
        assert verify_all(ctx8, tr.root(), 6, idx, v, r, pC, pH, policy, agg, 8, blobs).all()
    finally:
        hip_lib.wire_config_restore(old)


def test_oracle_proves_the_same_bytes(hip_lib, pyref, ctx8):
    """(2) Independent of the GPU prover: each distinct sub-proof equals pyref.range_prove under Tape(seed, stream_id = S) -- a fresh
    tape per statement, i.e. slot base 0."""
    H, agg, n_bits = 4, 3, 8
    idx, v, r, tr = _tree(hip_lib, ctx8, H, [4, 5, 12], seed=2)
    _, _, sv, sr = tr.paths(idx)
    _, _, blobs, unique = tr.prove_entities_shared(idx, hip_lib.POLICY_SPLITTING, agg, n_bits, SEED)
    plan = plan_of(pyref, 1, H, agg)
    assert plan == [(0, 2, 2), (2, 1, 1), (3, 1, 1)]
    off = _offsets(hip_lib, plan, n_bits)
    done = {}
    for e in range(len(idx)):
        for s, (start, count, m) in enumerate(plan):
            S = _key(idx[e], H, start + count)
            if (s, S) not in done:
                vals = [int(x) for x in sv[e, start:start + count]] + [0] * (m - count)
                bl = [int.from_bytes(sr[e, i].tobytes(), "little") for i in range(start, start + count)] + [1] * (m - count)
                done[(s, S)] = pyref.range_prove(vals, bl, n_bits, pyref.Tape(seed=SEED, stream_id=S))
            assert blobs[e, off[s]:off[s + 1]].tobytes() == done[(s, S)], (e, s)
    assert unique == len(done) == 7                      # keys 4, 4, 12 at depths 2 and 3, three leaves at depth 4


def test_one_flipped_byte_fails_one_entity_and_blobs_round_trip(hip_lib, ctx8, h6):
    """(4) a byte flipped inside a SHARED sub-proof of one entity's blob fails that entity only; a shared blob goes through
    R::serialize / deserialize unchanged."""
    idx, v, r, tr = h6
    policy, agg, n_bits = hip_lib.POLICY_PADDING, 3, 8
    pC, pH, blobs, _ = tr.prove_entities_shared(idx, policy, agg, n_bits, SEED)
    assert blobs[0, :64].tobytes() == blobs[3, :64].tobytes()            # leaves 0 and 3 share the aggregated proof (key 0 at depth 3)
    bad = blobs.copy()
    bad[3, 40] ^= 0x01
    ok = verify_all(ctx8, tr.root(), 6, idx, v, r, pC, pH, policy, agg, n_bits, bad)
    assert ok.tolist() == [1, 1, 1, 0, 1, 1, 1, 1]
    for e in (0, 7):
        wire = hip_lib.range_proofs_serialize(6, policy, agg, n_bits, blobs[e].tobytes())
        aggp, ind, used = hip_lib.range_proofs_deserialize(policy, n_bits, wire)
        assert b"".join(aggp) + b"".join(ind) == blobs[e].tobytes() and used == len(wire) and len(ind) == 3


def test_no_sharing_equals_the_per_entity_path(hip_lib, ctx8, h6):
    """(5) padding with aggregation = H, root side first: the only sub-proof has D = H, S = the leaf, slot base 0 -- prove_entities' bytes."""
    idx, v, r, tr = h6
    pC, pH, blobs, unique = tr.prove_entities_shared(idx, hip_lib.POLICY_PADDING, 6, 8, SEED)
    eC, eH, eblobs = tr.prove_entities(idx, hip_lib.POLICY_PADDING, 6, 8, SEED)
    assert blobs.tobytes() == eblobs.tobytes() and pC.tobytes() == eC.tobytes() and pH.tobytes() == eH.tobytes()
    assert unique == len(idx)


@pytest.mark.parametrize("leaf_first", ORDERS)
def test_key_edges_height_64(hip_lib, pyref, ctx8, leaf_first):
    """(6) H = 64: D = 64 (the key is the leaf, no shift by 64 the other way either) down to D = 1 and 2; 62 individual proofs per entity."""
    H, policy, agg = 64, hip_lib.POLICY_PADDING, 2
    idx, v, r, tr = _tree(hip_lib, ctx8, H, [0, 1, 1 << 63, (1 << 64) - 1], seed=3)
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        _, _, sv, sr = tr.paths(idx)
        pC, pH, blobs, unique = tr.prove_entities_shared(idx, policy, agg, 8, SEED)
        n_stmts = check_definition(hip_lib, pyref, ctx8, idx, sv, sr, policy, agg, 8, leaf_first, blobs)
        assert unique == n_stmts == hip_lib.shared_plan(H, idx, policy, agg)[1] < 4 * 63
        assert verify_all(ctx8, tr.root(), H, idx, v, r, pC, pH, policy, agg, 8, blobs).all()
    finally:
        hip_lib.wire_config_restore(old)


@pytest.mark.parametrize("leaf_first", ORDERS)
def test_key_edges_height_1_and_aggregation_0(hip_lib, pyref, ctx8, h6, leaf_first):
    """(6) H = 1 with both leaves (D = H = 1: nothing shared); aggregation_factor = 0: D = 0, one pad proof shared by all (at H = 6 and,
    with a shift of the full index width, at H = 64)."""
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        cases = [(1, _tree(hip_lib, ctx8, 1, [0, 1], seed=4), 0, 1), (1, _tree(hip_lib, ctx8, 1, [0, 1], seed=4), 1, 1),
                 (6, h6, 0, 0), (64, _tree(hip_lib, ctx8, 64, [5, 1 << 63], seed=5), 0, 0)]
        for H, (idx, v, r, tr), policy, agg in cases:
            _, _, sv, sr = tr.paths(idx)
            pC, pH, blobs, unique = tr.prove_entities_shared(idx, policy, agg, 8, SEED)
            n_stmts = check_definition(hip_lib, pyref, ctx8, idx, sv, sr, policy, agg, 8, leaf_first, blobs)
            assert unique == n_stmts == hip_lib.shared_plan(H, idx, policy, agg)[1]
            if agg == 0:
                ps = hip_lib.lib().dapol_range_proof_size(8, 1)
                assert len({blobs[e, :ps].tobytes() for e in range(len(idx))}) == 1          # the pad proof: one statement, key 0
            else:
                assert unique == 2
            assert verify_all(ctx8, tr.root(), H, idx, v, r, pC, pH, policy, agg, 8, blobs).all()
    finally:
        hip_lib.wire_config_restore(old)


def test_compacted_call_crosses_into_the_short_list_sweep(hip_lib, pyref, ctx1):
    """(7) H = 13, 2,500 leaves, 64-bit proofs, padding with aggregation 1 on a one-party context: all 13 sub-proofs have m = 1, so the
    compacted call is ONE call of well over 2,048 rows (the short-list sweep's regime), although no depth alone has that many below
    depth 12.  One leaf holds 2^63 (the top bit of a 64-bit proof)."""
    H, policy, agg, n_bits = 13, hip_lib.POLICY_PADDING, 1, 64
    rng = np.random.default_rng(13)
    idx = np.sort(rng.choice(1 << H, size=2500, replace=False)).astype(np.uint64)
    v = rng.integers(0, 1000, size=len(idx), dtype=np.uint64)
    v[1234] = 1 << 63
    r = _blindings(rng, len(idx))
    tr = hip_lib.Tree(ctx1, H, idx, v, r, SEED)
    _, _, sv, sr = tr.paths(idx)
    pC, pH, blobs, unique = tr.prove_entities_shared(idx, policy, agg, n_bits, SEED)
    n_sub, tot, per = hip_lib.shared_plan(H, idx, policy, agg)
    assert unique == tot and 2048 < tot < per == 2500 * 13
    pairs = [(int(e), int(s)) for e, s in zip(rng.integers(0, len(idx), size=64), rng.integers(0, 13, size=64))]
    for k, e in enumerate((0, 1233, 2499)):              # statements whose party IS the subtree that holds the 2^63 leaf: the sibling at
        s = H - (int(idx[e]) ^ int(idx[1234])).bit_length()      # the depth where e's path leaves that leaf's (sub-proof s = sibling s)
        assert sv[e, s] >= 1 << 63
        pairs[k] = (e, s)
    check_definition(hip_lib, pyref, ctx1, idx, sv, sr, policy, agg, n_bits, 0, blobs, pairs)
    assert verify_all(ctx1, tr.root(), H, idx, v, r, pC, pH, policy, agg, n_bits, blobs).all()


@pytest.mark.parametrize("leaf_first", ORDERS)
def test_shards_give_the_unsharded_bytes(hip_lib, ctx8, leaf_first):
    """(8) total height 6 in 4 shards: each shard's shared output for its leaves (upper siblings from dapol_shard_top_levels) equals the
    unsharded tree's shared output for the same leaves -- the key is made from the GLOBAL leaf index over H = tree height + n_upper."""
    from dapol_amd import sharded
    H, sb = 6, 2
    leaves = [0, 1, 2, 3, 16, 17, 21, 40, 44, 63]
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        idx, v, r, full = _tree(hip_lib, ctx8, H, leaves, seed=6)
        trees, recs = [], []
        for s in range(1 << sb):
            sel = (idx >> np.uint64(H - sb)) == s
            assert sel.any()
            t = hip_lib.Tree(ctx8, H, idx[sel], v[sel], r[sel], SEED, shard_bits=sb)
            trees.append((sel, t))
            recs.append(sharded.pack_record(t.root()))
        for policy, agg in ((hip_lib.POLICY_PADDING, 3), (hip_lib.POLICY_SPLITTING, 5), (hip_lib.POLICY_PADDING, 0)):
            shared_n = 0
            for s, (sel, t) in enumerate(trees):
                fC, fH, fblobs, _ = full.prove_entities_shared(idx[sel], policy, agg, 8, SEED)
                root, upper = hip_lib.shard_top_levels(ctx8, np.stack(recs), s)
                assert root == full.root()
                pC, pH, blobs, unique = t.prove_entities_shared(idx[sel], policy, agg, 8, SEED, upper=upper)
                assert blobs.tobytes() == fblobs.tobytes() and pC.tobytes() == fC.tobytes() and pH.tobytes() == fH.tobytes()
                assert unique == hip_lib.shared_plan(H, idx[sel], policy, agg)[1]
                shared_n += unique
            assert shared_n < len(idx) * len(hip_lib.shared_plan(H, idx, policy, agg)[0])
    finally:
        hip_lib.wire_config_restore(old)


def test_refusals(hip_lib, ctx8, ctx1, h6):
    """(9) unsorted -> 8; missing leaf -> 9 with the outputs untouched; aggregation > H -> 8; more parties than the context has -> 8;
    b = 0 -> OK."""
    idx, v, r, tr = h6
    for bad in ([1, 0], [2, 2], [0, 16, 3]):
        with pytest.raises(hip_lib.DapolError) as e:
            tr.prove_entities_shared(bad, 0, 3, 8, SEED)
        assert e.value.code == 8
    with pytest.raises(hip_lib.DapolError) as e:
        tr.prove_entities_shared(idx, 0, 7, 8, SEED)
    assert e.value.code == 8
    with pytest.raises(hip_lib.DapolError) as e:
        tr.prove_entities_shared(idx, 0, 3, 12, SEED)                    # n_bits
    assert e.value.code == 8
    i1, v1, r1, t1 = _tree(hip_lib, ctx1, 6, H6_LEAVES)
    with pytest.raises(hip_lib.DapolError) as e:
        t1.prove_entities_shared(i1, 0, 2, 8, SEED)                      # a two-party proof on a one-party context
    assert e.value.code == 8
    lib, p = hip_lib.lib(), (lambda a: a.ctypes.data_as(ctypes.c_void_p))
    seed = np.frombuffer(SEED, np.uint8).copy()
    es = lib.dapol_entity_proof_size(6, 0, 3, 8)
    want = np.array([0, 1, 5, 16], np.uint64)                           # no liability at leaf 5
    C, Hh, out = np.full((4, 6, 32), 0xAB, np.uint8), np.full((4, 6, 32), 0xAB, np.uint8), np.full((4, es), 0xAB, np.uint8)
    uniq = ctypes.c_uint64(12345)
    args = lambda n, ix: (ctx8.h, tr.h, n, p(ix), 0, 3, 8, p(seed), 0, None, None, None, None, p(C), p(Hh), p(out), ctypes.byref(uniq))
    assert lib.dapol_prove_entities_shared(*args(4, want)) == 9
    assert (C == 0xAB).all() and (Hh == 0xAB).all() and (out == 0xAB).all() and uniq.value == 12345
    assert lib.dapol_prove_entities_shared(*args(0, want)) == 0 and uniq.value == 0
    assert (out == 0xAB).all()
    assert lib.dapol_prove_entities_shared(ctx1.h, tr.h, 1, p(want), 0, 3, 8, p(seed), 0, None, None, None, None, p(C), p(Hh), p(out), None) == 8   # another context's tree
    # the call after the refusals is healthy
    assert tr.prove_entities_shared(idx, 0, 3, 8, SEED)[3] == 21
