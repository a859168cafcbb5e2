"""The compact form of shared proofs on the GPU: dapol_prove_entities_shared_compact leaves every distinct sub-proof once,
dapol_verify_entities_compact takes them once.  The tests pin the DEFINITIONS (include/dapol_hip.h): the expansion of the prover's
buffer is dapol_prove_entities_shared's output byte for byte, and the verifier's verdicts are dapol_verify_entities' over the
expansion of whatever buffer it is given -- tampered ones included -- with `unique` counting the heads (a new subtree key, or a covered
sibling commitment that differs from the row before).

The H = 6 tree has 8 leaves and at most 7 sub-proofs, so the tests set DAPOL_VSHARED_FORWARD_MAX=0 to run it through the kernels; the
forwarding test runs with the library's own limit."""
import ctypes

import numpy as np
import pytest

from test_gpu_forgeries import _Entities
from test_gpu_shared_proofs import _tree, check_definition
from test_gpu_verify_shared import Proven, _fallbacks
from test_shared_plan_abi import H6_CASES, H6_LEAVES, key_depth, plan_of

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))
ORDERS = [0, 1]                      # dapol_wire_config.siblings_leaf_first


@pytest.fixture(autouse=True)
def through_the_kernels(monkeypatch):
    monkeypatch.setenv("DAPOL_VSHARED_FORWARD_MAX", "0")


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


@pytest.fixture(scope="module")
def h6(hip_lib, ctx8):
    return Proven(hip_lib, ctx8, 6, H6_LEAVES, 0, 3, 8)


def compact_of(p):
    """The compact proofs of a Proven under its current (policy, aggregation factor), with everything the prover reports."""
    pC, pH, compact, unique = p.tree.prove_entities_shared_compact(p.idx, p.policy, p.agg, p.n_bits, SEED)
    return pC, pH, compact, unique


def both(p, compact, pC=None):
    """(verdicts, unique) of the compact verifier, after comparing the verdicts with dapol_verify_entities' over the expansion."""
    pC = p.pC if pC is None else pC
    head = (p.H, p.idx, p.lC, p.lH, pC, p.pH, p.root[0], p.root[1], p.policy, p.agg, p.n_bits)
    blobs = p.hip.shared_expand(p.H, p.idx, p.policy, p.agg, p.n_bits, compact)
    want = p.ctx.verify_entities(*head, blobs, verify_seed=SEED)
    ok, unique = p.ctx.verify_entities_compact(*head, compact, verify_seed=SEED)
    assert ok.tolist() == want.tolist()
    return ok.tolist(), unique


def head_count(pyref, p, pC, leaf_first=0):
    """The definition's heads, brute force: a new key, or a covered commitment that differs from the row before."""
    n = 0
    for start, count, _ in plan_of(pyref, p.policy, p.H, p.agg):
        sh = p.H - key_depth(start, count, p.H, leaf_first)
        key = lambda x: 0 if sh >= 64 else int(x) >> sh
        for e in range(len(p.idx)):
            n += int(e == 0 or key(p.idx[e]) != key(p.idx[e - 1]) or pC[e, start:start + count].tobytes() != pC[e - 1, start:start + count].tobytes())
    return n


# ------------------------------------------------------------------------------------------------ 1. prover = shared call
@pytest.mark.parametrize("leaf_first", ORDERS)
@pytest.mark.parametrize("policy,agg", H6_CASES)
def test_prover_equals_the_shared_call(hip_lib, pyref, ctx8, h6, policy, agg, leaf_first):
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        h6.prove(True, policy, agg)
        pC, pH, compact, unique = compact_of(h6)
        blobs = hip_lib.shared_expand(6, h6.idx, policy, agg, 8, compact)
        assert blobs.tobytes() == h6.blobs.tobytes()
        assert pC.tobytes() == h6.pC.tobytes() and pH.tobytes() == h6.pH.tobytes()
        assert unique == hip_lib.shared_plan(6, h6.idx, policy, agg)[1] == h6.proved
        assert compact.shape[0] == hip_lib.shared_compact_plan(6, h6.idx, policy, agg, 8)[2]
        assert hip_lib.shared_compress(6, h6.idx, policy, agg, 8, h6.blobs).tobytes() == compact.tobytes()
        _, _, sv, sr = h6.tree.paths(h6.idx)
        assert check_definition(hip_lib, pyref, ctx8, h6.idx, sv, sr, policy, agg, 8, leaf_first, blobs) == unique
    finally:
        hip_lib.wire_config_restore(old)
        h6.prove(True, 0, 3)


def test_nothing_shared_is_prove_entities_concatenated(hip_lib, h6):
    """Padding with aggregation = H, root side first: one sub-proof with D = H, every key a leaf -- the compact buffer is the blobs of
    prove_entities one after the other."""
    pC, pH, compact, unique = h6.tree.prove_entities_shared_compact(h6.idx, 0, 6, 8, SEED)
    eC, eH, eblobs = h6.tree.prove_entities(h6.idx, 0, 6, 8, SEED)
    assert compact.tobytes() == eblobs.tobytes() and pC.tobytes() == eC.tobytes() and pH.tobytes() == eH.tobytes()
    assert unique == len(h6.idx)


@pytest.mark.parametrize("leaf_first", ORDERS)
def test_shards_with_upper_siblings(hip_lib, ctx8, leaf_first):
    """Total height 6 in 4 shards: each shard's compact output (upper siblings from dapol_shard_top_levels) expands to that shard's
    shared output; the layout is that of the global leaf indexes over H = tree height + n_upper."""
    from dapol_amd import sharded
    H, sb = 6, 2
    leaves = [0, 1, 2, 3, 16, 17, 21, 40, 44, 63]
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        idx, v, r, _ = _tree(hip_lib, ctx8, H, leaves, seed=6)
        trees, recs = [], []
        for s in range(1 << sb):
            sel = (idx >> np.uint64(H - sb)) == s
            t = hip_lib.Tree(ctx8, H, idx[sel], v[sel], r[sel], SEED, shard_bits=sb)
            trees.append((sel, t))
            recs.append(sharded.pack_record(t.root()))
        for policy, agg in ((0, 3), (1, 5), (0, 0)):
            for s, (sel, t) in enumerate(trees):
                _, upper = hip_lib.shard_top_levels(ctx8, np.stack(recs), s)
                sC, sH, sblobs, proved = t.prove_entities_shared(idx[sel], policy, agg, 8, SEED, upper=upper)
                pC, pH, compact, unique = t.prove_entities_shared_compact(idx[sel], policy, agg, 8, SEED, upper=upper)
                assert hip_lib.shared_expand(H, idx[sel], policy, agg, 8, compact).tobytes() == sblobs.tobytes()
                assert pC.tobytes() == sC.tobytes() and pH.tobytes() == sH.tobytes()
                assert unique == proved == hip_lib.shared_plan(H, idx[sel], policy, agg)[1]
    finally:
        hip_lib.wire_config_restore(old)


# ------------------------------------------------------------------------------------------------ 2. verifier, honest
@pytest.mark.parametrize("leaf_first", ORDERS)
@pytest.mark.parametrize("policy,agg", H6_CASES)
def test_verifier_honest(hip_lib, h6, policy, agg, leaf_first):
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        h6.prove(True, policy, agg)
        _, _, compact, _ = compact_of(h6)
        fb = _fallbacks(hip_lib)
        ok, unique = both(h6, compact)
        assert ok == [1] * 8 and unique == h6.plan_total()
        assert _fallbacks(hip_lib) == fb
    finally:
        hip_lib.wire_config_restore(old)
        h6.prove(True, 0, 3)


def test_one_party_context_and_aggregation_0(hip_lib, ctx1):
    """Aggregation 0 on a one-party context: the siblingless pad proof is one compact row that all rows use."""
    t = Proven(hip_lib, ctx1, 6, H6_LEAVES, 0, 0, 8, seed=2)
    pC, pH, compact, unique = compact_of(t)
    assert hip_lib.shared_expand(6, t.idx, 0, 0, 8, compact).tobytes() == t.blobs.tobytes()
    ok, vu = both(t, compact)
    assert ok == [1] * 8 and vu == unique == t.plan_total() < 8 * 7
    bad = compact.copy()
    bad[9] ^= 0x01                                       # the pad proof: everybody's
    assert both(t, bad)[0] == [0] * 8


def test_the_latency_regime_forwards(hip_lib, h6, monkeypatch):
    """With the library's own limit: 8 entities x 4 sub-proofs = 32 <= 64 expand on the host, forward to dapol_verify_entities and
    report 32."""
    monkeypatch.delenv("DAPOL_VSHARED_FORWARD_MAX")
    _, _, compact, _ = compact_of(h6)
    ok, unique = both(h6, compact)
    assert ok == [1] * 8 and unique == 32
    bad = compact.copy()
    bad[40] ^= 0x01                                      # the aggregated proof that rows 0-3 use
    ok, unique = both(h6, bad)
    assert ok == [0, 0, 0, 0, 1, 1, 1, 1] and unique == 32


# ------------------------------------------------------------------------------------------------ 3. verifier, every region
@pytest.mark.parametrize("policy,agg", H6_CASES)
def test_every_region_of_the_compact_buffer(hip_lib, pyref, h6, policy, agg):
    """One byte flipped at the first and at the last byte of the first and of the last proof of every group: exactly the rows whose ref
    names that proof fail."""
    try:
        h6.prove(True, policy, agg)
        _, _, compact, _ = compact_of(h6)
        sub_off, ref, length = hip_lib.shared_compact_plan(6, h6.idx, policy, agg, 8)
        plan = plan_of(pyref, policy, 6, agg)
        groups = []                                        # runs of equal m: [first sub-proof, last sub-proof]
        for s, (_, _, m) in enumerate(plan):
            if groups and plan[groups[-1][1]][2] == m:
                groups[-1][1] = s
            else:
                groups.append([s, s])
        hit = 0
        for s_first, s_last in groups:
            for s, u in ((s_first, 0), (s_last, int(ref[s_last].max()))):
                ps = hip_lib.lib().dapol_range_proof_size(8, plan[s][2])
                for at in (int(sub_off[s]) + u * ps, int(sub_off[s]) + (u + 1) * ps - 1):
                    bad = compact.copy()
                    bad[at] ^= 0x01
                    ok, _ = both(h6, bad)
                    assert ok == [int(ref[s, e] != u) for e in range(8)], (policy, agg, s, u, at)
                    hit += 1
        assert hit == 4 * len(groups) and int(sub_off[-1]) == length == compact.shape[0]
    finally:
        h6.prove(True, 0, 3)


# ------------------------------------------------------------------------------------------------ 4. statement binding
def test_a_corrupted_commitment_fails_its_row_alone(hip_lib, pyref, h6):
    """Padding / 3, root side first, sub-proof 0 (siblings 0-2), the run of rows 0-3: another valid commitment at sibling 0 of row 0,
    then of row 1.  Only that row fails; the rest of its run keeps its verdict.  A verifier that took the statement from the key head
    alone would fail rows 0-3 in the first case; one that never compared commitments would report 21 heads."""
    _, _, compact, _ = compact_of(h6)
    _, ref, _ = hip_lib.shared_compact_plan(6, h6.idx, 0, 3, 8)
    assert ref[0].tolist() == [0, 0, 0, 0, 1, 1, 2, 3]
    assert both(h6, compact)[1] == 21 == head_count(pyref, h6, h6.pC)
    for e, heads in ((0, 22), (1, 23)):
        pC = h6.pC.copy()
        pC[e, 0] = h6.lC[5]
        ok, unique = both(h6, compact, pC=pC)
        assert ok == [int(i != e) for i in range(8)], e
        assert unique == heads == head_count(pyref, h6, pC), e


# ------------------------------------------------------------------------------------------------ 5. rejected by the algebra
@pytest.fixture(scope="module")
def ent8(hip_lib, gpu_ctx):
    return _Entities(hip_lib, gpu_ctx, 8, (200, 100))


@pytest.mark.parametrize("agg", [0, 2, 3, 6])
@pytest.mark.parametrize("policy", [0, 1])
def test_out_of_range_sums_are_rejected_by_the_algebra(hip_lib, ent8, policy, agg):
    """n_bits = 8, the heavy pair (200, 100) among light leaves: the prover proves the low bits of out-of-range sums, transcript-consistent;
    a forged shared sub-proof fails its whole run and nothing else."""
    e = ent8
    pC, pH, compact, unique = e.tree.prove_entities_shared_compact(e.idx, policy, agg, 8, SEED)
    ok, vu = e.ctx.verify_entities_compact(6, e.idx, e.lC, e.lH, pC, pH, e.root[0], e.root[1], policy, agg, 8, compact, verify_seed=SEED)
    assert ok.tolist() == e.want
    assert vu == unique == hip_lib.shared_plan(6, e.idx, policy, agg)[1]
    blobs = hip_lib.shared_expand(6, e.idx, policy, agg, 8, compact)
    assert e.verify(pC, pH, blobs, policy, agg) == e.want


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(hip_lib, ctx8, h6):
    lib, p = hip_lib.lib(), (lambda a: a.ctypes.data_as(ctypes.c_void_p))
    tr, idx = h6.tree, h6.idx
    seed = np.frombuffer(SEED, np.uint8).copy()
    need = hip_lib.shared_compact_plan(6, idx, 0, 3, 8)[2]
    C, Hh, out = np.full((8, 6, 32), 0xAB, np.uint8), np.full((8, 6, 32), 0xAB, np.uint8), np.full(need + 4096, 0xAB, np.uint8)
    n, uniq = ctypes.c_uint64(777), ctypes.c_uint64(12345)
    args = lambda b, ix, cap: (ctx8.h, tr.h, b, p(ix), 0, 3, 8, p(seed), 0, None, None, None, None, p(C), p(Hh), p(out), cap, ctypes.byref(n), ctypes.byref(uniq))
    untouched = lambda: (C == 0xAB).all() and (Hh == 0xAB).all() and (out == 0xAB).all() and (n.value, uniq.value) == (777, 12345)
    want = np.array([0, 1, 5, 16], np.uint64)                            # no liability at leaf 5
    assert lib.dapol_prove_entities_shared_compact(*args(4, want, out.shape[0])) == 9 and untouched()
    assert lib.dapol_prove_entities_shared_compact(*args(8, idx, need - 1)) == 8 and untouched()           # one byte short
    for bad in ([1, 0], [2, 2], [0, 16, 3]):
        ix = np.array(bad, np.uint64)
        assert lib.dapol_prove_entities_shared_compact(*args(len(bad), ix, out.shape[0])) == 8 and untouched()
    assert lib.dapol_prove_entities_shared_compact(*args(0, idx, 0)) == 0 and (n.value, uniq.value) == (0, 0) and (out == 0xAB).all()
    assert lib.dapol_prove_entities_shared_compact(*args(8, idx, need)) == 0 and (n.value, uniq.value) == (need, 21)       # exactly enough
    compact = out[:need].copy()
    assert (out[need:] == 0xAB).all() and hip_lib.shared_expand(6, idx, 0, 3, 8, compact).tobytes() == h6.blobs.tobytes()
    # the verifier
    a = lambda **kw: {**dict(height=6, leaf_idx=idx, leaf_C=h6.lC, leaf_H=h6.lH, path_C=h6.pC, path_H=h6.pH, root_C=h6.root[0], root_H=h6.root[1],
                             policy=0, aggregation_factor=3, n_bits=8, compact=compact, verify_seed=SEED), **kw}
    swapped = np.array([0, 1, 3, 2, 16, 17, 40, 63], np.uint64)
    for kw in (dict(leaf_idx=swapped), dict(leaf_idx=np.array([0, 1, 2, 2, 16, 17, 40, 63], np.uint64)), dict(policy=2), dict(aggregation_factor=7),
               dict(n_bits=12)):
        with pytest.raises(hip_lib.DapolError) as e:
            ctx8.verify_entities_compact(**a(**kw))
        assert e.value.code == 8, kw
    flat_C, flat_H = h6.pC.reshape(-1, 32), h6.pH.reshape(-1, 32)
    for kw in (dict(compact=compact[:-1]), dict(compact=np.concatenate([compact, compact[:1]])), dict(path_C=flat_C[:-1], path_H=flat_H[:-1]),
               dict(aggregation_factor=2)):
        ok, unique = ctx8.verify_entities_compact(**a(**kw))               # a proof of the wrong shape is an invalid proof
        assert ok.tolist() == [0] * 8 and unique == 0, kw
    okb, uniq = np.full(4, 0xAB, np.uint8), ctypes.c_uint64(12345)        # b = 0: nothing is touched but the count
    rC, rH = np.frombuffer(h6.root[0], np.uint8).copy(), np.frombuffer(h6.root[1], np.uint8).copy()
    assert lib.dapol_verify_entities_compact(ctx8.h, 6, 0, None, None, None, 0, None, None, p(rC), p(rH), 0, 3, 8, None, 0, None, p(okb), ctypes.byref(uniq)) == 0
    assert (okb == 0xAB).all() and uniq.value == 0
    ok, unique = ctx8.verify_entities_compact(**a())                      # the call after the refusals is healthy
    assert ok.tolist() == [1] * 8 and unique == 21


# ------------------------------------------------------------------------------------------------ 7. the proof store
@pytest.mark.parametrize("leaf_first", ORDERS)
@pytest.mark.parametrize("policy,agg", [(0, 3), (1, 5), (0, 0), (0, 6)])
def test_store_read_compact(hip_lib, ctx8, policy, agg, leaf_first):
    """read_compact() = compress(read of all rows): after the first refresh, after an update of one leaf and a refresh (in place), and
    after an insert that moves rows."""
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        idx, v, r, tree = _tree(hip_lib, ctx8, 6, H6_LEAVES, seed=9)
        store = hip_lib.ProofStore(tree, policy, agg, 8, SEED)
        try:
            cidx, compact = store.read_compact()                          # an empty store
            assert (len(cidx), len(compact)) == (0, 0)

            def check(rows):
                ridx, _, _, blobs = store.read()
                cidx, compact = store.read_compact()
                assert len(ridx) == rows and cidx.tolist() == ridx.tolist()
                assert compact.tobytes() == hip_lib.shared_compress(6, ridx, policy, agg, 8, blobs).tobytes()
                assert hip_lib.shared_expand(6, ridx, policy, agg, 8, compact).tobytes() == blobs.tobytes()
                assert len(compact) == hip_lib.shared_compact_plan(6, ridx, policy, agg, 8)[2]
                return compact

            store.refresh()
            first = check(8)
            tree.update(np.array([17], np.uint64), np.array([5], np.uint64), r[:1])
            store.refresh()
            assert check(8).tobytes() != first.tobytes()
            tree.insert(np.array([9, 41], np.uint64), np.array([1, 2], np.uint64), r[1:3])
            store.refresh()
            check(10)
            # a cap one byte short writes nothing
            lib, out, n = hip_lib.lib(), np.full(len(first) * 2, 0xAB, np.uint8), ctypes.c_uint64(777)
            need = hip_lib.shared_compact_plan(6, store.read()[0], policy, agg, 8)[2]
            assert lib.dapol_proof_store_read_compact(store.h, out.ctypes.data_as(ctypes.c_void_p), need - 1, ctypes.byref(n)) == 8
            assert (out == 0xAB).all() and n.value == 777
        finally:
            store.close()
    finally:
        hip_lib.wire_config_restore(old)
