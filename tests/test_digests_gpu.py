"""SHA-256 and SHA3-256 as node and leaf-derivation digests (DAPOL_DIGEST_SHA256 = 4, DAPOL_DIGEST_SHA3_256 = 5) on the GPU.  Every call
goes through the C ABI on a context of that digest; the checker is oracle/pyref.py with hashlib's sha256 / sha3_256 registered as its
digests (OpenSSL; pinned by tests/test_digests_cpu.py), and hashlib itself for the device unit."""
import os

import numpy as np
import pytest

import digest_shims as S
from test_digests_cpu import KAT_INDEX, KAT_LIABILITIES

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
NAMES = sorted(S.NEW_DIGESTS)
N_BITS = 8
EID_LENGTHS = (13, 14, 21, 22, 23, 77, 78, 93, 94, 95)   # audit_id (32) || "index_seed" (10) || eid: 55, 56, 63, 64, 65, 119, 120, 135, 136, 137 bytes


@pytest.fixture(scope="module")
def oracle(pyref):
    S.register(pyref)
    return pyref


@pytest.fixture(scope="module")
def ctxs(hip_lib):
    """one context of 8 parties per digest, and a BLAKE3 one to disagree with"""
    out = {name: hip_lib.Context(0, 8, digest=S.NEW_DIGESTS[name][0]) for name in NAMES}
    out["blake3"] = hip_lib.Context(0, 8)
    return out


def _levels(tree, height):
    """{level: {index: (v, r, C, H, is padding)}} of every stored node"""
    out = {}
    for k in range(height + 1):
        idx, v, r, C, H, pad = tree.level_nodes(k)
        out[k] = {int(i): (int(vv), rr.tobytes(), c.tobytes(), h.tobytes(), int(p)) for i, vv, rr, c, h, p in zip(idx, v, r, C, H, pad)}
    return out


def _same_as_oracle(tree, pt, height):
    for k in range(height + 1):
        idx, v, r, C, H, pad = tree.level_nodes(k)
        assert H.shape[1] == 32
        got = {int(i): (int(vv), c.tobytes(), h.tobytes()) for i, vv, c, h in zip(idx, v, C, H)}
        assert got == {i: (n.v, n.C, n.H) for i, n in pt.levels[k].items()}, k
        assert {int(i) for i, p in zip(idx, pad) if p} == pt.pad[k], k


def _liabilities(n, first=0):
    """ids whose hash inputs end at every padding edge of both digests, one internal id of 1,500 bytes"""
    out = []
    for i in range(first, first + n):
        iid = b"int-%04d" % i + (b"x" * 1492 if i == first + 3 else b"")
        out.append((iid, bytes((7 * i + k) & 255 for k in range(EID_LENGTHS[i % len(EID_LENGTHS)])), 3 * i + 1))
    return out


class _env:
    """environment variables for the block: a value of None removes the variable"""

    def __init__(self, **kv):
        self.kv = kv

    def _set(self, kv):
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.kv}
        self._set(self.kv)

    def __exit__(self, *exc):
        self._set(self.saved)


# ------------------------------------------------------------------------------------------------ 5. device unit
@pytest.fixture(scope="module")
def shims():
    return S.host_cases(), S.dev_cases()


@pytest.mark.parametrize("name", NAMES)
def test_device_streaming_digest_and_node_hashes(shims, name):
    """The gfx950 compilation of hash.h: one launch in which lane L hashes the L-byte counter pattern through the streaming digest
    (L = 0 .. 299), one launch of both node hashes on 64 random inputs, all zero and all 0xFF -- against hashlib, and word for word
    against the host's compilation of the same text."""
    host, dev = shims
    kind, ctor = S.NEW_DIGESTS[name]
    got = dev.stream_cases(kind, S.DEV_LANES)
    for n in range(S.DEV_LANES):
        assert got[n].astype("<u4").tobytes() == ctor(S.counter(n)).digest(), n
    assert np.array_equal(got, host.stream_cases(kind, S.DEV_LANES))
    inputs = S.node_inputs()
    d32, d128 = dev.node_cases(kind, inputs)
    for i, row in enumerate(inputs):
        b = row.astype("<u4").tobytes()
        assert d32[i].astype("<u4").tobytes() == ctor(b[:32]).digest() and d128[i].astype("<u4").tobytes() == ctor(b).digest(), i
    h32, h128 = host.node_cases(kind, inputs)
    assert np.array_equal(d32, h32) and np.array_equal(d128, h128)


# ------------------------------------------------------------------------------------------------ 6. tree
@pytest.mark.parametrize("name", NAMES)
def test_kat_tree_every_node(hip_lib, ctxs, oracle, name):
    """The reference's KAT liabilities at height 4 under the new digest: the indexes tests/test_digests_cpu.py pins, every node of
    every level, root value 26."""
    ctx, dg = ctxs[name], S.NEW_DIGESTS[name][0]
    out = ctx.build_leaf_nodes(KAT_LIABILITIES, b"test", 4, dg)
    assert [int(x) for x in out["idx_by_entity"]] == [KAT_INDEX[name][l[0]] for l in KAT_LIABILITIES]
    tree = hip_lib.Tree(ctx, 4, out["leaf_idx"], out["v"], out["r"], SEED, enforce_sparsity=True)
    pt, id_map = oracle.dapol_new(KAT_LIABILITIES, b"test", 4, SEED, dg=name)
    assert id_map == KAT_INDEX[name]
    C, H, v, r = tree.root()
    assert (C, H, v) == (pt.root.C, pt.root.H, 26)
    _same_as_oracle(tree, pt, 4)


@pytest.mark.parametrize("name", NAMES)
def test_derived_tree_every_node(hip_lib, ctxs, oracle, name):
    """24 derived leaves at height 8"""
    ctx, dg = ctxs[name], S.NEW_DIGESTS[name][0]
    liab = _liabilities(24)
    out = ctx.build_leaf_nodes(liab, b"audit seed", 8, dg)
    tree = hip_lib.Tree(ctx, 8, out["leaf_idx"], out["v"], out["r"], SEED, enforce_sparsity=True)
    pt, id_map = oracle.dapol_new(liab, b"audit seed", 8, SEED, dg=name)
    assert [int(x) for x in out["idx_by_entity"]] == [id_map[l[0]] for l in liab]
    assert tree.root()[:3] == (pt.root.C, pt.root.H, pt.root.v)
    _same_as_oracle(tree, pt, 8)


# ------------------------------------------------------------------------------------------------ 7. leaf derivation under collisions
@pytest.mark.parametrize("height,n", [(6, 16), (8, 64)])
@pytest.mark.parametrize("name", NAMES)
def test_leaf_derivation_vs_oracle_with_collisions(ctxs, oracle, name, height, n):
    """Heights that force retries of shuffle_index; external ids that put the hash inputs' ends on both digests' padding edges."""
    ctx, dg = ctxs[name], S.NEW_DIGESTS[name][0]
    liab, seed = _liabilities(n), b"audit seed 3"             # (a seed under which all four cases collide on their first candidates)
    leaves, idm = oracle.build_leaf_nodes(liab, seed, height, name)
    first = [oracle.shuffle_index(oracle.digest(name, oracle.digest(name, seed, i_), b"index_seed", e_), height, set(), name) for i_, e_, _ in liab]
    assert len(set(first)) < n, "the case must exercise collisions"
    out = ctx.build_leaf_nodes(liab, seed, height, dg)
    assert [int(x) for x in out["idx_by_entity"]] == [idm[l[0]] for l in liab]
    assert [int(x) for x in out["leaf_idx"]] == [i for i, _ in leaves]
    for p, (i, nd) in enumerate(leaves):
        assert int(out["v"][p]) == nd.v and out["r"][p].tobytes() == nd.r.to_bytes(32, "little")
    with _env(DAPOL_LEAF_SERIAL="1"):                          # the one-lane resolution gives the same arrays
        ser = ctx.build_leaf_nodes(liab, seed, height, dg)
    for key in ("leaf_idx", "v", "r", "order", "idx_by_entity"):
        assert np.array_equal(ser[key], out[key]), key


@pytest.mark.parametrize("name", NAMES)
def test_leaf_derivation_refusals(hip_lib, ctxs, oracle, name):
    """DuplicatedInternalId, and FailedToMapIndex under the lowered limit DAPOL_LEAF_MAX_TRIES (the same code path as 128 tries, at
    the sparsity bound): the entity the reference's loop stops at, by both resolutions."""
    ctx, dg = ctxs[name], S.NEW_DIGESTS[name][0]
    with pytest.raises(hip_lib.DapolError) as e:
        ctx.build_leaf_nodes([(b"a", b"w", 1), (b"b", b"x", 2), (b"a", b"y", 3)], b"test", 8, dg)
    assert e.value.code == 4
    height, n = 9, 256
    liabs = [(b"int-%d" % i, b"ext-%d" % (i * 7), i + 1) for i in range(n)]
    seen = 0
    for serial in (None, "1"):
        for tries in (1, 3):
            try:
                want, want_fail = oracle.build_leaf_nodes(liabs, b"audit", height, name, max_tries=tries)[0], None
            except oracle.DapolError as err:
                want_fail = err.args[1]
            with _env(DAPOL_LEAF_MAX_TRIES=str(tries), DAPOL_LEAF_SERIAL=serial):
                if want_fail is None:
                    out = ctx.build_leaf_nodes(liabs, b"audit", height, dg)
                    assert [int(x) for x in out["leaf_idx"]] == [i for i, _ in want]
                else:
                    seen += 1
                    with pytest.raises(hip_lib.DapolError) as e:
                        ctx.build_leaf_nodes(liabs, b"audit", height, dg)
                    assert e.value.code == 5
                    assert "within %d tries (liability %d in input order)" % (tries, want_fail) in str(e.value)
    assert seen >= 2                                            # (one try cannot place 256 entities in 512 slots)


# ------------------------------------------------------------------------------------------------ 8. insert by liability id
@pytest.mark.parametrize("name", NAMES)
def test_insert_liabilities_equals_the_derivation_of_old_and_new(hip_lib, ctxs, oracle, name):
    ctx, dg = ctxs[name], S.NEW_DIGESTS[name][0]
    height, seed = 6, b"audit seed"
    old, new = _liabilities(8), _liabilities(8, first=8)
    out = ctx.build_leaf_nodes(old, seed, height, dg)
    tree = hip_lib.Tree(ctx, height, out["leaf_idx"], out["v"], out["r"], SEED)
    leaves, idm = oracle.build_leaf_nodes(old + new, seed, height, name)
    by_e = tree.insert_liabilities(new, seed, dg)
    assert [int(x) for x in by_e] == [idm[l[0]] for l in new]
    _same_as_oracle(tree, oracle.Tree(height, leaves, SEED, name), height)


# ------------------------------------------------------------------------------------------------ 9. prove and verify
@pytest.mark.parametrize("policy", ["padding", "splitting"])
@pytest.mark.parametrize("name", NAMES)
def test_prove_and_verify(hip_lib, ctxs, oracle, name, policy):
    """Height 4, aggregation factor 2: path hashes against the oracle's siblings, both verifiers, the batch proof for [a, b]; the
    same proofs under a BLAKE3 context and under the other new digest, and with one byte of a path hash flipped."""
    ctx, dg = ctxs[name], S.NEW_DIGESTS[name][0]
    pol = hip_lib.POLICY_PADDING if policy == "padding" else hip_lib.POLICY_SPLITTING
    out = ctx.build_leaf_nodes(KAT_LIABILITIES, b"test", 4, dg)
    tree = hip_lib.Tree(ctx, 4, out["leaf_idx"], out["v"], out["r"], SEED, enforce_sparsity=True)
    pt, id_map = oracle.dapol_new(KAT_LIABILITIES, b"test", 4, SEED, dg=name)
    leaf_idx = out["leaf_idx"]
    C, H, v, r = tree.root()
    pC, pH, proofs = tree.prove_entities(leaf_idx, pol, 2, N_BITS, SEED)
    for k, li in enumerate(leaf_idx):
        sibs = pt.path_siblings(int(li))
        assert [pH[k, s].tobytes() for s in range(4)] == [x.H for x in sibs]
        assert [pC[k, s].tobytes() for s in range(4)] == [x.C for x in sibs]
    lC, lH = ctx.commit_hash_batch(out["v"], out["r"])
    assert [h.tobytes() for h in lH] == [pt.levels[0][int(i)].H for i in leaf_idx]
    assert ctx.verify_entities(4, leaf_idx, lC, lH, pC, pH, C, H, pol, 2, N_BITS, proofs, verify_seed=SEED).all()
    batch = sorted([id_map[b"a"], id_map[b"b"]])
    at = [int(np.searchsorted(leaf_idx, np.uint64(i))) for i in batch]
    level, index, sC, sH, blob = tree.prove_batch(batch, pol, 2, N_BITS, SEED)
    assert [h.tobytes() for h in sH] == [pt.levels[lv][ix].H for lv, ix in oracle.batch_siblings(4, batch)]
    assert ctx.verify_batch(4, batch, lC[at], lH[at], sC, sH, C, H, pol, 2, N_BITS, blob, verify_seed=SEED)
    for other in ("blake3", [n for n in NAMES if n != name][0]):
        assert not ctxs[other].verify_batch(4, batch, lC[at], lH[at], sC, sH, C, H, pol, 2, N_BITS, blob, verify_seed=SEED)
        assert not ctxs[other].verify_entities(4, leaf_idx, lC, lH, pC, pH, C, H, pol, 2, N_BITS, proofs, verify_seed=SEED).any()
    bad = pH.copy()
    bad[1, 2, 17] ^= 0x20
    assert ctx.verify_entities(4, leaf_idx, lC, lH, pC, bad, C, H, pol, 2, N_BITS, proofs, verify_seed=SEED).tolist() == [1, 0, 1, 1]
    badb = sH.copy()
    badb[0, 31] ^= 1
    assert not ctx.verify_batch(4, batch, lC[at], lH[at], sC, badb, C, H, pol, 2, N_BITS, blob, verify_seed=SEED)


# ------------------------------------------------------------------------------------------------ 10. edits
@pytest.mark.parametrize("name", NAMES)
def test_edits_equal_a_fresh_build(hip_lib, ctxs, name):
    """update, insert and remove on a 16-leaf tree at height 8: after each, every level equals a fresh build over the same leaves."""
    ctx, height = ctxs[name], 8
    rng = np.random.default_rng(108)
    idx = np.sort(rng.choice(1 << height, size=22, replace=False).astype(np.uint64))
    v = rng.integers(0, 1 << 20, size=22, dtype=np.uint64)
    r = rng.integers(0, 256, size=(22, 32), dtype=np.uint8)
    r[:, 31] &= 0x0F
    live = {int(i): (int(vv), rr.copy()) for i, vv, rr in zip(idx[:16], v[:16], r[:16])}

    def fresh():
        ii = np.array(sorted(live), np.uint64)
        return hip_lib.Tree(ctx, height, ii, np.array([live[int(i)][0] for i in ii], np.uint64), np.stack([live[int(i)][1] for i in ii]), SEED)

    tree = fresh()
    # update: three leaves get new values and blindings
    for i in idx[[1, 7, 15]]:
        live[int(i)] = (live[int(i)][0] + 5, np.roll(live[int(i)][1], 1) & 0x7F)
    tree.update(idx[[1, 7, 15]], [live[int(i)][0] for i in idx[[1, 7, 15]]], np.stack([live[int(i)][1] for i in idx[[1, 7, 15]]]))
    assert _levels(tree, height) == _levels(fresh(), height)
    # insert: six new leaves, out of order
    new = idx[16:][::-1]
    for i, vv, rr in zip(idx[16:], v[16:], r[16:]):
        live[int(i)] = (int(vv), rr.copy())
    tree.insert(new, [live[int(i)][0] for i in new], np.stack([live[int(i)][1] for i in new]))
    assert _levels(tree, height) == _levels(fresh(), height)
    # remove: three leaves
    gone = sorted(live)[2:5]
    for i in gone:
        del live[i]
    tree.remove(gone)
    assert _levels(tree, height) == _levels(fresh(), height)


# ------------------------------------------------------------------------------------------------ 11. paths with no hashing of their own
@pytest.mark.parametrize("name", NAMES)
def test_shared_prover_store_and_shards(hip_lib, ctxs, name):
    """A 12-leaf tree at height 8, padding / 3: the shared prover under both verifiers, the proof store across an edit, and two
    logical shards whose replicated top merge gives the unsharded root."""
    from dapol_amd import sharded
    ctx, height, pol, agg = ctxs[name], 8, hip_lib.POLICY_PADDING, 3
    rng = np.random.default_rng(811)
    idx = np.sort(np.concatenate([rng.choice(128, size=6, replace=False).astype(np.uint64) + np.uint64(128 * s) for s in range(2)]))
    v = rng.integers(0, 16, size=12, dtype=np.uint64)
    r = rng.integers(0, 256, size=(12, 32), dtype=np.uint8)
    r[:, 31] &= 0x0F
    tree = hip_lib.Tree(ctx, height, idx, v, r, SEED)
    C, H, rv, rr = tree.root()
    lC, lH = ctx.commit_hash_batch(v, r)
    pC, pH, blobs, unique = tree.prove_entities_shared(idx, pol, agg, N_BITS, SEED)
    ok = ctx.verify_entities(height, idx, lC, lH, pC, pH, C, H, pol, agg, N_BITS, blobs, verify_seed=SEED)
    ok_shared, _ = ctx.verify_entities_shared(height, idx, lC, lH, pC, pH, C, H, pol, agg, N_BITS, blobs, verify_seed=SEED)
    assert ok.tolist() == ok_shared.tolist() == [1] * 12
    bad = pH.copy()
    bad[5, 0, 0] ^= 1
    ok = ctx.verify_entities(height, idx, lC, lH, pC, bad, C, H, pol, agg, N_BITS, blobs, verify_seed=SEED)
    ok_shared, _ = ctx.verify_entities_shared(height, idx, lC, lH, pC, bad, C, H, pol, agg, N_BITS, blobs, verify_seed=SEED)
    assert ok.tolist() == ok_shared.tolist() == [1] * 5 + [0] + [1] * 6
    # two logical shards on one device
    recs = []
    for s in range(2):
        sel = (idx >> np.uint64(height - 1)) == s
        recs.append(sharded.pack_record(hip_lib.Tree(ctx, height, idx[sel], v[sel], r[sel], SEED, shard_bits=1).root()))
    records = sharded.unpack_records(np.stack(recs), 2)
    for s in range(2):
        root, upper = sharded.top_levels(ctx, records, s)
        assert root == (C, H, rv, rr)
    # the store: refresh, an edit, refresh, verify
    store = hip_lib.ProofStore(tree, pol, agg, N_BITS, SEED)
    try:
        store.refresh()
        assert store.rows == 12 and store.verify(SEED).tolist() == [1] * 12
        tree.update(idx[3:4], [int(v[3]) + 1], r[3:4])
        proved, kept, moved = store.refresh()
        assert proved > 0
        assert store.verify(SEED).tolist() == [1] * 12
    finally:
        store.close()


# ------------------------------------------------------------------------------------------------ 12. refusals
@pytest.mark.parametrize("bad", [3, 6, -1])
def test_other_digest_ids_stay_refused(hip_lib, ctxs, bad):
    """3 is reserved; everything but 0, 1, 2, 4, 5 is DapolError::InvalidDigestSize, as a node digest and as a leaf-derivation digest."""
    with pytest.raises(hip_lib.DapolError) as e:
        hip_lib.Context(0, 8, digest=bad)
    assert e.value.code == 3
    with pytest.raises(hip_lib.DapolError) as e:
        ctxs["sha256"].build_leaf_nodes(KAT_LIABILITIES, b"test", 4, bad)
    assert e.value.code == 3
