"""dapol_tree_derive_leaves / dapol_tree_insert_liabilities: new liabilities join a built tree BY ID.  The rule is the reference's
shuffle_index (src/dapol/mod.rs:408-441) with tree_index_set starting as the tree's current leaves.  Expected values come from
oracle/pyref.py: with nothing removed, build_leaf_nodes over (old + new) -- the first n0 rows are the tree, the others what the batch
must get; after removals, shuffle_index walked over the batch with taken = the surviving leaves.  The liabilities, seed and sizes are
fixed, and every case first asserts -- from the oracle -- that its inputs really collide (with old leaves, with earlier new ones, with
both), so that no case passes on inputs whose first candidates are all free."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
AUDIT = b"audit"
DIGESTS = ["blake3", "blake2s"]


def _liabs(a, b):
    return [(b"int-%d" % i, b"ext-%d" % (i * 7), i + 1) for i in range(a, b)]


def _dg(hip_lib, digest):
    return hip_lib.DIGEST_BLAKE3 if digest == "blake3" else hip_lib.DIGEST_BLAKE2S


def _same_tree(a, b, n_levels, what):
    assert a.root() == b.root(), what
    assert a.node_count() == b.node_count(), what
    for level in range(n_levels):
        for x, y in zip(a.level_nodes(level), b.level_nodes(level)):
            assert np.array_equal(x, y), (what, level)


class _Rows:
    """Leaf rows (index, value, blinding), sorted by index, with the input position of each."""

    def __init__(self, rows):                              # [(idx, v, r int, input position)]
        rows = sorted(rows)
        self.idx = np.array([x[0] for x in rows], np.uint64)
        self.v = np.array([x[1] for x in rows], np.uint64)
        self.r = np.frombuffer(b"".join(x[2].to_bytes(32, "little") for x in rows), np.uint8).reshape(len(rows), 32).copy()
        self.order = np.array([x[3] for x in rows], np.uint32)

    def leaves(self):
        return self.idx, self.v, self.r


_ORACLE = {}


def _oracle(pyref, height, n0, k, digest):
    """pyref.build_leaf_nodes over the n0 old and the k new liabilities, computed once per shape: (old rows, new rows, all rows,
    idx_by_entity of the new ones, seeds).  seeds[j] = (index_seed, blinding) of liability j, for the walks below."""
    key = (height, n0, k, digest)
    if key not in _ORACLE:
        liabs = _liabs(0, n0 + k)
        _, id_map = pyref.build_leaf_nodes(liabs, AUDIT, height, digest)
        seeds = []
        for iid, eid, _ in liabs:
            audit_id = pyref.digest(digest, AUDIT, iid)
            seeds.append((pyref.digest(digest, audit_id, b"index_seed", eid), pyref.scalar_from_bits(pyref.digest(digest, audit_id, b"blind_seed", eid))))
        by_e = [id_map[l[0]] for l in liabs]
        row = lambda j, base: (by_e[j], liabs[j][2], seeds[j][1], j - base)
        _ORACLE[key] = (_Rows([row(j, 0) for j in range(n0)]), _Rows([row(j, n0) for j in range(n0, n0 + k)]),
                        _Rows([row(j, 0) for j in range(n0 + k)]), by_e[n0:], seeds)
    return _ORACLE[key]


def _candidates(pyref, index_seed, height, digest, final):
    """The candidates shuffle_index drew for a liability that ended at `final`, in order (the last one is `final`)."""
    out = []
    while not out or out[-1] != final:
        index_seed = pyref.digest(digest, index_seed)
        out.append(int.from_bytes(index_seed[:8], "big") >> (64 - height))
        assert len(out) <= 128
    return out


def _collisions(pyref, height, n0, k, digest):
    """(met an old leaf, met an earlier new liability, met both, first candidate is an old leaf) among the k new liabilities."""
    old, _, _, by_e, seeds = _oracle(pyref, height, n0, k, digest)
    old_set, earlier = set(int(x) for x in old.idx), set()
    met_old = met_new = met_both = first_old = 0
    for j in range(k):
        walk = _candidates(pyref, seeds[n0 + j][0], height, digest, by_e[j])
        a, b = any(c in old_set for c in walk), any(c in earlier for c in walk)
        met_old, met_new, met_both, first_old = met_old + a, met_new + b, met_both + (a and b), first_old + (walk[0] in old_set)
        earlier.add(by_e[j])
    return met_old, met_new, met_both, first_old


def _walk(pyref, seeds, height, digest, taken, max_tries=128):
    """The sequential rule over a batch: pyref.shuffle_index with `taken` starting as the current leaves.  (indexes, None), or
    (None, position within the batch of the liability that ran out of candidates)."""
    taken, out = set(taken), []
    for pos, (index_seed, _) in enumerate(seeds):
        idx = pyref.shuffle_index(index_seed, height, taken, digest, max_tries)
        if idx is None:
            return None, pos
        out.append(idx)
    return out, None


def _check_derived(out, want, by_e):
    assert [int(x) for x in out["leaf_idx"]] == [int(x) for x in want.idx]
    assert [int(x) for x in out["idx_by_entity"]] == by_e
    assert np.array_equal(out["r"], want.r)
    assert np.array_equal(out["v"], want.v)
    assert np.array_equal(out["order"], want.order)


@contextlib.contextmanager
def _env(**knobs):
    saved = {k: os.environ.get(k) for k in knobs}
    os.environ.update({k: v for k, v in knobs.items() if v is not None})
    try:
        yield
    finally:
        for k, val in saved.items():
            if val is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = val


def _join(hip_lib, gpu_ctx, pyref, height, n0, k, digest, path=None, every_level=True):
    """derive_leaves on a tree over the old rows, then insert_liabilities on it: the oracle's rows, and the build over all of them."""
    old, new, both, by_e, _ = _oracle(pyref, height, n0, k, digest)
    tree = hip_lib.Tree(gpu_ctx, height, *old.leaves(), SEED)
    before = tree.root()
    _check_derived(tree.derive_leaves(_liabs(n0, n0 + k), AUDIT, _dg(hip_lib, digest)), new, by_e)
    assert tree.root() == before                           # deriving writes nothing
    got = tree.insert_liabilities(_liabs(n0, n0 + k), AUDIT, _dg(hip_lib, digest))
    assert [int(x) for x in got] == by_e
    if path is not None:
        assert tree.last_update_path() in path
    want = hip_lib.Tree(gpu_ctx, height, *both.leaves(), SEED)
    if every_level:
        _same_tree(tree, want, height + 1, (height, n0, k, digest))
    assert tree.root() == want.root() and tree.node_count() == want.node_count()
    assert tree.root()[2] == sum(range(1, n0 + k + 1))
    tree.close()
    want.close()


@pytest.mark.parametrize("digest", DIGESTS)
def test_case1_half_full_tree_outside_the_gate(hip_lib, gpu_ctx, pyref, digest):
    """Height 9, 128 old + 128 new: the oracle counts 41 / 36 new liabilities (BLAKE3 / Blake2s) that meet an old leaf, 22 / 23 that meet
    an earlier new one, 16 / 10 that meet both.  128 > 128 / 8 + 1: the insert rebuilds (path 0)."""
    met_old, met_new, met_both, _ = _collisions(pyref, 9, 128, 128, digest)
    assert met_old >= 20 and met_new >= 10 and met_both >= 5, (met_old, met_new, met_both)
    _join(hip_lib, gpu_ctx, pyref, 9, 128, 128, digest, path=(0,))


@pytest.mark.parametrize("digest", DIGESTS)
def test_case2_inside_the_in_place_gate(hip_lib, gpu_ctx, pyref, digest):
    """Height 12, 1,024 old + 64 new: 19 / 23 first candidates are old leaves; the batch goes in place (path 2 or 5)."""
    assert _collisions(pyref, 12, 1024, 64, digest)[3] >= 10
    _join(hip_lib, gpu_ctx, pyref, 12, 1024, 64, digest, path=(2, 5))


@pytest.mark.parametrize("digest", DIGESTS)
def test_case3_batch_crosses_a_block(hip_lib, gpu_ctx, pyref, digest):
    """Height 10, 200 old + 300 new (more than one 256-thread block): 73 / 77 meet old leaves, 67 / 58 earlier new ones."""
    met_old, met_new, _, _ = _collisions(pyref, 10, 200, 300, digest)
    assert met_old >= 20 and met_new >= 20, (met_old, met_new)
    old, new, both, by_e, _ = _oracle(pyref, 10, 200, 300, digest)
    tree = hip_lib.Tree(gpu_ctx, 10, *old.leaves(), SEED)
    got = tree.insert_liabilities(_liabs(200, 500), AUDIT, _dg(hip_lib, digest))
    assert [int(x) for x in got] == by_e
    want = hip_lib.Tree(gpu_ctx, 10, *both.leaves(), SEED)
    assert tree.root() == want.root()
    assert np.array_equal(tree.level_nodes(0)[0], want.level_nodes(0)[0])


@pytest.mark.parametrize("digest", DIGESTS)
@pytest.mark.parametrize("height,n0,k", [(5, 8, 8), (6, 1, 31), (63, 5, 6), (64, 5, 6)])
def test_case4_small_edges(hip_lib, gpu_ctx, pyref, digest, height, n0, k):
    """The sparsity bound met exactly (2^5 = 2 * 16); a binary search over ONE leaf; height 63 (the last with a spare key for "empty")
    and height 64 (the one-lane resolver): nothing collides up there, the point is that both paths return the oracle's indexes."""
    _join(hip_lib, gpu_ctx, pyref, height, n0, k, digest)


@pytest.mark.parametrize("digest", DIGESTS)
def test_case4_one_lane_resolver_with_real_collisions(hip_lib, gpu_ctx, pyref, digest):
    """Case 1 under DAPOL_LEAF_SERIAL=1: k_leaf_resolve's look-up, with the collisions case 1 asserts."""
    old, new, _, by_e, _ = _oracle(pyref, 9, 128, 128, digest)
    tree = hip_lib.Tree(gpu_ctx, 9, *old.leaves(), SEED)
    with _env(DAPOL_LEAF_SERIAL="1"):
        _check_derived(tree.derive_leaves(_liabs(128, 256), AUDIT, _dg(hip_lib, digest)), new, by_e)
    tree.close()


@pytest.mark.parametrize("digest", DIGESTS)
def test_case5_after_a_removal(hip_lib, gpu_ctx, pyref, digest):
    """Height 9, 128 old.  Of the old leaves that some new liability's FIRST candidate hits (by index), every second one is removed: 15 leaves for both digests.  The 128 new liabilities then follow the sequential rule over the survivors:
    the oracle finds 17 / 16 of them elsewhere than in case 1, and 15 on a removed slot."""
    height, n0, k = 9, 128, 128
    old, _, _, by_e1, seeds = _oracle(pyref, height, n0, k, digest)
    old_set = set(int(x) for x in old.idx)
    firsts = {int.from_bytes(pyref.digest(digest, index_seed)[:8], "big") >> (64 - height) for index_seed, _ in seeds[n0:]}
    gone = sorted(firsts & old_set)[::2]
    assert len(gone) == 15
    survivors = old_set - set(gone)
    want_idx, fail = _walk(pyref, seeds[n0:], height, digest, survivors)
    assert fail is None
    assert sum(a != b for a, b in zip(want_idx, by_e1)) >= 8
    assert sum(x in set(gone) for x in want_idx) >= 8
    tree = hip_lib.Tree(gpu_ctx, height, *old.leaves(), SEED)
    tree.remove(np.array(gone, np.uint64))
    out = tree.derive_leaves(_liabs(n0, n0 + k), AUDIT, _dg(hip_lib, digest))
    assert [int(x) for x in out["idx_by_entity"]] == want_idx
    assert [int(x) for x in out["leaf_idx"]] == sorted(want_idx)
    got = tree.insert_liabilities(_liabs(n0, n0 + k), AUDIT, _dg(hip_lib, digest))
    assert [int(x) for x in got] == want_idx
    keep = np.array([int(x) not in set(gone) for x in old.idx])
    new = _Rows([(want_idx[j], n0 + j + 1, seeds[n0 + j][1], j) for j in range(k)])
    idx = np.concatenate([old.idx[keep], new.idx])
    o = np.argsort(idx, kind="stable")
    want = hip_lib.Tree(gpu_ctx, height, idx[o], np.concatenate([old.v[keep], new.v])[o], np.concatenate([old.r[keep], new.r])[o], SEED)
    _same_tree(tree, want, height + 1, digest)


@pytest.mark.parametrize("digest", DIGESTS)
@pytest.mark.parametrize("serial", [False, True])
def test_case6_failed_to_map_index(hip_lib, gpu_ctx, pyref, digest, serial):
    """Case 1's tree, built under the real limit; DAPOL_LEAF_MAX_TRIES lowered for the insert only.  The oracle: 1, 2, 3 and 5 tries fail
    at batch position 1, 1, 24, 24 (BLAKE3) and 2, 2, 2, none (Blake2s).  Code 5, the message's position, nothing inserted."""
    height, n0, k = 9, 128, 128
    old, _, _, by_e, seeds = _oracle(pyref, height, n0, k, digest)
    old_set = set(int(x) for x in old.idx)
    tree = hip_lib.Tree(gpu_ctx, height, *old.leaves(), SEED)
    same = hip_lib.Tree(gpu_ctx, height, *old.leaves(), SEED)
    fails = []
    with _env(DAPOL_LEAF_SERIAL="1" if serial else None, DAPOL_LEAF_MAX_TRIES="128"):
        for tries in (1, 2, 3, 5):
            os.environ["DAPOL_LEAF_MAX_TRIES"] = str(tries)
            want_idx, want_fail = _walk(pyref, seeds[n0:], height, digest, old_set, tries)
            fails.append(want_fail)
            if want_fail is None:
                out = tree.derive_leaves(_liabs(n0, n0 + k), AUDIT, _dg(hip_lib, digest))
                assert [int(x) for x in out["idx_by_entity"]] == want_idx == by_e
                continue
            for call in (tree.derive_leaves, tree.insert_liabilities):
                with pytest.raises(hip_lib.DapolError) as e:
                    call(_liabs(n0, n0 + k), AUDIT, _dg(hip_lib, digest))
                assert e.value.code == 5
                assert "within %d tries (liability %d in input order)" % (tries, want_fail) in str(e.value)
            _same_tree(tree, same, height + 1, (digest, tries))
    assert fails == ([1, 1, 24, 24] if digest == "blake3" else [2, 2, 2, None])


def test_case7_refusals_leave_the_tree_as_it_was(hip_lib, gpu_ctx, pyref):
    height, n0 = 6, 16
    old, _, _, _, _ = _oracle(pyref, height, n0, 16, "blake3")
    tree = hip_lib.Tree(gpu_ctx, height, *old.leaves(), SEED)
    same = hip_lib.Tree(gpu_ctx, height, *old.leaves(), SEED)

    def refused(code, liabs, t=tree, digest=hip_lib.DIGEST_BLAKE3, says=None):
        for call in (t.derive_leaves, t.insert_liabilities):
            with pytest.raises(hip_lib.DapolError) as e:
                call(liabs, AUDIT, digest)
            assert e.value.code == code, str(e.value)
            assert says is None or says in str(e.value)

    refused(4, _liabs(16, 20) + [_liabs(17, 18)[0][:1] + (b"other", 9)])             # an internal id twice in the batch
    refused(2, _liabs(16, 33))                                                       # 2^6 < 2 (16 + 17)
    refused(3, _liabs(16, 20), digest=hip_lib.DIGEST_BLAKE2B)
    assert len(tree.derive_leaves([], AUDIT)["leaf_idx"]) == 0                       # k = 0: nothing to do
    assert len(tree.insert_liabilities([], AUDIT)) == 0
    _same_tree(tree, same, height + 1, "refusals")
    assert len(tree.insert_liabilities(_liabs(16, 32), AUDIT)) == 16                 # ... and exactly at the bound it goes in
    # a shard tree holds only its shard's leaves: not the whole occupied set
    top = old.idx >> np.uint64(height - 1) == 0
    shard = hip_lib.Tree(gpu_ctx, height, old.idx[top], old.v[top], old.r[top], SEED, shard_bits=1)
    root = shard.root()
    refused(8, _liabs(16, 18), t=shard, says="shard")
    assert shard.root() == root
    # a tree on a Blake2b context: leaf derivation under Blake2b is what Dapol::new refuses
    ctx_b = hip_lib.Context(0, 8, digest=hip_lib.DIGEST_BLAKE2B)
    wide = hip_lib.Tree(ctx_b, height, *old.leaves(), SEED)
    root = wide.root()
    refused(3, _liabs(16, 18), t=wide, digest=hip_lib.DIGEST_BLAKE2B)
    assert wide.root() == root
    wide.close()
    ctx_b.close()


def test_case8_proof_store_after_an_id_insert(hip_lib, gpu_ctx, pyref):
    """No store code changes with the id insert; this pins the interplay: refresh on the edited tree, then every row verifies."""
    height, n0, k, n_bits = 6, 16, 16, 16
    old, _, _, by_e, _ = _oracle(pyref, height, n0, k, "blake3")
    tree = hip_lib.Tree(gpu_ctx, height, *old.leaves(), SEED)
    store = hip_lib.ProofStore(tree, hip_lib.POLICY_PADDING, 3, n_bits, SEED)
    try:
        assert store.refresh()[0] > 0 and store.rows == n0
        tree.insert_liabilities(_liabs(n0, n0 + 2), AUDIT)
        assert not store.verify().all()                    # stale: the root moved
        store.refresh()
        assert store.rows == n0 + 2 and store.verify().tolist() == [1] * (n0 + 2)
        assert [int(x) for x in store.read()[0]] == sorted([int(x) for x in old.idx] + by_e[:2])
    finally:
        store.close()
        tree.close()
