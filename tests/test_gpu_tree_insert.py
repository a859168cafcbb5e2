"""dapol_tree_insert: new leaves join a built tree, whatever nodes their chains share.  Padding nodes are keyed by position, so the tree
after an insert has exactly one correct form -- dapol_tree_build over the old and the new leaves with the tree's own pad seed -- and
every path (the disjoint-chain insert, the general in-place insert, the rebuild) must give it bit for bit at every level."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
NONCE = bytes(range(100, 132))


def _ref_root(ref, height, idx, v, r):
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    idx, v, r = np.ascontiguousarray(idx), np.ascontiguousarray(v), np.ascontiguousarray(r)
    t = ctypes.c_void_p(ref.ref_tree_build(height, ctypes.c_size_t(len(idx)), p(idx), p(v), p(r), SEED, 0))
    C, H, rr, vv = [ctypes.create_string_buffer(32) for _ in range(3)] + [ctypes.c_uint64()]
    ref.ref_tree_root(t, C, H, ctypes.byref(vv), rr)
    ref.ref_tree_free(t)
    return C.raw, H.raw, vv.value, rr.raw


def _rand_idx(rng, height, n, avoid=()):
    top = 1 << height
    out, avoid = set(), set(avoid)
    n = min(n, top - len(avoid))
    while len(out) < n:
        x = int(rng.integers(0, top - 1, dtype=np.uint64, endpoint=True))
        if x not in avoid:
            out.add(x)
    return out


def _with_values(rng, idx, bits=40, beyond_l=True):
    """(idx sorted, v, r) for a set of indexes; one blinding in sixteen is >= l (bit 255 aside, a leaf keeps it as given)."""
    idx = np.array(sorted(idx), np.uint64)
    v = rng.integers(0, 2**bits, size=len(idx), dtype=np.uint64)
    r = rng.integers(0, 256, size=(len(idx), 32), dtype=np.uint8)
    r[:, 31] &= 0x0F
    if beyond_l:
        r[::16, 31] |= 0x70
    return idx, v, r


def _union(a, b):
    idx = np.concatenate([a[0], b[0]])
    o = np.argsort(idx, kind="stable")
    return idx[o], np.concatenate([a[1], b[1]])[o], np.concatenate([a[2], b[2]])[o]


def _new_chains_share_a_node(old, new, height):
    """k_tree_ins_plan's rule, as in test_gpu_parity.py (Python integers, so that a shift by 64 is defined): a new leaf's chain runs up
    to its first ancestor that exists; do two (neighbouring) new leaves have chains that share a node?"""
    old, new = [int(x) for x in old], sorted(int(x) for x in new)
    level = [{x >> t for x in old} for t in range(height + 1)]
    for a in range(1, len(new)):
        m = next(t for t in range(height + 1) if (new[a] >> t) in level[t])
        if any((new[a] >> t) == (new[a - 1] >> t) for t in range(m)):
            return True
    return False


def _expected_path(height, old_idx, new_idx):
    """dapol_tree_insert's routing: inside the removal's gate in place -- the disjoint-chain insert (2) for up to 4,096 leaves whose
    chains share nothing, the general path (5) otherwise; outside it the rebuild (0)."""
    k = len(new_idx)
    if height < 1 or k > 65536 or k > len(old_idx) // 8 + 1:
        return 0
    return 2 if k <= 4096 and not _new_chains_share_a_node(old_idx, new_idx, height) else 5


def _same_tree(a, b, n_levels, what):
    assert a.root() == b.root(), what
    assert a.node_count() == b.node_count(), what
    for level in range(n_levels):
        for x, y in zip(a.level_nodes(level), b.level_nodes(level)):
            assert np.array_equal(x, y), (what, level)


class _forced_rebuild:
    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.saved = self.ctx.get_options()
        o = self.ctx.get_options()
        o.update_incremental_max = -1
        self.ctx.set_options(o)

    def __exit__(self, *a):
        self.ctx.set_options(self.saved)


def _check_insert(hip_lib, ctx, height, old, new, what, ref=None, shard_bits=0):
    """Inserts `new` (shuffled) into a tree over `old`, in place where the gate admits it and by the forced rebuild; both equal a
    fresh build over the union.  Returns the path the first took."""
    kw = {"shard_bits": shard_bits} if shard_bits else {}
    n_levels = height - shard_bits + 1
    both = _union(old, new)
    want = hip_lib.Tree(ctx, height, *both, SEED, **kw)
    assert want.root()[2] == int(both[1].sum(dtype=np.uint64))
    if ref is not None:
        assert want.root() == _ref_root(ref, height, *both), what
    order = np.random.default_rng(len(new[0])).permutation(len(new[0]))     # the batch arrives unsorted
    tr = hip_lib.Tree(ctx, height, *old, SEED, **kw)
    tr.insert(new[0][order], new[1][order], new[2][order])
    path = tr.last_update_path()
    assert path == _expected_path(n_levels - 1, old[0], new[0]), what
    _same_tree(tr, want, n_levels, what)
    probe = new[0][:4]
    for a, b in zip(tr.paths(probe), want.paths(probe)):
        assert np.array_equal(a, b), what
    tr.close()
    with _forced_rebuild(ctx):
        tr = hip_lib.Tree(ctx, height, *old, SEED, **kw)
        tr.insert(*new)
        assert tr.last_update_path() == 0, what
        _same_tree(tr, want, n_levels, what + " (rebuild)")
        tr.close()
    want.close()
    return path


def _shape(rng, height, n_old):
    """Old leaves that leave an aligned block and, where there is room, an aligned pair elsewhere and both ends of the range free."""
    top = 1 << height
    sub_bits = 3 if height > 4 else 2
    blk = int(rng.integers(0, top >> sub_bits, dtype=np.uint64)) << sub_bits
    block = {blk + i for i in range(1 << sub_bits)}
    if height == 4:
        return set(range(top)) - block, blk, sub_bits, blk
    pair = blk
    while pair in block:
        pair = int(rng.integers(1, (top >> 1) - 1, dtype=np.uint64)) * 2
    return _rand_idx(rng, height, n_old, avoid=block | {pair, pair + 1, 0, top - 1}), blk, sub_bits, pair


def _cases(rng, height, old, blk, sub_bits, pair):
    top = 1 << height
    block = {blk + i for i in range(1 << sub_bits)}
    free = (lambda n: _rand_idx(rng, height, n, avoid=old)) if height > 4 else (lambda n: set(sorted(set(range(top)) - old)[:n]))
    beside = next(x ^ 1 for x in sorted(old) if (x ^ 1) not in old) if height > 4 else None
    cases = {"one": free(1), "siblings": {pair, pair + 1}, "subtree": block, "random64": free(64), "subtree+20": block | free(20)}
    if beside is not None:
        cases["beside"] = {beside}
    for name, x in (("index0", 0), ("index_max", top - 1)):
        if x not in old:
            cases[name] = {x}
    return cases


@pytest.mark.parametrize("height,n_old", [(4, 12), (11, 600), (24, 1000), (32, 1000), (64, 1000)])
def test_insert_equals_build_every_level(hip_lib, ref, height, n_old):
    ctx = hip_lib.Context(0, 8)
    rng = np.random.default_rng(6000 + height)
    old_set, blk, sub_bits, pair = _shape(rng, height, n_old)
    old = _with_values(rng, old_set)
    oracle = ref if height <= 24 else None
    for name, new_set in _cases(rng, height, old_set, blk, sub_bits, pair).items():
        path = _check_insert(hip_lib, ctx, height, old, _with_values(rng, new_set), "h%d %s" % (height, name), oracle)
        if name == "one":
            assert path == 2
        if height >= 11 and name in ("siblings", "subtree", "subtree+20"):
            assert path == 5, name                                    # the shared-chain cases run on the general device path
    # a leaf in the so-far-empty half under the root (m = height); at height 4 beside an existing leaf as well
    half = 1 << (height - 1)
    low = _with_values(rng, {x for x in old_set if x < half} | {1})
    assert _check_insert(hip_lib, ctx, height, low, _with_values(rng, {half + (blk % half)}), "h%d empty half" % height, oracle) == 2
    if height == 4:
        assert _check_insert(hip_lib, ctx, height, _with_values(rng, set(range(2, 16, 2))), _with_values(rng, {3}), "h4 beside", oracle) == 2
    ctx.close()


def test_insert_across_the_disjoint_paths_size_limit(hip_lib):
    """5,000 new leaves (> 4,096, <= n0 / 8 + 1) into 40,000: the general path, whatever their chains share."""
    ctx = hip_lib.Context(0, 8)
    rng = np.random.default_rng(6101)
    height = 32
    old_set = _rand_idx(rng, height, 40000)
    old, new = _with_values(rng, old_set), _with_values(rng, _rand_idx(rng, height, 5000, avoid=old_set))
    want = hip_lib.Tree(ctx, height, *_union(old, new), SEED)
    tr = hip_lib.Tree(ctx, height, *old, SEED)
    order = rng.permutation(5000)
    tr.insert(new[0][order], new[1][order], new[2][order])
    assert tr.last_update_path() == 5
    _same_tree(tr, want, height + 1, "5000 into 40000")
    for a, b in zip(tr.paths(new[0][::625]), want.paths(new[0][::625])):
        assert np.array_equal(a, b)


def test_insert_and_remove_undo_each_other(hip_lib):
    ctx = hip_lib.Context(0, 8)
    rng = np.random.default_rng(6103)
    height = 20
    old_set, blk, sub_bits, pair = _shape(rng, height, 800)
    S = {pair, pair + 1} | {blk + i for i in range(8)} | _rand_idx(rng, height, 30, avoid=old_set)
    old, extra = _with_values(rng, old_set), _with_values(rng, S)
    small, big = hip_lib.Tree(ctx, height, *old, SEED), hip_lib.Tree(ctx, height, *_union(old, extra), SEED)
    tr = hip_lib.Tree(ctx, height, *old, SEED)
    tr.insert(*extra)
    assert tr.last_update_path() == 5
    _same_tree(tr, big, height + 1, "insert")
    tr.remove(extra[0])
    assert tr.last_update_path() == 4
    _same_tree(tr, small, height + 1, "insert + remove")
    tr2 = hip_lib.Tree(ctx, height, *_union(old, extra), SEED)
    tr2.remove(extra[0])
    tr2.insert(*extra)
    assert tr2.last_update_path() == 5
    _same_tree(tr2, big, height + 1, "remove + insert")


def test_tree_grows_leaf_by_leaf_through_insert(hip_lib, ref):
    """test_tree_grows_leaf_by_leaf_like_the_reference_test's shape through insert: from one leaf, 60 single inserts at height 10."""
    ctx = hip_lib.Context(0, 8)
    rng = np.random.default_rng(41)
    height, n = 10, 61
    idx, v, r = _with_values(rng, _rand_idx(rng, height, n))
    order = rng.permutation(n)
    tr = hip_lib.Tree(ctx, height, idx[order[:1]], v[order[:1]], r[order[:1]], SEED)
    for i in range(1, n):
        e = order[i:i + 1]
        tr.insert(idx[e], v[e], r[e])
        assert tr.last_update_path() == 2
        if i % 10 == 0 or i == n - 1:
            have = np.sort(order[:i + 1])
            _same_tree(tr, hip_lib.Tree(ctx, height, idx[have], v[have], r[have], SEED), height + 1, i)
    assert tr.root() == _ref_root(ref, height, idx, v, r)


@pytest.mark.parametrize("digest", ["DIGEST_BLAKE2S", "DIGEST_BLAKE2B"])
def test_insert_with_other_digests(hip_lib, digest):
    ctx = hip_lib.Context(0, 8, digest=getattr(hip_lib, digest))
    rng = np.random.default_rng(6107)
    height = 9
    old_set, blk, sub_bits, pair = _shape(rng, height, 90)
    old = _with_values(rng, old_set)
    for name, new_set in _cases(rng, height, old_set, blk, sub_bits, pair).items():
        _check_insert(hip_lib, ctx, height, old, _with_values(rng, new_set), digest + " " + name)
    ctx.close()


def test_insert_in_a_shard_tree(hip_lib):
    ctx = hip_lib.Context(0, 8)
    rng = np.random.default_rng(6109)
    total, bits, prefix = 20, 4, 9
    sub = total - bits
    low_old = _rand_idx(rng, sub, 400, avoid={6, 7})
    low_new = {6, 7} | _rand_idx(rng, sub, 20, avoid=low_old | {6, 7})
    under = lambda s: {x | (prefix << sub) for x in s}
    old, new = _with_values(rng, under(low_old), 32), _with_values(rng, under(low_new), 32)
    assert _check_insert(hip_lib, ctx, total, old, new, "shard", shard_bits=bits) == 5
    # a leaf of another prefix: refused as dapol_tree_update refuses the same batch, nothing written
    bad = _with_values(rng, {int(new[0][0]), ((prefix + 1) << sub) | 5}, 32)
    codes = []
    for call in ("update", "insert"):
        tr = hip_lib.Tree(ctx, total, *old, SEED, shard_bits=bits)
        before = tr.root()
        with pytest.raises(hip_lib.DapolError) as e:
            getattr(tr, call)(*bad)
        codes.append(e.value.code)
        assert tr.root() == before
        tr.close()
    assert codes[0] == codes[1]


def _root_of_handle(hip_lib, h):
    C, H, r = (ctypes.create_string_buffer(32) for _ in range(3))
    v = ctypes.c_uint64()
    assert hip_lib.lib().dapol_tree_root(h, C, H, ctypes.byref(v), r) == 0
    return C.raw, H.raw, v.value, r.raw


def test_insert_errors_leave_the_tree_unchanged(hip_lib):
    ctx = hip_lib.Context(0, 8)
    rng = np.random.default_rng(6113)
    height = 12
    old_set = _rand_idx(rng, height, 200)
    idx, v, r = _with_values(rng, old_set)
    fresh = _with_values(rng, _rand_idx(rng, height, 6, avoid=old_set))
    tr = hip_lib.Tree(ctx, height, idx, v, r, SEED)
    root0, lvl0 = tr.root(), [tr.level_nodes(t) for t in range(height + 1)]

    def unchanged():
        assert tr.root() == root0
        for t in range(height + 1):
            for a, b in zip(tr.level_nodes(t), lvl0[t]):
                assert np.array_equal(a, b)

    def batch(extra_idx):
        bi = np.concatenate([fresh[0], np.array(extra_idx, np.uint64)])
        k = len(bi)
        return bi, np.resize(fresh[1], k), np.resize(fresh[2], (k, 32))
    for how in (contextlib.nullcontext(), _forced_rebuild(ctx)):     # the in-place gate and the rebuild refuse alike
        with how:
            for extra, text in (([idx[17]], "already a leaf"), ([fresh[0][2]], "twice")):
                with pytest.raises(hip_lib.DapolError) as e:
                    tr.insert(*batch(extra))
                assert e.value.code == 8 and text in str(e.value), text
                unchanged()
    outside = batch([1 << height])
    twin = hip_lib.Tree(ctx, height, idx, v, r, SEED)
    with pytest.raises(hip_lib.DapolError) as eu:
        twin.update(*outside)
    with pytest.raises(hip_lib.DapolError) as ei:
        tr.insert(*outside)
    assert ei.value.code == eu.value.code
    unchanged()
    tr.insert([], [], np.zeros((0, 32), np.uint8))                    # k = 0
    unchanged()
    tr.insert(*fresh)                                                 # the tree is still usable
    assert tr.last_update_path() in (2, 5)
    _same_tree(tr, hip_lib.Tree(ctx, height, *_union((idx, v, r), fresh), SEED), height + 1, "after the refusals")
    # a tree built from a padding tape
    level, index = hip_lib.tree_padding_positions(height, idx)
    taped = hip_lib.Tree(ctx, height, idx, v, r, None, pad_tape=np.random.default_rng(1).integers(0, 256, size=64 * len(level), dtype=np.uint8).tobytes())
    troot = taped.root()
    with pytest.raises(hip_lib.DapolError) as e:
        taped.insert(*fresh)
    assert e.value.code == 8 and taped.root() == troot
    # a workload tree (it does not own its leaves)
    w = hip_lib.Workload(ctx, height, idx, v, r)
    w.build(SEED)
    h = w.tree_handle()
    wroot = _root_of_handle(hip_lib, h)
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)
    assert hip_lib.lib().dapol_tree_insert(h, 1, p(fresh[0]), p(fresh[1]), p(fresh[2])) == 8
    assert _root_of_handle(hip_lib, h) == wroot
    w.close()


def test_failed_in_place_insert_marks_the_tree_invalid(hip_lib):
    ctx = hip_lib.Context(0, 8)
    rng = np.random.default_rng(6121)
    height = 10
    old_set, blk, sub_bits, pair = _shape(rng, height, 100)
    idx, v, r = _with_values(rng, old_set)
    new = _with_values(rng, {pair, pair + 1})
    tr = hip_lib.Tree(ctx, height, idx, v, r, SEED)
    saved = os.environ.get("DAPOL_TEST_FAIL_INSERT_MIDWAY")
    os.environ["DAPOL_TEST_FAIL_INSERT_MIDWAY"] = "1"
    try:
        with pytest.raises(hip_lib.DapolError) as e:
            tr.insert(*new)
    finally:
        if saved is None:
            os.environ.pop("DAPOL_TEST_FAIL_INSERT_MIDWAY", None)
        else:
            os.environ["DAPOL_TEST_FAIL_INSERT_MIDWAY"] = saved
    assert e.value.code == 17
    for call in (tr.root, tr.node_count, lambda: tr.level_nodes(0), lambda: tr.insert(*new), lambda: tr.remove(idx[2:3]), lambda: tr.update(idx[:1], v[:1], r[:1])):
        with pytest.raises(hip_lib.DapolError) as e:
            call()
        assert e.value.code == 8 and "left inconsistent" in str(e.value)
    tr.close()


def test_proofs_after_an_insert(hip_lib):
    ctx = hip_lib.Context(0, 16)
    rng = np.random.default_rng(6127)
    height, n_bits, agg = 11, 16, 4
    old_set, blk, sub_bits, pair = _shape(rng, height, 300)
    old = _with_values(rng, old_set, 6, beyond_l=False)               # subtree sums stay inside the 16-bit ranges
    new = _with_values(rng, {pair, pair + 1, blk, blk + 5} | _rand_idx(rng, height, 10, avoid=old_set), 6, beyond_l=False)
    tr = hip_lib.Tree(ctx, height, *old, SEED)
    tr.insert(*new)
    assert tr.last_update_path() == 5
    fresh = hip_lib.Tree(ctx, height, *_union(old, new), SEED)
    probe = np.array(sorted([pair, pair + 1, blk, blk + 5]), np.uint64)
    C, H, proofs = tr.prove_entities(probe, hip_lib.POLICY_PADDING, agg, n_bits, NONCE)
    fC, fH, fproofs = fresh.prove_entities(probe, hip_lib.POLICY_PADDING, agg, n_bits, NONCE)
    assert np.array_equal(C, fC) and np.array_equal(H, fH) and np.array_equal(proofs, fproofs)
    rC, rH, _, _ = tr.root()
    pos = np.searchsorted(new[0], probe)
    lC, lH = ctx.commit_hash_batch(new[1][pos], new[2][pos])
    assert ctx.verify_entities(height, probe, lC, lH, C, H, rC, rH, hip_lib.POLICY_PADDING, agg, n_bits, proofs, verify_seed=SEED).all()


def test_update_still_rebuilds_for_shared_chains(hip_lib):
    """dapol_tree_update is untouched: the batch that insert takes in place (path 5) still reports path 0 there, and gives the same tree."""
    ctx = hip_lib.Context(0, 8)
    rng = np.random.default_rng(6131)
    height = 24
    old_set, blk, sub_bits, pair = _shape(rng, height, 500)
    old, new = _with_values(rng, old_set), _with_values(rng, {pair, pair + 1, blk, blk + 1, blk + 6})
    a, b = hip_lib.Tree(ctx, height, *old, SEED), hip_lib.Tree(ctx, height, *old, SEED)
    a.update(*new)
    b.insert(*new)
    assert a.last_update_path() == 0 and b.last_update_path() == 5
    _same_tree(a, b, height + 1, "update against insert")
