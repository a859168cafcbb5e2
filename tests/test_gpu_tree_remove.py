"""dapol_tree_remove: leaves leave a built tree.  Padding nodes are keyed by position, so the tree after a removal has exactly one
correct form -- dapol_tree_build over the surviving leaves with the tree's own pad seed -- and both paths (in place on the device,
and the rebuild taken above update_incremental_max) must give it bit for bit at every level."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
NONCE = bytes(range(100, 132))


def _ref_root(ref, height, idx, v, r):
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    t = ctypes.c_void_p(ref.ref_tree_build(height, ctypes.c_size_t(len(idx)), p(idx), p(v), p(r), SEED, 0))
    C, H, rr, vv = [ctypes.create_string_buffer(32) for _ in range(3)] + [ctypes.c_uint64()]
    ref.ref_tree_root(t, C, H, ctypes.byref(vv), rr)
    ref.ref_tree_free(t)
    return C.raw, H.raw, vv.value, rr.raw


def _leaves(rng, height, n, sub_bits=3):
    """n random leaves plus, on purpose, a pair of sibling leaves and a full subtree of 2^sub_bits leaves (shared chains)."""
    top = 1 << height if height < 64 else 1 << 64
    pair = int(rng.integers(0, top >> 1, dtype=np.uint64)) * 2
    blk = (int(rng.integers(0, top >> sub_bits, dtype=np.uint64)) << sub_bits)
    forced = {pair, pair + 1} | {blk + i for i in range(1 << sub_bits)}
    rest = set()
    while len(rest) + len(forced) < n:
        x = int(rng.integers(0, top - 1, dtype=np.uint64, endpoint=True)) if height == 64 else int(rng.integers(0, top))
        if x not in forced:
            rest.add(x)
    idx = np.array(sorted(forced | rest), np.uint64)
    v = rng.integers(0, 2**40, size=len(idx), dtype=np.uint64)
    r = rng.integers(0, 256, size=(len(idx), 32), dtype=np.uint8)
    r[:, 31] &= 0x0F
    return idx, v, r, pair, blk, sub_bits


def _cases(rng, idx, pair, blk, sub_bits):
    n = len(idx)
    pos = {int(x): i for i, x in enumerate(idx)}
    cases = {"one": [int(rng.integers(0, n))],
             "siblings": [pos[pair], pos[pair + 1]],
             "subtree": [pos[blk + i] for i in range(1 << sub_bits)]}
    if n >= 64 * 8:
        cases["random64"] = sorted(rng.choice(n, size=64, replace=False).tolist())
    keep = int(rng.integers(0, n))
    cases["all_but_one"] = [i for i in range(n) if i != keep]
    return cases


def _same_tree(a, b, height, what):
    assert a.root() == b.root(), what
    assert a.node_count() == b.node_count(), what
    for level in range(height + 1):
        for x, y in zip(a.level_nodes(level), b.level_nodes(level)):
            assert np.array_equal(x, y), (what, level)


def _forced_rebuild(hip_lib, ctx):
    class _Opt:
        def __enter__(self):
            self.saved = ctx.get_options()
            o = ctx.get_options()
            o.update_incremental_max = -1
            ctx.set_options(o)

        def __exit__(self, *a):
            ctx.set_options(self.saved)
    return _Opt()


def _check_remove(hip_lib, ctx, height, idx, v, r, sel, what, ref=None):
    """Removes idx[sel] in place (where the limit admits it) and by the forced rebuild; both equal a fresh build over the survivors."""
    keep = np.setdiff1d(np.arange(len(idx)), sel)
    want = hip_lib.Tree(ctx, height, idx[keep], v[keep], r[keep], SEED)
    assert want.root()[2] == int(v[keep].sum(dtype=np.uint64))
    if ref is not None:
        assert want.root() == _ref_root(ref, height, idx[keep], v[keep], r[keep]), what
    order = np.random.default_rng(len(sel)).permutation(len(sel))     # the list arrives unsorted
    tr = hip_lib.Tree(ctx, height, idx, v, r, SEED)
    tr.remove(idx[sel][order])
    in_place = len(sel) <= len(idx) // 8 + 1
    assert tr.last_update_path() == (4 if in_place else 0), what
    _same_tree(tr, want, height, what)
    tr.close()
    with _forced_rebuild(hip_lib, ctx):
        tr = hip_lib.Tree(ctx, height, idx, v, r, SEED)
        tr.remove(idx[sel])
        assert tr.last_update_path() == 0, what
        _same_tree(tr, want, height, what + " (rebuild)")
        tr.close()
    want.close()
    return in_place


@pytest.mark.parametrize("height,n", [(4, 12), (11, 600), (24, 1000), (32, 1000), (64, 1000)])
def test_remove_equals_build_every_level(hip_lib, ref, height, n):
    ctx = hip_lib.Context(0, 8)
    rng = np.random.default_rng(4000 + height)
    idx, v, r, pair, blk, sb = _leaves(rng, height, n)
    for name, sel in _cases(rng, idx, pair, blk, sb).items():
        in_place = _check_remove(hip_lib, ctx, height, idx, v, r, np.array(sel), "h%d %s" % (height, name), ref if height <= 24 else None)
        if height >= 11 and name in ("siblings", "subtree", "random64", "one"):
            assert in_place, name                                     # the shared-chain cases run on the device path
    ctx.close()


@pytest.mark.parametrize("digest", ["DIGEST_BLAKE2S", "DIGEST_BLAKE2B"])
def test_remove_with_other_digests(hip_lib, digest):
    ctx = hip_lib.Context(0, 8, digest=getattr(hip_lib, digest))
    rng = np.random.default_rng(17)
    height = 9
    idx, v, r, pair, blk, sb = _leaves(rng, height, 90, sub_bits=2)
    for name, sel in _cases(rng, idx, pair, blk, sb).items():
        _check_remove(hip_lib, ctx, height, idx, v, r, np.array(sel), digest + " " + name)
    ctx.close()


def test_remove_in_a_shard_tree(hip_lib):
    ctx = hip_lib.Context(0, 8)
    rng = np.random.default_rng(23)
    total, bits, prefix = 20, 4, 9
    low = np.sort(rng.choice(1 << (total - bits), size=400, replace=False).astype(np.uint64))
    low = np.union1d(low, [6, 7]).astype(np.uint64)                    # a sibling pair
    idx = low | np.uint64(prefix << (total - bits))
    v = rng.integers(0, 2**32, size=len(idx), dtype=np.uint64)
    r = rng.integers(0, 256, size=(len(idx), 32), dtype=np.uint8)
    r[:, 31] &= 0x0F
    sel = np.union1d(rng.choice(len(idx), size=20, replace=False), np.flatnonzero(np.isin(low, [6, 7])))
    keep = np.setdiff1d(np.arange(len(idx)), sel)
    tr = hip_lib.Tree(ctx, total, idx, v, r, SEED, shard_bits=bits)
    want = hip_lib.Tree(ctx, total, idx[keep], v[keep], r[keep], SEED, shard_bits=bits)
    before = tr.root()
    other = np.uint64(((prefix + 1) << (total - bits)) | int(low[0]))       # the same low bits under another prefix
    with pytest.raises(hip_lib.DapolError) as e:
        tr.remove([idx[0], other])
    assert e.value.code == 9 and tr.root() == before
    tr.remove(idx[sel])
    assert tr.last_update_path() == 4
    _same_tree(tr, want, total - bits, "shard")


def _root_of_handle(hip_lib, h):
    C, H, r = (ctypes.create_string_buffer(32) for _ in range(3))
    v = ctypes.c_uint64()
    assert hip_lib.lib().dapol_tree_root(h, C, H, ctypes.byref(v), r) == 0
    return C.raw, H.raw, v.value, r.raw


def test_remove_errors_leave_the_tree_unchanged(hip_lib):
    ctx = hip_lib.Context(0, 8)
    rng = np.random.default_rng(31)
    height = 12
    idx, v, r, pair, blk, sb = _leaves(rng, height, 200)
    tr = hip_lib.Tree(ctx, height, idx, v, r, SEED)
    root0, lvl0 = tr.root(), tr.level_nodes(0)
    absent = next(x for x in range(1 << height) if x not in set(map(int, idx)))

    def unchanged():
        assert tr.root() == root0
        for a, b in zip(tr.level_nodes(0), lvl0):
            assert np.array_equal(a, b)
    for bad, code in (([idx[3], absent, idx[5]], 9),                 # one unknown index among valid ones
                      ([idx[3], 1 << height], 9),                    # outside the tree
                      (idx, 8),                                      # every leaf (rebuild path)
                      (list(idx) + list(idx[:5]), 8)):               # every leaf, with duplicates
        with pytest.raises(hip_lib.DapolError) as e:
            tr.remove(bad)
        assert e.value.code == code
        unchanged()
    tr.remove([])                                                    # k = 0
    unchanged()
    one = hip_lib.Tree(ctx, height, idx[:1], v[:1], r[:1], SEED)     # a single leaf: removing it would empty the tree (in-place limit)
    with pytest.raises(hip_lib.DapolError) as e:
        one.remove(idx[:1])
    assert e.value.code == 8
    # duplicates are removed once
    dup = np.array([idx[7], idx[7], idx[40], idx[7]], np.uint64)
    tr.remove(dup)
    assert tr.last_update_path() == 4
    keep = np.setdiff1d(np.arange(len(idx)), [7, 40])
    _same_tree(tr, hip_lib.Tree(ctx, height, idx[keep], v[keep], r[keep], SEED), height, "duplicates")
    # a tree built from a padding tape
    level, index = hip_lib.tree_padding_positions(height, idx)
    taped = hip_lib.Tree(ctx, height, idx, v, r, None, pad_tape=np.random.default_rng(1).integers(0, 256, size=64 * len(level), dtype=np.uint8).tobytes())
    troot = taped.root()
    with pytest.raises(hip_lib.DapolError) as e:
        taped.remove(idx[:1])
    assert e.value.code == 8 and taped.root() == troot
    # a workload tree (it does not own its leaves)
    w = hip_lib.Workload(ctx, height, idx, v, r)
    w.build(SEED)
    h = w.tree_handle()
    wroot = _root_of_handle(hip_lib, h)
    one_idx = np.array([idx[0]], np.uint64)
    assert hip_lib.lib().dapol_tree_remove(h, 1, one_idx.ctypes.data_as(ctypes.c_void_p)) == 8
    assert _root_of_handle(hip_lib, h) == wroot
    w.close()
    assert hip_lib.lib().dapol_tree_remove(None, 1, one_idx.ctypes.data_as(ctypes.c_void_p)) == 8


def test_failed_in_place_remove_marks_the_tree_invalid(hip_lib):
    ctx = hip_lib.Context(0, 8)
    rng = np.random.default_rng(37)
    height = 10
    idx, v, r, pair, blk, sb = _leaves(rng, height, 100)
    tr = hip_lib.Tree(ctx, height, idx, v, r, SEED)
    saved = os.environ.get("DAPOL_TEST_FAIL_REMOVE_MIDWAY")
    os.environ["DAPOL_TEST_FAIL_REMOVE_MIDWAY"] = "1"
    try:
        with pytest.raises(hip_lib.DapolError) as e:
            tr.remove(idx[:2])
    finally:
        if saved is None:
            os.environ.pop("DAPOL_TEST_FAIL_REMOVE_MIDWAY", None)
        else:
            os.environ["DAPOL_TEST_FAIL_REMOVE_MIDWAY"] = saved
    assert e.value.code == 17
    for call in (tr.root, tr.node_count, lambda: tr.level_nodes(0), lambda: tr.remove(idx[2:3]), lambda: tr.update(idx[:1], v[:1], r[:1])):
        with pytest.raises(hip_lib.DapolError) as e:
            call()
        assert e.value.code == 8 and "left inconsistent" in str(e.value)
    tr.close()


def test_remove_then_update_sequences(hip_lib):
    ctx = hip_lib.Context(0, 8)
    rng = np.random.default_rng(41)
    height = 20
    idx, v, r, pair, blk, sb = _leaves(rng, height, 800)
    full = hip_lib.Tree(ctx, height, idx, v, r, SEED)
    sel = np.union1d(rng.choice(len(idx), size=50, replace=False), np.searchsorted(idx, [pair, pair + 1]))
    tr = hip_lib.Tree(ctx, height, idx, v, r, SEED)
    tr.remove(idx[sel])
    assert tr.last_update_path() == 4
    tr.update(idx[sel], v[sel], r[sel])                              # the same triples back: the original tree
    _same_tree(tr, full, height, "remove + re-insert")
    # remove, replace, remove again
    s1 = rng.choice(len(idx), size=30, replace=False)
    rest = np.setdiff1d(np.arange(len(idx)), s1)
    s2 = rng.choice(rest, size=40, replace=False)                    # replaced
    s3 = np.setdiff1d(rng.choice(rest, size=60, replace=False), s2)  # removed after the replacement
    v2, r2 = v.copy(), r.copy()
    v2[s2] = rng.integers(0, 2**40, size=len(s2), dtype=np.uint64)
    r2[s2] = rng.integers(0, 256, size=(len(s2), 32), dtype=np.uint8)
    r2[s2, 31] &= 0x0F
    tr2 = hip_lib.Tree(ctx, height, idx, v, r, SEED)
    tr2.remove(idx[s1])
    tr2.update(idx[s2], v2[s2], r2[s2])
    assert tr2.last_update_path() == 1
    tr2.remove(idx[s3])
    assert tr2.last_update_path() == 4
    keep = np.setdiff1d(np.arange(len(idx)), np.union1d(s1, s3))
    _same_tree(tr2, hip_lib.Tree(ctx, height, idx[keep], v2[keep], r2[keep], SEED), height, "remove + replace + remove")


def test_proofs_after_a_removal(hip_lib):
    ctx = hip_lib.Context(0, 16)
    rng = np.random.default_rng(43)
    height, n_bits, agg = 16, 16, 4
    idx, v, r, pair, blk, sb = _leaves(rng, height, 300)
    v %= np.uint64(100)                                              # subtree sums stay inside the 16-bit ranges
    sel = np.union1d(rng.choice(len(idx), size=25, replace=False), np.searchsorted(idx, [pair, blk, blk + 1]))
    keep = np.setdiff1d(np.arange(len(idx)), sel)
    tr = hip_lib.Tree(ctx, height, idx, v, r, SEED)
    probe = idx[keep[:6]]
    oC, oH, old = tr.prove_entities(probe, hip_lib.POLICY_PADDING, agg, n_bits, NONCE)
    tr.remove(idx[sel])
    assert tr.last_update_path() == 4
    fresh = hip_lib.Tree(ctx, height, idx[keep], v[keep], r[keep], SEED)
    C, H, proofs = tr.prove_entities(probe, hip_lib.POLICY_PADDING, agg, n_bits, NONCE)
    fC, fH, fproofs = fresh.prove_entities(probe, hip_lib.POLICY_PADDING, agg, n_bits, NONCE)
    assert np.array_equal(C, fC) and np.array_equal(H, fH) and np.array_equal(proofs, fproofs)
    rC, rH, _, _ = tr.root()
    pos = np.searchsorted(idx, probe)
    lC, lH = ctx.commit_hash_batch(v[pos], r[pos])
    assert ctx.verify_entities(height, probe, lC, lH, C, H, rC, rH, hip_lib.POLICY_PADDING, agg, n_bits, proofs, verify_seed=SEED).all()
    assert not ctx.verify_entities(height, probe, lC, lH, oC, oH, rC, rH, hip_lib.POLICY_PADDING, agg, n_bits, old, verify_seed=SEED).any()
    batch = [int(x) for x in probe[:3]]
    got = tr.prove_batch(batch, hip_lib.POLICY_SPLITTING, 2, n_bits, NONCE)
    exp = fresh.prove_batch(batch, hip_lib.POLICY_SPLITTING, 2, n_bits, NONCE)
    for a, b in zip(got[:4], exp[:4]):
        assert np.array_equal(a, b)
    assert got[4] == exp[4]
    assert ctx.verify_batch(height, batch, lC[:3], lH[:3], got[2], got[3], rC, rH, hip_lib.POLICY_SPLITTING, 2, n_bits, got[4], verify_seed=SEED)
    for call in (lambda: tr.paths(idx[sel[:1]]), lambda: tr.prove_entities(idx[sel[:1]], hip_lib.POLICY_PADDING, agg, n_bits, NONCE)):
        with pytest.raises(hip_lib.DapolError) as e:
            call()
        assert e.value.code == 9


def test_remove_at_2e20_leaves(hip_lib, gpu_ctx):
    from bench import synth_inputs
    height, n = 32, 1 << 20
    idx, v, r = synth_inputs(n, height, 0, n)
    rng = np.random.default_rng(47)
    tr = hip_lib.Tree(gpu_ctx, height, idx, v, r, SEED)
    alive = np.ones(n, bool)
    for k in (1, 64, 4096):
        sel = rng.choice(np.flatnonzero(alive), size=k, replace=False)
        tr.remove(idx[sel])
        assert tr.last_update_path() == 4
        alive[sel] = False
        want = hip_lib.Tree(gpu_ctx, height, idx[alive], v[alive], r[alive], SEED)
        assert tr.root() == want.root() and tr.node_count() == want.node_count(), k
        assert tr.root()[2] == int(v[alive].sum(dtype=np.uint64))
        sample = idx[rng.choice(np.flatnonzero(alive), size=64, replace=False)]
        for a, b in zip(tr.paths(sample), want.paths(sample)):
            assert np.array_equal(a, b), k
        want.close()
    tr.close()
