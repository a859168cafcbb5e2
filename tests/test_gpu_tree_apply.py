"""dapol_tree_apply: removals, new leaves and replacements as ONE all-or-nothing edit.  Padding nodes are keyed by position, so the tree
after an edit has exactly one correct form -- dapol_tree_build over (old leaves - removed) + puts with the tree's own pad seed -- and
both paths (the in-place mixed edit, path 6, and the rebuild, path 0) must give it bit for bit at every level.  Every refusal leaves
every array of every level as it was."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from test_gpu_tree_insert import SEED, NONCE, _forced_rebuild, _rand_idx, _ref_root, _root_of_handle, _same_tree, _with_values

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx8(hip_lib):
    c = hip_lib.Context(0, 8)
    yield c
    c.close()


def _model(arrays):
    return {int(x): (int(v), r.copy()) for x, v, r in zip(*arrays)}


def _arrays(model):
    idx = np.array(sorted(model), np.uint64)
    return idx, np.array([model[int(x)][0] for x in idx], np.uint64), np.stack([model[int(x)][1] for x in idx]) if len(idx) else np.zeros((0, 32), np.uint8)


def _edited(model, rm, puts):
    out = {x: lv for x, lv in model.items() if x not in rm}
    out.update(_model(puts))
    return out


def _puts(rng, idx, **kw):
    return _with_values(rng, set(int(x) for x in idx), **kw) if len(idx) else (np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros((0, 32), np.uint8))


def _gate(n_levels, n_old, rm, puts):
    """dapol_tree_apply's gate (every index in range): in place (6) or the rebuild (0)."""
    k = len(set(rm)) + len(puts[0])
    return 6 if n_levels - 1 >= 1 and k <= 65536 and k <= n_old // 8 + 1 else 0


def _levels(tr, n_levels):
    return [tr.level_nodes(t) for t in range(n_levels)]


def _unchanged(tr, root0, lvl0):
    assert tr.root() == root0
    for t, before in enumerate(lvl0):
        for a, b in zip(tr.level_nodes(t), before):
            assert np.array_equal(a, b), t


def _check_apply(hip_lib, ctx, height, old, rm, puts, what, ref=None, shard_bits=0):
    """Applies (rm, puts), both shuffled, to a tree over `old`: where the gate says so in place, and by the forced rebuild; both equal
    a fresh build over the model's leaf set.  Returns the path the first took."""
    kw = {"shard_bits": shard_bits} if shard_bits else {}
    n_levels = height - shard_bits + 1
    model = _model(old)
    after = _arrays(_edited(model, rm, puts))
    want = hip_lib.Tree(ctx, height, *after, SEED, **kw)
    if ref is not None:
        assert want.root() == _ref_root(ref, height, *after), what
    rng = np.random.default_rng(len(rm) * 131 + len(puts[0]))
    rm_arr = rng.permutation(np.array(sorted(rm), np.uint64))
    order = rng.permutation(len(puts[0]))
    path = None
    for how, label in ((contextlib.nullcontext(), ""), (_forced_rebuild(ctx), " (rebuild)")):
        with how:
            tr = hip_lib.Tree(ctx, height, *old, SEED, **kw)
            was_new = tr.apply(rm_arr, puts[0][order], puts[1][order], puts[2][order])
            assert was_new.tolist() == [int(x) not in model for x in puts[0][order]], what + label
            if label:
                assert tr.last_update_path() == 0, what + label
            else:
                path = tr.last_update_path()
                assert path == _gate(n_levels, len(old[0]), rm, puts), what
            _same_tree(tr, want, n_levels, what + label)
            probe = after[0][:: max(1, len(after[0]) // 4)]
            for a, b in zip(tr.paths(probe), want.paths(probe)):
                assert np.array_equal(a, b), what + label
            tr.close()
    want.close()
    return path


def _pick(rng, pool, n, avoid=()):
    pool = sorted(set(pool) - set(avoid))
    return {pool[i] for i in rng.choice(len(pool), size=min(n, len(pool)), replace=False)} if pool and n else set()     # (by position: 64-bit indexes stay Python integers)


def _fresh_idx(rng, height, old_set, n):
    if height <= 11:
        return _pick(rng, set(range(1 << height)) - set(old_set), n)
    return _rand_idx(rng, height, n, avoid=old_set)


@pytest.mark.parametrize("height,n_old", [(1, 2), (2, 3), (4, 12), (11, 600), (24, 1000), (32, 1000), (64, 1000)])
def test_apply_equals_build_every_level(hip_lib, ref, ctx8, height, n_old):
    ctx = ctx8
    rng = np.random.default_rng(8000 + height)
    top = 1 << height
    oracle = ref if height <= 24 else None
    blk = blk2 = pair = None
    if height >= 11:                      # an aligned free block of 8 beside a full one, and a free aligned pair elsewhere
        blk = (int(rng.integers(1, (top >> 4) - 1, dtype=np.uint64)) << 4)
        blk2, pair = blk + 8, (blk + (top >> 1)) % top & ~1
        reserved = {blk + i for i in range(16)} | {pair, pair + 1}
        old_set = _rand_idx(rng, height, n_old - 8, avoid=reserved) | {blk2 + i for i in range(8)}
    else:
        old_set = _pick(rng, range(top), n_old)
    old = _with_values(rng, old_set)
    room = len(old_set) // 8 + 1
    batches = []                          # (name, removed, put indexes)
    if room >= 3:                         # random mixed batches inside the gate, all three kinds in each
        for i, r in enumerate((1, max(1, room // 6), room // 3)):
            rm = _pick(rng, old_set, r)
            batches.append(("mixed%d" % i, rm, _pick(rng, old_set, r, avoid=rm) | _fresh_idx(rng, height, old_set, r)))
    else:                                 # the gate admits one or two edits: the three kinds across the batches, and all three by the rebuild
        a, b = sorted(_pick(rng, old_set, 2))
        batches += [("remove", {a}, set()), ("replace", set(), {b}), ("remove+replace", {a}, {b})]
        n1 = sorted(_fresh_idx(rng, height, old_set, 2))      # (the height-1 tree is full: no index is free)
        if n1:
            batches += [("new", set(), {n1[0]}), ("remove+new", {a}, {n1[0]}), ("new+replace", set(), {n1[-1], b}), ("all three", {a}, {n1[0], b})]
    if blk is not None:                   # clustered batches: sibling pairs, a whole new block, a block removed beside a block added
        full, free = {blk2 + i for i in range(8)}, {blk + i for i in range(8)}
        batches += [("sibling pairs", {blk2 + 2, blk2 + 3}, {pair, pair + 1, blk2 + 4, blk2 + 5}),
                    ("new block", set(), free | {blk2}),
                    ("block swap", full, free),
                    ("block emptied and repopulated", full - {blk2 + 5}, {blk2 + 5}),
                    ("block emptied, a put lands beside it", full, {blk + 7}),
                    ("scattered + block", full | _pick(rng, old_set, 20, avoid=full), free | _fresh_idx(rng, height, old_set | free, 20))]
    kinds = set()
    for name, rm, put_idx in batches:
        puts = _puts(rng, put_idx)
        path = _check_apply(hip_lib, ctx, height, old, rm, puts, "h%d %s" % (height, name), oracle)
        if path == 6:
            kinds |= {"rm"} if rm else set()
            kinds |= {"new"} if put_idx - old_set else set()
            kinds |= {"repl"} if put_idx & old_set else set()
        if height >= 11:
            assert path == 6, name
    assert kinds == ({"rm", "new", "repl"} if height >= 2 else {"rm", "repl"}), kinds       # each kind of edit ran in place at this shape


def test_directed_shapes_on_the_device(hip_lib, ref, ctx8):
    """The shapes tests/test_tree_apply_plan_cpu.py plans, run at height 11 around two reserved blocks of a 300-leaf tree."""
    rng = np.random.default_rng(8100)
    height, a, far = 11, 512, 1536
    U = 1 << height
    reserved = {a + i for i in range(16)} | {far + i for i in range(16)} | {0, 1, U - 2, U - 1} | {64 + i for i in range(64)}
    base = _rand_idx(rng, height, 300, avoid=reserved)
    blk = {a + i for i in range(8)}
    shapes = [
        ({a + 1, far}, {a + 1}, {a}),                               # level 0 loses and gains at one lower bound
        ({a, far}, {a}, {a + 1}),
        ({a, a + 1, a + 3, far}, {a, a + 1, a + 3}, {a + 2}),       # a subtree emptied and repopulated
        (blk | {far}, blk - {a + 5}, {a + 5}),
        (blk | {far}, set(blk), {a + 8}),
        ({a, a + 2, far}, {a}, {a + 3}),                            # a chain top dies beside an S under which a put lands
        ({a, a + 2, far}, {a}, {a + 2}),
        ({a, a + 4, far}, {a}, {a + 6}),
        ({a, a + 1, a + 2, far}, {a + 2}, {a + 3}),                 # a put takes away the has_pad a removal would have given
        ({a, a + 1, a + 2, a + 3, far}, {a + 2, a + 3}, set()),     # ... and without it S is decoded beside its new padding node
        (blk | {far}, set(blk), set()), ({a, a + 4, far}, {a + 4}, set()),                       # only removals
        ({far}, set(), set(blk)), ({a + 3, far}, set(), blk - {a + 3}),                          # only new puts
        (blk | {far}, set(), set(blk)), (blk | {far}, set(), {a, a + 7, far}),                   # only replacements
        ({0, U - 1}, {0, U - 1}, {1, U - 2}), ({1, U - 2}, {1}, {0, U - 1}),                     # the two ends of the index range
        ({64, 96, 97}, {64}, {98}),                                 # level 0 keeps its size, level 5 loses a node
    ]
    for i, (extra, rm, put_idx) in enumerate(shapes):
        old = _with_values(rng, base | extra)
        assert _check_apply(hip_lib, ctx8, height, old, rm, _puts(rng, put_idx), "directed %d" % i, ref) == 6
    # every leaf but one removed: the gate admits it only in a tiny tree (two leaves), otherwise the rebuild
    assert _check_apply(hip_lib, ctx8, height, _with_values(rng, {a, far}), {a}, _puts(rng, []), "all but one of two") == 6
    assert _check_apply(hip_lib, ctx8, height, _with_values(rng, blk | {far}), set(blk), _puts(rng, []), "all but one of nine", ref) == 0


def test_apply_equals_the_three_calls(hip_lib, ctx8):
    rng = np.random.default_rng(8200)
    height = 20
    old_set = _rand_idx(rng, height, 800)
    old = _with_values(rng, old_set)
    rm = _pick(rng, old_set, 30)
    new = _with_values(rng, _rand_idx(rng, height, 28, avoid=old_set) | {min(rm) ^ 1} - old_set)
    repl = _with_values(rng, _pick(rng, old_set, 30, avoid=rm))
    a, b = hip_lib.Tree(ctx8, height, *old, SEED), hip_lib.Tree(ctx8, height, *old, SEED)
    puts = tuple(np.concatenate([x, y]) for x, y in zip(new, repl))
    was_new = a.apply(sorted(rm), *puts)
    assert a.last_update_path() == 6 and was_new.tolist() == [True] * len(new[0]) + [False] * len(repl[0])
    b.remove(np.array(sorted(rm), np.uint64))
    b.insert(*new)
    b.update(*repl)
    _same_tree(a, b, height + 1, "apply against remove + insert + update")


def test_twenty_applies_in_a_row(hip_lib, ctx8):
    """Every apply moves the changed levels into their other LevelAlt buffer."""
    rng = np.random.default_rng(8300)
    height = 16
    model = _model(_with_values(rng, _rand_idx(rng, height, 400)))
    tr = hip_lib.Tree(ctx8, height, *_arrays(model), SEED)
    for step in range(20):
        rm = _pick(rng, model, 1 + step % 4)
        put_idx = _pick(rng, model, 1 + step % 3, avoid=rm) | _rand_idx(rng, height, 1 + (step * 7) % 5, avoid=set(model))
        if step % 5 == 4:
            put_idx |= {min(rm) ^ 1} - rm                                             # beside a leaf that goes
        puts = _puts(rng, put_idx)
        tr.apply(sorted(rm), *puts)
        assert tr.last_update_path() == 6
        model = _edited(model, rm, puts)
        _same_tree(tr, hip_lib.Tree(ctx8, height, *_arrays(model), SEED), height + 1, step)


@pytest.mark.parametrize("route", ["in place", "rebuild"])
def test_refusals_leave_every_level_unchanged(hip_lib, ctx8, route):
    ctx = ctx8
    rng = np.random.default_rng(8400)
    height = 12
    old_set = _rand_idx(rng, height, 200)
    idx, v, r = _with_values(rng, old_set)
    fresh = _with_values(rng, _rand_idx(rng, height, 4, avoid=old_set))
    absent = sorted(_rand_idx(rng, height, 2, avoid=old_set | set(int(x) for x in fresh[0])))
    # the rebuild route: the same broken batch above the gate (60 valid replacements more than an eighth of the tree admits)
    bulk = _with_values(rng, set(int(x) for x in idx[100:160])) if route == "rebuild" else _puts(rng, [])
    tr = hip_lib.Tree(ctx, height, idx, v, r, SEED)
    root0, lvl0 = tr.root(), _levels(tr, height + 1)

    def batch(extra_idx):
        bi = np.concatenate([fresh[0], bulk[0], np.array(extra_idx, np.uint64)])
        k = len(bi)
        return bi, np.resize(np.concatenate([fresh[1], bulk[1]]), k), np.resize(np.concatenate([fresh[2], bulk[2]]), (k, 32))

    def refused(rm, puts, code, text):
        with pytest.raises(hip_lib.DapolError) as e:
            tr.apply(rm, *puts)
        assert e.value.code == code and text in str(e.value), (e.value, text)
        _unchanged(tr, root0, lvl0)

    refused([idx[3], absent[0]], batch([]), 9, "not a leaf")
    refused([idx[3], 1 << height], batch([]), 9, "not a leaf")                         # outside the tree
    refused([idx[3]], batch([fresh[0][1]]), 8, "twice")
    refused([idx[3], idx[5]], batch([idx[5]]), 8, "both removed and put")
    refused([absent[0]], batch([fresh[0][1]]), 8, "twice")                             # the host's own rules come first
    twin = hip_lib.Tree(ctx, height, idx, v, r, SEED)
    outside = batch([1 << height])
    with pytest.raises(hip_lib.DapolError) as eu:
        twin.update(*outside)
    twin.close()
    with pytest.raises(hip_lib.DapolError) as ea:
        tr.apply([idx[3]], *outside)
    assert ea.value.code == eu.value.code
    _unchanged(tr, root0, lvl0)
    refused([absent[1]], outside, 9, "not a leaf")                                     # a removal that is not a leaf, before the range
    assert tr.apply([], *_puts(rng, [])).tolist() == []                                # nothing to do
    _unchanged(tr, root0, lvl0)
    # a result with no leaf: the gate admits all of a one-leaf tree's leaves, the rebuild takes all of this one's
    if route == "in place":
        one = hip_lib.Tree(ctx, height, idx[:1], v[:1], r[:1], SEED)
        before = one.root(), _levels(one, height + 1)
        with pytest.raises(hip_lib.DapolError) as e:
            one.apply(idx[:1], *_puts(rng, []))
        assert e.value.code == 8 and "empty tree" in str(e.value)
        _unchanged(one, *before)
        one.apply(idx[:1], fresh[0][:1], fresh[1][:1], fresh[2][:1])                   # its leaf goes, another comes: not empty
        assert one.last_update_path() == 0                                             # (two edits of a one-leaf tree: above the gate)
        _same_tree(one, hip_lib.Tree(ctx, height, fresh[0][:1], fresh[1][:1], fresh[2][:1], SEED), height + 1, "one leaf swapped")
    else:
        refused(idx, _puts(rng, []), 8, "empty tree")
    # still usable
    tr.apply([idx[3], idx[3]], *batch([]))                                             # a duplicate removal removes its leaf once
    assert tr.last_update_path() == (6 if route == "in place" else 0)
    model = _edited(_model((idx, v, r)), {int(idx[3])}, batch([]))
    _same_tree(tr, hip_lib.Tree(ctx, height, *_arrays(model), SEED), height + 1, "after the refusals")


def test_apply_refuses_the_trees_the_other_edits_refuse(hip_lib, ctx8):
    ctx = ctx8
    rng = np.random.default_rng(8500)
    height = 10
    idx, v, r = _with_values(rng, _rand_idx(rng, height, 100))
    level, index = hip_lib.tree_padding_positions(height, idx)
    taped = hip_lib.Tree(ctx, height, idx, v, r, None, pad_tape=np.random.default_rng(1).integers(0, 256, size=64 * len(level), dtype=np.uint8).tobytes())
    troot = taped.root()
    with pytest.raises(hip_lib.DapolError) as e:
        taped.apply(idx[:1], idx[1:2], v[1:2], r[1:2])
    assert e.value.code == 8 and "padding tape" in str(e.value) and taped.root() == troot
    w = hip_lib.Workload(ctx, height, idx, v, r)
    w.build(SEED)
    h = w.tree_handle()
    wroot = _root_of_handle(hip_lib, h)
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)
    assert hip_lib.lib().dapol_tree_apply(h, 1, p(idx[:1]), 1, p(idx[1:2]), p(v[1:2]), p(r[1:2]), None) == 8
    assert _root_of_handle(hip_lib, h) == wroot
    w.close()


def test_failed_in_place_apply_marks_the_tree_invalid(hip_lib, ctx8):
    rng = np.random.default_rng(8600)
    height = 10
    idx, v, r = _with_values(rng, _rand_idx(rng, height, 100))
    tr = hip_lib.Tree(ctx8, height, idx, v, r, SEED)
    saved = os.environ.get("DAPOL_TEST_FAIL_APPLY_MIDWAY")
    os.environ["DAPOL_TEST_FAIL_APPLY_MIDWAY"] = "1"
    try:
        with pytest.raises(hip_lib.DapolError) as e:
            tr.apply(idx[:2], idx[2:4], v[:2], r[:2])
    finally:
        if saved is None:
            os.environ.pop("DAPOL_TEST_FAIL_APPLY_MIDWAY", None)
        else:
            os.environ["DAPOL_TEST_FAIL_APPLY_MIDWAY"] = saved
    assert e.value.code == 17
    for call in (tr.root, lambda: tr.level_nodes(0), lambda: tr.apply(idx[:2], idx[2:4], v[:2], r[:2]), lambda: tr.remove(idx[2:3]),
                 lambda: tr.update(idx[:1], v[:1], r[:1])):
        with pytest.raises(hip_lib.DapolError) as e:
            call()
        assert e.value.code == 8 and "left inconsistent" in str(e.value)
    tr.close()


def test_apply_in_a_shard_tree(hip_lib, ctx8):
    rng = np.random.default_rng(8700)
    total, bits, prefix = 20, 4, 9
    sub = total - bits
    under = lambda s: {int(x) | (prefix << sub) for x in s}
    low_old = _rand_idx(rng, sub, 400, avoid={6, 7})
    old = _with_values(rng, under(low_old), 32)
    rm = under(_pick(rng, low_old, 10))
    put_idx = under({6, 7} | _rand_idx(rng, sub, 10, avoid=low_old | {6, 7})) | _pick(rng, under(low_old), 10, avoid=rm)
    assert _check_apply(hip_lib, ctx8, total, old, rm, _puts(rng, put_idx, bits=32), "shard", shard_bits=bits) == 6
    tr = hip_lib.Tree(ctx8, total, *old, SEED, shard_bits=bits)
    root0, lvl0 = tr.root(), _levels(tr, sub + 1)
    bad = _puts(rng, {((prefix + 1) << sub) | 5, min(put_idx)}, bits=32)              # a put of another prefix: update's code for the same batch
    twin = hip_lib.Tree(ctx8, total, *old, SEED, shard_bits=bits)
    with pytest.raises(hip_lib.DapolError) as eu:
        twin.update(*bad)
    with pytest.raises(hip_lib.DapolError) as ea:
        tr.apply(sorted(rm), *bad)
    assert ea.value.code == eu.value.code
    _unchanged(tr, root0, lvl0)
    with pytest.raises(hip_lib.DapolError) as e:                                       # a removal of another prefix is no leaf of this tree
        tr.apply([min(rm), ((prefix - 1) << sub) | int(min(low_old))], *_puts(rng, {min(put_idx)}, bits=32))
    assert e.value.code == 9
    _unchanged(tr, root0, lvl0)


@pytest.mark.parametrize("digest", ["DIGEST_BLAKE2S", "DIGEST_SHA256", "DIGEST_SHA3_256", "DIGEST_BLAKE2B"])
def test_apply_with_other_digests(hip_lib, digest):
    """Blake2b: a 64-byte digest, whose hash chain is laid again after the edit -- every level's H (64 bytes wide) equals the build's."""
    ctx = hip_lib.Context(0, 8, digest=getattr(hip_lib, digest))
    rng = np.random.default_rng(8800)
    height = 11
    old_set = _rand_idx(rng, height, 600)
    old = _with_values(rng, old_set)
    rm = _pick(rng, old_set, 20)
    put_idx = _pick(rng, old_set, 20, avoid=rm) | _fresh_idx(rng, height, old_set, 20) | {min(rm) ^ 1} - rm
    assert _check_apply(hip_lib, ctx, height, old, rm, _puts(rng, put_idx), digest) == 6
    if digest == "DIGEST_BLAKE2B":
        tr = hip_lib.Tree(ctx, height, *old, SEED)
        assert tr.level_nodes(3)[4].shape[1] == 64
        tr.close()
    ctx.close()


def test_proofs_and_the_proof_store_after_an_apply(hip_lib):
    ctx = hip_lib.Context(0, 16)
    rng = np.random.default_rng(8900)
    height, n_bits, agg = 11, 16, 4
    old_set = _rand_idx(rng, height, 300)
    old = _with_values(rng, old_set, 6, beyond_l=False)                                # subtree sums stay inside the 16-bit ranges
    model = _model(old)
    tr = hip_lib.Tree(ctx, height, *old, SEED)
    store = hip_lib.ProofStore(tr, hip_lib.POLICY_PADDING, agg, n_bits, NONCE)
    try:
        store.refresh()
        rm = _pick(rng, old_set, 8)
        puts = _puts(rng, _pick(rng, old_set, 8, avoid=rm) | _rand_idx(rng, height, 8, avoid=old_set), bits=6, beyond_l=False)
        was_new = tr.apply(sorted(rm), *puts)
        assert tr.last_update_path() == 6 and was_new.tolist() == [int(x) not in model for x in puts[0]] and was_new.sum() == 8
        model = _edited(model, rm, puts)
        idx, v, r = _arrays(model)
        fresh = hip_lib.Tree(ctx, height, idx, v, r, SEED)
        untouched = np.array(sorted(set(model) - set(int(x) for x in puts[0]))[::60], np.uint64)
        probe = np.sort(np.concatenate([puts[0], untouched]))
        C, H, proofs = tr.prove_entities(probe, hip_lib.POLICY_PADDING, agg, n_bits, NONCE)
        fC, fH, fproofs = fresh.prove_entities(probe, hip_lib.POLICY_PADDING, agg, n_bits, NONCE)
        assert np.array_equal(C, fC) and np.array_equal(H, fH) and np.array_equal(proofs, fproofs)
        rC, rH, _, _ = tr.root()
        pos = np.searchsorted(idx, probe)
        lC, lH = ctx.commit_hash_batch(v[pos], r[pos])
        assert ctx.verify_entities(height, probe, lC, lH, C, H, rC, rH, hip_lib.POLICY_PADDING, agg, n_bits, proofs, verify_seed=SEED).all()
        proved, kept, moved = store.refresh()                                          # the leaf set changed: every surviving row moves
        assert proved > 0 and kept > 0 and moved == len(old_set) - len(rm)
        sidx, sC, sH, blobs = store.read()
        wC, wH, wblobs, _ = fresh.prove_entities_shared(idx, hip_lib.POLICY_PADDING, agg, n_bits, NONCE)
        assert sidx.tolist() == idx.tolist() and sC.tobytes() == wC.tobytes() and sH.tobytes() == wH.tobytes() and blobs.tobytes() == wblobs.tobytes()
        # the re-prover fed with the rows of before the edit gives the same bytes
        oC, oH, oblobs, _ = hip_lib.Tree(ctx, height, *old, SEED).prove_entities_shared(old[0], hip_lib.POLICY_PADDING, agg, n_bits, NONCE)
        out = tr.reprove_entities_shared(idx, old[0], oC, oblobs, hip_lib.POLICY_PADDING, agg, n_bits, NONCE)
        assert out[0].tobytes() == wC.tobytes() and out[2].tobytes() == wblobs.tobytes()
    finally:
        store.close()
