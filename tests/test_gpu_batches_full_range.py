"""The many-batch family -- dapol_prove_batches / dapol_verify_batches, dapol_reprove_batches, dapol_batch_store_* -- at the edge of the
range the library accepts: a tree of height 64 with leaf indexes on both sides of 2^31, 2^32 and 2^63, batches of 62 to 256 siblings
on a context of 64 parties, and (height 6, 8 parties) the three other 32-byte digests.

Every comparison is byte for byte or verdict for verdict.  The references are dapol_prove_batch / dapol_verify_batch_checked batch by
batch, the C oracle's tree and range prover for sampled batches, the Python oracle's sibling positions, Merkle verifier and trees, and
for the re-proving calls a brute-force model on Python integers: a pair (batch, sub-proof) is dirty exactly when an edited leaf lies
below one of the sub-proof's siblings."""
import contextlib
import ctypes

import numpy as np
import pytest

import digest_shims
from test_gpu_reprove_batches import _Old

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
H = 64
T, M = 1 << 63, (1 << 64) - 1
LEAVES = [0, 1, 5, (1 << 31) + 3, 1 << 32, (1 << 32) + 1, (1 << 40) + 7, (1 << 62) + 9,
          T, T + 1, T + 2, T + 3, T + (1 << 20), T + (1 << 62) + 5, M - 1, M]
FIVE = [5, (1 << 31) + 3, (1 << 40) + 7, (1 << 62) + 9, T + (1 << 20)]
DISTINCT = [[0], [M], [T], [0, M], [M - 1, M], [T, T + 1, T + 2, T + 3], [0, 1], [0, 1, 5], [0, T], [1, 1 << 32, T + 1], FIVE,
            [T + (1 << 62) + 5, M], [0, 1, T, T + 1, M - 1, M]]
# caller order: the 13 batches and a second copy of [T] and of [0, M], shuffled with a fixed permutation
ORDER = [10, 2, 13, 7, 0, 12, 5, 14, 3, 9, 1, 11, 6, 8, 4]
BATCHES = [(DISTINCT + [[T], [0, M]])[i] for i in ORDER]
SAMPLED = [[0, M], [T, T + 1, T + 2, T + 3], FIVE]              # the batches that go against the C oracle
# (policy, aggregation, n_bits, leaf_first)
PAD62, SPLIT62, PAD0, PAD16 = (0, 62, 64, 0), (1, 62, 64, 0), (0, 0, 64, 0), (0, 16, 8, 0)
CONFIGS = [PAD62, SPLIT62, PAD0, PAD16]
PAD62_LEAF_FIRST = (0, 62, 64, 1)
IDS = lambda c: "p%d-a%d-n%d-lf%d" % c
REPROVE_LANES = 16                                              # kernels_reprove.h: lanes that stride over a pair's 16-byte pieces
# the edits of the tree, one dapol_tree_update each: (replaced leaves, new leaves).  A = the last leaf alone; B = leaf 5, which lies below the
# sibling at level 2 of every path from leaf 0 or 1 -- position 61 of a batch whose first 62 siblings are one sub-proof; C = three
# replaced leaves and two new ones.  No replacement of one of the 16 leaves reaches sibling positions 48 .. 59 of any batch (the
# classes m = 8 and m = 4 under splitting / 62), so C also inserts the leaves 2^6 and 2^10, below positions 57 and 53 of the batch [0].
EDITS = {"A": ([M], []), "B": ([5], []), "C": ([5, (1 << 31) + 3, (1 << 40) + 7], [1 << 6, 1 << 10])}
EDITED = {name: sorted(a + b) for name, (a, b) in EDITS.items()}


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _blindings(rng, n):
    r = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    r[:, 31] &= 0x0F
    return r


def _liabilities():
    rng = np.random.default_rng(6464)
    return rng.integers(0, 1 << 28, size=len(LEAVES)).astype(np.uint64), _blindings(rng, len(LEAVES))       # sums stay below 2^32


def _edit(tree, name):
    """new values (none of them an old one) and blindings at the replaced leaves, new liabilities at the inserted ones"""
    rng = np.random.default_rng(sum(name.encode()))
    idx = EDITED[name]
    tree.update(idx, rng.integers(1 << 28, 1 << 29, size=len(idx)).astype(np.uint64), _blindings(rng, len(idx)))


@contextlib.contextmanager
def _order(hip_lib, cfg):
    saved = hip_lib.wire_config_set(siblings_leaf_first=cfg[3])
    try:
        yield
    finally:
        hip_lib.wire_config_restore(saved)


def _plan(pyref, cfg, S):
    """[(first sibling, siblings, parties m)] of the sub-proofs of a batch of S siblings, in blob order"""
    plan, pos = pyref.policy_plan("padding" if cfg[0] == 0 else "splitting", S, cfg[1])
    return [(s, c, m) for s, c, m in plan] + [(i, 1, 1) for i in range(pos, S)]


def _positions(pyref, cfg, batch):
    """[(level, index)] of the batch's siblings in the configuration's proof order: level by level from the root side, or from the leaf
    level up; left to right within a level either way"""
    pos = pyref.batch_siblings(H, batch)
    return sorted(pos) if cfg[3] else pos


def _model(pyref, cfg, batches, edited, has_old=None):
    """{(batch j, sub-proof s): (m, dirty, sibling positions within the sub-proof that moved)} on Python integers"""
    out = {}
    for j, b in enumerate(batches):
        pos = _positions(pyref, cfg, b)
        for s, (start, count, m) in enumerate(_plan(pyref, cfg, len(pos))):
            moved = [i for i in range(count) if any((x >> pos[start + i][0]) == pos[start + i][1] for x in edited)]
            out[j, s] = (m, bool(moved) or (has_old is not None and not has_old[j]), moved)
    return out


def _pieces(hip_lib, pyref, cfg, f, j):
    """[(first byte, last byte + 1)] of the sub-proofs of batch j inside the blob of the call"""
    at, out = int(f.ro[j]), []
    for _, _, m in _plan(pyref, cfg, int(f.so[j + 1] - f.so[j])):
        size = hip_lib.lib().dapol_range_proof_size(cfg[2], m)
        out.append((at, at + size))
        at += size
    assert at == int(f.ro[j + 1])
    return out


def _fallbacks(hip_lib):
    n = ctypes.c_uint64()
    assert hip_lib.lib().dapol_diag_verify_fallbacks(ctypes.byref(n)) == 0
    return n.value


def _new_tree(hip_lib, ctx):
    v, r = _liabilities()
    return hip_lib.Tree(ctx, H, np.array(LEAVES, np.uint64), v, r, SEED)


@pytest.fixture(scope="module")
def ctx64(hip_lib):
    c = hip_lib.Context(0, 64)
    yield c
    c.close()


class _World:
    """The unedited tree and, per configuration, the proofs of BATCHES in one call: computed once, never changed."""

    def __init__(self, hip_lib, ctx):
        self.hip_lib, self.ctx = hip_lib, ctx
        self.v, self.r = _liabilities()
        self.tree = _new_tree(hip_lib, ctx)
        self.root = self.tree.root()
        self.lC, self.lH = ctx.commit_hash_batch(self.v, self.r)
        self.sel = [LEAVES.index(x) for b in BATCHES for x in b]
        self.loff = np.concatenate([[0], np.cumsum([len(b) for b in BATCHES])]).astype(int)
        self.made = {}

    def call(self, cfg):
        if cfg not in self.made:
            with _order(self.hip_lib, cfg):
                self.made[cfg] = _Old(self.tree.prove_batches(BATCHES, cfg[0], cfg[1], cfg[2], SEED))
        return self.made[cfg]

    def verify(self, cfg, **over):
        f = self.call(cfg)
        a = dict(so=f.so, ro=f.ro, sC=f.sC, sH=f.sH, blob=f.blob, batches=BATCHES)
        a.update(over)
        return self.ctx.verify_batches(H, a["batches"], self.lC[self.sel], self.lH[self.sel], a["so"], a["sC"], a["sH"], self.root[0], self.root[1],
                                       cfg[0], cfg[1], cfg[2], a["ro"], a["blob"], verify_seed=SEED).tolist()

    def verify_one(self, cfg, j, **over):
        """dapol_verify_batch_checked for batch j of the (possibly tampered) call"""
        f = self.call(cfg)
        a = dict(so=f.so, ro=f.ro, sC=f.sC, sH=f.sH, blob=f.blob, batches=BATCHES)
        a.update(over)
        s0, s1, r0, r1, l0, l1 = int(a["so"][j]), int(a["so"][j + 1]), int(a["ro"][j]), int(a["ro"][j + 1]), self.loff[j], self.loff[j + 1]
        return int(self.ctx.verify_batch(H, np.array(a["batches"][j], np.uint64), self.lC[self.sel][l0:l1], self.lH[self.sel][l0:l1], a["sC"][s0:s1],
                                         a["sH"][s0:s1], self.root[0], self.root[1], cfg[0], cfg[1], cfg[2], a["blob"][r0:r1].tobytes(), verify_seed=SEED))


@pytest.fixture(scope="module")
def world(hip_lib, ctx64):
    w = _World(hip_lib, ctx64)
    yield w
    w.tree.close()


# ------------------------------------------------------------------------------------------------ 1. the shapes (host calls only)
def test_the_call_has_the_shapes_it_is_meant_to_have(hip_lib, pyref):
    assert len(DISTINCT) == 13 and sorted(ORDER) == list(range(15)) and ORDER != sorted(ORDER)
    assert all(b in BATCHES for b in DISTINCT) and BATCHES.count([T]) == 2 and BATCHES.count([0, M]) == 2
    assert all(x in LEAVES for b in BATCHES for x in b) and len(LEAVES) == 16 == len(set(LEAVES)) and LEAVES == sorted(LEAVES)
    assert any(1 << 32 <= x < T for x in LEAVES) and sum(x >= T for x in LEAVES) >= 6
    ns, so, _, ng = hip_lib.batches_plan(H, BATCHES, *PAD62[:3])
    ns = [int(x) for x in ns]
    assert ns == [len(pyref.batch_siblings(H, b)) for b in BATCHES]
    assert [ns[BATCHES.index(b)] for b in DISTINCT] == [64, 64, 64, 126, 63, 62, 63, 64, 126, 157, 256, 124, 184]
    assert (min(ns), max(ns)) == (62, 256) and int(so[-1]) == sum(ns) > 1500
    rows = {s: ns.count(s) for s in set(ns)}
    assert ng == len(rows) >= 8 and max(rows.values()) >= 3 and 1 in rows.values()
    classes = {m for S in ns for _, _, m in _plan(pyref, SPLIT62, S)}
    assert classes == {1, 2, 4, 8, 16, 32}                                           # six size classes in one call
    assert max(c for S in ns for _, c, _ in _plan(pyref, PAD62, S)) == 62            # 124 pieces: 8 strides of 16 lanes, 2 pad parties
    assert {m for S in ns for _, _, m in _plan(pyref, PAD62, S)} == {1, 64} and {m for S in ns for _, _, m in _plan(pyref, PAD16, S)} == {1, 16}
    assert max(len(_plan(pyref, PAD0, S)) for S in ns) == 257                        # the pad proof and one proof per sibling
    for cfg in CONFIGS:
        pairs = sum(len(_plan(pyref, cfg, S)) for S in ns)
        assert hip_lib.reprove_batches_plan(H, BATCHES, [], cfg[0], cfg[1], cfg[2], has_old=[0] * len(BATCHES))[1] == pairs


def test_the_edits_dirty_what_they_are_meant_to(hip_lib, pyref):
    """Edit B under padding / 62: a 62-sibling sub-proof whose only moved commitment lies past the first stride of the dirty kernel.
    Edit C under splitting / 62: every size class has a dirty and a kept pair.  The library's host planner agrees with the model."""
    model = _model(pyref, PAD62, BATCHES, EDITED["B"])
    late = {k: moved for k, (m, dirty, moved) in model.items() if m == 64 and dirty and min(moved) >= 8}
    assert late and all(moved == [61] for moved in late.values())                    # siblings 0 .. 60 of the sub-proof are unchanged:
    assert all(2 * min(moved) >= REPROVE_LANES for moved in late.values())           # the first differing 16-byte piece is piece 122
    assert (BATCHES.index([0]), 0) in late and (BATCHES.index([0, 1]), 0) in late
    assert any(m == 64 and dirty and moved == [0] for m, dirty, moved in model.values())         # (and one found in the first stride)
    model = _model(pyref, SPLIT62, BATCHES, EDITED["C"])
    for cls in (1, 2, 4, 8, 16, 32):
        states = {dirty for m, dirty, _ in model.values() if m == cls}
        assert states == {False, True}, cls
    for name, edited in EDITED.items():
        for cfg in CONFIGS + [PAD62_LEAF_FIRST]:
            with _order(hip_lib, cfg):
                n_proved, tot, sm, sm_all = hip_lib.reprove_batches_plan(H, BATCHES, edited, cfg[0], cfg[1], cfg[2])
            model = _model(pyref, cfg, BATCHES, edited)
            assert [int(x) for x in n_proved] == [sum(d for (j, _), (_, d, _) in model.items() if j == jj) for jj in range(len(BATCHES))]
            assert (tot, sm, sm_all) == (sum(d for _, d, _ in model.values()), sum(m for m, d, _ in model.values() if d), sum(m for m, _, _ in model.values()))
            assert 0 < tot < len(model), (name, cfg)


# ------------------------------------------------------------------------------------------------ 2. prove_batches
@pytest.mark.parametrize("cfg", CONFIGS + [PAD62_LEAF_FIRST], ids=IDS)
def test_bytes_equal_prove_batch(hip_lib, pyref, world, cfg):
    f = world.call(cfg)
    with _order(hip_lib, cfg):
        _, pso, pro, _ = hip_lib.batches_plan(H, BATCHES, cfg[0], cfg[1], cfg[2])
        assert f.so.tolist() == pso.tolist() and f.ro.tolist() == pro.tolist()
        for j, b in enumerate(BATCHES):
            level, index, wC, wH, wb = world.tree.prove_batch(np.array(b, np.uint64), cfg[0], cfg[1], cfg[2], SEED)
            assert list(zip(map(int, level), map(int, index))) == _positions(pyref, cfg, b), (j, "sibling positions")
            s0, s1, r0, r1 = int(f.so[j]), int(f.so[j + 1]), int(f.ro[j]), int(f.ro[j + 1])
            assert f.sC[s0:s1].tobytes() == wC.tobytes() and f.sH[s0:s1].tobytes() == wH.tobytes(), (j, b, "siblings")
            assert f.blob[r0:r1].tobytes() == wb, (j, b, "range blob")
    if cfg == PAD62_LEAF_FIRST:                                   # the same records in the other order, and other bytes for it
        g = world.call(PAD62)
        for j, b in enumerate(BATCHES):
            s0, s1 = int(f.so[j]), int(f.so[j + 1])
            at = [_positions(pyref, cfg, b).index(p) for p in _positions(pyref, PAD62, b)]
            assert f.sC[s0:s1][at].tobytes() == g.sC[s0:s1].tobytes() and f.sH[s0:s1][at].tobytes() == g.sH[s0:s1].tobytes()
        assert f.blob.tobytes() != g.blob.tobytes()


@pytest.fixture(scope="module")
def oracle_tree(ref):
    """the C oracle's tree over the same leaves -> path(leaf) = (C, H, v, r) of its 64 siblings, root side first"""
    v, r = _liabilities()
    idx = np.array(LEAVES, np.uint64)
    t = ctypes.c_void_p(ref.ref_tree_build(H, ctypes.c_size_t(len(LEAVES)), _p(idx), _p(v), _p(r), SEED, 0))
    assert t
    paths = {}

    def path(leaf):
        if leaf not in paths:
            sC, sH, s_r, s_v = [ctypes.create_string_buffer(32 * H) for _ in range(3)] + [(ctypes.c_uint64 * H)()]
            assert ref.ref_tree_path(t, ctypes.c_uint64(leaf), sC, sH, s_v, s_r) == 1
            cut = lambda buf: [buf.raw[32 * i:32 * i + 32] for i in range(H)]
            paths[leaf] = (cut(sC), cut(sH), list(s_v), cut(s_r))
        return paths[leaf]
    yield path
    ref.ref_tree_free(t)


def _oracle_blob(ref, plan, n_bits, sib_v, sib_r, seed, stream):
    """R::generate_proof with the C oracle's prover: the sub-proofs in plan order on one nonce stream, the slot base advancing by m (2n + 4)"""
    out, slot = b"", 0
    for start, cnt, m in plan:
        v = np.zeros(m, np.uint64)
        r = np.zeros((m, 32), np.uint8)
        v[:cnt] = sib_v[start:start + cnt]
        r[:cnt] = sib_r[start:start + cnt]
        r[cnt:, 0] = 1                                         # a pad party is (0, Scalar::one())
        buf = ctypes.create_string_buffer(ref.ref_range_proof_size(n_bits, m))
        assert ref.ref_range_prove(n_bits, m, _p(v), _p(r), seed, ctypes.c_uint64(stream), ctypes.c_uint64(slot), None, 0, buf) == 0
        out += buf.raw
        slot += m * (2 * n_bits + 4)
    return out


@pytest.mark.parametrize("sample", range(len(SAMPLED)), ids=["S%d" % s for s in (126, 62, 256)])
@pytest.mark.parametrize("cfg", [PAD62, SPLIT62], ids=IDS)
def test_sampled_batches_equal_the_c_oracle(hip_lib, ref, pyref, world, oracle_tree, cfg, sample):
    """Siblings from the C oracle's tree, the blob from its range prover sub-proof by sub-proof: the seed chained through the batch's
    leaves, the stream id the batch's first leaf.  (One batch a case: the oracle takes 17 ms per one-party proof on one core.)"""
    f, b = world.call(cfg), SAMPLED[sample]
    j = BATCHES.index(b)
    pos = pyref.batch_siblings(H, b)
    level, index = hip_lib.batch_siblings(H, np.array(b, np.uint64))
    assert list(zip(map(int, level), map(int, index))) == pos
    sC, sH, sv, sr = [], [], [], []
    for lv, ix in pos:                                         # the sibling at (level, index), on the path of a leaf of the batch beside it
        src = next(x for x in b if (x >> lv) ^ 1 == ix)
        pC, pH, pv, pr = oracle_tree(src)
        sC.append(pC[H - 1 - lv]), sH.append(pH[H - 1 - lv]), sv.append(pv[H - 1 - lv]), sr.append(pr[H - 1 - lv])
    s0, s1, r0, r1 = int(f.so[j]), int(f.so[j + 1]), int(f.ro[j]), int(f.ro[j + 1])
    assert s1 - s0 == len(pos)
    assert f.sC[s0:s1].tobytes() == b"".join(sC) and f.sH[s0:s1].tobytes() == b"".join(sH), (b, "siblings")
    want = _oracle_blob(ref, _plan(pyref, cfg, len(pos)), cfg[2], np.array(sv, np.uint64), np.frombuffer(b"".join(sr), np.uint8).reshape(-1, 32),
                        pyref.batch_nonce_seed(SEED, b), b[0])
    assert f.blob[r0:r1].tobytes() == want, (b, "range blob")


# ------------------------------------------------------------------------------------------------ 3. verify_batches
@pytest.mark.parametrize("cfg", [PAD62, SPLIT62, PAD0, PAD62_LEAF_FIRST], ids=IDS)
def test_the_provers_output_verifies_without_a_fallback(hip_lib, world, cfg):
    world.call(cfg)
    with _order(hip_lib, cfg):
        before = _fallbacks(hip_lib)
        assert world.verify(cfg) == [1] * len(BATCHES)
        assert _fallbacks(hip_lib) == before


def test_eight_bit_proofs_of_larger_sums_are_rejected_as_verify_batch_rejects_them(hip_lib, pyref, world):
    """padding / 16 / 8 on liabilities of 28 bits: a batch verifies iff every sibling's sum is below 2^8 -- here none does."""
    want = []
    for b in BATCHES:
        sums = [sum(int(v) for x, v in zip(LEAVES, world.v) if x >> lv == ix) for lv, ix in pyref.batch_siblings(H, b)]
        want.append(int(all(s < 256 for s in sums)))
    assert want == [0] * len(BATCHES)
    assert world.verify(PAD16) == want
    assert [world.verify_one(PAD16, j) for j in (0, 3, len(BATCHES) - 1)] == [0, 0, 0]


def test_the_python_oracle_accepts_the_paths(pyref, world):
    f = world.call(PAD62)
    for b in (FIVE, [0, 1, T, T + 1, M - 1, M]):
        j = BATCHES.index(b)
        rows = [LEAVES.index(x) for x in b]
        leaves = [(x, world.lC[i].tobytes(), world.lH[i].tobytes()) for x, i in zip(b, rows)]
        sibs = [(f.sC[s].tobytes(), f.sH[s].tobytes()) for s in range(int(f.so[j]), int(f.so[j + 1]))]
        assert pyref.verify_batch_paths(world.root[0], world.root[1], H, leaves, sibs)
        assert not pyref.verify_batch_paths(world.root[0], world.root[1], H, leaves, sibs[:40] + [sibs[41], sibs[40]] + sibs[42:])


def test_five_tampered_batches_fail_and_nothing_else(hip_lib, world):
    cfg = PAD62
    f = world.call(cfg)
    a, b, c, e = BATCHES.index([0]), BATCHES.index([M]), BATCHES.index([0, 1, 5]), BATCHES.index(FIVE)
    d = BATCHES.index([T])
    twin = BATCHES.index([T], d + 1)
    sC, sH, blob = f.sC.copy(), f.sH.copy(), f.blob.copy()
    pos = [hip_lib.batch_siblings(H, np.array(BATCHES[j], np.uint64))[0] for j in (a, b)]
    assert int(pos[0][0]) == H - 1 and int(pos[1][-1]) == 0
    sH[int(f.so[a]), 9] ^= 1                                      # a: the sibling hash next to the root
    sH[int(f.so[b + 1]) - 1, 30] ^= 0x80                          # b: the sibling hash at level 0
    sC[int(f.so[c]) + 3], sC[int(f.so[c]) + 4] = f.sC[int(f.so[c]) + 4], f.sC[int(f.so[c]) + 3]      # c: two neighbouring commitments swapped
    batches = [list(x) for x in BATCHES]
    batches[d] = [T ^ (1 << 63)]                                  # d: the proof of leaf 2^63 presented for its mirror, leaf 0 (S stays 64)
    blob[int(f.ro[e + 1]) - 3] ^= 4                               # e: one bit of the last of its 195 sub-proofs
    over = dict(sC=sC, sH=sH, blob=blob, batches=batches)
    bad = {a, b, c, d, e}
    assert len(bad) == 5 and twin not in bad
    want = [int(j not in bad) for j in range(len(BATCHES))]
    assert world.verify(cfg, **over) == want
    assert [world.verify_one(cfg, j, **over) for j in range(len(BATCHES))] == want


# ------------------------------------------------------------------------------------------------ 4. reprove_batches
class _Edited:
    """A tree of its own after one edit, and the fresh proofs of BATCHES on it per configuration."""

    def __init__(self, hip_lib, ctx, name):
        self.hip_lib, self.name = hip_lib, name
        self.tree = _new_tree(hip_lib, ctx)
        _edit(self.tree, name)
        self.made = {}

    def fresh(self, cfg):
        if cfg not in self.made:
            with _order(self.hip_lib, cfg):
                self.made[cfg] = _Old(self.tree.prove_batches(BATCHES, cfg[0], cfg[1], cfg[2], SEED))
        return self.made[cfg]

    def reprove(self, cfg, oC, oR, **kw):
        with _order(self.hip_lib, cfg):
            return self.tree.reprove_batches(BATCHES, oC, oR, cfg[0], cfg[1], cfg[2], SEED, **kw)


@pytest.fixture(scope="module")
def edited(hip_lib, ctx64):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Edited(hip_lib, ctx64, name)
        return made[name]
    yield get
    for e in made.values():
        e.tree.close()


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("name", sorted(EDITS))
def test_reprove_equals_a_fresh_call_and_proves_what_the_model_says(hip_lib, pyref, world, edited, name, cfg):
    old, e = world.call(cfg), edited(name)
    f = e.fresh(cfg)
    model = _model(pyref, cfg, BATCHES, EDITED[name])
    so, ro, sC, sH, blob, proved, kept, calls = e.reprove(cfg, old.sC, old.blob)
    assert so.tolist() == f.so.tolist() and ro.tolist() == f.ro.tolist()
    assert sC.tobytes() == f.sC.tobytes() and sH.tobytes() == f.sH.tobytes(), "siblings"
    for j in range(len(BATCHES)):
        for s, (a, z) in enumerate(_pieces(hip_lib, pyref, cfg, f, j)):
            assert blob[a:z].tobytes() == f.blob[a:z].tobytes(), (j, s, "the fresh call's bytes")
            assert (blob[a:z].tobytes() != old.blob[a:z].tobytes()) == model[j, s][1], (j, s, "kept bytes are the old ones, dirty ones are new")
    n_dirty = sum(d for _, d, _ in model.values())
    assert proved == n_dirty > 0 and proved + kept == len(model) and kept > 0
    assert 1 <= calls <= len({m for m, d, _ in model.values() if d})


def test_reprove_with_some_batches_without_an_old_proof(hip_lib, pyref, world, edited):
    cfg, e = PAD62, edited("B")
    old, f = world.call(cfg), e.fresh(cfg)
    flags = [int(j % 3 != 1) for j in range(len(BATCHES))]
    oC, oR = old.sC.copy(), old.blob.copy()
    for j, has in enumerate(flags):
        if not has:                                               # junk where the old rows would be: a kept byte of it would show
            oC[int(old.so[j]):int(old.so[j + 1])] = 0xEE
            oR[int(old.ro[j]):int(old.ro[j + 1])] = 0xEE
    so, ro, sC, sH, blob, proved, kept, calls = e.reprove(cfg, oC, oR, has_old=flags)
    assert sC.tobytes() == f.sC.tobytes() and sH.tobytes() == f.sH.tobytes() and blob.tobytes() == f.blob.tobytes()
    model = _model(pyref, cfg, BATCHES, EDITED["B"], has_old=flags)
    assert proved == sum(d for _, d, _ in model.values()) and proved + kept == len(model)
    assert proved > sum(d for _, d, _ in _model(pyref, cfg, BATCHES, EDITED["B"]).values()) and kept > 0


def test_reprove_outputs_may_alias_the_old_arrays(hip_lib, world, edited):
    cfg, e = PAD62, edited("A")
    old, f = world.call(cfg), e.fresh(cfg)
    separate = e.reprove(cfg, old.sC, old.blob)
    aC, aR = old.sC.copy(), old.blob.copy()
    aliased = e.reprove(cfg, aC, aR, alias=True)
    assert np.shares_memory(aliased[2], aC) and np.shares_memory(aliased[4], aR)
    assert aC.tobytes() == separate[2].tobytes() == f.sC.tobytes() and aR.tobytes() == separate[4].tobytes() == f.blob.tobytes()
    assert aliased[3].tobytes() == separate[3].tobytes() and aliased[5:] == separate[5:]


# ------------------------------------------------------------------------------------------------ 5. BatchStore
def _same(store, want):
    C, Hh, blob = store.read()
    return C.tobytes() == want.sC.tobytes() and Hh.tobytes() == want.sH.tobytes() and blob.tobytes() == want.blob.tobytes()


@pytest.mark.parametrize("cfg", [PAD62, PAD0], ids=IDS)
def test_batch_store_fill_edit_refresh_relist_fetch_verify(hip_lib, pyref, ctx64, world, cfg):
    tree = _new_tree(hip_lib, ctx64)
    store = hip_lib.BatchStore(tree, cfg[0], cfg[1], cfg[2], SEED)
    try:
        # 1. filled, the store holds prove_batches' rows
        old = world.call(cfg)
        n_pairs = len(_model(pyref, cfg, BATCHES, []))
        proved, kept, calls, moved = store.refresh(BATCHES)
        assert (proved, kept, moved) == (n_pairs, 0, 0) and calls >= 1 and store.rows == len(BATCHES)
        assert _same(store, old)
        batches, so, ro = store.layout()
        assert batches == BATCHES and so.tolist() == old.so.tolist() and ro.tolist() == old.ro.tolist()
        # 2. edit B and a refresh of the list it holds: in place
        _edit(tree, "B")
        fresh = _Old(tree.prove_batches(BATCHES, cfg[0], cfg[1], cfg[2], SEED))
        model = _model(pyref, cfg, BATCHES, EDITED["B"])
        proved, kept, calls, moved = store.refresh()
        assert (proved, kept, moved) == (sum(d for _, d, _ in model.values()), sum(not d for _, d, _ in model.values()), 0)
        assert _same(store, fresh)
        # 3. another list: two batches dropped, one new, the rest in another order
        dropped = (BATCHES.index(FIVE), BATCHES.index([0]))
        new = [1, T]
        rest = [j for j in range(len(BATCHES)) if j not in dropped][::-1]
        rows = rest[:4] + [None] + rest[4:]
        relist = [new if j is None else BATCHES[j] for j in rows]
        assert new not in BATCHES and len(relist) == len(BATCHES) - 1
        lowest = [None if j is None else BATCHES.index(BATCHES[j]) for j in rows]     # the continuation: the lowest equal old row
        _, pso, pro, _ = hip_lib.batches_plan(H, relist, cfg[0], cfg[1], cfg[2])
        sizes = [(int(pso[j + 1] - pso[j]), int(pro[j + 1] - pro[j])) for j in range(len(relist))]
        oC, oR = fresh.rows(list(zip(lowest, sizes)))
        ref_counters = tree.reprove_batches(relist, oC, oR, cfg[0], cfg[1], cfg[2], SEED, has_old=[int(j is not None) for j in rows])[5:8]
        proved, kept, calls, moved = store.refresh(relist)
        want = _Old(tree.prove_batches(relist, cfg[0], cfg[1], cfg[2], SEED))
        assert _same(store, want) and store.layout()[0] == relist
        assert (proved, kept, calls) == ref_counters and moved == len(relist) - 1
        assert proved == len(_plan(pyref, cfg, len(pyref.batch_siblings(H, new)))) and kept > 0      # nothing was edited: only the new batch
        # 4. rows in a scrambled order with a repeat
        query = [7, 0, len(relist) - 1, 7, 4, 2]
        qs, qr, C, Hh, blob = store.fetch(query)
        _, fso, fro, _ = hip_lib.batches_plan(H, [relist[q] for q in query], cfg[0], cfg[1], cfg[2])
        assert qs.tolist() == fso.tolist() and qr.tolist() == fro.tolist()
        for i, q in enumerate(query):
            s0, s1, r0, r1 = int(want.so[q]), int(want.so[q + 1]), int(want.ro[q]), int(want.ro[q + 1])
            assert C[int(qs[i]):int(qs[i + 1])].tobytes() == want.sC[s0:s1].tobytes(), (i, q)
            assert Hh[int(qs[i]):int(qs[i + 1])].tobytes() == want.sH[s0:s1].tobytes(), (i, q)
            assert blob[int(qr[i]):int(qr[i + 1])].tobytes() == want.blob[r0:r1].tobytes(), (i, q)
        # 5. every row verifies against the tree as it is now
        assert store.verify(SEED).tolist() == [1] * len(relist)
    finally:
        store.close()
        tree.close()


# ------------------------------------------------------------------------------------------------ 6. the other 32-byte digests
DG_H = 6
DG_LEAVES = [1, 5, 9, 12, 20, 21, 22, 23, 33, 44, 57, 63]
DG_BATCHES = [[21], [1, 63], [20, 21, 22, 23], [5, 9, 12], [63], [9, 33, 44, 57]]       # S = 6, 10, 4, 9, 6, 13
DG_CFG = (0, 4, 8)
DIGESTS = {"blake2s": 1, "sha256": digest_shims.NEW_DIGESTS["sha256"][0], "sha3_256": digest_shims.NEW_DIGESTS["sha3_256"][0]}


@pytest.fixture(scope="module")
def blake3_ctx8(hip_lib):
    c = hip_lib.Context(0, 8)
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(DIGESTS))
def test_the_family_under_another_digest(hip_lib, pyref, blake3_ctx8, name):
    digest_shims.register(pyref)
    assert (hip_lib.DIGEST_BLAKE2S, hip_lib.DIGEST_SHA256, hip_lib.DIGEST_SHA3_256) == (DIGESTS["blake2s"], DIGESTS["sha256"], DIGESTS["sha3_256"])
    rng = np.random.default_rng(66)
    idx = np.array(DG_LEAVES, np.uint64)
    v, r = rng.integers(0, 4, size=len(DG_LEAVES)).astype(np.uint64), _blindings(rng, len(DG_LEAVES))
    ns = [len(pyref.batch_siblings(DG_H, b)) for b in DG_BATCHES]
    assert {len(b) for b in DG_BATCHES} == {1, 2, 3, 4} and min(ns) == DG_CFG[1] and len(set(ns)) >= 4
    ctx = hip_lib.Context(0, 8, digest=DIGESTS[name])
    tree = hip_lib.Tree(ctx, DG_H, idx, v, r, SEED)
    store = hip_lib.BatchStore(tree, *DG_CFG, SEED)
    try:
        # prove_batches against prove_batch, and its sibling hashes against the Python oracle's tree under this digest
        f = _Old(tree.prove_batches(DG_BATCHES, *DG_CFG, SEED))
        pt = pyref.Tree(DG_H, [(x, pyref.node_new(int(vv), int.from_bytes(rr.tobytes(), "little"), name)) for x, vv, rr in zip(DG_LEAVES, v, r)], SEED, name)
        root = tree.root()
        assert (root[0], root[1]) == (pt.root.C, pt.root.H)
        for j, b in enumerate(DG_BATCHES):
            _, _, wC, wH, wb = tree.prove_batch(np.array(b, np.uint64), *DG_CFG, SEED)
            s0, s1, r0, r1 = int(f.so[j]), int(f.so[j + 1]), int(f.ro[j]), int(f.ro[j + 1])
            assert f.sC[s0:s1].tobytes() == wC.tobytes() and f.sH[s0:s1].tobytes() == wH.tobytes() and f.blob[r0:r1].tobytes() == wb, (j, b)
            nodes = [pt.levels[lv][ix] for lv, ix in pyref.batch_siblings(DG_H, b)]
            assert [f.sH[s].tobytes() for s in range(s0, s1)] == [n.H for n in nodes] and [f.sC[s].tobytes() for s in range(s0, s1)] == [n.C for n in nodes]
        # verify_batches: all 1, as the Python oracle's Merkle verifier under this digest; all 0 on a BLAKE3 context; one flipped hash
        lC, lH = ctx.commit_hash_batch(v, r)
        sel = [DG_LEAVES.index(x) for b in DG_BATCHES for x in b]
        verify = lambda c, sH, h=None: c.verify_batches(DG_H, DG_BATCHES, lC[sel], (lH if h is None else h)[sel], f.so, f.sC, sH, root[0], root[1], *DG_CFG,
                                                         f.ro, f.blob, verify_seed=SEED).tolist()
        assert verify(ctx, f.sH) == [1] * len(DG_BATCHES)
        for j, b in enumerate(DG_BATCHES):
            leaves = [(x, lC[DG_LEAVES.index(x)].tobytes(), lH[DG_LEAVES.index(x)].tobytes()) for x in b]
            sibs = [(f.sC[s].tobytes(), f.sH[s].tobytes()) for s in range(int(f.so[j]), int(f.so[j + 1]))]
            assert pyref.verify_batch_paths(root[0], root[1], DG_H, leaves, sibs, dg=name), (j, b)
            assert not pyref.verify_batch_paths(root[0], root[1], DG_H, leaves, sibs, dg="blake3")
        assert verify(blake3_ctx8, f.sH) == [0] * len(DG_BATCHES)
        assert verify(blake3_ctx8, f.sH, blake3_ctx8.commit_hash_batch(v, r)[1]) == [0] * len(DG_BATCHES)    # (with BLAKE3 leaf hashes too)
        bad = f.sH.copy()
        bad[int(f.so[3]) + 2, 17] ^= 2
        assert verify(ctx, bad) == [1, 1, 1, 0, 1, 1]
        # a store filled before, and reprove_batches and the store's refresh after, one update
        assert store.refresh(DG_BATCHES)[:2] == (sum(n - DG_CFG[1] + 1 for n in ns), 0) and _same(store, f)
        tree.update([44], [3], _blindings(rng, 1))
        g = _Old(tree.prove_batches(DG_BATCHES, *DG_CFG, SEED))
        model = {(j, s): any((44 >> lv) == ix for lv, ix in pyref.batch_siblings(DG_H, b)[start:start + count])
                 for j, b in enumerate(DG_BATCHES) for s, (start, count, _) in enumerate(_plan(pyref, DG_CFG + (0,), ns[j]))}
        so, ro, sC, sH, blob, proved, kept, calls = tree.reprove_batches(DG_BATCHES, f.sC, f.blob, *DG_CFG, SEED)
        assert sC.tobytes() == g.sC.tobytes() and sH.tobytes() == g.sH.tobytes() and blob.tobytes() == g.blob.tobytes()
        assert (proved, kept) == (sum(model.values()), len(model) - sum(model.values())) and proved > 0 and kept > 0
        assert g.sH.tobytes() != f.sH.tobytes()
        assert store.refresh() == (proved, kept, calls, 0) and _same(store, g)
        v[DG_LEAVES.index(44)] = 3
        assert store.verify(SEED).tolist() == [1] * len(DG_BATCHES)
    finally:
        store.close()
        tree.close()
        ctx.close()
