"""The shared-proof entity family -- dapol_prove_entities_shared(_compact), dapol_reprove_entities_shared, dapol_proof_store_*,
dapol_verify_entities_shared / _compact / _compact_paths -- at the edge of the range the library accepts: a tree of height 64 with 18
leaves on both sides of 2^31, 2^32 and 2^63, 64-bit proofs of up to 64 parties on a context of 64 parties (one leaf holds 2^63), plans of
1 to 65 sub-proofs in up to six size classes under both sibling orders, and (height 6, 8 parties) the three other 32-byte digests.

Every comparison is byte for byte or verdict for verdict.  The references are dapol_range_prove_batch statement by statement
(check_definition), the C oracle's tree, range prover and range verifier for four sampled statements (161 parties of 64 bits in all:
measured once, 0.5 to 0.6 s to prove and verify each of the two 64-party ones on the GPU machine's CPU, 1.4 s for the four; a sample
of every statement would take minutes), dapol_verify_entities for every verdict vector, the
Python oracle's trees under each digest, and for the re-proving calls a brute-force model on Python integers: a pair (entity, sub-proof)
is dirty exactly when the entity is new or an edited leaf lies below one of the sub-proof's siblings.

The shapes are chosen for what the smaller suites cannot reach: spans of 62 and 64 siblings (124 and 128 commitment pieces, eight
strides of the 16-lane compare loops), a single moved sibling at piece 122 of such a span, key shifts of 62, 63 and 64, stream ids at
and above 2^63, count = 64 and start = 63 in the plan tables next to aggregated sub-proofs."""
import contextlib
import ctypes

import numpy as np
import pytest

import digest_shims
from test_gpu_reprove import heads_and_kept
from test_gpu_shared_proofs import check_definition
from test_shared_plan_abi import H6_LEAVES, key_depth, plan_of

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
H = 64
T, M = 1 << 63, (1 << 64) - 1
LEAVES = [0, 1, 2, 3, 5, (1 << 31) + 3, 1 << 32, (1 << 32) + 1, (1 << 40) + 7, (1 << 62) + 9,
          T, T + 1, T + 2, T + 3, T + (1 << 20), T + (1 << 62) + 5, M - 1, M]
# (policy, aggregation, n_bits, leaf_first)
PAD62, PAD62_LF = (0, 62, 64, 0), (0, 62, 64, 1)
SPLIT63, SPLIT63_LF = (1, 63, 64, 0), (1, 63, 64, 1)
PAD64, PAD0 = (0, 64, 64, 0), (0, 0, 64, 0)
PAD16, PAD16_LF = (0, 16, 64, 0), (0, 16, 64, 1)
CONFIGS = [PAD62, PAD62_LF, SPLIT63, SPLIT63_LF, PAD64, PAD0, PAD16, PAD16_LF]
IDS = lambda c: "p%d-a%d-n%d-lf%d" % c
# what a big-integer model of the fixture gives: (distinct statements, entity x sub-proof pairs); the tests recompute both
TABLE = {PAD62: (40, 54), PAD62_LF: (24, 54), SPLIT63: (74, 126), SPLIT63_LF: (46, 126), PAD64: (18, 18), PAD0: (457, 1170), PAD16: (385, 882),
         PAD16_LF: (317, 882)}
REPROVE_LANES = 16                                              # kernels_reprove.h, kernels_verify_compact.h: lanes that stride over a span's 16-byte pieces
# the edits of the tree, one dapol_tree_update each: (replaced leaves, new leaves).  A = the last leaf (a new blinding under its value of
# 2^63); B = leaf 5, which lies below the sibling at level 2 of the leaves 0 .. 3 and nowhere else on their paths; C = three replaced
# leaves and three new ones between old ones: T + 2^33 opens a run of its own, 2^6 sits inside the run of key 0.
EDITS = {"A": ([M], []), "B": ([5], []), "C": ([5, (1 << 31) + 3, (1 << 40) + 7], [1 << 6, 1 << 10, T + (1 << 33)])}
EDITED = {name: sorted(a + b) for name, (a, b) in EDITS.items()}


@pytest.fixture(autouse=True)
def through_the_kernels(monkeypatch):
    monkeypatch.setenv("DAPOL_VSHARED_FORWARD_MAX", "0")          # 18 x 3 pairs would forward to dapol_verify_entities


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _blindings(rng, n):
    r = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    r[:, 31] &= 0x0F
    return r


def _liabilities():
    rng = np.random.default_rng(6464)
    v = rng.integers(0, 1 << 28, size=len(LEAVES)).astype(np.uint64)
    v[-1] = 1 << 63                                               # the top bit of a 64-bit party; the sum of all stays below 2^64
    return v, _blindings(rng, len(LEAVES))


@contextlib.contextmanager
def _order(hip_lib, cfg):
    saved = hip_lib.wire_config_set(siblings_leaf_first=cfg[3])
    try:
        yield
    finally:
        hip_lib.wire_config_restore(saved)


def _fallbacks(hip_lib):
    n = ctypes.c_uint64()
    assert hip_lib.lib().dapol_diag_verify_fallbacks(ctypes.byref(n)) == 0
    return n.value


# ------------------------------------------------------------------------------------------------ the model, on Python integers
def _plan(pyref, cfg):
    return plan_of(pyref, cfg[0], H, cfg[1])


def _level(cfg, i):
    """the level (0 = leaves) of sibling i of a path"""
    return i if cfg[3] else H - 1 - i


def _shift(cfg, start, count):
    return H - key_depth(start, count, H, cfg[3])


def _key(x, shift):
    return 0 if shift >= 64 else x >> shift


def _statements(pyref, cfg, leaves):
    """distinct subtree keys per sub-proof of the plan"""
    return [len({_key(x, _shift(cfg, start, count)) for x in leaves}) for start, count, _ in _plan(pyref, cfg)]


def _model(pyref, cfg, leaves, edited, old=None):
    """{(sub-proof s, row e): (m, dirty, head, sibling positions within the sub-proof that moved)}.  leaves = the rows of the call,
    old = the leaves that have an old row (default: all)."""
    old = set(leaves) if old is None else set(old)
    out = {}
    for s, (start, count, m) in enumerate(_plan(pyref, cfg)):
        sh, prev = _shift(cfg, start, count), False
        for e, x in enumerate(leaves):
            lv = [_level(cfg, start + i) for i in range(count)]
            moved = [i for i in range(count) if any((y >> lv[i]) == (x >> lv[i]) ^ 1 for y in edited)]
            dirty = x not in old or bool(moved)
            head = dirty and (e == 0 or _key(x, sh) != _key(leaves[e - 1], sh) or not prev)
            out[s, e] = (m, dirty, head, moved)
            prev = dirty
    return out


def _counts(model):
    """(heads, kept pairs)"""
    return sum(h for _, _, h, _ in model.values()), sum(not d for _, d, _, _ in model.values())


def _late(model):
    """the pairs with exactly one moved sibling, at a position >= 8 of a span of more than 8: the first differing piece is >= 16"""
    return {k: mv for k, (_, d, _, mv) in model.items() if len(mv) == 1 and mv[0] >= 8 and 2 * mv[0] >= REPROVE_LANES}


def _offsets(hip_lib, pyref, cfg):
    sizes = [hip_lib.lib().dapol_range_proof_size(cfg[2], m) for _, _, m in _plan(pyref, cfg)]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(int)


def _verifier_heads(hip_lib, pyref, cfg, idx, pC, blobs=None):
    """The heads of the verifiers' definitions over the bytes.  blobs None: dapol_verify_entities_compact's (a new key, or a covered
    commitment that differs from the row before); otherwise dapol_verify_entities_shared's (proof bytes or covered commitments that
    differ from the row before)."""
    off, n = _offsets(hip_lib, pyref, cfg), 0
    for s, (start, count, _) in enumerate(_plan(pyref, cfg)):
        sh = _shift(cfg, start, count)
        for e in range(len(idx)):
            com = e > 0 and pC[e, start:start + count].tobytes() != pC[e - 1, start:start + count].tobytes()
            if blobs is None:
                n += int(e == 0 or _key(int(idx[e]), sh) != _key(int(idx[e - 1]), sh) or com)
            else:
                n += int(e == 0 or com or blobs[e, off[s]:off[s + 1]].tobytes() != blobs[e - 1, off[s]:off[s + 1]].tobytes())
    return n


# ------------------------------------------------------------------------------------------------ the tree and its proofs
@pytest.fixture(scope="module")
def ctx64(hip_lib):
    c = hip_lib.Context(0, 64)
    yield c
    c.close()


class _World:
    """A tree over LEAVES, the liabilities it holds (edited together) and, per configuration, the shared call over all its leaves:
    computed once per state of the tree."""

    def __init__(self, hip_lib, ctx, edits=()):
        self.hip_lib, self.ctx = hip_lib, ctx
        v, r = _liabilities()
        self.book = {x: (int(v[i]), r[i]) for i, x in enumerate(LEAVES)}
        self.tree = hip_lib.Tree(ctx, H, np.array(LEAVES, np.uint64), v, r, SEED)
        self.made = {}
        for name in edits:
            self.edit(name)

    def edit(self, name):
        """new values (none of them an old one; the last leaf keeps its 2^63) and blindings at the replaced leaves, new liabilities at
        the inserted ones"""
        rng = np.random.default_rng(sum(name.encode()))
        idx = EDITED[name]
        v, r = rng.integers(1 << 28, 1 << 29, size=len(idx)).astype(np.uint64), _blindings(rng, len(idx))
        for i, x in enumerate(idx):
            if x == M:
                v[i] = 1 << 63
            self.book[x] = (int(v[i]), r[i])
        self.tree.update(np.array(idx, np.uint64), v, r)
        self.made = {}

    @property
    def leaves(self):
        return sorted(self.book)

    @property
    def idx(self):
        return np.array(self.leaves, np.uint64)

    def leaf_nodes(self):
        if "leaf" not in self.made:
            v, r = np.array([self.book[x][0] for x in self.leaves], np.uint64), np.stack([self.book[x][1] for x in self.leaves])
            self.made["leaf"] = self.ctx.commit_hash_batch(v, r)
        return self.made["leaf"]

    def call(self, cfg):
        """(path_C, path_H, blobs, unique) of prove_entities_shared over every leaf"""
        if cfg not in self.made:
            with _order(self.hip_lib, cfg):
                self.made[cfg] = self.tree.prove_entities_shared(self.idx, cfg[0], cfg[1], cfg[2], SEED)
        return self.made[cfg]

    def compact(self, cfg):
        """(path_C, path_H, compact, unique) of prove_entities_shared_compact over every leaf"""
        if ("compact", cfg) not in self.made:
            with _order(self.hip_lib, cfg):
                self.made["compact", cfg] = self.tree.prove_entities_shared_compact(self.idx, cfg[0], cfg[1], cfg[2], SEED)
        return self.made["compact", cfg]

    def head(self, cfg, pC=None, pH=None):
        """the arguments every verifier takes before the proofs"""
        lC, lH = self.leaf_nodes()
        root = self.tree.root()
        c = self.call(cfg)
        return (H, self.idx, lC, lH, c[0] if pC is None else pC, c[1] if pH is None else pH, root[0], root[1], cfg[0], cfg[1], cfg[2])

    def verdicts(self, cfg, pC=None, pH=None, blobs=None):
        """dapol_verify_entities over the (possibly tampered) shared call"""
        blobs = self.call(cfg)[2] if blobs is None else blobs
        with _order(self.hip_lib, cfg):
            return self.ctx.verify_entities(*self.head(cfg, pC, pH), blobs, verify_seed=SEED).tolist()


@pytest.fixture(scope="module")
def world(hip_lib, ctx64):
    w = _World(hip_lib, ctx64)
    yield w
    w.tree.close()


@pytest.fixture(scope="module")
def edited(hip_lib, ctx64):
    """a tree of its own after one edit, per edit"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = _World(hip_lib, ctx64, edits=[name])
        return made[name]
    yield get
    for w in made.values():
        w.tree.close()


# ------------------------------------------------------------------------------------------------ 0. the shapes (host calls only)
def test_the_fixture_has_the_shapes_it_is_meant_to_have(hip_lib, pyref):
    assert len(LEAVES) == 18 == len(set(LEAVES)) and LEAVES == sorted(LEAVES) and LEAVES[-1] == M
    assert any(1 << 32 <= x < T for x in LEAVES) and sum(x >= T for x in LEAVES) == 8
    v, _ = _liabilities()
    assert int(v[-1]) == 1 << 63 and all(int(x) < 1 << 28 for x in v[:-1]) and sum(int(x) for x in v) + 6 * (1 << 29) < 1 << 64
    assert [(c, m) for _, c, m in _plan(pyref, PAD62)] == [(62, 64), (1, 1), (1, 1)]
    assert [(c, m) for _, c, m in _plan(pyref, SPLIT63)] == [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2), (1, 1), (1, 1)]      # six groups
    assert _plan(pyref, PAD64) == [(0, 64, 64)] and len(_plan(pyref, PAD0)) == 65 and len(_plan(pyref, PAD16)) == 49
    assert max(start for cfg in CONFIGS for start, _, _ in _plan(pyref, cfg)) == 63
    for cfg in CONFIGS:
        with _order(hip_lib, cfg):
            n_sub, tot, per = hip_lib.shared_plan(H, LEAVES, cfg[0], cfg[1])
        want = _statements(pyref, cfg, LEAVES)
        assert [int(x) for x in n_sub] == want, cfg
        assert (tot, per) == (sum(want), len(LEAVES) * len(want)) == TABLE[cfg], cfg
    shifts = lambda cfg: {_shift(cfg, start, count) for start, count, _ in _plan(pyref, cfg)}
    assert {62, 63} <= shifts(PAD62_LF) and 63 not in shifts(PAD62) and 64 in shifts(PAD0)         # the key is the top bit alone; the key is 0


def test_the_edits_dirty_what_they_are_meant_to(hip_lib, pyref):
    """Conditions of the tests below, asserted from the model so that a change of the fixture cannot lose them silently; and the
    library's host planner agrees with the model for every edit and configuration."""
    # both outcomes in every size class
    both = [_model(pyref, SPLIT63, LEAVES, EDITED["B"]), _model(pyref, SPLIT63, sorted(set(LEAVES) | set(EDITED["C"])), EDITED["C"], old=LEAVES)]
    for cls in (32, 16, 8, 4, 2, 1):
        assert {d for model in both for m, d, _, _ in model.values() if m == cls} == {False, True}, cls
    # a single late sibling: pieces 0 .. 15 of the span are equal, one of the later strides has to find the difference
    late = {cfg: _late(_model(pyref, cfg, LEAVES, EDITED["B"])) for cfg in CONFIGS}
    assert {cfg: len(x) for cfg, x in late.items() if x} == {PAD62: 8, PAD62_LF: 4, SPLIT63: 3, SPLIT63_LF: 2, PAD64: 8}
    for e in range(4):                                          # leaves 0 .. 3, root side first: sibling 61 alone, pieces 122 and 123
        assert late[PAD62][0, e] == [61] and late[PAD64][0, e] == [61]
    # the new leaves of edit C: between old ones, one opens a run, one sits inside the run of key 0
    after = sorted(set(LEAVES) | set(EDITED["C"]))
    model = _model(pyref, PAD62, after, EDITED["C"], old=LEAVES)
    for x in EDITS["C"][1]:
        assert x not in LEAVES and LEAVES[0] < x < LEAVES[-1]
    e = after.index(T + (1 << 33))
    assert model[0, e][2] and (T + (1 << 33)) >> 2 not in {y >> 2 for y in LEAVES}
    e = after.index(1 << 6)
    assert _key(1 << 6, 32) == 0 and _model(pyref, SPLIT63, after, EDITED["C"], old=LEAVES)[0, e][1]
    for name in sorted(EDITS):
        rows = sorted(set(LEAVES) | set(EDITED[name]))
        has_old = [int(x in LEAVES) for x in rows]
        for cfg in CONFIGS:
            model = _model(pyref, cfg, rows, EDITED[name], old=LEAVES)
            with _order(hip_lib, cfg):
                n_sub, tot, sm, _ = hip_lib.reprove_plan(H, rows, EDITED[name], cfg[0], cfg[1], has_old)
            assert [int(x) for x in n_sub] == [sum(h for (s, _), (_, _, h, _) in model.items() if s == ss) for ss in range(len(_plan(pyref, cfg)))], (name, cfg)
            assert (tot, sm) == (_counts(model)[0], sum(m for m, _, h, _ in model.values() if h))
            # (edit C reaches below a sibling of every path: under padding / 64, one span per row, nothing is kept)
            assert 0 < tot and (_counts(model)[1] > 0) == ((name, cfg) != ("C", PAD64)), (name, cfg)


# ------------------------------------------------------------------------------------------------ 1. the prover's definition
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_every_sub_proof_is_the_range_provers_row_of_its_statement(hip_lib, pyref, ctx64, world, cfg):
    idx = world.idx
    pC, pH, blobs, unique = world.call(cfg)
    with _order(hip_lib, cfg):
        sC, sH, sv, sr = world.tree.paths(idx)
        assert pC.tobytes() == sC.tobytes() and pH.tobytes() == sH.tobytes()
        n_stmts = check_definition(hip_lib, pyref, ctx64, idx, sv, sr, cfg[0], cfg[1], cfg[2], cfg[3], blobs)
        n_sub, tot, per = hip_lib.shared_plan(H, idx, cfg[0], cfg[1])
    assert unique == tot == n_stmts == sum(_statements(pyref, cfg, LEAVES)) == TABLE[cfg][0]
    assert per == TABLE[cfg][1] and (unique == per) == (cfg == PAD64)                 # one span down to the leaf: nothing is shared
    cC, cH, compact, cunique = world.compact(cfg)
    assert cC.tobytes() == sC.tobytes() and cH.tobytes() == sH.tobytes() and cunique == unique


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


# (configuration, leaf, sub-proof): a 64-party statement whose key is 2^63 (and whose second party, the subtree that holds the last
# leaf, exceeds 2^63); the 64-party statement whose last party is the leaf that holds exactly 2^63; a 32-party one; a one-party one
# under shift 63, whose key is the index's top bit alone
SAMPLED = [(PAD62, T, 0), (PAD64, M - 1, 0), (SPLIT63, 0, 0), (PAD62_LF, M, 2)]


@pytest.mark.parametrize("cfg,leaf,s", SAMPLED, ids=["m64-key-2^63", "m64-party-2^63", "m32", "m1-shift-63"])
def test_sampled_statements_equal_the_c_oracle(hip_lib, ref, pyref, world, oracle_tree, cfg, leaf, s):
    """Independent of the GPU prover and of the GPU tree: siblings from the C oracle's tree, the proof from its range prover under
    stream id = the subtree key and slot base 0, and its range verifier accepts what the GPU wrote."""
    start, count, m = _plan(pyref, cfg)[s]
    shift = _shift(cfg, start, count)
    stream = _key(leaf, shift) << shift if shift < 64 else 0
    oC, oH, ov, o_r = oracle_tree(leaf)
    at = [H - 1 - _level(cfg, start + i) for i in range(count)]           # the oracle's rows are root side first
    v, r = np.zeros(m, np.uint64), np.zeros((m, 32), np.uint8)
    v[:count] = [ov[j] for j in at]
    r[:count] = [np.frombuffer(o_r[j], np.uint8) for j in at]
    r[count:, 0] = 1                                                      # a pad party is (0, Scalar::one())
    if (cfg, leaf) == (PAD62, T):
        assert (m, stream) == (64, T) and int(v[1]) > T
    if (cfg, leaf) == (PAD64, M - 1):
        assert (m, stream) == (64, M - 1) and int(v[63]) == T
    if cfg == SPLIT63:
        assert m == 32
    if cfg == PAD62_LF:
        assert (m, shift, stream) == (1, 63, T)
    e = LEAVES.index(leaf)
    pC, pH, blobs, _ = world.call(cfg)
    assert [pC[e, start + i].tobytes() for i in range(count)] == [oC[j] for j in at] and [pH[e, start + i].tobytes() for i in range(count)] == [oH[j] for j in at]
    ps = ref.ref_range_proof_size(cfg[2], m)
    off = _offsets(hip_lib, pyref, cfg)
    assert off[s + 1] - off[s] == ps
    buf = ctypes.create_string_buffer(ps)
    assert ref.ref_range_prove(cfg[2], m, _p(v), _p(r), SEED, ctypes.c_uint64(stream), ctypes.c_uint64(0), None, 0, buf) == 0
    got = blobs[e, off[s]:off[s + 1]].tobytes()
    assert got == buf.raw
    Vs = b"".join(oC[j] for j in at) + pyref.B_BLINDING.compress() * (m - count)
    assert ref.ref_range_verify(cfg[2], m, got, ctypes.c_size_t(ps), Vs, bytes([7]) + bytes(31), 0) == 1


# ------------------------------------------------------------------------------------------------ 2. the verifiers agree
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_the_verifiers_agree_and_check_each_statement_once(hip_lib, pyref, ctx64, world, cfg):
    idx = world.idx
    pC, pH, blobs, unique = world.call(cfg)
    _, _, compact, _ = world.compact(cfg)
    head = world.head(cfg)
    want = world.verdicts(cfg)
    assert want == [1] * len(LEAVES) and unique == TABLE[cfg][0]
    with _order(hip_lib, cfg):
        before = _fallbacks(hip_lib)
        ok, n = ctx64.verify_entities_shared(*head, blobs, verify_seed=SEED)
        assert ok.tolist() == want and n == unique == _verifier_heads(hip_lib, pyref, cfg, idx, pC, blobs)
        ok, n = ctx64.verify_entities_compact(*head, compact, verify_seed=SEED)
        assert ok.tolist() == want and n == unique == _verifier_heads(hip_lib, pyref, cfg, idx, pC)
        cC, cH = world.tree.paths_compact(idx)
        ok, n, merges = ctx64.verify_entities_compact_paths(*head[:4], cC, cH, *head[6:], compact, verify_seed=SEED)
        assert ok.tolist() == want and n == unique and merges == len(cC) == hip_lib.compact_paths_plan(H, idx, want_ref=False)[2]
        store = hip_lib.ProofStore(world.tree, cfg[0], cfg[1], cfg[2], SEED)
        try:
            assert store.refresh() == (unique, 0, 0)
            assert store.verify(SEED).tolist() == want
            sidx, scompact = store.read_compact()
            assert sidx.tolist() == idx.tolist() and scompact.tobytes() == compact.tobytes()
        finally:
            store.close()
        assert _fallbacks(hip_lib) == before
        assert hip_lib.shared_compress(H, idx, cfg[0], cfg[1], cfg[2], blobs).tobytes() == compact.tobytes()
        assert hip_lib.shared_expand(H, idx, cfg[0], cfg[1], cfg[2], compact).tobytes() == blobs.tobytes()
        assert len(compact) == hip_lib.shared_compact_plan(H, idx, cfg[0], cfg[1], cfg[2])[2]


# ------------------------------------------------------------------------------------------------ 3. tampering at late pieces
def _both_verifiers(hip_lib, pyref, ctx, world, cfg, pC=None, blobs=None):
    """(verdicts, unique of verify_entities_shared, unique of verify_entities_compact) over a tampered shared call, after comparing
    both verdict vectors with dapol_verify_entities' on the same input and both counts with the definitions' heads over the bytes"""
    c = world.call(cfg)
    pC = c[0] if pC is None else pC
    tampered_blobs = blobs is not None
    blobs = c[2] if blobs is None else blobs
    want = world.verdicts(cfg, pC=pC, blobs=blobs)
    head = world.head(cfg, pC=pC)
    with _order(hip_lib, cfg):
        ok, n_shared = ctx.verify_entities_shared(*head, blobs, verify_seed=SEED)
        assert ok.tolist() == want
        assert n_shared == _verifier_heads(hip_lib, pyref, cfg, world.idx, pC, blobs)
        n_compact = None
        if not tampered_blobs:                                    # (the compact form holds one copy of a run's proof: no row of its own to tamper)
            ok, n_compact = ctx.verify_entities_compact(*head, world.compact(cfg)[2], verify_seed=SEED)
            assert ok.tolist() == want
            assert n_compact == _verifier_heads(hip_lib, pyref, cfg, world.idx, pC)
    return want, n_shared, n_compact


# (configuration, tampered sibling): the last sibling of the 62-sibling span (pieces 122 and 123 of 124); the last of the 32-sibling
# span of splitting / 63 (pieces 62 and 63 of 64); sibling 61 under splitting / 63, inside its two-party sub-proof
TAMPERS = [(PAD62, 61), (SPLIT63, 31), (SPLIT63, 61)]


@pytest.mark.parametrize("cfg,sib", TAMPERS, ids=lambda x: IDS(x) if isinstance(x, tuple) else "sib%d" % x)
def test_a_tampered_late_commitment_fails_its_row_alone(hip_lib, pyref, ctx64, world, cfg, sib):
    """(a) in the head row of a shared run, (b) in a follower.  A compare loop that stopped after its first stride would not see the
    difference: the followers would inherit the head's failure, or the tampered follower its head's success."""
    plan = _plan(pyref, cfg)
    s = next(i for i, (start, count, _) in enumerate(plan) if start <= sib < start + count)
    start, count, m = plan[s]
    sh = _shift(cfg, start, count)
    run = [e for e, x in enumerate(LEAVES) if _key(x, sh) == 0]
    assert run[:4] == [0, 1, 2, 3] and len(run) == (4 if sh == 2 else 6) and sib == start + count - 1
    if sib != 61 or cfg == PAD62:
        assert 2 * (sib - start) >= REPROVE_LANES and count > 8
    unique = world.call(cfg)[3]
    for row, more in ((0, 1), (2, 2)):                            # the row behind a tampered one opens a run of its own
        pC = world.call(cfg)[0].copy()
        pC[row, sib, 9] ^= 0x20
        want, n_shared, n_compact = _both_verifiers(hip_lib, pyref, ctx64, world, cfg, pC=pC)
        assert want == [int(e != row) for e in range(len(LEAVES))], (row, "only the tampered row fails")
        assert n_shared == n_compact == unique + more, row


@pytest.mark.parametrize("cfg", [PAD62, SPLIT63], ids=IDS)
def test_a_tampered_last_piece_of_a_followers_proof_fails_that_row_alone(hip_lib, pyref, ctx64, world, cfg):
    """(c) the last 16-byte piece of the largest proof (66 pieces of a 64-party proof, 62 of a 32-party one) in one follower's blob"""
    off = _offsets(hip_lib, pyref, cfg)
    assert (off[1] - off[0]) // 16 == (66 if cfg == PAD62 else 62)
    blobs = world.call(cfg)[2].copy()
    assert blobs[2, :off[1]].tobytes() == blobs[0, :off[1]].tobytes()
    blobs[2, off[1] - 5] ^= 0x01
    want, n_shared, _ = _both_verifiers(hip_lib, pyref, ctx64, world, cfg, blobs=blobs)
    assert want == [int(e != 2) for e in range(len(LEAVES))]
    assert n_shared == world.call(cfg)[3] + 2


@pytest.mark.parametrize("cfg", [PAD62, SPLIT63], ids=IDS)
def test_a_tampered_compact_path_record_fails_the_rows_below_it(hip_lib, pyref, ctx64, world, cfg):
    """(d) one record of the compact paths at depth 62: the sibling that the leaves 0 .. 3 share (and nobody else), then the one that
    T .. T + 3 share.  The verdicts are dapol_verify_entities_compact's over the expansion."""
    idx = world.idx
    compact = world.compact(cfg)[2]
    head = world.head(cfg)
    depth_off, ref_rows, n_records = hip_lib.compact_paths_plan(H, idx)
    keys = sorted({x >> 2 for x in LEAVES})                      # the records of depth 62, in ascending key order
    with _order(hip_lib, cfg):
        cC, cH = world.tree.paths_compact(idx)
        assert len(cC) == n_records
        for first in (0, T):
            rows = [e for e, x in enumerate(LEAVES) if x >> 2 == first >> 2]
            assert [LEAVES[e] for e in rows] == [first, first + 1, first + 2, first + 3]
            rec = int(depth_off[62]) + keys.index(first >> 2)
            assert all(int(depth_off[62]) + int(ref_rows[61][e]) == rec for e in rows)
            bad = cC.copy()
            bad[rec, 9] ^= 0x20
            pC, pH = hip_lib.compact_paths_expand(H, idx, bad, cH)
            want, _ = ctx64.verify_entities_compact(*head[:4], pC, pH, *head[6:], compact, verify_seed=SEED)
            ok, _, _ = ctx64.verify_entities_compact_paths(*head[:4], bad, cH, *head[6:], compact, verify_seed=SEED)
            assert ok.tolist() == want.tolist() == [int(e not in rows) for e in range(len(LEAVES))], first


# ------------------------------------------------------------------------------------------------ 4. re-proving after an edit
def _reprove_and_check(hip_lib, pyref, w, cfg, old, edited_leaves):
    """old = (leaves, path_C, blobs) of the shared call before the edit, w = the edited world.  Re-proves and compares everything with
    a fresh shared call, the model, the HEAD rule over the bytes and the planner; returns (the new state, proved, kept)."""
    old_leaves, oC, oblobs = old
    idx, rows = w.idx, w.leaves
    fC, fH, fblobs, _ = w.call(cfg)
    with _order(hip_lib, cfg):
        pC, pH, blobs, proved, kept = w.tree.reprove_entities_shared(idx, np.array(old_leaves, np.uint64), oC, oblobs, cfg[0], cfg[1], cfg[2], SEED)
    assert pC.tobytes() == fC.tobytes() and pH.tobytes() == fH.tobytes()
    assert blobs.tobytes() == fblobs.tobytes(), "the fresh call's bytes"
    model = _model(pyref, cfg, rows, edited_leaves, old=old_leaves)
    assert (proved, kept) == _counts(model)
    has_old = np.array([int(x in old_leaves) for x in rows], np.uint8)
    at = [old_leaves.index(x) if x in old_leaves else 0 for x in rows]
    assert (proved, kept) == heads_and_kept(pyref, H, cfg[0], cfg[1], cfg[3], idx, has_old, oC[at], fC)
    with _order(hip_lib, cfg):
        assert proved == hip_lib.reprove_plan(H, idx, sorted(edited_leaves), cfg[0], cfg[1], has_old)[1]
    off = _offsets(hip_lib, pyref, cfg)
    for (s, e), (_, dirty, _, _) in model.items():
        if has_old[e]:
            assert (blobs[e, off[s]:off[s + 1]].tobytes() != oblobs[at[e], off[s]:off[s + 1]].tobytes()) == dirty, (s, e, "kept bytes are the old ones, dirty ones are new")
    assert w.verdicts(cfg, pC=pC, pH=pH, blobs=blobs) == [1] * len(rows)
    return (rows, pC, blobs), proved, kept


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("name", sorted(EDITS))
def test_reprove_equals_a_fresh_call_and_proves_what_the_model_says(hip_lib, pyref, world, edited, name, cfg):
    oC, _, oblobs, unique = world.call(cfg)
    _, proved, kept = _reprove_and_check(hip_lib, pyref, edited(name), cfg, (LEAVES, oC, oblobs), EDITED[name])
    assert 0 < proved and (kept > 0) == ((name, cfg) != ("C", PAD64))
    if name == "B" and cfg in (PAD62, PAD64):                     # the run 0 .. 3 is dirty through pieces 122 and 123 alone
        model = _model(pyref, cfg, LEAVES, EDITED[name])
        assert all(model[0, e][1] and model[0, e][3] == [61] for e in range(4))


@pytest.mark.parametrize("cfg", [PAD62, SPLIT63_LF], ids=IDS)
def test_reprove_chained_over_three_edits_of_one_tree(hip_lib, pyref, ctx64, world, cfg):
    oC, _, oblobs, _ = world.call(cfg)
    w = _World(hip_lib, ctx64)
    try:
        state = (LEAVES, oC, oblobs)
        for name in "ABC":
            w.edit(name)
            state, proved, kept = _reprove_and_check(hip_lib, pyref, w, cfg, state, EDITED[name])
            assert 0 < proved and 0 < kept
    finally:
        w.tree.close()


# ------------------------------------------------------------------------------------------------ 5. the proof store
@pytest.mark.parametrize("cfg", [PAD62_LF, SPLIT63, PAD0], ids=IDS)
def test_proof_store_fill_edit_refresh_insert_fetch_read_verify(hip_lib, pyref, ctx64, world, cfg):
    """Rows of 128 commitment pieces and up to 2,730 blob pieces through the store's move, fetch and compact kernels."""
    w = _World(hip_lib, ctx64)
    assert hip_lib.lib().dapol_entity_proof_size(H, *PAD0[:3]) // 16 == 2730
    with _order(hip_lib, cfg):
        store = hip_lib.ProofStore(w.tree, cfg[0], cfg[1], cfg[2], SEED)
        try:
            def same(want):
                sidx, C, Hh, blobs = store.read()
                return sidx.tolist() == w.leaves and C.tobytes() == want[0].tobytes() and Hh.tobytes() == want[1].tobytes() and blobs.tobytes() == want[2].tobytes()

            assert store.refresh() == (TABLE[cfg][0], 0, 0) and same(world.call(cfg))
            w.edit("B")
            assert store.refresh() == _counts(_model(pyref, cfg, LEAVES, EDITED["B"])) + (0,)
            assert same(w.call(cfg))
            w.edit("C")
            assert store.refresh(w.idx) == _counts(_model(pyref, cfg, w.leaves, EDITED["C"], old=LEAVES)) + (len(LEAVES),)
            fC, fH, fblobs, _ = w.call(cfg)
            assert store.rows == len(LEAVES) + 3 and same((fC, fH, fblobs))
            # rows by leaf: the last row first, one leaf the store does not hold
            query = [M, 0, 7, T]
            found, C, Hh, blobs = store.fetch(query)
            assert found.tolist() == [1, 1, 0, 1]
            for i, x in enumerate(query):
                if x in w.leaves:
                    e = w.leaves.index(x)
                    assert C[i].tobytes() == fC[e].tobytes() and Hh[i].tobytes() == fH[e].tobytes() and blobs[i].tobytes() == fblobs[e].tobytes(), x
                else:
                    assert not C[i].any() and not Hh[i].any() and not blobs[i].any()
            found, C, Hh, blobs = store.fetch([M])
            assert found.tolist() == [1] and w.leaves[-1] == M
            assert C[0].tobytes() == fC[-1].tobytes() and Hh[0].tobytes() == fH[-1].tobytes() and blobs[0].tobytes() == fblobs[-1].tobytes()
            # a window over the row of leaf 2^63
            e = w.leaves.index(T)
            ridx, C, Hh, blobs = store.read(e - 1, 3)
            assert ridx.tolist() == w.leaves[e - 1:e + 2] and ridx[0] < T
            assert C.tobytes() == fC[e - 1:e + 2].tobytes() and Hh.tobytes() == fH[e - 1:e + 2].tobytes() and blobs.tobytes() == fblobs[e - 1:e + 2].tobytes()
            sidx, compact = store.read_compact()
            assert sidx.tolist() == w.leaves and compact.tobytes() == w.compact(cfg)[2].tobytes()
            assert store.verify(SEED).tolist() == [1] * store.rows
        finally:
            store.close()
            w.tree.close()


# ------------------------------------------------------------------------------------------------ 6. the other 32-byte digests
DG_H, DG_BITS = 6, 8
DG_CASES = [(0, 3), (1, 5)]                                     # padding / 3, splitting / 5
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
    idx = np.array(H6_LEAVES, np.uint64)
    v, r = rng.integers(0, 21, size=len(idx)).astype(np.uint64), _blindings(rng, len(idx))        # every sum fits the 8-bit proofs
    ctx = hip_lib.Context(0, 8, digest=DIGESTS[name])
    tree = hip_lib.Tree(ctx, DG_H, idx, v, r, SEED)
    stores = {}
    try:
        # the shared call; its path hashes against the Python oracle's tree under this digest
        pt = pyref.Tree(DG_H, [(x, pyref.node_new(int(vv), int.from_bytes(rr.tobytes(), "little"), name)) for x, vv, rr in zip(H6_LEAVES, v, r)], SEED, name)
        root = tree.root()
        assert (root[0], root[1]) == (pt.root.C, pt.root.H)
        lC, lH = ctx.commit_hash_batch(v, r)
        cC, cH = tree.paths_compact(idx)
        old = {}
        for policy, agg in DG_CASES:
            pC, pH, blobs, unique = tree.prove_entities_shared(idx, policy, agg, DG_BITS, SEED)
            old[policy, agg] = (pC, blobs)
            for e, x in enumerate(H6_LEAVES):
                sibs = pt.path_siblings(x)
                assert [pH[e, i].tobytes() for i in range(DG_H)] == [n.H for n in sibs] and [pC[e, i].tobytes() for i in range(DG_H)] == [n.C for n in sibs], (e, x)
            assert unique == hip_lib.shared_plan(DG_H, idx, policy, agg)[1] < len(idx) * len(plan_of(pyref, policy, DG_H, agg))
            _, _, compact, cunique = tree.prove_entities_shared_compact(idx, policy, agg, DG_BITS, SEED)
            assert cunique == unique and hip_lib.shared_expand(DG_H, idx, policy, agg, DG_BITS, compact).tobytes() == blobs.tobytes()
            # the verifiers: all ones, as dapol_verify_entities; all zeros on a BLAKE3 context; one flipped path hash
            head = lambda h: (DG_H, idx, lC, lH, pC, h, root[0], root[1], policy, agg, DG_BITS)
            chead = (DG_H, idx, lC, lH, cC, cH, root[0], root[1], policy, agg, DG_BITS)
            for c, want in ((ctx, [1] * len(idx)), (blake3_ctx8, [0] * len(idx))):
                assert c.verify_entities(*head(pH), blobs, verify_seed=SEED).tolist() == want
                assert c.verify_entities_shared(*head(pH), blobs, verify_seed=SEED)[0].tolist() == want
                assert c.verify_entities_compact(*head(pH), compact, verify_seed=SEED)[0].tolist() == want
                assert c.verify_entities_compact_paths(*chead, compact, verify_seed=SEED)[0].tolist() == want
            assert ctx.verify_entities_shared(*head(pH), blobs, verify_seed=SEED)[1] == unique == ctx.verify_entities_compact(*head(pH), compact, verify_seed=SEED)[1]
            bad = pH.copy()
            bad[5, 2, 17] ^= 2
            want = ctx.verify_entities(*head(bad), blobs, verify_seed=SEED).tolist()
            assert want == [int(e != 5) for e in range(len(idx))]
            assert ctx.verify_entities_shared(*head(bad), blobs, verify_seed=SEED)[0].tolist() == want
            assert ctx.verify_entities_compact(*head(bad), compact, verify_seed=SEED)[0].tolist() == want
            stores[policy, agg] = hip_lib.ProofStore(tree, policy, agg, DG_BITS, SEED)
            assert stores[policy, agg].refresh() == (unique, 0, 0)
            assert stores[policy, agg].read_compact()[1].tobytes() == compact.tobytes()
        # one edit; the re-prover and the store's refresh equal a fresh call
        tree.update(np.array([17], np.uint64), np.array([5], np.uint64), _blindings(rng, 1))
        assert tree.root()[1] != root[1]
        for policy, agg in DG_CASES:
            oC, oblobs = old[policy, agg]
            fC, fH, fblobs, _ = tree.prove_entities_shared(idx, policy, agg, DG_BITS, SEED)
            pC, pH, blobs, proved, kept = tree.reprove_entities_shared(idx, idx, oC, oblobs, policy, agg, DG_BITS, SEED)
            assert pC.tobytes() == fC.tobytes() and pH.tobytes() == fH.tobytes() and blobs.tobytes() == fblobs.tobytes()
            assert (proved, kept) == heads_and_kept(pyref, DG_H, policy, agg, 0, idx, np.ones(len(idx), np.uint8), oC, fC)
            assert proved == hip_lib.reprove_plan(DG_H, idx, [17], policy, agg)[1] > 0 and kept > 0 and fH.tobytes() != old[policy, agg][0].tobytes()
            store = stores[policy, agg]
            assert store.refresh() == (proved, kept, 0)
            sidx, C, Hh, sblobs = store.read()
            assert C.tobytes() == fC.tobytes() and Hh.tobytes() == fH.tobytes() and sblobs.tobytes() == fblobs.tobytes()
            _, _, compact, _ = tree.prove_entities_shared_compact(idx, policy, agg, DG_BITS, SEED)
            assert store.read_compact()[1].tobytes() == compact.tobytes()
            assert store.verify(SEED).tolist() == [1] * len(idx)
    finally:
        for store in stores.values():
            store.close()
        tree.close()
        ctx.close()
