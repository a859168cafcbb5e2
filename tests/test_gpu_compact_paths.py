"""Compact Merkle paths on the GPU: dapol_tree_paths_compact leaves every distinct sibling once, dapol_verify_entities_compact_paths
merges every distinct node once.  The tests pin the DEFINITIONS (include/dapol_hip.h, "COMPACT Merkle paths"): the expansion of the
prover's buffer is dapol_tree_paths' (C, H) byte for byte, and the verifier's verdicts are dapol_verify_entities_compact's over the
expansion of whatever buffer it is given -- tampered ones included -- with path_merges = the record count whenever sharing answered.

Calls with b x plan size <= 64 forward; DAPOL_VSHARED_FORWARD_MAX=0 sends the small trees through the kernels, and the forwarding test
runs with the library's own limit."""
import numpy as np
import pytest

from test_gpu_forgeries import _blindings

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))
N_BITS = 8
# RFC 9496, 4.3.1: s must be the canonical encoding of a field element.  These 32 bytes are p = 2^255 - 19 itself, i.e. s = 0 (the
# identity) written non-canonically: a decoder that reduces instead of rejecting takes it for a valid point.
NON_CANONICAL = bytes([0xED] + [0xFF] * 30 + [0x7F])


def _scattered(rng, H, n, taken):
    out = set()
    while len(out) < n:
        x = int(rng.integers(0, 1 << 62)) % (1 << H) if H < 64 else int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
        if x not in taken:
            out.add(x)
    return out


def leaves_of(H):
    rng = np.random.default_rng(100 + H)
    if H == 1:
        return [0, 1]
    if H == 2:
        return [0, 1, 3]
    if H == 6:
        return list(range(64))                                  # every sibling is another row's ancestor
    if H == 12:
        run = set(range(1000, 1100))
        return sorted(run | _scattered(rng, H, 100, run))
    top = (1 << H) - 1
    fixed = {0, top, 4096, 4097, top - 9, top - 8} if H == 32 else {0, top, 1 << 63, (1 << 63) + 1}     # the ends, sibling pairs
    return sorted(fixed | _scattered(rng, H, (160 if H == 32 else 70) - len(fixed), fixed))


def policies_of(H):
    """padding at aggregation H, padding at aggregation 0, splitting at an aggregation between the two"""
    return [(0, H), (0, 0), (1, {1: 1, 2: 1, 6: 3, 12: 5, 32: 24, 64: 24}[H])]


class Case:
    """A tree, all its leaves as the rows of a call, their paths in both forms and the set model of the compact layout."""

    def __init__(self, hip, ctx, H, leaves=None):
        self.hip, self.ctx, self.H = hip, ctx, H
        rng = np.random.default_rng(H)
        self.leaves = leaves_of(H) if leaves is None else leaves
        self.idx = np.array(self.leaves, np.uint64)
        self.b = len(self.leaves)
        self.v = rng.integers(0, 2, size=self.b, dtype=np.uint64)           # the sum of all leaves stays below 2^8
        self.r = _blindings(rng, self.b)
        self.tree = hip.Tree(ctx, H, self.idx, self.v, self.r, SEED)
        self.lC, self.lH = ctx.commit_hash_batch(self.v, self.r)
        self.root = self.tree.root()
        self.pC, self.pH, _, _ = self.tree.paths(self.idx)
        self.cC, self.cH = self.tree.paths_compact(self.idx)
        key = lambda x, d: 0 if d == 0 else x >> (H - d)
        self.key = key
        self.keys = [sorted({key(x, d) for x in self.leaves}) for d in range(H + 1)]
        self.depth_off = [0, 0]
        for d in range(1, H + 1):
            self.depth_off.append(self.depth_off[-1] + len(self.keys[d]))
        self.n_records = self.depth_off[-1]
        self.proofs = {}

    def record(self, d, k):
        return self.depth_off[d] + self.keys[d].index(k)

    def rows_under(self, d, k):
        return {e for e, x in enumerate(self.leaves) if self.key(x, d) == k}

    def compact(self, policy, agg):
        if (policy, agg) not in self.proofs:
            _, _, compact, unique = self.tree.prove_entities_shared_compact(self.idx, policy, agg, N_BITS, SEED)
            assert unique == self.hip.shared_plan(self.H, self.idx, policy, agg)[1]
            self.proofs[policy, agg] = compact
        return self.proofs[policy, agg]

    def both(self, policy, agg, cC=None, cH=None, lC=None, lH=None, root=None, compact=None):
        """(verdicts, unique, path_merges, route) of the compact-path verifier, after comparing the verdicts elementwise with
        dapol_verify_entities_compact's over the host expansion of the same records."""
        cC = self.cC if cC is None else cC
        cH = self.cH if cH is None else cH
        lC = self.lC if lC is None else lC
        lH = self.lH if lH is None else lH
        root = self.root if root is None else root
        compact = self.compact(policy, agg) if compact is None else compact
        pC, pH = self.hip.compact_paths_expand(self.H, self.idx, cC, cH)
        want, want_unique = self.ctx.verify_entities_compact(self.H, self.idx, lC, lH, pC, pH, root[0], root[1], policy, agg, N_BITS, compact, verify_seed=SEED)
        ok, unique, merges = self.ctx.verify_entities_compact_paths(self.H, self.idx, lC, lH, cC, cH, root[0], root[1], policy, agg, N_BITS, compact,
                                                                    verify_seed=SEED)
        assert ok.tolist() == want.tolist()
        return ok.tolist(), unique, merges, self.hip.diag_compact_paths()[1], want_unique

    def failing(self, rows):
        return [int(e not in rows) for e in range(self.b)]


@pytest.fixture(autouse=True)
def through_the_kernels(monkeypatch):
    monkeypatch.setenv("DAPOL_VSHARED_FORWARD_MAX", "0")


@pytest.fixture(scope="module")
def ctx64(hip_lib):
    c = hip_lib.Context(0, 64, options=hip_lib.Options(window_bits=8))
    yield c
    c.close()


_CASES = {}


@pytest.fixture
def case(request, hip_lib, gpu_ctx, ctx64):
    H = request.param
    if H not in _CASES:
        _CASES[H] = Case(hip_lib, ctx64 if H == 64 else gpu_ctx, H)
    return _CASES[H]


HEIGHTS = [1, 2, 6, 12, 32, 64]


# ------------------------------------------------------------------------------------------------ (a) the prover's side
@pytest.mark.parametrize("case", HEIGHTS, indirect=True)
def test_paths_compact_expands_to_tree_paths(hip_lib, case):
    c = case
    assert c.cC.shape == (c.n_records, 32) and c.cH.shape == (c.n_records, 32)
    assert hip_lib.compact_paths_plan(c.H, c.idx, want_ref=False)[2] == c.n_records <= c.b * c.H
    for leaf_first in (0, 1):
        old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
        try:
            pC, pH, _, _ = c.tree.paths(c.idx)
            cC, cH = c.tree.paths_compact(c.idx)                      # the layout does not depend on the sibling order
            assert cC.tobytes() == c.cC.tobytes() and cH.tobytes() == c.cH.tobytes()
            eC, eH = hip_lib.compact_paths_expand(c.H, c.idx, cC, cH)
            assert eC.tobytes() == pC.tobytes() and eH.tobytes() == pH.tobytes()
            zC, zH = hip_lib.compact_paths_compress(c.H, c.idx, pC, pH)
            assert zC.tobytes() == cC.tobytes() and zH.tobytes() == cH.tobytes()
            e = c.b // 2
            oC, oH = hip_lib.compact_paths_expand(c.H, c.idx, cC, cH, first=e, count=1)
            assert oC.tobytes() == pC[e].tobytes() and oH.tobytes() == pH[e].tobytes()
        finally:
            hip_lib.wire_config_restore(old)


def test_a_subset_of_the_leaves_and_one_leaf(hip_lib, gpu_ctx):
    c = Case(hip_lib, gpu_ctx, 12) if 12 not in _CASES else _CASES[12]
    for rows in ([0], [c.b - 1], list(range(0, c.b, 3)), [3, 4]):
        idx = c.idx[rows]
        cC, cH = c.tree.paths_compact(idx)
        eC, eH = hip_lib.compact_paths_expand(12, idx, cC, cH)
        assert eC.tobytes() == c.pC[rows].tobytes() and eH.tobytes() == c.pH[rows].tobytes()
        assert len(cC) == hip_lib.compact_paths_plan(12, idx)[2]
    assert len(c.tree.paths_compact(c.idx[:1])[0]) == 12             # one row: its whole path, nothing shared


def test_prover_refusals(hip_lib, gpu_ctx):
    import ctypes
    c = Case(hip_lib, gpu_ctx, 12) if 12 not in _CASES else _CASES[12]
    lib, p = hip_lib.lib(), (lambda a: a.ctypes.data_as(ctypes.c_void_p))
    C, Hh, n = np.full((c.n_records + 8, 32), 0xAB, np.uint8), np.full((c.n_records + 8, 32), 0xAB, np.uint8), ctypes.c_uint64(777)
    untouched = lambda: (C == 0xAB).all() and (Hh == 0xAB).all() and n.value == 777
    call = lambda idx, cap: lib.dapol_tree_paths_compact(c.tree.h, len(idx), p(idx), p(C), p(Hh), cap, ctypes.byref(n))
    free = next(x for x in range(1 << 12) if x not in set(c.leaves))
    assert call(np.array(sorted([c.leaves[0], free, c.leaves[-1]]), np.uint64), len(C)) == 9 and untouched()        # no liability there
    assert call(np.array([c.leaves[0], 1 << 12], np.uint64), len(C)) == 9 and untouched()                            # outside the tree
    assert call(c.idx, c.n_records - 1) == 8 and untouched()                                                        # one record short
    for bad in ([c.leaves[1], c.leaves[0]], [c.leaves[2], c.leaves[2]]):
        assert call(np.array(bad, np.uint64), len(C)) == 8 and untouched()
    assert call(c.idx[:0], 0) == 0 and n.value == 0 and (C == 0xAB).all()
    assert call(c.idx, c.n_records) == 0 and n.value == c.n_records                                                  # exactly enough
    assert C[:c.n_records].tobytes() == c.cC.tobytes() and Hh[:c.n_records].tobytes() == c.cH.tobytes() and (C[c.n_records:] == 0xAB).all()


# ------------------------------------------------------------------------------------------------ (b) the verifier, honest
@pytest.mark.parametrize("case", HEIGHTS, indirect=True)
def test_verifier_honest(hip_lib, case):
    c = case
    for policy, agg in policies_of(c.H):
        ok, unique, merges, route, want_unique = c.both(policy, agg)
        assert ok == [1] * c.b, (policy, agg)
        assert merges == c.n_records and route == 1, (policy, agg)            # every distinct node once: sharing happened
        assert unique == want_unique == hip_lib.shared_plan(c.H, c.idx, policy, agg)[1], (policy, agg)


@pytest.mark.parametrize("case", [1, 6], indirect=True)
def test_fewer_rows_than_leaves(hip_lib, case):
    """H = 1 with b = 1, and a sparse choice of rows at H = 6: the records of the rows of the call, not of the tree."""
    c = case
    rows = [1] if c.H == 1 else [0, 1, 2, 3, 16, 17, 40, 63]
    idx = c.idx[rows]
    cC, cH = c.tree.paths_compact(idx)
    for policy, agg in policies_of(c.H):
        _, _, compact, _ = c.tree.prove_entities_shared_compact(idx, policy, agg, N_BITS, SEED)
        ok, unique, merges = c.ctx.verify_entities_compact_paths(c.H, idx, c.lC[rows], c.lH[rows], cC, cH, c.root[0], c.root[1], policy, agg, N_BITS, compact,
                                                                 verify_seed=SEED)
        assert ok.tolist() == [1] * len(rows) and merges == len(cC) and unique == hip_lib.shared_plan(c.H, idx, policy, agg)[1]


@pytest.mark.parametrize("leaf_first", [0, 1])
def test_verifier_under_both_sibling_orders(hip_lib, gpu_ctx, leaf_first):
    """The compact buffer is the same under both orders; the plan of the range proofs is not."""
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        c = Case(hip_lib, gpu_ctx, 6, leaves=[0, 1, 2, 3, 16, 17, 21, 40, 44, 63])
        for policy, agg in ((0, 3), (1, 5)):
            ok, unique, merges, route, _ = c.both(policy, agg)
            assert ok == [1] * c.b and merges == c.n_records and route == 1
            bad = c.cC.copy()
            bad[c.record(3, 2)] = np.frombuffer(NON_CANONICAL, np.uint8)       # the sibling of the rows under (3, 2): leaves 16, 17, 21
            ok, _, merges, route, _ = c.both(policy, agg, cC=bad)
            assert ok == c.failing({4, 5, 6}) and merges == c.n_records + c.b * 6 and route == 2
    finally:
        hip_lib.wire_config_restore(old)


# ------------------------------------------------------------------------------------------------ (c) the verifier, tampered
def tamper_cases(c):
    """(name, keyword arguments of Case.both, the rows that must fail, whether the path stage must have fallen back)"""
    H, b = c.H, c.b
    flip = lambda a, i, j=5, bit=0x04: _flipped(a, i, j, bit)
    out = []
    # a record that only row e uses: the sibling of its leaf
    e = b // 2
    rec = c.record(H, c.leaves[e])
    assert c.rows_under(H, c.leaves[e]) == {e}
    out.append(("private record, C", dict(cC=flip(c.cC, rec)), {e}, True))
    out.append(("private record, H", dict(cH=flip(c.cH, rec)), {e}, True))
    # a record of depth 1: the rows under that half use it (it is the other half's node)
    k = c.keys[1][0]
    out.append(("depth 1", dict(cH=flip(c.cH, c.record(1, k))), c.rows_under(1, k), True))
    out.append(("leaf C", dict(lC=flip(c.lC, b // 3)), {b // 3}, True))
    out.append(("leaf H", dict(lH=flip(c.lH, b - 1)), {b - 1}, True))
    out.append(("root", dict(root=(flip(np.frombuffer(c.root[0], np.uint8).reshape(1, 32), 0).tobytes(), c.root[1])), set(range(b)), True))
    # two records of one depth swapped (both arrays): the rows under either key
    d = H - 1 if H > 1 else 1
    ka, kb = c.keys[d][0], c.keys[d][-1]
    sw = lambda a: _swapped(a, c.record(d, ka), c.record(d, kb))
    out.append(("swap", dict(cC=sw(c.cC), cH=sw(c.cH)), c.rows_under(d, ka) | c.rows_under(d, kb), True))
    # a non-canonical encoding in a private record of a head row that another row joins above: leaves x (even, row h) and x + 1
    # are both rows, so row h + 1 joins row h's chain at depth H - 1, and the record (H, x) -- the leaf of row h + 1, as row h's
    # sibling -- is on row h's path alone
    h = next(i for i, x in enumerate(c.leaves) if x % 2 == 0 and i + 1 < b and c.leaves[i + 1] == x + 1)
    bad = c.cC.copy()
    bad[c.record(H, c.leaves[h])] = np.frombuffer(NON_CANONICAL, np.uint8)
    out.append(("non-canonical below a join", dict(cC=bad), {h}, True))
    # the same encoding in a record that several rows share
    d = max(1, H // 2)
    k = max(c.keys[d], key=lambda kk: len(c.rows_under(d, kk)))
    bad = c.cC.copy()
    bad[c.record(d, k)] = np.frombuffer(NON_CANONICAL, np.uint8)
    out.append(("non-canonical, shared", dict(cC=bad), c.rows_under(d, k), True))
    return out


def _flipped(a, i, j=5, bit=0x04):
    a = a.copy()
    a[i, j] ^= bit
    return a


def _swapped(a, i, j):
    a = a.copy()
    a[[i, j]] = a[[j, i]]
    return a


@pytest.mark.parametrize("case,which", [(6, 0), (12, 0), (12, 1), (12, 2), (32, 2), (64, 1)], indirect=["case"])
def test_verifier_tampered(hip_lib, case, which):
    c = case
    policy, agg = policies_of(c.H)[which]
    honest_unique = hip_lib.shared_plan(c.H, c.idx, policy, agg)[1]
    for name, kw, rows, fell_back in tamper_cases(c):
        ok, unique, merges, route, _ = c.both(policy, agg, **kw)
        assert ok == c.failing(rows), name
        assert 0 < len(rows) and (len(rows) < c.b or name == "root"), name     # each case alone among honest rows
        assert (route, merges) == (2, c.n_records + c.b * c.H), name            # the per-entity re-merge answered, after the shared one
        assert unique == honest_unique, name                                   # equal keys, equal records: the statements are the honest call's
    # one compact range proof corrupted: the rows its key names fail, the path verdicts are untouched (no fallback)
    sub_off, ref, _ = hip_lib.shared_compact_plan(c.H, c.idx, policy, agg, N_BITS)
    s = len(sub_off) - 2
    u = int(ref[s].max())
    bad = c.compact(policy, agg).copy()
    bad[int(sub_off[s + 1]) - 7] ^= 0x01                                        # inside the last proof of the last sub-proof
    ok, unique, merges, route, _ = c.both(policy, agg, compact=bad)
    assert ok == [int(ref[s, e] != u) for e in range(c.b)] and 0 in ok
    assert (route, merges, unique) == (1, c.n_records, honest_unique)


# ------------------------------------------------------------------------------------------------ the other 32-byte digests
@pytest.mark.parametrize("digest", ["DIGEST_BLAKE2S", "DIGEST_SHA256", "DIGEST_SHA3_256"])
def test_other_digests(hip_lib, digest):
    ctx = hip_lib.Context(0, 16, digest=getattr(hip_lib, digest), options=hip_lib.Options(window_bits=8))
    try:
        c = Case(hip_lib, ctx, 12)
        eC, eH = hip_lib.compact_paths_expand(12, c.idx, c.cC, c.cH)
        assert eC.tobytes() == c.pC.tobytes() and eH.tobytes() == c.pH.tobytes()
        for policy, agg in policies_of(12):
            ok, unique, merges, route, _ = c.both(policy, agg)
            assert ok == [1] * c.b and (route, merges) == (1, c.n_records) and unique == hip_lib.shared_plan(12, c.idx, policy, agg)[1]
        policy, agg = policies_of(12)[2]
        for name, kw, rows, _ in tamper_cases(c)[1::3]:                         # private record H, leaf H, non-canonical below a join
            ok, _, merges, route, _ = c.both(policy, agg, **kw)
            assert ok == c.failing(rows) and (route, merges) == (2, c.n_records + c.b * 12), name
    finally:
        ctx.close()


def test_a_64_byte_digest(hip_lib):
    """Blake2b: the prover's side and the host functions carry 64-byte hashes; the verifier refuses the context."""
    ctx = hip_lib.Context(0, 8, digest=hip_lib.DIGEST_BLAKE2B, options=hip_lib.Options(window_bits=8))
    try:
        rng = np.random.default_rng(3)
        idx = np.array([0, 1, 2, 3, 16, 17, 40, 63], np.uint64)
        v, r = rng.integers(0, 2, size=8, dtype=np.uint64), _blindings(rng, 8)
        tree = hip_lib.Tree(ctx, 6, idx, v, r, SEED)
        pC, pH, _, _ = tree.paths(idx)
        cC, cH = tree.paths_compact(idx)
        assert cH.shape == (len(cC), 64) and len(cC) == hip_lib.compact_paths_plan(6, idx)[2]
        eC, eH = hip_lib.compact_paths_expand(6, idx, cC, cH, hash_bytes=64)
        assert eC.tobytes() == pC.tobytes() and eH.tobytes() == pH.tobytes()
        lC, lH = ctx.commit_hash_batch(v, r)
        root = tree.root()
        with pytest.raises(hip_lib.DapolError) as e:
            ctx.verify_entities_compact_paths(6, idx, lC, lH, cC, cH, root[0], root[1], 0, 3, N_BITS, np.zeros(16, np.uint8), verify_seed=SEED)
        assert e.value.code == 8
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ (d) forwarding, refusals
def test_the_latency_regime_forwards(hip_lib, gpu_ctx, monkeypatch):
    """With the library's own limit: 8 rows x 4 sub-proofs = 32 <= 64 expand on the host, forward to dapol_verify_entities_compact and
    report b x H merges."""
    monkeypatch.delenv("DAPOL_VSHARED_FORWARD_MAX")
    c = Case(hip_lib, gpu_ctx, 6, leaves=[0, 1, 2, 3, 16, 17, 40, 63])
    ok, unique, merges, route, want_unique = c.both(0, 3)
    assert ok == [1] * 8 and (merges, route) == (48, 0) and unique == want_unique == 32
    bad = c.cC.copy()
    bad[c.record(6, 16), 3] ^= 0x10                                             # the sibling of leaf 16 = the leaf of row 5, on row 4's path
    ok, _, merges, route, _ = c.both(0, 3, cC=bad)
    assert ok == c.failing({4}) and (merges, route) == (48, 0)
    c2 = Case(hip_lib, gpu_ctx, 12) if 12 not in _CASES else _CASES[12]          # 200 rows: the kernels, whatever the limit
    assert c2.both(0, 12)[2:4] == (c2.n_records, 1)


def test_the_per_entity_route_alone(hip_lib, gpu_ctx, monkeypatch):
    """DAPOL_CPATHS_FALLBACK (the measurement knob of tools/bench_compact_paths.py): device expansion + the per-entity re-merge and
    nothing else for the paths -- same verdicts, b x H merges, route 3."""
    monkeypatch.setenv("DAPOL_CPATHS_FALLBACK", "1")
    c = Case(hip_lib, gpu_ctx, 12) if 12 not in _CASES else _CASES[12]
    policy, agg = policies_of(12)[2]
    ok, unique, merges, route, want_unique = c.both(policy, agg)
    assert ok == [1] * c.b and (merges, route) == (c.b * 12, 3) and unique == want_unique
    name, kw, rows, _ = tamper_cases(c)[7]
    ok, _, merges, route, _ = c.both(policy, agg, **kw)
    assert name == "non-canonical below a join" and ok == c.failing(rows) and (merges, route) == (c.b * 12, 3)


def test_verifier_refusals(hip_lib, gpu_ctx):
    import ctypes
    c = Case(hip_lib, gpu_ctx, 6, leaves=[0, 1, 2, 3, 16, 17, 40, 63])
    compact = c.compact(0, 3)
    a = lambda **kw: {**dict(height=6, leaf_idx=c.idx, leaf_C=c.lC, leaf_H=c.lH, cpath_C=c.cC, cpath_H=c.cH, root_C=c.root[0], root_H=c.root[1], policy=0,
                             aggregation_factor=3, n_bits=N_BITS, compact=compact, verify_seed=SEED), **kw}
    for kw in (dict(leaf_idx=np.array([0, 1, 3, 2, 16, 17, 40, 63], np.uint64)), dict(leaf_idx=np.array([0, 1, 2, 2, 16, 17, 40, 63], np.uint64)),
               dict(leaf_idx=np.array([0, 1, 2, 3, 16, 17, 40, 64], np.uint64)), dict(policy=2), dict(aggregation_factor=7), dict(n_bits=12), dict(height=0),
               dict(height=65)):
        with pytest.raises(hip_lib.DapolError) as e:
            gpu_ctx.verify_entities_compact_paths(**a(**kw))
        assert e.value.code == (1 if kw.get("height") == 65 else 8), kw
    for kw in (dict(compact=compact[:-1]), dict(compact=np.concatenate([compact, compact[:1]])), dict(cpath_C=c.cC[:-1], cpath_H=c.cH[:-1]),
               dict(cpath_C=np.concatenate([c.cC, c.cC[:1]]), cpath_H=np.concatenate([c.cH, c.cH[:1]])), dict(aggregation_factor=2)):
        ok, unique, merges = gpu_ctx.verify_entities_compact_paths(**a(**kw))   # a buffer of the wrong shape is an invalid proof
        assert ok.tolist() == [0] * 8 and (unique, merges) == (0, 0), kw
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    okb, uniq, mer = np.full(4, 0xAB, np.uint8), ctypes.c_uint64(12345), ctypes.c_uint64(12345)      # b = 0: nothing is touched but the counts
    rC, rH = np.frombuffer(c.root[0], np.uint8).copy(), np.frombuffer(c.root[1], np.uint8).copy()
    assert hip_lib.lib().dapol_verify_entities_compact_paths(gpu_ctx.h, 6, 0, None, None, None, 0, None, None, p(rC), p(rH), 0, 3, N_BITS, None, 0, None, p(okb),
                                                             ctypes.byref(uniq), ctypes.byref(mer)) == 0
    assert (okb == 0xAB).all() and (uniq.value, mer.value) == (0, 0)
    ok, unique, merges = gpu_ctx.verify_entities_compact_paths(**a())           # the call after the refusals is healthy
    assert ok.tolist() == [1] * 8 and (unique, merges) == (21, c.n_records)
