"""dapol_verify_entities_shared: dapol_verify_entities' verdict vector with every run of equal sub-proofs checked once.  The tests pin
the DEFINITION (include/dapol_hip.h): row e of sub-proof s repeats row e - 1 iff the sub-proof's bytes and the sibling commitments it
covers are equal; a head is verified once and its run inherits the verdict; `unique` counts the heads.  Every verdict vector is compared
with dapol_verify_entities on the same input.

Calls with b x plan size <= 64 forward to dapol_verify_entities (and report b x plan size).  The H = 6 tree of the prover's tests has
8 leaves and at most 7 sub-proofs, so these tests set DAPOL_VSHARED_FORWARD_MAX=0 to run it through the kernels; the forwarding test
runs with the library's own limit."""
import ctypes

import numpy as np
import pytest

from test_shared_plan_abi import H6_CASES, H6_LEAVES

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


def _blindings(rng, n):
    r = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    r[:, 31] &= 0x0F
    return r


def _fallbacks(hip_lib):
    n = ctypes.c_uint64()
    assert hip_lib.lib().dapol_diag_verify_fallbacks(ctypes.byref(n)) == 0
    return n.value


class Proven:
    """A tree, b of its leaves and their proofs under one (policy, aggregation factor, n_bits): everything a verifier call takes."""

    def __init__(self, hip_lib, ctx, H, leaves, policy, agg, n_bits, seed=1, shared=True, values=None):
        rng = np.random.default_rng(seed)
        self.hip, self.ctx, self.H, self.policy, self.agg, self.n_bits = hip_lib, ctx, H, policy, agg, n_bits
        self.idx = np.array(sorted(leaves), np.uint64)
        self.v = rng.integers(0, 21, size=len(self.idx), dtype=np.uint64) if values is None else values
        self.r = _blindings(rng, len(self.idx))
        self.tree = hip_lib.Tree(ctx, H, self.idx, self.v, self.r, SEED)
        self.lC, self.lH = ctx.commit_hash_batch(self.v, self.r)
        self.root = self.tree.root()
        self.prove(shared)

    def prove(self, shared=True, policy=None, agg=None):
        if policy is not None:
            self.policy, self.agg = policy, agg
        if shared:
            self.pC, self.pH, self.blobs, self.proved = self.tree.prove_entities_shared(self.idx, self.policy, self.agg, self.n_bits, SEED)
        else:
            self.pC, self.pH, self.blobs = self.tree.prove_entities(self.idx, self.policy, self.agg, self.n_bits, SEED)
        return self

    def plan_total(self, rows=None):
        idx = self.idx if rows is None else self.idx[rows]
        return self.hip.shared_plan(self.H, idx, self.policy, self.agg)[1]

    def both(self, blobs=None, pC=None, rows=None):
        """(verdicts, unique) of the shared call, after comparing the verdicts with dapol_verify_entities' on the same input."""
        blobs = self.blobs if blobs is None else blobs
        pC = self.pC if pC is None else pC
        sel = slice(None) if rows is None else rows
        args = (self.H, self.idx[sel], self.lC[sel], self.lH[sel], pC[sel], self.pH[sel], self.root[0], self.root[1], self.policy, self.agg, self.n_bits,
                blobs[sel])
        want = self.ctx.verify_entities(*args, verify_seed=SEED)
        ok, unique = self.ctx.verify_entities_shared(*args, verify_seed=SEED)
        assert ok.tolist() == want.tolist()
        return ok.tolist(), unique


@pytest.fixture(scope="module")
def h6(hip_lib, ctx8):
    return Proven(hip_lib, ctx8, 6, H6_LEAVES, 0, 3, 8)


# ------------------------------------------------------------------------------------------------ 1. equal verdicts, both orders
@pytest.mark.parametrize("leaf_first", ORDERS)
@pytest.mark.parametrize("policy,agg", H6_CASES)
def test_equal_verdicts_and_unique_counts(hip_lib, h6, policy, agg, leaf_first):
    """Blobs of prove_entities_shared: equal keys are equal bytes over equal commitments, another key is another nonce stream, so the
    heads are exactly the distinct statements -- unique == shared_plan's total.  Blobs of prove_entities: the nonce streams are keyed
    per leaf, nothing repeats, unique == b x plan size.  All ones, as dapol_verify_entities says, and no combined check fails."""
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        fb = _fallbacks(hip_lib)
        h6.prove(True, policy, agg)
        ok, unique = h6.both()
        assert ok == [1] * 8 and unique == h6.plan_total() == h6.proved
        h6.prove(False)
        ok, unique = h6.both()
        n_sub = len(hip_lib.shared_plan(6, h6.idx, policy, agg)[0])
        assert ok == [1] * 8 and unique == 8 * n_sub
        assert _fallbacks(hip_lib) == fb
    finally:
        hip_lib.wire_config_restore(old)
        h6.prove(True, 0, 3)


# ------------------------------------------------------------------------------------------------ 2. tamper matrix
def test_tamper_matrix(hip_lib, h6):
    """Padding / 3, root side first: leaves 0-3 share the aggregated proof (four parties of 8 bits: 608 bytes -- A, S, T1, T2, three
    scalars, five L / R pairs, a, b).  A tampered copy fails its own entity only, wherever it stands in the run: as the head it fails alone
    (row 1 differs from it and opens a run of its own), in the middle the rows behind it restart."""
    assert h6.blobs[0, :608].tobytes() == h6.blobs[3, :608].tobytes()
    _, unique0 = h6.both()
    assert unique0 == 21
    for e, more in ((3, 1), (0, 1), (1, 2)):            # a tampered row is a head; so is the row behind it unless the run ends there or it was one already
        bad = h6.blobs.copy()
        bad[e, 40] ^= 0x01
        ok, unique = h6.both(bad)
        assert ok == [int(i != e) for i in range(8)], e
        assert unique == unique0 + more, e
    bad = h6.blobs.copy()
    bad[:4, 40] ^= 0x01                                  # the same byte in all four copies: still one run, and it fails as one
    ok, unique = h6.both(bad)
    assert ok == [0, 0, 0, 0, 1, 1, 1, 1] and unique == unique0
    for at in (5, 40, 70, 100, 130, 170, 200, 230, 530, 550, 590):      # A, S, T1, T2, t_x, t_x_blinding, e_blinding, L_1, R_5, a, b
        bad = h6.blobs.copy()
        bad[3, at] ^= 0x02
        ok, _ = h6.both(bad)
        assert ok == [1, 1, 1, 0, 1, 1, 1, 1], at
    bad = h6.blobs.copy()                                # an individual proof (sibling 4: leaves 2 and 3 share it), last byte of the blob too
    bad[2, 608 + 480 + 7] ^= 0x10
    bad[6, -1] ^= 0x80
    ok, _ = h6.both(bad)
    assert ok == [1, 1, 0, 1, 1, 1, 0, 1]


# ------------------------------------------------------------------------------------------------ 3. commitments are part of the row
def test_a_commitment_that_differs_under_equal_proof_bytes_is_not_inherited(hip_lib, h6):
    """Sibling 0 lies inside the aggregated proof's span (siblings 0-2) and nowhere else.  Another valid commitment there, in a middle
    row of the run of leaves 0-3, makes that row and its successor heads (+2; +1 in the run's last row); the row fails -- its proof
    bytes are its neighbours', its statement is not -- and nobody else does.  Sibling 5 lies outside that span and inside one whose
    rows are all heads already (the leaf-level sibling): the count does not move."""
    _, unique0 = h6.both()
    for e, more in ((1, 2), (2, 2), (3, 1)):
        pC = h6.pC.copy()
        pC[e, 0] = h6.lC[5]
        ok, unique = h6.both(pC=pC)
        assert ok == [int(i != e) for i in range(8)] and unique == unique0 + more, e
    pC = h6.pC.copy()
    pC[1, 5] = h6.lC[5]
    ok, unique = h6.both(pC=pC)
    assert ok == [1, 0, 1, 1, 1, 1, 1, 1] and unique == unique0
    pC = h6.pC.copy()                                    # sibling 4 (covered by the individual proof that leaves 0 and 1 share): that run splits
    pC[1, 4] = h6.lC[5]
    ok, unique = h6.both(pC=pC)
    assert ok == [1, 0, 1, 1, 1, 1, 1, 1] and unique == unique0 + 1


# ------------------------------------------------------------------------------------------------ 4. long runs
@pytest.fixture(scope="module")
def h10(hip_lib, ctx8):
    values = (np.arange(600) % 3 == 0).astype(np.uint64)                 # 200 in all: every sibling sum fits the 8-bit proofs
    return Proven(hip_lib, ctx8, 10, range(600), 0, 2, 8, seed=4, values=values)


def test_runs_longer_than_a_wavefront_and_a_scan_block(hip_lib, h10):
    """H = 10, leaves 0 .. 599, padding / 2: the aggregated proof speaks about depth 2 (runs of 256, 256 and 88 rows), the individual
    proof of sibling 2 about depth 3 (runs of 128), and so on down to the leaves.  Tampered copies at the edges of wavefronts, of the
    compare kernel's blocks and of the runs themselves fail alone."""
    ok, unique = h10.both()
    assert ok == [1] * 600 and unique == h10.plan_total() == h10.proved < 600 * 9
    bad = h10.blobs.copy()
    hit = (63, 64, 255, 256, 599)
    for e in hit:
        bad[e, 33] ^= 0x04
    ok, unique2 = h10.both(bad)
    assert ok == [int(e not in hit) for e in range(600)]
    # new heads: 63 (64 carries the same tampered bytes, repeats it and inherits its failure) and 65 behind them; 255, and 257 behind
    # 256 (a head already: another key); 599 ends its run
    assert unique2 == unique + 5


# ------------------------------------------------------------------------------------------------ 5. order is not required
def test_shuffled_rows_share_less_and_verify_the_same(hip_lib, h6):
    _, unique0 = h6.both()
    rows = np.random.default_rng(5).permutation(8)
    assert rows.tolist() != sorted(rows.tolist())
    ok, unique = h6.both(rows=rows)
    assert ok == [1] * 8 and unique0 <= unique <= 32
    bad = h6.blobs.copy()
    bad[3, 40] ^= 0x01
    ok, _ = h6.both(bad, rows=rows)
    assert ok == [int(r != 3) for r in rows]


# ------------------------------------------------------------------------------------------------ 6. edges
def test_edges(hip_lib, ctx8, h6):
    ok, unique = h6.both(rows=np.array([5]))             # b = 1
    assert ok == [1] and unique == 4
    lib, p = hip_lib.lib(), (lambda a: a.ctypes.data_as(ctypes.c_void_p))
    okb, uniq = np.full(4, 0xAB, np.uint8), ctypes.c_uint64(12345)      # b = 0: nothing is touched but the count
    rC, rH = np.frombuffer(h6.root[0], np.uint8).copy(), np.frombuffer(h6.root[1], np.uint8).copy()
    assert lib.dapol_verify_entities_shared(ctx8.h, 6, 0, None, None, None, 0, None, None, p(rC), p(rH), 0, 3, 8, None, 0, None, p(okb), ctypes.byref(uniq)) == 0
    assert (okb == 0xAB).all() and uniq.value == 0
    for policy, agg in ((0, 1), (1, 1), (1, 0), (0, 0)):  # H = 1 with both leaves: one sibling, nothing shared but padding / 0's pad proof
        t1 = Proven(hip_lib, ctx8, 1, [0, 1], policy, agg, 8, seed=6)
        ok, unique = t1.both()
        assert ok == [1, 1] and unique == t1.plan_total()
    h6.prove(True, 0, 0)                                 # aggregation 0: the siblingless pad proof is one run of all rows
    try:
        ok, unique = h6.both()
        assert ok == [1] * 8 and unique == h6.plan_total() < 8 * 7
        assert len({h6.blobs[e, :480].tobytes() for e in range(8)}) == 1
        bad = h6.blobs.copy()
        bad[4, 9] ^= 0x01                                # its copy in the middle of the run
        ok, unique2 = h6.both(bad)
        assert ok == [1, 1, 1, 1, 0, 1, 1, 1] and unique2 == unique + 2
    finally:
        h6.prove(True, 0, 3)


@pytest.mark.parametrize("leaf_first", ORDERS)
def test_height_64(hip_lib, ctx8, leaf_first):
    """H = 64, leaves 0, 1, 2^63, 2^64 - 1, padding / 2: a plan of 63 sub-proofs, 62 of them in one group."""
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        t = Proven(hip_lib, ctx8, 64, [0, 1, 1 << 63, (1 << 64) - 1], 0, 2, 8, seed=3)
        ok, unique = t.both()
        assert ok == [1] * 4 and unique == t.plan_total() == t.proved < 4 * 63
        bad = t.blobs.copy()
        bad[1, -1] ^= 0x01                               # the last byte of the last sub-proof
        bad[2, 0] ^= 0x01                                # the first byte of the first
        assert t.both(bad)[0] == [1, 0, 0, 1]
    finally:
        hip_lib.wire_config_restore(old)


def test_the_latency_regime_forwards(hip_lib, h10, monkeypatch):
    """With the library's own limit: 7 entities x 9 sub-proofs = 63 forward to dapol_verify_entities and report 63; 8 x 9 = 72 go
    through the kernels and report the heads."""
    monkeypatch.delenv("DAPOL_VSHARED_FORWARD_MAX")
    rows7, rows8 = np.arange(300, 307), np.arange(300, 308)
    ok, unique = h10.both(rows=rows7)
    assert ok == [1] * 7 and unique == 63
    ok, unique = h10.both(rows=rows8)
    assert ok == [1] * 8 and unique == h10.plan_total(rows8) < 72
    bad = h10.blobs.copy()
    bad[303, 33] ^= 0x04
    assert h10.both(bad, rows=rows7)[0] == h10.both(bad, rows=rows8)[0][:7] == [1, 1, 1, 0, 1, 1, 1]


# ------------------------------------------------------------------------------------------------ 7. into the combined check
def test_the_compact_batch_crosses_into_the_combined_check(hip_lib, ctx1):
    """H = 13, 2,500 leaves, 64-bit proofs, padding / 1 on a one-party context: 13 sub-proofs of m = 1 in ONE group of well over 2,048
    distinct proofs -- the compact batch is one random linear combination.  No fallback while all are valid; two tampered entities
    (one of them in a copy that hundreds of rows share) fail alone."""
    H, n_bits = 13, 64
    rng = np.random.default_rng(13)
    leaves = np.sort(rng.choice(1 << H, size=2500, replace=False))
    v = rng.integers(0, 1000, size=2500, dtype=np.uint64)
    v[1234] = 1 << 63
    t = Proven(hip_lib, ctx1, H, leaves, 0, 1, n_bits, seed=13, values=v)
    fb = _fallbacks(hip_lib)
    ok, unique = t.ctx.verify_entities_shared(H, t.idx, t.lC, t.lH, t.pC, t.pH, t.root[0], t.root[1], 0, 1, n_bits, t.blobs, verify_seed=SEED)
    assert ok.all() and 2048 < unique == t.plan_total() == t.proved < 2500 * 13
    assert _fallbacks(hip_lib) == fb
    bad = t.blobs.copy()
    bad[700, 5] ^= 0x01                                  # sub-proof 0 (depth 1): shared by half the tree
    bad[2499, -3] ^= 0x01                                # the last entity's leaf-level proof
    ok, unique2 = t.both(bad)
    assert [e for e in range(2500) if not ok[e]] == [700, 2499] and unique2 == unique + 2
    assert _fallbacks(hip_lib) > fb


# ------------------------------------------------------------------------------------------------ 8. 64-byte digests
def test_blake2b_context(hip_lib):
    ctx = hip_lib.Context(0, 8, digest=hip_lib.DIGEST_BLAKE2B)
    try:
        t = Proven(hip_lib, ctx, 5, [1, 2, 3, 9, 20, 31], 0, 3, 8, seed=64)         # new_blank + build
        assert t.pH.shape == (6, 5, 64)
        ok, unique = t.both()
        assert ok == [1] * 6 and unique == t.plan_total()
        bad = t.blobs.copy()
        bad[1, 40] ^= 0x01
        assert t.both(bad)[0] == [1, 0, 1, 1, 1, 1]
        pH = t.pH.copy()
        pH[4, 2, 63] ^= 0x01                             # a node hash: the Merkle re-merge is per entity
        ok, _ = ctx.verify_entities_shared(5, t.idx, t.lC, t.lH, t.pC, pH, t.root[0], t.root[1], 0, 3, 8, t.blobs, verify_seed=SEED)
        assert ok.tolist() == [1, 1, 1, 1, 0, 1]
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 9. wrong lengths and refusals
def test_wrong_lengths_and_refusals(hip_lib, ctx1, h6):
    a = lambda **kw: {**dict(height=6, leaf_idx=h6.idx, leaf_C=h6.lC, leaf_H=h6.lH, path_C=h6.pC, path_H=h6.pH, root_C=h6.root[0], root_H=h6.root[1],
                             policy=0, aggregation_factor=3, n_bits=8, range_proofs=h6.blobs, verify_seed=SEED), **kw}
    flat_C, flat_H = h6.pC.reshape(-1, 32), h6.pH.reshape(-1, 32)
    for kw in (dict(path_C=flat_C[:-1], path_H=flat_H[:-1]), dict(range_proofs=h6.blobs.reshape(-1)[:-1]), dict(height=5), dict(aggregation_factor=2)):
        ok, unique = h6.ctx.verify_entities_shared(**a(**kw))            # a proof of the wrong shape is an invalid proof
        assert ok.tolist() == [0] * 8 and unique == 0, kw
    for kw in (dict(policy=2), dict(aggregation_factor=7), dict(aggregation_factor=-1), dict(n_bits=12)):
        with pytest.raises(hip_lib.DapolError) as e:
            h6.ctx.verify_entities_shared(**a(**kw))
        assert e.value.code == 8, kw
    with pytest.raises(hip_lib.DapolError) as e:
        ctx1.verify_entities_shared(**a())                                # a four-party proof on a one-party context
    assert e.value.code == 8
    with pytest.raises(hip_lib.DapolError) as e:
        h6.ctx.verify_entities_shared(**a(height=65))
    assert e.value.code == 1
    ok, unique = h6.ctx.verify_entities_shared(**a())                     # the call after the refusals is healthy
    assert ok.tolist() == [1] * 8 and unique == 21
