"""Every verifier path against proofs that ONLY THE ALGEBRA can reject.

A flipped byte enters the Merlin transcript, changes every later challenge and fails both halves of the verifier's check at once -- the
polynomial equation it weighs by c (t) and the inner-product equation (P) -- so it only shows that the byte is read.  The proofs here are
consistent in the transcript and wrong in one term of one equation:

  * tests/golden/forgeries.json (tests/golden/gen_forgeries.py, oracle/pyref.py range_prove(forge=)): every kind of forged element at
    (n, m) = (8,1), (8,4), (8,8), each row known to violate t, P or both and to leave the identity in the other half;
  * the GPU prover's own forgeries: k_rp_commit_V commits to the full uint64 while the bit kernels read the low n bits, so a value >= 2^n
    (or a sibling subtree whose sum passes 2^n, or wraps at 2^64) gives an otherwise honest proof of a false statement at any shape.  Its
    only defect is c z^(2+j) (v_j - v_j mod 2^n) B in the t-equation.

Every case verifies forged rows AMONG HONEST ONES PROVED ON THE GPU and asserts verdict 0 on exactly the forged rows.  Where a path is one
random linear combination of many proofs, a forged row stands ALONE in the combination under test: with two in it the second would hide
a path that loses the first one's term (a failed combination only sends its proofs on to the proof-by-proof check).
The paths are those verify_plan.inc chooses among; where size and not a knob puts a case on its path the arithmetic is in a comment."""
import ctypes
import os
import time

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
C7 = bytes([7]) + bytes(31)
RLC2 = {"DAPOL_VERIFY_RLC_MIN": "2"}


def _with_env(env, fn):
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in env:
            os.environ.pop(k, None)


def _fallbacks(hip_lib):
    n = ctypes.c_uint64()
    assert hip_lib.lib().dapol_diag_verify_fallbacks(ctypes.byref(n)) == 0
    return n.value


def _blindings(rng, *shape):
    r = rng.integers(0, 256, size=shape + (32,), dtype=np.uint8)
    r[..., 31] &= 0x0F
    return r


_ROWS = {}


def _rows(m):
    """(forged rows, their proofs [F][ps], their commitments [F][m][32], the honest row's proof [1][ps] and commitments) of shape (8, m)"""
    if m not in _ROWS:
        rows = [r for r in load_golden("forgeries.json")["rows"] if r["m"] == m]
        forged, honest = [r for r in rows if r["kind"] != "honest"], [r for r in rows if r["kind"] == "honest"]
        P = lambda rs: np.array([list(bytes.fromhex(r["proof"])) for r in rs], np.uint8)
        V = lambda rs: np.array([[list(bytes.fromhex(c)) for c in r["commitments"]] for r in rs], np.uint8)
        assert len(honest) == 1 and len(forged) >= 30
        _ROWS[m] = (forged, P(forged), V(forged), P(honest), V(honest))
    return _ROWS[m]


_HONEST = {}


def _honest(ctx, n, m, b):
    """b honest proofs of the GPU prover and their commitments (proved once per shape and count, never written to)"""
    key = (id(ctx), n, m, b)
    if key not in _HONEST:
        rng = np.random.default_rng(1000 * n + 10 * m + b)
        v = rng.integers(0, 2**n if n < 64 else 2**63, size=(b, m), dtype=np.uint64)
        r = _blindings(rng, b, m)
        proofs = ctx.range_prove_batch(n, m, v, r, nonce_seed=SEED, stream_id=np.arange(b, dtype=np.uint64))
        C, _ = ctx.commit_hash_batch(v.reshape(-1), r.reshape(-1, 32))
        _HONEST[key] = (proofs, C.reshape(b, m, 32))
    return _HONEST[key]


def _name(row):
    return (row["kind"], row["position"], row["violates"])


def _expect(ok, zeros, what):
    """verdict 0 on exactly `zeros` ({row: label}) and 1 elsewhere"""
    ok = np.asarray(ok)
    accepted = [zeros[i] for i in sorted(zeros) if ok[i]]
    assert not accepted, ("FORGERY ACCEPTED", what, accepted)
    rejected = [int(i) for i in np.flatnonzero(ok == 0) if int(i) not in zeros]
    assert not rejected, ("honest proof rejected", what, rejected)


# ------------------------------------------------------------------------------------------------ a. proof by proof, from the fixture
@pytest.mark.parametrize("m", [1, 4, 8])
def test_fixture_proof_by_proof(gpu_ctx, hip_lib, m):
    """b = 100 < RLC_MIN_DEFAULT = 112 (verify_plan.inc): the call goes proof by proof (range_verify_device; N < 256, so no small-call
    shapes: a lane replays each transcript), by default, with the wavefront absorb kernel ahead of the replay (k_rv_absorb_V, then resume)
    and under DAPOL_VERIFY_NO_RLC.  Every fixture row of the shape is in the batch -- rows 0, 63, 64 (either side of a wavefront) and the
    last among them -- beside the fixture's own honest proof and honest proofs of the GPU prover; then the forged rows alone."""
    forged, fp, fV, hp, hV = _rows(m)
    b, F = 100, len(forged)
    gp, gV = _honest(gpu_ctx, 8, m, b)
    rng = np.random.default_rng(m)
    pos = [0, 63, 64, b - 1] + [int(p) for p in rng.permutation(b) if p not in (0, 1, 63, 64, b - 1)][:F - 4]
    proofs, V = gp.copy(), gV.copy()
    proofs[pos], V[pos] = fp, fV
    proofs[1], V[1] = hp[0], hV[0]
    zeros = {p: _name(r) for p, r in zip(pos, forged)}
    for env in ({}, {"DAPOL_VERIFY_WAVE_TRANSCRIPT": "1"}, {"DAPOL_VERIFY_NO_RLC": "1"}, {"DAPOL_VERIFY_NO_RLC": "1", "DAPOL_VERIFY_WAVE_TRANSCRIPT": "1"}):
        fb = _fallbacks(hip_lib)
        _expect(_with_env(env, lambda: gpu_ctx.range_verify_batch(8, m, proofs, V, verify_seed=SEED)), zeros, env)
        _expect(_with_env(env, lambda: gpu_ctx.range_verify_batch(8, m, fp, fV, verify_seed=SEED)), {i: _name(r) for i, r in enumerate(forged)}, (env, "forged only"))
        assert _fallbacks(hip_lib) == fb, "no combined check: these calls go proof by proof"
    assert list(gpu_ctx.range_verify_batch(8, m, proofs, V, verify_seed=None)) == [int(i not in zeros) for i in range(b)]      # an OS-random c


# ------------------------------------------------------------------------------------------------ b. one linear combination, from the fixture
def _alone(ctx, hip_lib, m, b, env, rows=None):
    """Each forged row in turn ALONE among b - 1 honest proofs (at the first, the last and a middle row in turn): the combined check of
    the whole call must fail (dapol_diag_verify_fallbacks moves) and the verdict vector name exactly that row."""
    forged, fp, fV, hp, hV = _rows(m)
    gp, gV = _honest(ctx, 8, m, b)
    proofs, V = gp.copy(), gV.copy()
    proofs[1], V[1] = hp[0], hV[0]
    fb = _fallbacks(hip_lib)
    assert _with_env(env, lambda: ctx.range_verify_batch(8, m, proofs, V, verify_seed=SEED)).all()
    assert _fallbacks(hip_lib) == fb, "honest proofs pass the combined check at once"
    for i in (range(len(forged)) if rows is None else rows):
        at = (0, b - 1, b // 2)[i % 3]
        keep = proofs[at].copy(), V[at].copy()
        proofs[at], V[at] = fp[i], fV[i]
        fb = _fallbacks(hip_lib)
        _expect(_with_env(env, lambda: ctx.range_verify_batch(8, m, proofs, V, verify_seed=SEED)), {at: _name(forged[i])}, env)
        assert _fallbacks(hip_lib) > fb, ("the combined check passed with a forgery in it", env, _name(forged[i]))
        proofs[at], V[at] = keep


@pytest.mark.parametrize("m,extra", [(1, {}), (4, {}), (8, {}), (8, {"DAPOL_VERIFY_GH_EAGER": "1"}),
                                     (1, {"DAPOL_VERIFY_LANE_TRANSCRIPT": "1"}), (4, {"DAPOL_VERIFY_LANE_TRANSCRIPT": "1"}), (8, {"DAPOL_VERIFY_LANE_TRANSCRIPT": "1"})])
def test_fixture_alone_in_one_combination(gpu_ctx, hip_lib, m, extra):
    """DAPOL_VERIFY_RLC_MIN=2 batches a call of 10.  N = 8 and 32: TP = max(64, 2N) = 64, nch = TP >> 6 = 1, eager generator scalars;
    N = 64: TP = 128, nch = 2 > 1, lazy scalars (k_rvb_gh_lazy) unless DAPOL_VERIFY_GH_EAGER.  10 < 64: a failed combination goes straight
    to the proof-by-proof check, so the combination that sees the forgery is the call's only one."""
    _alone(gpu_ctx, hip_lib, m, 10, dict(RLC2, **extra))


@pytest.mark.parametrize("m", [1, 4, 8])
def test_fixture_bisection_into_eighths(gpu_ctx, hip_lib, m):
    """b = 640 under DAPOL_VERIFY_RLC_MIN=2 (bisect_failed_chunk, host_verify.inc): part = (640 + 7) / 8 = 80 >= 64, so a part that fails
    is split again into parts of 10 (< 64: those go proof by proof), and a part that passes vouches for its proofs.
    (1) every forged row alone in its part of 10 (row i in part (64 i) / F of the 64, at offset i mod 10): each of those combined checks sees
        one forgery only, and one that wrongly passes shows as verdict 1 on it;
    (2) all forged rows inside the second and the sixth eighth, the other six eighths vouching for 480 honest proofs."""
    forged, fp, fV, hp, hV = _rows(m)
    b, F = 640, len(forged)
    assert F <= 64
    gp, gV = _honest(gpu_ctx, 8, m, b)
    spread = [10 * ((64 * i) // F) + i % 10 for i in range(F)]
    assert len({p // 10 for p in spread}) == F
    eighths = [(80 if i % 2 == 0 else 400) + 4 * (i // 2) + i % 2 for i in range(F)]
    assert {p // 80 for p in eighths} == {1, 5}
    for pos in (spread, eighths):
        proofs, V = gp.copy(), gV.copy()
        proofs[pos], V[pos] = fp, fV
        fb = _fallbacks(hip_lib)
        ok = _with_env(RLC2, lambda: gpu_ctx.range_verify_batch(8, m, proofs, V, verify_seed=SEED))
        _expect(ok, {p: _name(r) for p, r in zip(pos, forged)}, "spread" if pos is spread else "two eighths")
        # the whole call, then every eighth with a forgery in it (and, spread, every part of 10 of those that is below 64 no more)
        assert _fallbacks(hip_lib) - fb >= 1 + len({p // 80 for p in pos})


@pytest.mark.parametrize("one_stream", [False, True])
def test_fixture_alone_in_the_bucket_method(gpu_ctx, hip_lib, one_stream):
    """(8,8): K = 4 + 2 lgN + m = 4 + 12 + 8 = 24 own points a proof; b = 512 gives 512 x 24 = 12,288 >= DAPOL_VERIFY_PIPPENGER_MIN=12288
    (the knob's floor), so the call's first combination sums the own points by the bucket method -- on the side stream behind its decode,
    or on the one stream.  Its parts (64 proofs: 1,536 points) are below the switch, so the bucket method sees each forgery exactly once:
    alone among 511 honest proofs."""
    env = dict(RLC2, DAPOL_VERIFY_PIPPENGER_MIN="12288")
    if one_stream:
        env["DAPOL_VERIFY_ONE_STREAM"] = "1"
    _alone(gpu_ctx, hip_lib, 8, 512, env)


# ------------------------------------------------------------------------------------------------ c. large shapes, forged by the GPU prover
def _gpu_forged(ctx, n, m, b, parties, seed):
    """b honest proofs (rows 0 .. b-1) and one forged proof per party in `parties` (rows b ...): that party's value is >= 2^n, the
    commitment holds it whole and the bits are its low n."""
    rng = np.random.default_rng(seed)
    k = len(parties)
    v = rng.integers(0, 2**n, size=(b + k, m), dtype=np.uint64)
    for i, j in enumerate(parties):
        v[b + i, j] += np.uint64((1 + i % 3) << n)
    r = _blindings(rng, b + k, m)
    proofs = ctx.range_prove_batch(n, m, v, r, nonce_seed=SEED, stream_id=np.arange(b + k, dtype=np.uint64))
    C, _ = ctx.commit_hash_batch(v.reshape(-1), r.reshape(-1, 32))
    return proofs, C.reshape(b + k, m, 32)


def _placed(proofs, V, b, at, n_honest):
    """the first b rows with row at[i] replaced by forged row i (which _gpu_forged put at n_honest + i)"""
    p, vv = proofs[:b].copy(), V[:b].copy()
    for i, row in at.items():
        p[row], vv[row] = proofs[n_honest + i], V[n_honest + i]
    return p, vv


@pytest.mark.parametrize("n,m,parties", [(8, 32, (0, 7, 8, 31)), (32, 8, (0, 3, 7))])
def test_out_of_range_party_at_256_generators(gpu_ctx, hip_lib, ref, n, m, parties):
    """N = 256: (8,32) has lb = 4 > lgn = 3, (32,8) lb = 4 < lgn = 5 (rv_q_split).  The reference verdict is the C oracle's on the first forged
    and the first honest row.
    b = 6 <= 128 and N >= 256: the small call (a wavefront replays each transcript, quad generators, quad own points on a side stream), and
    each of its knobs; b = 130 under DAPOL_VERIFY_NO_RLC: proof by proof without the small-call shapes; b = 130 >= RLC_MIN_DEFAULT = 112:
    one combination (quad generator MSM; DAPOL_NO_QUAD: the lane kernel), each forged row alone in it -- its parts of 17 < 112 go proof by
    proof."""
    k = len(parties)
    proofs, V = _gpu_forged(gpu_ctx, n, m, 130, parties, 77 * n + m)
    ps = proofs.shape[1]
    assert ref.ref_range_verify(n, m, proofs[130].tobytes(), ctypes.c_size_t(ps), V[130].tobytes(), C7, 0) == 0
    assert ref.ref_range_verify(n, m, proofs[0].tobytes(), ctypes.c_size_t(ps), V[0].tobytes(), C7, 0) == 1
    label = lambda at: {row: ("value >= 2^n", "party", parties[i]) for i, row in at.items()}
    at = dict(zip(range(k), (0, 2, 3, 5)))
    p6, V6 = _placed(proofs, V, 6, at, 130)
    for env in ({}, {"DAPOL_NO_QUAD": "1"}, {"DAPOL_VERIFY_ONE_STREAM": "1"}, {"DAPOL_VERIFY_LANE_TRANSCRIPT": "1"}, {"DAPOL_NO_SPLIT": "1"}, {"DAPOL_NO_SMALL_HI": "1"}):
        _expect(_with_env(env, lambda: gpu_ctx.range_verify_batch(n, m, p6, V6, verify_seed=SEED)), label(at), (n, m, 6, env))
    at = dict(zip(range(k), (0, 63, 64, 129)))
    p130, V130 = _placed(proofs, V, 130, at, 130)
    fb = _fallbacks(hip_lib)
    _expect(_with_env({"DAPOL_VERIFY_NO_RLC": "1"}, lambda: gpu_ctx.range_verify_batch(n, m, p130, V130, verify_seed=SEED)), label(at), (n, m, 130, "no rlc"))
    assert _fallbacks(hip_lib) == fb
    for env in ({}, {"DAPOL_NO_QUAD": "1"}):
        for i in range(k):
            at = {i: (0, 129, 64, 63)[i]}
            pp, vv = _placed(proofs, V, 130, at, 130)
            fb = _fallbacks(hip_lib)
            _expect(_with_env(env, lambda: gpu_ctx.range_verify_batch(n, m, pp, vv, verify_seed=SEED)), label(at), (n, m, 130, env))
            assert _fallbacks(hip_lib) > fb, ("the combined check passed with a forgery in it", env, parties[i])


def test_out_of_range_party_at_1024_parties(hip_lib):
    """The 1,024-party context of test_config4_shape_1024_party_verification, at (8,1024): N = 8,192, b = 3, a value >= 2^8 at party 0, 255,
    256 or 1,023 (either side of a 256-commitment block of the wavefront absorb, the default for m >= 256).  One by one (3 < 112); under
    DAPOL_VERIFY_RLC_MIN=2 one combination whose generator MSM is the window sweep (N >= 4096 on a context without high-half rows), and
    once more with DAPOL_VERIFY_GEN_STRAUS=1; each forged row alone.  All cases share the one context (what it costs is printed).
    No oracle verdict here, the one allowance the cases make: the C oracle takes about 3 s to prove and as long to verify ONE proof of 8,192
    generators."""
    t0 = time.time()
    ctx = hip_lib.Context(0, 1024)
    parties = (0, 255, 256, 1023)
    proofs, V = _gpu_forged(ctx, 8, 1024, 3, parties, 1024)
    t1 = time.time()
    assert ctx.range_verify_batch(8, 1024, proofs[:3], V[:3], verify_seed=SEED).all()
    for env in ({}, RLC2, dict(RLC2, DAPOL_VERIFY_GEN_STRAUS="1")):
        for i, j in enumerate(parties):
            at = {i: i % 3}
            pp, vv = _placed(proofs, V, 3, at, 3)
            fb = _fallbacks(hip_lib)
            _expect(_with_env(env, lambda: ctx.range_verify_batch(8, 1024, pp, vv, verify_seed=SEED)), {i % 3: ("value >= 2^n", "party", j)}, env)
            assert (_fallbacks(hip_lib) > fb) == bool(env), (env, j)
    print("1,024-party context + 7 proofs: %.1f s; 13 verifier calls: %.1f s" % (t1 - t0, time.time() - t1))
    ctx.close()


# ------------------------------------------------------------------------------------------------ d. entities
H = 6
LIGHT = [1, 5, 9, 12, 17, 23, 26, 30, 33, 37, 40, 44, 47, 50, 54, 57, 60, 63]
HEAVY = (20, 21)                                        # one sibling pair


def _sibling_sums(idx, values):
    """[entity][sibling] true sums (Python integers: no wrap) of the sibling subtrees of each leaf's path, root side first"""
    out = []
    for x in map(int, idx):
        row = []
        for k in range(H - 1, -1, -1):
            s = (x >> k) ^ 1
            row.append(sum(v for i, v in zip(map(int, idx), values) if i >> k == s))
        out.append(row)
    return out


class _Entities:
    def __init__(self, hip_lib, ctx, n_bits, heavy_values):
        self.hip, self.ctx, self.n_bits = hip_lib, ctx, n_bits
        rng = np.random.default_rng(n_bits)
        self.idx = np.array(sorted(LIGHT + list(HEAVY)), np.uint64)
        self.values = [heavy_values[HEAVY.index(i)] if i in HEAVY else int(rng.integers(0, 4)) for i in map(int, self.idx)]
        self.v = np.array(self.values, np.uint64)
        self.r = _blindings(rng, len(self.idx))
        self.tree = hip_lib.Tree(ctx, H, self.idx, self.v, self.r, SEED)
        self.root = self.tree.root()
        self.lC, self.lH = ctx.commit_hash_batch(self.v, self.r)
        self.sums = _sibling_sums(self.idx, self.values)
        # "every sibling sum on the path < 2^n_bits": only the two heavy leaves' paths never meet an ancestor of the pair
        self.want = [int(all(s < 2**n_bits for s in row)) for row in self.sums]
        assert self.want == [int(int(i) in HEAVY) for i in self.idx]
        _, _, pv, _ = self.tree.paths(self.idx)                            # the tree's own levels (they wrap at 2^64)
        assert pv.tolist() == [[s % 2**64 for s in row] for row in self.sums]

    def verify(self, pC, pH, blobs, policy, agg, rows=slice(None)):
        return self.ctx.verify_entities(H, self.idx[rows], self.lC[rows], self.lH[rows], pC[rows], pH[rows], self.root[0], self.root[1], policy, agg,
                                        self.n_bits, blobs[rows], verify_seed=SEED).tolist()


@pytest.fixture(scope="module")
def ent8(hip_lib, gpu_ctx):
    return _Entities(hip_lib, gpu_ctx, 8, (200, 100))


@pytest.fixture(scope="module")
def ent64(hip_lib, gpu_ctx):
    return _Entities(hip_lib, gpu_ctx, 64, (2**63, 2**63))


@pytest.mark.parametrize("agg", [0, 2, 3, H])
@pytest.mark.parametrize("policy", [0, 1])
def test_entities_with_an_out_of_range_sibling(hip_lib, pyref, ent8, policy, agg):
    """n_bits = 8, 20 leaves of value <= 3 and the pair (200, 100): every ancestor of the pair sums to >= 300, so every other entity has exactly
    one out-of-range sibling, at the level where its path leaves the pair's -- in an aggregated proof (first, last real party, beside padding
    parties) or an individual one, as the aggregation factor has it.  The prover commits to the whole sum and proves its low 8 bits.
    verify_entities over all 20 (grouped; 20 x plan size > 64: no lanes) and over four subsets of 5 (b x proofs <= 64: the groups on lanes),
    default, DAPOL_NO_LANES, DAPOL_NO_GROUP; verify_entities_shared on the blobs of prove_entities_shared, through its kernels and in its
    forwarding regime; ProofStore.verify on the device."""
    e = ent8
    pC, pH, blobs = e.tree.prove_entities(e.idx, policy, agg, 8, SEED)
    if (policy, agg) == (0, 3):                          # the Python oracle's policy check on one valid and two invalid entities
        name = "padding"
        plan, pos = pyref.policy_plan(name, H, agg)
        for row in (list(map(int, e.idx)).index(HEAVY[0]), 0, len(e.idx) - 1):
            cut, aggregated, individual = 0, [], []
            for _, _, mm in plan:
                aggregated.append(blobs[row, cut:cut + pyref.range_proof_size(8, mm)].tobytes())
                cut += len(aggregated[-1])
            for _ in range(pos, H):
                individual.append(blobs[row, cut:cut + pyref.range_proof_size(8, 1)].tobytes())
                cut += len(individual[-1])
            assert cut == blobs.shape[1]
            assert pyref.policy_verify(name, aggregated, individual, [pC[row, k].tobytes() for k in range(H)], n=8) == bool(e.want[row])
    for env in ({}, {"DAPOL_NO_LANES": "1"}, {"DAPOL_NO_GROUP": "1"}, {"DAPOL_NO_LANES": "1", "DAPOL_NO_GROUP": "1"}):
        assert _with_env(env, lambda: e.verify(pC, pH, blobs, policy, agg)) == e.want, env
        for first in range(4):
            rows = slice(first, None, 4)
            assert _with_env(env, lambda: e.verify(pC, pH, blobs, policy, agg, rows)) == e.want[rows], (env, first)
    sC, sH, sblobs, proved = e.tree.prove_entities_shared(e.idx, policy, agg, 8, SEED)
    args = (H, e.idx, e.lC, e.lH, sC, sH, e.root[0], e.root[1], policy, agg, 8, sblobs)
    assert e.ctx.verify_entities(*args, verify_seed=SEED).tolist() == e.want
    ok, unique = _with_env({"DAPOL_VSHARED_FORWARD_MAX": "0"}, lambda: e.ctx.verify_entities_shared(*args, verify_seed=SEED))
    assert ok.tolist() == e.want                         # a forged shared sub-proof fails its whole run and nothing else
    assert unique == hip_lib.shared_plan(H, e.idx, policy, agg)[1] == proved
    ok, _ = e.ctx.verify_entities_shared(*args, verify_seed=SEED)
    assert ok.tolist() == e.want
    rows = slice(2, 12, 3)                                # 4 entities x plan size <= 7 = 28 <= VSHARED_FORWARD_MAX = 64: forwarded
    ok, _ = e.ctx.verify_entities_shared(H, e.idx[rows], e.lC[rows], e.lH[rows], sC[rows], sH[rows], e.root[0], e.root[1], policy, agg, 8, sblobs[rows], verify_seed=SEED)
    assert ok.tolist() == e.want[rows]
    store = hip_lib.ProofStore(e.tree, policy, agg, 8, SEED)
    try:
        store.refresh()
        assert store.verify(SEED).tolist() == e.want
        assert store.verify(None).tolist() == e.want
    finally:
        store.close()


@pytest.mark.parametrize("policy", [0, 1])
def test_batch_proof_with_an_out_of_range_sibling(hip_lib, ent8, policy):
    """verify_batch, one proof over the deduplicated siblings of three leaves: with both heavy leaves in the batch every ancestor of the pair
    is on the batch's own paths and no sibling is heavy -- valid; three light leaves have an ancestor of the pair among their siblings."""
    e = ent8
    where = {int(i): k for k, i in enumerate(e.idx)}
    for leaves, want in (((20, 21, 44), True), ((1, 30, 44), False), ((17, 23, 63), False)):
        level, index = hip_lib.batch_siblings(H, np.array(leaves, np.uint64))
        heavy = [int(l) >= 1 and (HEAVY[0] >> int(l)) == int(i) for l, i in zip(level, index)]      # a sibling that is an ancestor of the pair
        assert any(heavy) == (not want)
        sel = [where[x] for x in leaves]
        S = len(level)
        for agg in (0, 2, S):
            _, _, sC, sH, blob = e.tree.prove_batch(np.array(leaves, np.uint64), policy, agg, 8, SEED)
            for env in ({}, {"DAPOL_NO_LANES": "1"}):
                got = _with_env(env, lambda: e.ctx.verify_batch(H, np.array(leaves, np.uint64), e.lC[sel], e.lH[sel], sC, sH, e.root[0], e.root[1], policy, agg, 8, blob,
                                                                verify_seed=SEED))
                assert got == want, (leaves, agg, env)


@pytest.mark.parametrize("policy,agg", [(0, 0), (0, H), (1, 3)])
def test_entities_with_a_sum_that_wraps_at_2e64(hip_lib, ref, ent64, policy, agg):
    """n_bits = 64 and the pair (2^63, 2^63): the parent's value wraps to 0 while its commitment holds 2^64 B, so every entity but the two heavy
    leaves has a sibling whose commitment no 64-bit proof covers.  The reference verdict is the C oracle's on the individual proof of that
    sibling (and of the one beside it) at aggregation 0."""
    e = ent64
    pC, pH, blobs = e.tree.prove_entities(e.idx, policy, agg, 64, SEED)
    for env in ({}, {"DAPOL_NO_LANES": "1", "DAPOL_NO_GROUP": "1"}):
        assert _with_env(env, lambda: e.verify(pC, pH, blobs, policy, agg)) == e.want, env
        assert _with_env(env, lambda: e.verify(pC, pH, blobs, policy, agg, slice(1, None, 4))) == e.want[1::4], env
    if agg == 0 and policy == 0:
        row = 0
        assert blobs.shape[1] == (H + 1) * 672                             # padding / 0: a one-party proof of the padding commitment, then one per sibling
        for k in range(H):
            sub = blobs[row, 672 * (k + 1):672 * (k + 2)].tobytes()
            assert ref.ref_range_verify(64, 1, sub, ctypes.c_size_t(672), pC[row, k].tobytes(), C7, 0) == int(e.sums[row][k] < 2**64), k
        assert sum(s >= 2**64 for s in e.sums[row]) == 1
    store = hip_lib.ProofStore(e.tree, policy, agg, 64, SEED)
    try:
        store.refresh()
        assert store.verify(SEED).tolist() == e.want
    finally:
        store.close()
